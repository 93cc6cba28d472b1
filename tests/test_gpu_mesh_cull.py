"""GPU tests of mesh culling (neurecon_amd.mesh_cull, libnrhip nr_mask_dilate / nr_mesh_view_test,
neurecon_amd/csrc/nr_meshcull.hip) against the numpy restatement of the two rules (tests/mesh_cull_ref.py), by
integer equality.  The visibility rule is given the device's own depth frames (render_mesh's depth_z and face_id),
so the comparison is of the view test alone; the frames have their own tests (tests/test_gpu_mesh_render.py)."""
import json

import numpy as np
import pytest
import torch

from mesh_cull_ref import IN_IMAGE, IN_MASK, VISIBLE, ref_dilate, ref_view_test
from test_mesh_cull import facing_cosine, hull_scene, orbit, sphere_scene
from test_mesh_render import H_STD, W_STD, icosphere, sphere_attributes, std_intrinsics

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


def device_frames(verts, faces, poses, K, H, W, near=1e-4):
    from neurecon_amd.mesh_util import render_mesh
    out = render_mesh(verts, faces, np.asarray(poses).reshape(-1, 4, 4), K, H, W, near=near)
    return out['depth_z'].cpu().numpy(), out['face_id'].cpu().numpy()


def views(verts, faces, poses, K, H, W, **kw):
    from neurecon_amd.mesh_cull import vertex_views
    out = vertex_views(verts, faces, poses, K, H, W, return_flags=True, **kw)
    assert set(out) == {'n_in_image', 'n_in_mask', 'n_visible', 'flags', 'n_views'}
    B, V = (poses.shape[0] if len(poses.shape) == 3 else 1), len(verts)
    assert out['n_views'] == B and out['flags'].is_cuda and out['flags'].dtype == torch.uint8
    assert tuple(out['flags'].shape) == (B, V)
    for k in ('n_in_image', 'n_in_mask', 'n_visible'):
        assert out[k] is None or (out[k].is_cuda and out[k].dtype == torch.int32 and tuple(out[k].shape) == (V,)), k
    return out


def check_counts(out):
    """the counts are the column sums of the flags"""
    fl = out['flags'].cpu().numpy()
    for key, bit in (('n_in_image', IN_IMAGE), ('n_in_mask', IN_MASK), ('n_visible', VISIBLE)):
        if out[key] is None:
            assert not (fl & bit).any(), key
        else:
            assert np.array_equal(out[key].cpu().numpy(), ((fl & bit) != 0).sum(0)), key


def same(a, b):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and torch.equal(a[k], b[k]))
               for k in ('n_in_image', 'n_in_mask', 'n_visible', 'flags'))


# ------------------------------------------------------------------------------------------------
# 1. dilation
# ------------------------------------------------------------------------------------------------
def mask_set(H, W, seed):
    """a pixel at each corner, two random masks and an empty one -> bool [7, H, W]"""
    rng = np.random.default_rng(seed)
    m = np.zeros((7, H, W), bool)
    m[0, 0, 0] = m[1, 0, W - 1] = m[2, H - 1, 0] = m[3, H - 1, W - 1] = True
    m[4] = rng.random((H, W)) < 0.02
    m[5] = rng.random((H, W)) < 0.3
    return m


@pytest.mark.parametrize('H, W', [(H_STD, W_STD), (1, 1), (1, 300), (300, 1), (65, 257)])
def test_dilate_masks_equals_the_rule(H, W):
    from neurecon_amd.mesh_cull import dilate_masks
    m = mask_set(H, W, H * 1000 + W)
    for r in (0, 1, 3, 7, 64, max(H, W), max(H, W) + 5):
        got = dilate_masks(m, r)
        assert got.is_cuda and got.dtype == torch.bool and tuple(got.shape) == m.shape
        assert np.array_equal(got.cpu().numpy(), ref_dilate(m, r)), (H, W, r)
    one = dilate_masks(torch.from_numpy(m[4]).cuda(), 3)                    # rank 2 in, rank 2 out; a device tensor
    assert tuple(one.shape) == (H, W) and np.array_equal(one.cpu().numpy(), ref_dilate(m[4], 3))
    u8 = dilate_masks(m[5].astype(np.uint8) * 200, 1)                       # uint8: non-zero is set
    assert np.array_equal(u8.cpu().numpy(), ref_dilate(m[5], 1))


def test_dilate_masks_stack_of_three():
    from neurecon_amd.mesh_cull import dilate_masks
    rng = np.random.default_rng(11)
    m = rng.random((3, H_STD, W_STD)) < np.array([0.01, 0.05, 0.5])[:, None, None]
    for r in (0, 1, 3, 7, 64, W_STD):
        got = dilate_masks(m, r)
        assert np.array_equal(got.cpu().numpy(), ref_dilate(m, r)), r
        assert torch.equal(got, dilate_masks(m, r)), 'a second run differs'
    assert dilate_masks(np.zeros((0, 4, 5), bool), 2).shape == (0, 4, 5)


# ------------------------------------------------------------------------------------------------
# 2. flags against the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('subdiv', [2, 3])
def test_flags_equal_the_rule(subdiv):
    v, f = icosphere(subdiv)
    v = (np.float32(0.8) * v).astype(np.float32)
    poses, K = orbit(4), std_intrinsics()
    masks = hull_scene()[5]                                                # the silhouettes of a 0.5 sphere
    zd, fid = device_frames(v, f, poses, K, H_STD, W_STD)
    for dilate in (0, 2):
        out = views(v, f, poses, K, H_STD, W_STD, masks=masks, dilate=dilate, depth_tol=1e-3)
        ref = ref_view_test(v, poses, K, H_STD, W_STD, masks=ref_dilate(masks, dilate), zdepth=zd, face_id=fid,
                            depth_tol=1e-3)
        fl = out['flags'].cpu().numpy()
        assert np.array_equal(fl, ref['flags']), (subdiv, dilate)
        assert np.array_equal(torch.stack([out['n_in_image'], out['n_in_mask'], out['n_visible']], 1).cpu().numpy(),
                              ref['counts'])
        assert (fl & IN_IMAGE).any()                                       # (out of the image: the hand-made cases)
        for bit in (IN_MASK, VISIBLE):                                     # both answers occur
            assert 0 < ((fl & bit) != 0).sum() < fl.size, bit
        check_counts(out)
        assert same(out, views(v, f, poses, K, H_STD, W_STD, masks=masks, dilate=dilate, depth_tol=1e-3)), 'a second run differs'
    # tensors on the device, int64 faces and uint8 masks go the same way
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    again = views(t(v), t(f).long(), t(poses), t(K), H_STD, W_STD, masks=t(masks.astype(np.uint8)), dilate=2,
                  depth_tol=1e-3)
    assert same(out, again)


def hand_scene():
    """c2w = I, fx = fy = 32, cx = 16, cy = 8, no skew, 33 x 17 pixels: u = 32 x / z + 16 and v = 32 y / z + 8 are
    exact for the coordinates below.  A quad in the plane z = 1 covers the whole image (its depth is exactly 1).
    -> verts, faces, K, H, W, near, names of the probe vertices (after the quad's four)"""
    H, W, near = 17, 33, 2.0 ** -10
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 32
    K[0, 2], K[1, 2] = 16, 8
    f32 = np.float32
    below, above = lambda x: np.nextafter(f32(x), f32(-np.inf)), lambda x: np.nextafter(f32(x), f32(np.inf))
    probes = [
        ('u=0', (-0.5, 0, 1)), ('u=W-1', (0.5, 0, 1)), ('u<0', (below(-0.5), 0, 1)), ('u>W-1', (above(0.5), 0, 1)),
        ('v=0', (0, -0.25, 1)), ('v=H-1', (0, 0.25, 1)), ('v<0', (0, below(-0.25), 1)), ('v>H-1', (0, above(0.25), 1)),
        ('u=4.5', ((4.5 - 16) / 32, 0, 1)), ('u=5.5', ((5.5 - 16) / 32, 0, 1)),
        ('v=2.5', (0, (2.5 - 8) / 32, 1)), ('v=3.5', (0, (3.5 - 8) / 32, 1)),
        ('z<near', (0, 0, below(near))), ('z=near', (0, 0, near)), ('behind', (0, 0, -1)),
        ('nan', (np.nan, 0, 1)), ('inf', (0, np.inf, 1)), ('zinf', (0, 0, np.inf)),
        ('tie', (0.1, 0.1, 1 + 2.0 ** -10)), ('past', (0.1, 0.1, 1 + 2.0 ** -10 + 2.0 ** -23)),
    ]
    quad = [(-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]
    verts = np.array(quad + [p for _, p in probes], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return verts, faces, K, H, W, near, [n for n, _ in probes]


def test_flags_on_hand_made_cases():
    verts, faces, K, H, W, near, names = hand_scene()
    assert float(verts[4 + names.index('past'), 2]) > float(verts[4 + names.index('tie'), 2]) == 1 + 2.0 ** -10
    pose = np.eye(4, dtype=np.float32)[None]
    masks = np.zeros((1, H, W), bool)
    masks[0, :, [4, 6]] = True          # u = 4.5 -> column 4, u = 5.5 -> column 6 (half to even); 5 is unset
    masks[0, [2, 4], :] = True          # v = 2.5 -> row 2, v = 3.5 -> row 4; row 3 is unset but for columns 4 and 6
    masks[0, 8, 16] = masks[0, 8, 0] = masks[0, 8, 32] = True
    tol = 2.0 ** -10
    zd, fid = device_frames(verts, faces, pose, K, H, W, near=near)
    assert (fid >= 0).all() and (zd == 1.0).all()                          # the quad's depth is exactly 1
    out = views(verts, faces, pose, K, H, W, masks=masks, depth_tol=tol, near=near)
    ref = ref_view_test(verts, pose, K, H, W, masks=masks, zdepth=zd, face_id=fid, depth_tol=tol, near=near)
    fl = out['flags'].cpu().numpy()
    assert np.array_equal(fl, ref['flags'])
    check_counts(out)
    got = {n: int(fl[0, 4 + k]) for k, n in enumerate(names)}
    print(got)
    for n in ('u<0', 'u>W-1', 'v<0', 'v>H-1', 'z<near', 'behind', 'nan', 'inf', 'zinf'):
        assert got[n] == 0, n
    for n in ('u=0', 'u=W-1', 'u=4.5', 'u=5.5', 'v=2.5', 'v=3.5', 'z=near'):
        assert got[n] == IN_IMAGE | IN_MASK | VISIBLE, n
    for n in ('v=0', 'v=H-1'):
        assert got[n] == IN_IMAGE | VISIBLE, n                             # column 16 of rows 0 and 16 is unset
    assert got['tie'] & VISIBLE and got['tie'] & IN_IMAGE                  # 1 + 2^-10 <= 1 + depth_tol: a tie is visible
    assert got['past'] & IN_IMAGE and not got['past'] & VISIBLE            # one fp32 step farther is not
    # with depth_tol 0 the quad's own vertices (z = 1, off the image) stay out and the tie is lost
    out0 = views(verts, faces, pose, K, H, W, depth_tol=0.0, near=near)
    assert out0['n_in_mask'] is None and int(out0['n_visible'][4 + names.index('tie')]) == 0
    assert int(out0['n_visible'][4 + names.index('u=0')]) == 1


# ------------------------------------------------------------------------------------------------
# 3. counts, chunks, empty inputs
# ------------------------------------------------------------------------------------------------
def test_counts_chunks_and_empty_inputs():
    v, f, poses, _, _ = sphere_scene(4)
    K = std_intrinsics()
    masks = hull_scene()[5]
    whole = views(v, f, poses, K, H_STD, W_STD, masks=masks, dilate=1, depth_tol=1e-3)
    check_counts(whole)
    assert int(whole['n_in_image'].max()) == 4
    for nbytes in (0, 8 * H_STD * W_STD, 3 * 8 * H_STD * W_STD):          # one, one and three views per chunk
        assert same(whole, views(v, f, poses, K, H_STD, W_STD, masks=masks, dilate=1, depth_tol=1e-3,
                                 max_frame_bytes=nbytes)), nbytes
    # without depth: one call over all views, faces not needed, the same first two bits
    flat = views(v, None, poses, K, H_STD, W_STD, masks=masks, dilate=1)
    assert flat['n_visible'] is None
    assert torch.equal(flat['flags'], whole['flags'] & (IN_IMAGE | IN_MASK))
    assert torch.equal(flat['n_in_mask'], whole['n_in_mask']) and torch.equal(flat['n_in_image'], whole['n_in_image'])
    check_counts(flat)
    bare = views(v, None, poses, K, H_STD, W_STD)
    assert bare['n_in_mask'] is None and bare['n_visible'] is None
    assert torch.equal(bare['flags'], whole['flags'] & IN_IMAGE)
    # no face: nothing is in front of anything, every in-image vertex is visible
    nof = views(v, np.zeros((0, 3), np.int32), poses, K, H_STD, W_STD, depth_tol=0.0)
    assert torch.equal(nof['n_visible'], nof['n_in_image']) and torch.equal(nof['n_in_image'], whole['n_in_image'])
    # no vertex
    nov = views(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), poses, K, H_STD, W_STD, masks=masks, depth_tol=1e-3)
    assert nov['n_in_image'].numel() == 0 and tuple(nov['flags'].shape) == (4, 0)


# ------------------------------------------------------------------------------------------------
# 4. cull_mesh
# ------------------------------------------------------------------------------------------------
def test_cull_mesh_on_the_hull_scene():
    from neurecon_amd.mesh_cull import cull_mesh
    verts, faces, nA, fA, poses, masks = hull_scene()
    K = std_intrinsics()
    normals, colors = sphere_attributes(verts)
    out = cull_mesh(verts, faces, poses, K, H_STD, W_STD, masks=masks, dilate=1, normals=normals, colors=colors)
    assert set(out) == {'verts', 'faces', 'index', 'normals', 'colors', 'kept', 'n_in_image', 'n_in_mask', 'n_visible',
                        'n_views'}
    assert out['kept'].dtype == torch.bool and out['n_visible'] is None and out['n_views'] == 4
    assert np.array_equal(out['kept'].cpu().numpy(), np.arange(len(verts)) < nA)
    assert np.array_equal(out['verts'].cpu().numpy(), verts[:nA]) and np.array_equal(out['faces'].cpu().numpy(), faces[:fA])
    assert np.array_equal(out['index'].cpu().numpy(), np.arange(nA))
    assert np.array_equal(out['normals'].cpu().numpy(), normals[:nA])
    assert np.array_equal(out['colors'].cpu().numpy(), colors[:nA])
    assert (out['n_in_image'][nA:] == 4).all()                             # B is seen by all four and voted out
    # the nearest pixel of a silhouette vertex can be uncovered: without dilation A loses vertices, B stays out
    raw = cull_mesh(dict(verts=verts, faces=faces, normals=normals, colors=None), None, poses, K, H_STD, W_STD, masks=masks)
    kept = raw['kept'].cpu().numpy()
    assert 0 < kept[:nA].sum() < nA and not kept[nA:].any()
    assert raw['colors'] is None and np.array_equal(raw['normals'].cpu().numpy(), normals[raw['index'].cpu().numpy()])
    assert np.array_equal(raw['verts'].cpu().numpy(), verts[kept])
    # the component filter follows the vertex mask: without masks both spheres stay, 'largest' keeps A
    big = cull_mesh(verts, faces, poses, K, H_STD, W_STD, keep='largest')
    assert np.array_equal(big['index'].cpu().numpy(), np.arange(nA)) and big['kept'].all()


def test_cull_mesh_drops_the_far_hemisphere():
    from neurecon_amd.mesh_cull import cull_mesh
    v, f, poses, _, _ = sphere_scene(4)
    K = std_intrinsics()
    zd, fid = device_frames(v, f, poses[:1], K, H_STD, W_STD)
    out = cull_mesh(v, f, poses[:1], K, H_STD, W_STD, depth_tol=1e-3, min_visible=1)
    ref = ref_view_test(v, poses[:1], K, H_STD, W_STD, zdepth=zd, face_id=fid, depth_tol=1e-3)
    kept = out['kept'].cpu().numpy()
    assert np.array_equal(kept, (ref['flags'][0] & VISIBLE) != 0)
    c = facing_cosine(v, poses[0])
    inimg = (ref['flags'][0] & IN_IMAGE) != 0
    back = inimg & (c <= -0.25)
    assert kept[inimg & (c >= 0.25)].all()
    assert np.isinf(ref['zmax'][0][back & kept]).all()                     # what stays of the back touches a miss
    assert 0 < (back & kept).sum() < back.sum() / 2 and not kept[~inimg].any()
    assert out['n_in_mask'] is None and np.array_equal(out['verts'].cpu().numpy(), v[kept])
    # min_visible = 2 with one view leaves nothing: filter_mesh says so
    with pytest.raises(ValueError, match='no vertex'):
        cull_mesh(v, f, poses[:1], K, H_STD, W_STD, depth_tol=1e-3, min_visible=2)


# ------------------------------------------------------------------------------------------------
# 5. the command line
# ------------------------------------------------------------------------------------------------
def test_cli(tmp_path, capsys):
    from neurecon_amd.mesh_cull import cull_mesh, load_cameras_npz, main
    from neurecon_amd.mesh_util import read_ply, write_ply
    verts, faces, nA, fA, poses, masks = hull_scene()
    normals, _ = sphere_attributes(verts)
    write_ply(tmp_path / 'in.ply', verts, faces, normals=normals)
    np.save(tmp_path / 'masks.npy', masks)
    S = np.diag([2.0, 2.0, 2.0, 1.0])
    S[:3, 3] = [10.0, -20.0, 30.0]
    K3 = std_intrinsics().astype(np.float64)[:3, :3]
    cams = {}
    for i, pose in enumerate(poses):
        world = np.eye(4)
        world[:3] = K3 @ np.linalg.inv(pose.astype(np.float64))[:3]
        cams[f'world_mat_{i}'], cams[f'scale_mat_{i}'] = world @ np.linalg.inv(S), S   # P = world_mat @ scale_mat
    np.savez(tmp_path / 'cameras.npz', **cams)
    c2w, K, scale0 = load_cameras_npz(tmp_path / 'cameras.npz')
    api = cull_mesh(read_ply(tmp_path / 'in.ply'), None, c2w, K, H_STD, W_STD, masks=masks, dilate=2)
    assert api['verts'].shape[0] == nA and api['faces'].shape[0] == fA
    args = [str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply'), '--cameras', str(tmp_path / 'cameras.npz'), '--H',
            str(H_STD), '--W', str(W_STD), '--masks', str(tmp_path / 'masks.npy'), '--dilate', '2']
    assert main(args) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (line['views'], line['verts_in'], line['faces_in'], line['verts_out'], line['faces_out']) == \
        (4, len(verts), len(faces), nA, fA)
    got = read_ply(tmp_path / 'out.ply')
    assert np.array_equal(got['verts'], api['verts'].cpu().numpy()) and np.array_equal(got['faces'], api['faces'].cpu().numpy())
    assert np.array_equal(got['normals'], api['normals'].cpu().numpy()) and got['colors'] is None
    # --to-world: the same mesh through scale_mat_0
    args[1] = str(tmp_path / 'world.ply')
    assert main(args + ['--to-world']) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['to_world'] is True and line['verts_out'] == nA
    world = read_ply(tmp_path / 'world.ply')
    want = (api['verts'].cpu().numpy().astype(np.float64) @ S[:3, :3].T + S[:3, 3]).astype(np.float32)
    assert np.array_equal(world['verts'], want) and np.array_equal(world['faces'], got['faces'])
    assert np.abs(world['normals'] - got['normals']).max() <= 2.0 ** -22      # a uniform scale leaves them alone
    # visibility and the component filter go through as well
    vis = cull_mesh(read_ply(tmp_path / 'in.ply'), None, c2w, K, H_STD, W_STD, masks=masks, dilate=2, depth_tol=1e-3,
                    min_visible=2, keep='largest', min_faces=3)
    assert main(args + ['--depth-tol', '1e-3', '--min-visible', '2', '--keep', 'largest', '--min-faces', '3']) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert 0 < line['verts_out'] == vis['verts'].shape[0] < nA and line['faces_out'] == vis['faces'].shape[0]
    assert np.array_equal(read_ply(tmp_path / 'world.ply')['verts'], vis['verts'].cpu().numpy())
