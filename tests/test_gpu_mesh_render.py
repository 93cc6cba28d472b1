"""GPU tests of the mesh renderer (neurecon_amd.mesh_util.render_mesh, libnrhip nr_mesh_render,
neurecon_amd/csrc/nr_meshrender.hip) against the two numpy references of tests/test_mesh_render.py:
(A) `ref_raster`, the rule restated operation for operation (face ids and masks: integer equality), and
(B) `ref_cast`, an independent float64 ray cast (what pins the geometry and the alignment with get_rays)."""
import numpy as np
import pytest
import torch

import weightgen as wg
from helpers import neus_model
from test_gpu_mcubes import _sphere
from test_mesh_render import (AT, H_STD, RT, W_STD, check_against_casts, fan_expected_mask, fan_scene, five_casts,
                              icosphere, ref_raster, sphere_attributes, std_intrinsics, std_pose)

pytestmark = pytest.mark.gpu
MAPS = ('rgb', 'depth', 'depth_z', 'normal', 'mask', 'face_id', 'bary')
COUNTS = ('n_clipped', 'n_degenerate', 'n_large')


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


def render(verts, faces, c2w, K, H, W, **kw):
    from neurecon_amd.mesh_util import render_mesh
    out = render_mesh(verts, faces, c2w, K, H, W, **kw)
    assert set(out) == set(MAPS) | set(COUNTS)
    for k in MAPS:
        assert out[k].is_cuda and tuple(out[k].shape[:2]) == (H, W), k
    assert out['mask'].dtype == torch.bool and out['face_id'].dtype == torch.int32
    assert all(out[k].is_cuda and out[k].dtype == torch.int64 for k in COUNTS)
    return out


def same_bits(a, b, keys=MAPS + ('n_clipped',)):
    return all(torch.equal(a[k], b[k]) for k in keys)


def close(name, got, want, rt=RT, at=AT):
    got, want = got.cpu().numpy().astype(np.float64), np.asarray(want).astype(np.float64)
    err = np.abs(got - want)
    print(f'{name}: max abs err {err.max() if err.size else 0:.3e}')
    assert (err <= rt * np.abs(want) + at).all(), name


def check_against_rule(name, out, ref):
    """face_id / mask: integer equality on every pixel; depth, normal, rgb: RT, AT; bary: 1e-6 absolute"""
    assert np.array_equal(out['face_id'].cpu().numpy(), ref['face_id']), name
    assert np.array_equal(out['mask'].cpu().numpy(), ref['mask']), name
    assert int(out['n_clipped']) == ref['n_clipped'] and int(out['n_degenerate']) == ref['n_degenerate']
    for k in ('depth', 'depth_z', 'normal', 'rgb'):
        close(f'{name} {k}', out[k], ref[k])
    close(f'{name} bary', out['bary'], ref['bary'], 0.0, 1e-6)


@pytest.fixture(scope='module')
def spheres():
    """subdiv -> (verts, faces, normals, colors) of the standard scene's icospheres"""
    out = {}
    for s in (1, 2):
        v, f = icosphere(s)
        out[s] = (v, f) + sphere_attributes(v)
    return out


# ------------------------------------------------------------------------------------------------
# 1. the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('attrs', [False, True])
@pytest.mark.parametrize('subdiv', [1, 2])
def test_device_against_the_rule(spheres, subdiv, attrs):
    v, f, n, c = spheres[subdiv]
    kw = dict(normals=n, colors=c) if attrs else {}
    c2w, K = std_pose(), std_intrinsics()
    out = render(v, f, c2w, K, H_STD, W_STD, **kw)
    ref = ref_raster(v, f, c2w, K, H_STD, W_STD, **kw)
    assert 0 < ref['mask'].sum() < H_STD * W_STD
    check_against_rule(f'{len(f)} faces, attrs {attrs}', out, ref)
    assert same_bits(out, render(v, f, c2w, K, H_STD, W_STD, **kw)), 'a second run differs'
    # tensors on the device, int64 faces and uint8 colours go the same way
    t = lambda a: torch.from_numpy(a).cuda()
    kw2 = dict(normals=t(n), colors=t(c)) if attrs else {}
    assert same_bits(out, render(t(v), t(f).long(), t(c2w), t(K), H_STD, W_STD, **kw2))
    if attrs:
        c8 = np.floor(c.astype(np.float64) * 255 + 0.5).astype(np.uint8)
        check_against_rule('uint8 colours', render(v, f, c2w, K, H_STD, W_STD, normals=n, colors=c8),
                           ref_raster(v, f, c2w, K, H_STD, W_STD, normals=n, colors=c8.astype(np.float32) / np.float32(255)))


def test_fill_rule_on_the_device():
    """shared edges and a shared vertex exactly on pixel samples: each sample of the union belongs to one face"""
    v, f, c2w, K, H, W = fan_scene()
    out = render(v, f, c2w, K, H, W)
    check_against_rule('fan', out, ref_raster(v, f, c2w, K, H, W))
    assert np.array_equal(out['mask'].cpu().numpy(), fan_expected_mask())
    total = sum(int(render(v, f[k:k + 1], c2w, K, H, W)['mask'].sum()) for k in range(len(f)))
    assert total == int(fan_expected_mask().sum())


def test_batched_cameras(spheres):
    v, f, n, c = spheres[1]
    poses = np.stack([std_pose(), std_pose(a=-0.3, b=0.9), std_pose(dist=2.5)])
    out = render(v, f, poses[0], std_intrinsics(), H_STD, W_STD)
    from neurecon_amd.mesh_util import render_mesh
    many = render_mesh(v, f, poses, std_intrinsics(), H_STD, W_STD)
    assert many['depth'].shape == (3, H_STD, W_STD) and many['n_clipped'].shape == (3,)
    assert all(torch.equal(many[k][0], out[k]) for k in MAPS)
    for b in (1, 2):
        ref = ref_raster(v, f, poses[b], std_intrinsics(), H_STD, W_STD)
        assert np.array_equal(many['face_id'][b].cpu().numpy(), ref['face_id'])


# ------------------------------------------------------------------------------------------------
# 2. alignment with get_rays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('subdiv', [1, 2])
def test_device_against_ray_cast_through_get_rays(spheres, subdiv):
    from neurecon_amd.rend_util import get_rays
    v, f, _, _ = spheres[subdiv]
    c2w, K = std_pose(), std_intrinsics()
    ro, rd, _ = get_rays(torch.from_numpy(c2w).cuda(), torch.from_numpy(K).cuda(), H_STD, W_STD)
    assert rd.shape == (H_STD * W_STD, 3)
    centre = (ro[0].double().cpu().numpy(), rd.double().cpu().numpy())
    fs, ds = five_casts(v, f, c2w, K, H_STD, W_STD, centre=centre)
    out = render(v, f, c2w, K, H_STD, W_STD)
    check_against_casts(f'device, {len(f)} faces', out['face_id'].cpu().numpy(), out['depth'].cpu().numpy(), fs, ds)


# ------------------------------------------------------------------------------------------------
# 3. both paths
# ------------------------------------------------------------------------------------------------
def quad_and_triangle():
    """identity pose, the fan scene's camera at 53 x 37: faces 0, 1 = a quad at z = 2 that covers the whole
    frame, face 2 = a small triangle at z = 1 in front of it"""
    _, _, c2w, K, _, _ = fan_scene()
    v = np.array([[-2, -2, 2], [16, -2, 2], [16, 12, 2], [-2, 12, 2], [1.1, 0.6, 1], [2.3, 0.9, 1], [1.4, 1.9, 1]],
                 np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.int32)
    return v, f, c2w, K


def test_both_paths_give_the_same_bits(spheres):
    scenes = [(spheres[1][0], spheres[1][1], std_pose(), std_intrinsics()),
              (spheres[2][0], spheres[2][1], std_pose(), std_intrinsics()), quad_and_triangle()]
    for v, f, c2w, K in scenes:
        default = render(v, f, c2w, K, H_STD, W_STD)
        large = render(v, f, c2w, K, H_STD, W_STD, large_threshold=0)
        small = render(v, f, c2w, K, H_STD, W_STD, large_threshold=2 ** 40)
        mid = render(v, f, c2w, K, H_STD, W_STD, large_threshold=7)
        assert same_bits(default, large) and same_bits(default, small) and same_bits(default, mid)
        assert int(default['mask'].sum()) > 0
        # the thresholds really chose the path: 0 queues every face with a non-empty box, a huge one none
        drawn = ref_raster(v, f, c2w, K, H_STD, W_STD)['n_drawn']
        assert 0 < drawn <= len(f)
        assert int(large['n_large']) == drawn and int(small['n_large']) == 0
        assert int(small['n_large']) <= int(default['n_large']) <= int(mid['n_large']) <= drawn
        assert all(int(r['n_degenerate']) == int(default['n_degenerate']) for r in (large, small, mid))


# ------------------------------------------------------------------------------------------------
# 4. edge cases
# ------------------------------------------------------------------------------------------------
def test_no_faces_and_no_vertices():
    for v, f in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
                 (icosphere(0)[0], np.zeros((0, 3), np.int32))):
        out = render(v, f, std_pose(), std_intrinsics(), H_STD, W_STD, background=(0.1, 0.2, 0.3))
        assert not out['mask'].any() and bool((out['face_id'] == -1).all()) and int(out['n_clipped']) == 0
        for k in ('depth', 'depth_z', 'normal', 'bary'):
            assert not out[k].any(), k
        assert torch.equal(out['rgb'].cpu(), torch.tensor([0.1, 0.2, 0.3]).expand(H_STD, W_STD, 3))


def test_mesh_behind_the_camera(spheres):
    v, f = spheres[1][:2]
    c2w = std_pose(dist=-3.2)                            # the same orientation, the sphere now behind it
    out = render(v, f, c2w, std_intrinsics(), H_STD, W_STD)
    assert not out['mask'].any() and int(out['n_clipped']) == len(f)
    check_against_rule('behind', out, ref_raster(v, f, c2w, std_intrinsics(), H_STD, W_STD))


def test_face_across_the_near_plane_is_dropped_and_counted(spheres):
    v, f = spheres[1][:2]
    c2w, K = std_pose(), std_intrinsics()
    cam = c2w[:3, 3].astype(np.float64)
    fwd = c2w[:3, 2].astype(np.float64)
    extra = np.array([cam + 1.5 * fwd + [0.1, 0, 0], cam + 1.5 * fwd + [0, 0.1, 0], cam - 0.5 * fwd], np.float32)
    v2 = np.concatenate([v, extra])
    f2 = np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    plain, out = render(v, f, c2w, K, H_STD, W_STD), render(v2, f2, c2w, K, H_STD, W_STD)
    assert int(plain['n_clipped']) == 0 and int(out['n_clipped']) == 1
    assert same_bits(plain, out, MAPS)
    # unclipped, the same face (its third vertex in front of the camera) would hide part of the sphere
    v3 = v2.copy()
    v3[-1] = (cam + 1.5 * fwd + [0, 0, 0.1]).astype(np.float32)
    seen = render(v3, f2, c2w, K, H_STD, W_STD)
    assert int(seen['n_clipped']) == 0 and bool((seen['face_id'] == len(f)).any())
    # a non-finite vertex flags its faces too
    v4 = v2.copy()
    v4[-1] = np.nan
    assert same_bits(out, render(v4, f2, c2w, K, H_STD, W_STD))


def test_face_far_outside_the_image():
    """vertices at about +-2.4e5 pixels (within 2^20): the visible part is rendered; beyond 2^20: dropped"""
    _, _, c2w, K, _, _ = fan_scene()
    v = np.array([[-60000, -50000, 2], [60000, -40000, 2], [100, 61000, 2]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    out = render(v, f, c2w, K, H_STD, W_STD)
    check_against_rule('huge face', out, ref_raster(v, f, c2w, K, H_STD, W_STD))
    assert bool(out['mask'].all()) and int(out['n_clipped']) == 0
    close('huge face depth_z', out['depth_z'], np.full((H_STD, W_STD), 2.0))
    out = render(v * np.float32([8, 8, 1]), f, c2w, K, H_STD, W_STD)       # 8 * 6e4 * 8 / 2 = 1.9e6 > 2^20
    assert not out['mask'].any() and int(out['n_clipped']) == 1


def test_quad_behind_a_small_triangle():
    v, f, c2w, K = quad_and_triangle()
    out = render(v, f, c2w, K, H_STD, W_STD)
    check_against_rule('quad + triangle', out, ref_raster(v, f, c2w, K, H_STD, W_STD))
    fid = out['face_id'].cpu().numpy()
    alone = render(v, f[2:], c2w, K, H_STD, W_STD)['mask'].cpu().numpy()
    assert 0 < alone.sum() < 200 and bool(out['mask'].all())
    assert np.array_equal(fid == 2, alone)                     # the triangle wins exactly its own pixels
    assert set(np.unique(fid[~alone]).tolist()) == {0, 1}
    assert ref_raster(v, f[:2], c2w, K, H_STD, W_STD)['cover'].max() == 1      # the quad's diagonal: one face each


def test_duplicate_and_zero_area_faces(spheres):
    v, f = spheres[1][:2]
    c2w, K = std_pose(), std_intrinsics()
    plain = render(v, f, c2w, K, H_STD, W_STD)
    # every face twice: the lower index wins every tie
    twice = render(v, np.concatenate([f, f]), c2w, K, H_STD, W_STD)
    assert same_bits(plain, twice)
    swapped = render(v, np.concatenate([f[::-1], f]), c2w, K, H_STD, W_STD)
    hit = plain['mask']
    assert torch.equal(swapped['depth'], plain['depth'])
    assert torch.equal(swapped['face_id'][hit].long(), len(f) - 1 - plain['face_id'][hit].long())
    # zero-area faces (a repeated index, coincident vertices in front of the sphere) and bad indices are ignored
    p, q = [-0.8, -0.5, -1.0], [-0.9, -0.4, -1.2]
    vz = np.concatenate([v, [p, p, q, p]]).astype(np.float32)
    V = len(v)
    extra = np.array([[0, 0, 1], [3, 3, 3], [V, V + 1, V + 2], [V, V + 1, V + 3], [0, 1, V + 4], [-1, 0, 1]], np.int32)
    out = render(vz, np.concatenate([f, extra]), c2w, K, H_STD, W_STD)
    assert same_bits(plain, out) and int(out['n_degenerate']) == len(extra) and int(plain['n_degenerate']) == 0
    check_against_rule('zero-area', out, ref_raster(vz, np.concatenate([f, extra]), c2w, K, H_STD, W_STD))


def test_permuting_the_faces_changes_only_the_ids(spheres):
    """on the closed icosphere the two faces a ray meets (front and back) lie far apart: no depth tie, so the
    ids map through the permutation on every hit pixel"""
    v, f, n, c = spheres[2]
    c2w, K = std_pose(), std_intrinsics()
    perm = np.random.default_rng(5).permutation(len(f))
    a = render(v, f, c2w, K, H_STD, W_STD, normals=n, colors=c)
    b = render(v, f[perm], c2w, K, H_STD, W_STD, normals=n, colors=c)
    for k in ('depth', 'depth_z', 'mask', 'normal', 'rgb', 'bary'):
        assert torch.equal(a[k], b[k]), k
    hit = a['mask'].cpu().numpy()
    assert np.array_equal(perm[b['face_id'].cpu().numpy()[hit]], a['face_id'].cpu().numpy()[hit])


# ------------------------------------------------------------------------------------------------
# 5. dense and watertight
# ------------------------------------------------------------------------------------------------
def test_dense_mesh_has_no_holes():
    """marching cubes of a sphere at 24^3 seen at 24 x 18: a grid cell (2 / 23) projects to under a pixel
    (28 * (2 / 23) / (3.2 - 0.6) = 0.94), so the faces are sub-pixel"""
    from neurecon_amd.mesh_util import marching_cubes
    vol = torch.from_numpy(_sphere((24, 24, 24), (0.05, -0.02, 0.03), 0.6)).cuda()
    verts, faces = marching_cubes(vol, 0.0, spacing=[2 / 23] * 3, origin=[-1.0] * 3)
    H, W = 18, 24
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1] = 28, 26, 11.7, 8.6, 0.3
    c2w = std_pose()
    out = render(verts, faces, c2w, K, H, W)
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    fs, ds = five_casts(v, f, c2w, K, H, W)
    all_hit, all_miss = (fs >= 0).all(0), (fs < 0).all(0)
    mask, depth = out['mask'].cpu().numpy(), out['depth'].cpu().numpy().astype(np.float64)
    print(f'dense: {len(f)} faces, {int(all_hit.sum())} pixels where all five casts hit, {int(all_miss.sum())} where '
          f'all miss, holes {int((all_hit & ~mask).sum())}, false hits {int((all_miss & mask).sum())}')
    # sphere area / cell face area = 4 pi 0.36 / (2 / 23)^2 ~ 600 cut cells, two faces or more each; the disc of
    # radius 0.6 * 27 / 3.2 ~ 5 pixels holds ~ 80 pixels, most of them a DELTA inside it
    assert len(f) > 1000 and all_hit.sum() > 60
    assert not (all_hit & ~mask).any(), 'a hole'
    assert not (all_miss & mask).any()
    d5 = ds[:, all_hit]
    band = (d5.max(0) - d5.min(0)) + RT * np.abs(d5[0]) + AT
    err = np.abs(depth[all_hit] - ds[0][all_hit])
    print(f'dense: max depth err {err.max():.3e}, widest band {band.max():.3e}')
    assert (err <= band).all()
    assert same_bits(out, render(verts, faces, c2w, K, H, W, large_threshold=0))


# ------------------------------------------------------------------------------------------------
# 6. end to end
# ------------------------------------------------------------------------------------------------
def test_extract_read_render_against_sphere_tracing(tmp_path):
    """extract_mesh -> read_ply -> render_mesh vs the sphere-traced surface depth of the same net through the
    same camera.  Bound: the interpolated surface lies within h (the grid step) of the zero set along the
    normal, hence within h / |n . d| along the ray: |depth difference| <= 2 h where |n . d| >= 0.5."""
    from neurecon_amd.mesh_util import extract_mesh, read_ply, render_mesh
    from neurecon_amd.ray_casting import sphere_tracing_surface_points
    from neurecon_amd.rend_util import get_rays
    m = neus_model(wg.neus_state(seed=1), precision='f16x3')
    N, s = 64, 1.5
    h = s / (N - 1)
    path = tmp_path / 'mesh.ply'
    extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=path, marching='native', coords='sampled',
                 vertex_normals=True, vertex_colors=True, model=m)
    mesh = read_ply(path)
    assert mesh['normals'] is not None and mesh['colors'] is not None and mesh['colors'].dtype == np.uint8
    H, W = 48, 64
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 70, 68, 31.8, 23.3
    c2w = std_pose(dist=2.4)
    out = render_mesh(mesh, None, c2w, K, H, W)
    assert same_bits(out, render_mesh(mesh['verts'], mesh['faces'], c2w, K, H, W, normals=mesh['normals'],
                                      colors=mesh['colors']))
    ro, rd, _ = get_rays(torch.from_numpy(c2w).cuda(), torch.from_numpy(K).cuda(), H, W)
    dirs = torch.nn.functional.normalize(rd, dim=-1)
    with torch.no_grad():
        d_ref, _, hit_ref = sphere_tracing_surface_points(m.implicit_surface, ro, dirs, near=0.0, far=6.0, N_iters=100)
    d_ref, hit_ref = d_ref.reshape(H, W), hit_ref.reshape(H, W)
    both = out['mask'] & hit_ref
    cos = (out['normal'] * dirs.reshape(H, W, 3)).sum(-1).abs()
    judged = both & (cos >= 0.5)
    err = (out['depth'] - d_ref).abs()[judged]
    n_hit = int((out['mask'] | hit_ref).sum())
    print(f'end to end: {len(mesh["faces"])} faces, {n_hit} hit pixels, {int(both.sum())} hit by both, '
          f'{int(judged.sum())} judged, max |d depth| {float(err.max()):.3e}, 2 h = {2 * h:.3e}')
    assert n_hit > 100 and int(judged.sum()) >= 0.6 * n_hit          # enough pixels for the 60 % to mean something
    assert float(err.max()) <= 2 * h
    rgb = out['rgb'][out['mask']]
    assert float(rgb.min()) >= 0 and float(rgb.max()) <= 1 and float(rgb.std()) > 0
    assert bool((out['rgb'][~out['mask']] == 1).all())
