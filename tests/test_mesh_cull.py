"""CPU checks of mesh culling (neurecon_amd.mesh_cull, nr_meshcull.hip): the numpy restatement of the two rules
(tests/mesh_cull_ref.py) that the GPU tests compare the device against, checked here against scipy, a box-count
restatement, analytic visibility on a sphere and the visual hull of a known scene; load_K_Rt_from_P; and the
argument checks of the C-ABI and the Python layer.  No GPU: the library loads without one."""
import ctypes
import os

import numpy as np
import pytest

from mesh_cull_ref import IN_IMAGE, IN_MASK, VISIBLE, ref_dilate, ref_project, ref_view_test
from test_mesh_render import H_STD, W_STD, icosphere, ref_raster, std_intrinsics, std_pose


# ------------------------------------------------------------------------------------------------
# scenes (shared with tests/test_gpu_mesh_cull.py)
# ------------------------------------------------------------------------------------------------
def orbit(n):
    """n cameras around the origin -> [n, 4, 4] float32"""
    return np.stack([std_pose(3.2, a=0.7 + 2 * np.pi * k / n, b=-0.4 + 0.25 * np.sin(k)) for k in range(n)])


_FRAMES = {}


def depth_frames(key, verts, faces, poses):
    """ref_raster's depth_z / face_id of each pose, computed once per key -> ([B, H, W] float32, [B, H, W] int32)"""
    if key not in _FRAMES:
        fr = [ref_raster(verts, faces, p, std_intrinsics(), H_STD, W_STD) for p in poses]
        _FRAMES[key] = (np.stack([f['depth_z'] for f in fr]), np.stack([f['face_id'] for f in fr]))
    return _FRAMES[key]


def sphere_scene(n):
    """0.8 icosphere(3) (642 vertices) seen by orbit(n) -> verts, faces, poses, depth_z, face_id"""
    v, f = icosphere(3)
    v = (np.float32(0.8) * v).astype(np.float32)
    poses = orbit(n)
    zd, fid = depth_frames(('sphere', n), v, f, poses)
    return v, f, poses, zd, fid


def facing_cosine(verts, pose):
    """cosine between the sphere's normal at each vertex and the direction to the camera"""
    p = verts.astype(np.float64)
    n = p / np.linalg.norm(p, axis=1, keepdims=True)
    d = pose[:3, 3].astype(np.float64)[None] - p
    return (n * d).sum(1) / np.linalg.norm(d, axis=1)


def hull_scene():
    """A = 0.5 icosphere(3), B = 0.1 icosphere(2) + (0.8, 0.1, 0.15); four cameras; the masks are the silhouettes
    of A alone -> verts (A's first), faces, number of A's vertices and faces, poses, masks bool [4, H, W]"""
    va, fa = icosphere(3)
    vb, fb = icosphere(2)
    va = (np.float32(0.5) * va).astype(np.float32)
    vb = (np.float32(0.1) * vb + np.array([0.8, 0.1, 0.15], np.float32)).astype(np.float32)
    poses = orbit(4)
    _, fid = depth_frames('hull', va, fa, poses)
    verts = np.concatenate([va, vb])
    faces = np.concatenate([fa, fb + len(va)]).astype(np.int32)
    return verts, faces, len(va), len(fa), poses, fid >= 0


# ------------------------------------------------------------------------------------------------
# 1. the dilation rule
# ------------------------------------------------------------------------------------------------
def box_count_dilate(mask, r):
    """the definition, through an integral image: set iff the clipped (2 r + 1)^2 window holds a set pixel"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = m.cumsum(0).cumsum(1)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    j0, j1 = np.maximum(j - r, 0), np.minimum(j + r, H - 1) + 1
    i0, i1 = np.maximum(i - r, 0), np.minimum(i + r, W - 1) + 1
    return (S[j1, i1] - S[j0, i1] - S[j1, i0] + S[j0, i0]) > 0


def dilation_masks():
    rng = np.random.default_rng(5)
    return dict(random=rng.random((H_STD, W_STD)) < 0.02, empty=np.zeros((H_STD, W_STD), bool),
                full=np.ones((H_STD, W_STD), bool))


@pytest.mark.parametrize('r', [0, 1, 3, 40, 60])
def test_dilation_rule(r):
    ndimage = pytest.importorskip('scipy.ndimage')
    for name, m in dilation_masks().items():
        got = ref_dilate(m, r)
        assert got.dtype == bool and got.shape == m.shape
        want = ndimage.binary_dilation(m, structure=np.ones((2 * r + 1, 2 * r + 1), bool))
        assert np.array_equal(got, want), (name, r)
        assert np.array_equal(got, box_count_dilate(m, r)), (name, r)
        assert np.array_equal(ref_dilate(m.astype(np.uint8) * 7, r), got)          # non-zero is set
    m = dilation_masks()['random']
    assert 0 < m.sum() < m.size and np.array_equal(ref_dilate(m, 0), m)
    stack = np.stack([m, m[::-1], np.zeros_like(m)])
    assert np.array_equal(ref_dilate(stack, r), np.stack([ref_dilate(s, r) for s in stack]))


# ------------------------------------------------------------------------------------------------
# 2. the visibility rule against analytic visibility on a sphere
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 3, 4])
def test_visibility_rule_on_a_sphere(n):
    v, f, poses, zd, fid = sphere_scene(n)
    assert len(v) == 642
    K = std_intrinsics()
    out = ref_view_test(v, poses, K, H_STD, W_STD, zdepth=zd, face_id=fid, depth_tol=1e-3)
    out0 = ref_view_test(v, poses, K, H_STD, W_STD, zdepth=zd, face_id=fid, depth_tol=0.0)
    for b in range(n):
        c = facing_cosine(v, poses[b])
        inimg = (out['flags'][b] & IN_IMAGE) != 0
        vis = (out['flags'][b] & VISIBLE) != 0
        front, back = inimg & (c >= 0.25), inimg & (c <= -0.25)
        lost0 = int((front & ((out0['flags'][b] & VISIBLE) == 0)).sum())
        share = float((front | back).sum()) / max(int(inimg.sum()), 1)
        print(f'view {b}/{n}: {int(inimg.sum())} in image, {int(front.sum())} front ({int((front & ~vis).sum())} lost, '
              f'{lost0} with depth_tol 0), {int(back.sum())} back ({int((back & vis).sum())} reported visible), '
              f'judged share {share:.3f}')
        assert inimg.sum() > 0 and (vis <= inimg).all()
        assert (vis[front]).all()                                # what faces the camera is visible
        assert np.isinf(out['zmax'][b][back & vis]).all()        # a back vertex passes only through a miss
        assert share >= 0.7
    assert np.array_equal(out['counts'][:, 0], ((out['flags'] & IN_IMAGE) != 0).sum(0))
    assert np.array_equal(out['counts'][:, 2], ((out['flags'] & VISIBLE) != 0).sum(0))
    assert (out['counts'][:, 1] == 0).all()                      # no masks: nothing is in a mask


# ------------------------------------------------------------------------------------------------
# 3. the hull rule
# ------------------------------------------------------------------------------------------------
def hull_kept(counts):
    return counts[:, 1] == counts[:, 0]


def test_hull_rule():
    verts, faces, nA, _, poses, masks = hull_scene()
    K = std_intrinsics()
    kept = {}
    for r in (0, 1, 2):
        out = ref_view_test(verts, poses, K, H_STD, W_STD, masks=ref_dilate(masks, r))
        assert (out['counts'][nA:, 0] == 4).all()                # every vertex of B is in all four images
        assert ((out['flags'] & IN_MASK) <= 2 * (out['flags'] & IN_IMAGE)).all()
        kept[r] = hull_kept(out['counts'])
        print(f'dilate {r}: {int(kept[r][:nA].sum())}/{nA} of A kept, {int(kept[r][nA:].sum())}/{len(verts) - nA} of B')
    for r in (1, 2):
        assert kept[r][:nA].all() and not kept[r][nA:].any()     # exactly A
    assert 0 < kept[0][:nA].sum() < nA                           # a silhouette vertex's nearest pixel can be uncovered
    assert not kept[0][nA:].any()


# ------------------------------------------------------------------------------------------------
# 4. load_K_Rt_from_P, load_cameras_npz
# ------------------------------------------------------------------------------------------------
def _known_camera(seed):
    rng = np.random.default_rng(seed)
    K = np.array([[2892.3, 0.7 + seed, 823.2], [0, 2883.2, 619.1], [0, 0, 1.0]])
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R = q * np.sign(np.linalg.det(q))                            # a rotation, world -> camera
    c = rng.normal(size=3) * 2
    return K, R, c, K @ np.concatenate([R, -(R @ c)[:, None]], 1)


def _rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()


@pytest.mark.parametrize('scale', [1.0, 3.7, -0.02])
def test_load_K_Rt_from_P(scale):
    from neurecon_amd.rend_util import load_K_Rt_from_P
    for seed in range(4):
        K, R, c, P = _known_camera(seed)
        intr, pose = load_K_Rt_from_P(scale * P)
        assert intr.shape == (4, 4) and intr.dtype == np.float64 and pose.shape == (4, 4) and pose.dtype == np.float32
        assert intr[2, 2] == 1.0 and (np.diag(intr) > 0).all() and intr[1, 0] == 0 and intr[2, 0] == 0 and intr[2, 1] == 0
        assert np.array_equal(intr[3], [0, 0, 0, 1]) and np.array_equal(intr[:3, 3], [0, 0, 0])
        assert np.array_equal(pose[3], [0, 0, 0, 1])
        assert _rel(intr[:3, :3], K) <= 1e-9
        assert np.linalg.det(pose[:3, :3].astype(np.float64)) > 0
        # K comes back in float64.  The pose is the reference's float32: a value within 1e-9 of the true one,
        # rounded to float32, lies within one float32 step of the rounded true one (entries of R are <= 1 in
        # magnitude, so a step is <= 2^-23; the centre's steps are relative to its largest entry) plus the 1e-9
        assert np.abs(pose[:3, :3].astype(np.float64) - R.T).max() <= 2.0 ** -23 + 1e-9
        assert np.abs(pose[:3, 3].astype(np.float64) - c).max() <= (2.0 ** -23 + 1e-9) * np.abs(c).max()
        # and in float64, before that rounding: M = s K R with the recovered K, so R follows from P itself
        M = scale * P[:, :3]
        s = np.cbrt(np.linalg.det(M) / np.linalg.det(intr[:3, :3]))
        assert _rel(np.linalg.solve(s * intr[:3, :3], M), R) <= 1e-9
        assert _rel(-np.linalg.solve(M, scale * P[:, 3]), c) <= 1e-9
    with pytest.raises(ValueError, match=r'\[3, 4\]'):
        load_K_Rt_from_P(np.eye(4))


def test_load_cameras_npz(tmp_path):
    from neurecon_amd.mesh_cull import load_cameras_npz
    from neurecon_amd.rend_util import load_K_Rt_from_P
    data, want = {}, []
    K3 = np.array([[2892.3, 0.7, 823.2], [0, 2883.2, 619.1], [0, 0, 1.0]])
    for i, pose in enumerate(orbit(3)):                          # cameras that look at the origin from 3.2
        world = np.eye(4)
        world[:3] = 1.7 * K3 @ np.linalg.inv(pose.astype(np.float64))[:3]
        scale = np.diag([1.5 + i, 1.5 + i, 1.5 + i, 1.0])
        scale[:3, 3] = [0.1 * i, -0.2, 0.3]
        data[f'world_mat_{i}'], data[f'scale_mat_{i}'] = world, scale
        want.append(load_K_Rt_from_P((world.astype(np.float32) @ scale.astype(np.float32))[:3, :4]))
    path = tmp_path / 'cameras.npz'
    np.savez(path, **data)
    c2w, K, scale0 = load_cameras_npz(path)
    assert c2w.shape == (3, 4, 4) and c2w.dtype == np.float32 and K.shape == (3, 4, 4) and K.dtype == np.float64
    assert np.array_equal(scale0, data['scale_mat_0']) and scale0.dtype == np.float64
    for i in range(3):
        assert np.array_equal(K[i], want[i][0]) and np.array_equal(c2w[i], want[i][1])
    # the cameras see what P projects: a point of the normalised space lands on the same pixel either way
    x = np.array([0.1, -0.2, 0.05])
    for i in range(3):
        P = (data[f'world_mat_{i}'] @ data[f'scale_mat_{i}'])[:3]
        h = P @ np.append(x, 1.0)
        z, u, v = ref_project(x[None].astype(np.float32), c2w[i], K[i])
        assert z[0] > 0 and abs(u[0] - h[0] / h[2]) <= 2e-2 and abs(v[0] - h[1] / h[2]) <= 2e-2   # fp32 pose, 3000 px focal
    c2w2, _, _ = load_cameras_npz(path, n_views=2)
    assert np.array_equal(c2w2, c2w[:2])
    with pytest.raises(ValueError, match='lacks'):
        load_cameras_npz(path, n_views=4)


# ------------------------------------------------------------------------------------------------
# 5. the C-ABI and the Python layer without a GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from neurecon_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def _view_args(V=100, n_views=3, H=H_STD, W=W_STD):
    """valid arguments with fake device pointers: the checks come before any HIP call"""
    from neurecon_amd import _lib
    a = _lib.NrMeshViewArgs()
    a.verts, a.V, a.n_views, a.cams, a.H, a.W = 0x1000, V, n_views, 0x2000, H, W
    a.masks, a.zdepth, a.face_id, a.depth_tol = 0x3000, 0x4000, 0x5000, 1e-3
    a.flags, a.counts, a.accumulate = 0x6000, 0x7000, 0
    return a


def test_view_test_checks_arguments_without_gpu(lib):
    def call(a):
        return lib.nr_mesh_view_test(None if a is None else ctypes.byref(a), None), lib.nr_last_error().decode()
    rc, msg = call(None)
    assert rc == -1 and 'null argument' in msg
    for kw in (dict(V=-1), dict(n_views=-1)):
        rc, msg = call(_view_args(**kw))
        assert rc == -1 and 'negative' in msg
    rc, msg = call(_view_args(V=2 ** 31))
    assert rc == -1 and 'INT32_MAX' in msg
    for H, W in ((0, W_STD), (H_STD, -2)):
        rc, msg = call(_view_args(H=H, W=W))
        assert rc == -1 and 'H and W' in msg
    rc, msg = call(_view_args(H=1 << 16, W=1 << 15))                      # H W = 2^31
    assert rc == -1 and '2^31' in msg
    for field in ('zdepth', 'face_id'):
        a = _view_args()
        setattr(a, field, None)
        rc, msg = call(a)
        assert rc == -1 and 'together' in msg, field
    for tol in (-1e-9, float('nan'), float('inf')):
        a = _view_args()
        a.depth_tol = tol
        rc, msg = call(a)
        assert rc == -1 and 'depth_tol' in msg, tol
    a = _view_args()
    a.cams = None
    rc, msg = call(a)
    assert rc == -1 and 'cams' in msg
    a = _view_args()
    a.verts = None
    assert call(a)[0] == -1
    a = _view_args()
    a.accumulate = 2
    assert call(a)[0] == -1
    # nothing to do is no error and launches nothing: no vertex, and no view with nothing to clear
    assert call(_view_args(V=0))[0] == 0
    a = _view_args(n_views=0)
    a.cams, a.accumulate = None, 1
    assert call(a)[0] == 0


def test_mask_dilate_checks_arguments_without_gpu(lib):
    ws = lib.nr_mask_dilate_workspace_bytes
    assert ws(-1, 1, 1) == 0 and ws(1, 0, 1) == 0 and ws(1, 1, 0) == 0 and ws(1, 1 << 16, 1 << 15) == 0
    assert ws(1 << 12, 1 << 10, 1 << 10) == 0                              # B H W = 2^32
    assert ws(0, 5, 5) == 0                                                # nothing to hold
    for B, H, W in ((1, 1, 1), (3, H_STD, W_STD), (64, 1200, 1600)):
        assert B * H * W <= ws(B, H, W) < B * H * W + 256 and ws(B, H, W) % 256 == 0

    def call(B=2, H=H_STD, W=W_STD, r=3, src=0x10000, dst=0x20000, wsp=0x30000, nbytes=None):
        nbytes = ws(max(B, 0), max(H, 1), max(W, 1)) if nbytes is None else nbytes
        return lib.nr_mask_dilate(src, dst, B, H, W, r, wsp, nbytes, None), lib.nr_last_error().decode()
    for kw, text in ((dict(H=0), 'H and W'), (dict(W=-1), 'H and W'), (dict(B=-1), 'B must'), (dict(r=-1), 'radius'),
                     (dict(r=1 << 15), 'radius'), (dict(H=1 << 16, W=1 << 15), '2^31'), (dict(src=None), 'null'),
                     (dict(dst=None), 'null'), (dict(dst=0x10000), 'alias'), (dict(dst=0x10000 + 2 * H_STD * W_STD - 1), 'alias')):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    rc, msg = call(nbytes=ws(2, H_STD, W_STD) - 1)
    assert rc == -4 and 'workspace' in msg
    assert call(wsp=None)[0] == -4
    assert call(B=0, src=None, dst=None, wsp=None)[0] == 0                 # an empty stack: nothing to do


def test_python_layer_refuses_bad_input_before_any_work():
    """every check below comes before the first touch of a device: they hold with and without a GPU"""
    import torch
    from neurecon_amd.mesh_cull import cull_mesh, dilate_masks, vertex_views
    verts, faces = icosphere(0)
    poses, K = orbit(2), std_intrinsics()
    good = np.ones((2, H_STD, W_STD), bool)
    for fn in (vertex_views, cull_mesh):
        for bad in (np.ones((3, H_STD, W_STD), bool), np.ones((2, H_STD + 1, W_STD), bool),
                    np.ones((2, H_STD, W_STD - 1), bool), np.ones((H_STD, W_STD), bool)):
            with pytest.raises(ValueError, match='masks must be'):
                fn(verts, faces, poses, K, H_STD, W_STD, masks=bad)
        with pytest.raises(ValueError, match='masks must be'):
            fn(verts, faces, poses, K, H_STD, W_STD, masks=good.astype(np.float32))
        with pytest.raises(ValueError, match='dilate'):
            fn(verts, faces, poses, K, H_STD, W_STD, masks=good, dilate=-1)
        for tol in (-1e-3, float('nan')):
            with pytest.raises(ValueError, match='depth_tol'):
                fn(verts, faces, poses, K, H_STD, W_STD, depth_tol=tol)
        with pytest.raises(ValueError, match='H, W'):
            fn(verts, faces, poses, K, 0, W_STD)
        with pytest.raises(ValueError, match='c2w'):
            fn(verts, faces, poses[:, :3], K, H_STD, W_STD)
    with pytest.raises(ValueError, match='faces'):
        vertex_views(verts, None, poses, K, H_STD, W_STD, depth_tol=1e-3)
    with pytest.raises(ValueError, match='faces'):
        cull_mesh(verts, None, poses, K, H_STD, W_STD)
    with pytest.raises(ValueError, match='keep'):
        cull_mesh(verts, faces, poses, K, H_STD, W_STD, keep='biggest')
    with pytest.raises(ValueError, match='normals'):
        cull_mesh(verts, faces, poses, K, H_STD, W_STD, normals=verts[:5])
    for r in (-1, 1 << 15, 1.5):
        with pytest.raises(ValueError, match='radius'):
            dilate_masks(good, r)
    with pytest.raises(ValueError, match='masks must be'):
        dilate_masks(np.ones((2, 2, 3, 3), bool), 1)
    if not torch.cuda.is_available():                                      # no device: the module's usual error
        with pytest.raises(RuntimeError, match='GPU'):
            vertex_views(verts, faces, poses, K, H_STD, W_STD, masks=good)
        with pytest.raises(RuntimeError, match='GPU'):
            dilate_masks(good, 1)
