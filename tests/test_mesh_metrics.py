"""CPU tests of the mesh metrics (neurecon_amd/mesh_metrics.py): the numpy restatement of the two device rules
(tests/mesh_metrics_ref.py) against independent answers, `metrics_from_distances` on hand-made arrays,
`read_ply_points`, and the C-ABI argument checks and workspace formulas with fake pointers (the checks come
before any HIP call).  The device itself is compared with the restatement in tests/test_gpu_mesh_metrics.py."""
import ctypes
import math
import os

import numpy as np
import pytest

import mesh_metrics_ref as ref


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def test_brute_force_matches_ckdtree():
    spatial = pytest.importorskip('scipy.spatial')
    rng = np.random.default_rng(0)
    p = rng.standard_normal((3000, 3)).astype(np.float32)
    q = rng.standard_normal((500, 3)).astype(np.float32)
    idx, d2 = ref.brute_nn(p, q)
    d, j = spatial.cKDTree(p.astype(np.float64)).query(q.astype(np.float64))
    assert np.all(np.abs(np.sqrt(d2) - d) <= 1e-12 * d)
    assert np.array_equal(idx, j)      # no exact ties in random data


def test_brute_force_rule():
    p = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [-1, 0, 0]], np.float32)
    q = np.array([[0.9, 0, 0], [0.5, 0, 0], [np.nan, 1, 1], [-3, 0, 0], [0, 0, -np.inf]], np.float32)
    idx, d2 = ref.brute_nn(p, q)
    assert idx.tolist() == [1, 0, -1, 5, -1]                # duplicate 1 / 2: the smaller; 0.5: tie 0 / 1 -> 0
    assert d2[1] == 0.25 and d2[3] == 4.0 and np.isinf(d2[[2, 4]]).all()
    idx, d2 = ref.brute_nn(p, q, max_dist=2.0)
    assert idx.tolist() == [1, 0, -1, 5, -1]                # d2 == max_dist^2 is kept
    idx, d2 = ref.brute_nn(p, q, max_dist=np.nextafter(2.0, 0.0))
    assert idx.tolist() == [1, 0, -1, -1, -1] and np.isinf(d2[3])
    for pts in (np.zeros((0, 3), np.float32), p[3:5]):      # no point, no finite point
        idx, d2 = ref.brute_nn(pts, q)
        assert (idx == -1).all() and np.isinf(d2).all()
    assert ref.brute_nn(p, np.zeros((0, 3)))[0].shape == (0,)
    a, b = ref.brute_nn(p, np.repeat(q, 100, 0), chunk=7)   # the chunking changes nothing
    assert np.array_equal(a, np.repeat(ref.brute_nn(p, q)[0], 100))


def test_exact_prefix_is_fsum():
    a = np.abs(np.random.default_rng(1).standard_normal(300)) * 10.0 ** np.random.default_rng(2).integers(-12, 12, 300)
    a[::7] = 0.0
    want = [math.fsum(a[:i + 1].tolist()) for i in range(len(a))]
    assert ref.exact_prefix(a).tolist() == want


def test_sampler_restatement():
    """a unit right triangle and a degenerate face beside it: every sample inside the triangle, stratified, the
    zero-area face never chosen, the end-of-cdf fallback names the last face with positive area"""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    faces = np.array([[3, 3, 3], [0, 1, 2], [0, 0, 1], [2, 1, 0], [1, 1, 1]], np.int32)
    areas, status = ref.face_areas(verts, faces)
    assert areas.tolist() == [0.0, 0.5, 0.0, 0.5, 0.0] and status == 0
    cdf = np.cumsum(areas)
    n = 1000
    u = np.random.default_rng(3).random((n, 3))
    u[-1, 0] = np.nextafter(1.0, 0.0)
    pts, face = ref.sample_ref(verts, faces, cdf, u)
    assert set(face.tolist()) == {1, 3} and (face[:n // 2] == 1).all() and (face[n // 2:] == 3).all()
    assert pts.dtype == np.float32 and (pts >= 0).all() and (pts[:, 0] + pts[:, 1] <= 1 + 1e-6).all()
    assert (pts[:, 2] == 0).all()
    # t == total exactly: searchsorted runs off the end, the fallback picks face 3, not the trailing face 4
    pts, face = ref.sample_ref(verts, faces, cdf, np.array([[1.0, 0.25, 0.25]]))
    assert face.tolist() == [3]
    areas, status = ref.face_areas(verts, np.array([[0, 1, 4], [0, 1, -1], [0, 1, 2]]))
    assert areas.tolist() == [0.0, 0.0, 0.5] and status == 1
    bad = verts.copy()
    bad[2, 1] = np.inf
    areas, status = ref.face_areas(bad, faces)
    assert areas.tolist() == [0.0] * 5 and status == 2


# ------------------------------------------------------------------------------------------------
# metrics_from_distances
# ------------------------------------------------------------------------------------------------
def test_metrics_known_answers():
    from neurecon_amd.mesh_metrics import metrics_from_distances
    dp = np.array([0.1, 0.2, 0.3, 5.0])
    dg = np.array([0.2, 0.4, np.inf])
    m = metrics_from_distances(dp, dg, max_dist=1.0, thresholds=(0.2, 0.05, 10.0))
    assert m['accuracy'] == pytest.approx(0.2, rel=1e-15) and m['completeness'] == pytest.approx(0.3, rel=1e-15)
    assert m['chamfer'] == pytest.approx(0.25, rel=1e-15)
    assert (m['n_pred'], m['n_pred_used'], m['n_pred_excluded']) == (4, 3, 1)      # 5.0 is excluded, not clipped
    assert (m['n_gt'], m['n_gt_used'], m['n_gt_excluded']) == (3, 2, 1)
    assert m['thresholds'] == [0.2, 0.05, 10.0]
    assert m['precision'] == [0.5, 0.0, 1.0]                # a distance equal to the threshold counts
    assert m['recall'] == [1 / 3, 0.0, 2 / 3]
    assert m['fscore'][0] == pytest.approx(2 * 0.5 / 3 / (0.5 + 1 / 3), rel=1e-15)
    assert m['fscore'][1] == 0.0                            # both 0: 0, not 0 / 0
    assert m['fscore'][2] == pytest.approx(2 * (2 / 3) / (1 + 2 / 3), rel=1e-15)
    # a distance equal to max_dist is excluded (< max_dist); without max_dist every finite distance counts
    m = metrics_from_distances(np.array([1.0, 3.0]), np.array([2.0]), max_dist=3.0)
    assert m['accuracy'] == 1.0 and m['n_pred_excluded'] == 1 and m['precision'] == []
    m = metrics_from_distances(dp, dg)
    assert m['accuracy'] == pytest.approx(1.4, rel=1e-15) and m['completeness'] == pytest.approx(0.3, rel=1e-15)
    assert m['n_gt_excluded'] == 1 and m['max_dist'] is None


def test_metrics_empty_sides_and_input_kinds():
    import torch
    from neurecon_amd.mesh_metrics import metrics_from_distances
    m = metrics_from_distances(np.zeros(0), np.array([0.5]), max_dist=1.0, thresholds=(1.0,))
    assert math.isnan(m['accuracy']) and m['completeness'] == 0.5 and math.isnan(m['chamfer'])
    assert math.isnan(m['precision'][0]) and m['recall'] == [1.0] and math.isnan(m['fscore'][0])
    m = metrics_from_distances([], [], thresholds=(1.0,))
    assert math.isnan(m['chamfer']) and m['n_pred'] == 0 and m['n_gt'] == 0
    m = metrics_from_distances(np.array([2.0]), np.array([3.0]), max_dist=1.0)     # nothing under max_dist
    assert math.isnan(m['accuracy']) and m['n_pred_excluded'] == 1
    a = metrics_from_distances(np.array([0.1, 0.7]), np.array([0.3]), max_dist=1.0, thresholds=(0.5,))
    b = metrics_from_distances(torch.tensor([0.1, 0.7], dtype=torch.float64), torch.tensor([0.3], dtype=torch.float64),
                               max_dist=1.0, thresholds=[0.5])
    assert a == b and isinstance(a['accuracy'], float) and isinstance(a['n_pred'], int)


# ------------------------------------------------------------------------------------------------
# read_ply_points
# ------------------------------------------------------------------------------------------------
def _cloud(n=17, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)


def test_read_ply_points_binary_vertex_only(tmp_path):
    from neurecon_amd.mesh_metrics import read_ply_points
    from neurecon_amd.mesh_util import read_ply
    pts, nrm = _cloud()
    rec = np.empty(len(pts), dtype=[('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('q', 'u1'), ('nx', '<f4'), ('ny', '<f4'),
                                    ('nz', '<f4')])
    for k, n in enumerate('xyz'):
        rec[n], rec['n' + n] = pts[:, k], nrm[:, k]
    rec['q'] = 7
    path = tmp_path / 'cloud.ply'
    header = (f'ply\nformat binary_little_endian 1.0\ncomment a cloud\nelement vertex {len(pts)}\nproperty float x\n'
              'property float y\nproperty float z\nproperty uchar q\nproperty float nx\nproperty float ny\n'
              'property float nz\nend_header\n')
    path.write_bytes(header.encode() + rec.tobytes())
    out = read_ply_points(path)
    assert np.array_equal(out['points'], pts) and np.array_equal(out['normals'], nrm)
    assert out['points'].dtype == np.float32
    with pytest.raises(ValueError, match='vertex and face'):          # read_ply stays as it is: no faces, no mesh
        read_ply(path)
    path.write_bytes(header.encode() + rec.tobytes()[:-1])
    with pytest.raises(ValueError, match='truncated'):
        read_ply_points(path)
    # double coordinates, no normals
    rec = np.empty(3, dtype=[('x', '<f8'), ('y', '<f8'), ('z', '<f8')])
    rec['x'], rec['y'], rec['z'] = [1, 2, 3], [4, 5, 6], [7, 8, 9]
    path.write_bytes(b'ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty double y\n'
                     b'property double z\nend_header\n' + rec.tobytes())
    out = read_ply_points(path)
    assert out['points'].tolist() == [[1, 4, 7], [2, 5, 8], [3, 6, 9]] and out['normals'] is None


def test_read_ply_points_ascii_and_written_mesh(tmp_path):
    from neurecon_amd.mesh_metrics import read_ply_points
    from neurecon_amd.mesh_util import write_ply
    pts, nrm = _cloud(5)
    path = tmp_path / 'a.ply'
    body = '\n'.join(' '.join(repr(float(x)) for x in row) for row in pts)
    path.write_text(f'ply\nformat ascii 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n'
                    f'end_header\n{body}\n')
    out = read_ply_points(path)
    assert np.array_equal(out['points'], pts) and out['normals'] is None
    path.write_text(f'ply\nformat ascii 1.0\nelement vertex 6\nproperty float x\nproperty float y\nproperty float z\n'
                    f'end_header\n{body}\n')
    with pytest.raises(ValueError, match='truncated'):
        read_ply_points(path)
    # a mesh written by write_ply: the faces that follow are not read
    faces = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    for kw in (dict(), dict(normals=nrm), dict(normals=nrm, colors=np.full((5, 3), 9, np.uint8))):
        write_ply(path, pts, faces, **kw)
        out = read_ply_points(path)
        assert np.array_equal(out['points'], pts)
        assert (out['normals'] is None) if 'normals' not in kw else np.array_equal(out['normals'], nrm)


@pytest.mark.parametrize('header, match', [
    ('ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n', 'first element'),
    ('ply\nformat ascii 1.0\nend_header\n', 'first element'),
    ('ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nend_header\n', 'x, y, z'),
    ('ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n'
     'property list uchar int k\nend_header\n', 'scalar'),
    ('ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n'
     'end_header\n', 'big-endian'),
    ('plx\n', 'not a PLY'),
])
def test_read_ply_points_rejections(tmp_path, header, match):
    from neurecon_amd.mesh_metrics import read_ply_points
    path = tmp_path / 'bad.ply'
    path.write_text(header)
    with pytest.raises(ValueError, match=match):
        read_ply_points(path)


def test_default_cell_size_respects_the_cell_cap():
    from neurecon_amd.mesh_metrics import default_cell_size
    for lo, hi, n in (((0, 0, 0), (1, 1, 1), 1 << 20), ((0, 0, 0), (2, 1, 0), 1000), ((0, 0, 0), (3, 0, 0), 64),
                      ((1, 1, 1), (1, 1, 1), 10), ((-5, 0, 2), (5, 1e-3, 2.5), 10 ** 7), ((0, 0, 0), (1, 1, 1), 0)):
        h = default_cell_size(lo, hi, n)
        assert h > 0 and math.isfinite(h)
        cells = math.prod(math.floor((b - a) / h) + 1 for a, b in zip(lo, hi))
        assert cells <= max(1, min(4 * n, 1 << 26)), (lo, hi, n, h, cells)
    # points on a plane: about 8 per cell
    h = default_cell_size((0, 0, 0), (1, 1, 0), 80000)
    assert h == pytest.approx(0.01)


# ------------------------------------------------------------------------------------------------
# C ABI: the argument checks come before any HIP call, so fake pointers are never dereferenced
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from neurecon_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


A, B, C, D, E, G, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x100000
INF = float('inf')


def _err(lib):
    return lib.nr_last_error().decode()


def _a256(x):
    return (x + 255) // 256 * 256


def _cap(N):
    return max(1, min(4 * N, 1 << 26))


def test_workspace_formulas(lib):
    ws = lib.nr_mesh_sample_workspace_bytes
    assert ws(-1) == 0 and ws(2 ** 31) == 0
    for F in (0, 1, 2048, 2049, 70000, 3_000_000, 2 ** 31 - 1):
        nb = max(1, -(-F // 2048))
        assert ws(F) == _a256(8 * nb) + _a256(4 * nb)
    ws = lib.nr_nn_workspace_bytes
    assert ws(-1, 0) == 0 and ws(0, -1) == 0 and ws(2 ** 31, 0) == 0 and ws(0, 2 ** 31) == 0
    for N, M in ((0, 0), (0, 5), (1, 1), (1000, 10), (70000, 4096), (1 << 20, 1 << 20), (1 << 26, 3), (2 ** 31 - 1, 1)):
        c = _cap(N)
        want = 256 + 2 * _a256(4 * (c + 1)) + _a256(4 * -(-(c + 1) // 1024)) + _a256(16 * N) + _a256(4 * M)
        assert ws(N, M) == want, (N, M)
        assert ws(N, 0) == want - _a256(4 * M)


def test_sampler_entries_check_arguments_without_gpu(lib):
    need = lib.nr_mesh_sample_workspace_bytes(50)

    def cdf(verts=A, V=100, faces=B, F=50, out=C, info=D, ws=WS, nbytes=need):
        return lib.nr_mesh_face_cdf(verts, V, faces, F, out, info, ws, nbytes, None)
    for kw in (dict(V=-1), dict(F=-1), dict(V=2 ** 31), dict(F=2 ** 31)):
        assert cdf(**kw) == -1 and 'INT32_MAX' in _err(lib), kw
    for kw in (dict(verts=None), dict(faces=None)):
        assert cdf(**kw) == -1 and 'null argument' in _err(lib), kw
    for kw in (dict(out=None), dict(info=None)):
        assert cdf(**kw) == -1 and 'null output' in _err(lib), kw
    assert cdf(nbytes=need - 1) == -4 and 'workspace' in _err(lib)
    assert cdf(ws=None) == -4
    assert cdf(F=70000, nbytes=need) == -4                               # 35 workgroups need more than one slot row

    def sample(verts=A, V=100, faces=B, F=50, c=C, u=D, n=10, points=E, face_id=G):
        return lib.nr_mesh_sample(verts, V, faces, F, c, u, n, points, face_id, None)
    for kw in (dict(V=-1), dict(F=-1), dict(F=2 ** 31)):
        assert sample(**kw) == -1 and 'INT32_MAX' in _err(lib), kw
    for kw in (dict(n=-1), dict(n=2 ** 31)):
        assert sample(**kw) == -1 and 'sample count' in _err(lib), kw
    for kw in (dict(verts=None), dict(faces=None), dict(c=None), dict(u=None)):
        assert sample(**kw) == -1 and 'null argument' in _err(lib), kw
    for kw in (dict(points=None), dict(face_id=None)):
        assert sample(**kw) == -1 and 'null output' in _err(lib), kw
    assert sample(n=0, u=None, points=None, face_id=None) == 0           # nothing to do: no launch


def test_nn_entries_check_arguments_without_gpu(lib):
    N, M = 1000, 10
    need_b, need_q = lib.nr_nn_workspace_bytes(N, 0), lib.nr_nn_workspace_bytes(N, M)
    assert need_b < need_q

    def build(points=A, n=N, h=0.1, ws=WS, nbytes=need_b):
        return lib.nr_nn_build(points, n, h, ws, nbytes, None)
    for kw in (dict(n=-1), dict(n=2 ** 31)):
        assert build(**kw) == -1 and 'INT32_MAX' in _err(lib), kw
    assert build(points=None) == -1 and 'null argument' in _err(lib)
    for h in (0.0, -1.0, float('nan'), INF, -INF):
        assert build(h=h) == -1 and 'cell size' in _err(lib), h
    assert build(nbytes=need_b - 1) == -4 and 'workspace' in _err(lib)
    assert build(ws=None) == -4

    def query(n=N, queries=B, m=M, md=INF, index=C, d2=D, status=E, ws=WS, nbytes=need_q):
        return lib.nr_nn_query(n, queries, m, md, index, d2, status, ws, nbytes, None)
    for kw in (dict(n=-1), dict(m=-1), dict(m=2 ** 31)):
        assert query(**kw) == -1 and 'INT32_MAX' in _err(lib), kw
    assert query(queries=None) == -1 and 'null argument' in _err(lib)
    for md in (-1.0, float('nan'), -INF):
        assert query(md=md) == -1 and 'max_dist' in _err(lib), md
    for kw in (dict(index=None), dict(d2=None), dict(status=None)):
        assert query(**kw) == -1 and 'null output' in _err(lib), kw
    assert query(nbytes=need_q - 1) == -4 and 'workspace' in _err(lib)
    assert query(nbytes=need_b) == -4                                     # the build's share is not enough
    assert query(ws=None) == -4

    def bounds(points=A, n=N, out=C, ws=WS, nbytes=256):
        return lib.nr_nn_bounds(points, n, out, ws, nbytes, None)
    assert bounds(n=-1) == -1 and bounds(points=None) == -1 and bounds(out=None) == -1
    assert bounds(nbytes=255) == -4 and bounds(ws=None) == -4


def test_python_entries_refuse_bad_input_before_any_work():
    import torch
    from neurecon_amd import mesh_metrics as mm
    z = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError, match='n must be'):
        mm.sample_mesh_surface(z, np.array([[0, 1, 2]]), -1)
    if not torch.cuda.is_available():                      # no fallback: host input without a device is refused
        with pytest.raises(RuntimeError, match='GPU'):
            mm.nearest_points(z, z)
        with pytest.raises(RuntimeError, match='GPU'):
            mm.sample_mesh_surface(z, np.array([[0, 1, 2]]), 4)
