"""GPU tests of the device marching cubes (nr_mc_count + nr_mc_emit, neurecon_amd.mesh_util.marching_cubes)
and of extract_mesh's native path end to end.

The numpy reference below computes the crossing-edge list in the order nr_mcubes.hip defines (owning
point's flat C index, then axis) and the positions by the float64 formula rounded to fp32 once.
The kernel rounds every float64 operation on its own, as numpy does, and its division is IEEE, so
check_mesh compares positions by equality; the few direct comparisons outside it keep the older bar of
one fp32 ulp of the largest |coordinate| in the mesh.  Faces are checked
by their properties (one cell per face, cell order, closed and consistently oriented surface, Euler
characteristic, signed volume) and, as the orders are fully defined, against the list the case table
(nr_mc_table) gives in numpy."""
import ctypes

import numpy as np
import pytest
import torch

import weightgen as wg
from helpers import neus_model
from test_mc_table import HEADER, edge_corners, read_ply

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


# ------------------------------------------------------------------------------------------------
# numpy reference
# ------------------------------------------------------------------------------------------------
def _vec(x):
    return np.broadcast_to(np.asarray(x, np.float64), (3,))


def ref_vertices(vol, level=0.0, spacing=1.0, origin=0.0, scale=1.0, offset=0.0):
    """-> key [V] int64 (3 * owning point's flat index + axis, ascending), pos [V, 3] fp32"""
    vol = np.asarray(vol, np.float32)
    lv = np.float32(level)
    ins = vol < lv
    keys, coords = [], []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = ins[lo] != ins[hi]
        ijk = np.argwhere(cross)
        v0, v1 = vol[lo][cross].astype(np.float64), vol[hi][cross].astype(np.float64)
        t = (np.float64(lv) - v0) / (v1 - v0)
        c = ijk.astype(np.float64)
        c[:, a] += t
        keys.append(np.ravel_multi_index(ijk.T, vol.shape).astype(np.int64) * 3 + a)
        coords.append(c)
    key, c = np.concatenate(keys), np.concatenate(coords)
    order = np.argsort(key, kind='stable')
    key, c = key[order], c[order]
    pos = ((c * _vec(spacing) + _vec(origin)) / np.float64(scale)) - _vec(offset)
    return key, pos.astype(np.float32)


def cell_cases(vol, level=0.0):
    """case index of every cell, [n0-1, n1-1, n2-1]: bit c = 4 d0 + 2 d1 + d2 set iff that corner is inside"""
    ins = np.asarray(vol, np.float32) < np.float32(level)
    n0, n1, n2 = ins.shape
    case = np.zeros((n0 - 1, n1 - 1, n2 - 1), np.int64)
    for c in range(8):
        d0, d1, d2 = (c >> 2) & 1, (c >> 1) & 1, c & 1
        case |= ins[d0:n0 - 1 + d0, d1:n1 - 1 + d1, d2:n2 - 1 + d2].astype(np.int64) << c
    return case


_TABLE = []


def mc_table():
    if not _TABLE:
        from neurecon_amd import _lib
        tri, cnt = np.zeros((256, 16), np.int8), np.zeros(256, np.int32)
        assert _lib.lib().nr_mc_table(ctypes.c_void_p(tri.ctypes.data), ctypes.c_void_p(cnt.ctypes.data)) == 0
        _TABLE.append((tri, cnt))
    return _TABLE[0]


def ref_faces(vol, level, key):
    """the face list the definitions give: cells in flat order, table order within a cell; also each face's cell"""
    tri, cnt = mc_table()
    case = cell_cases(vol, level)
    shape = np.asarray(vol).shape
    strides = np.array([shape[1] * shape[2], shape[2], 1], np.int64)
    cells = np.argwhere(cnt[case] > 0)
    cflat = cells @ strides
    ccase = case[tuple(cells.T)]
    edge_base = np.array([[(edge_corners(e)[0] >> 2) & 1, (edge_corners(e)[0] >> 1) & 1, edge_corners(e)[0] & 1]
                          for e in range(12)], np.int64)
    faces, order = [], []
    for t in range(5):
        sel = cnt[ccase] > t
        e = tri[ccase[sel], 3 * t:3 * t + 3].astype(np.int64)                     # [m, 3] cube edge ids
        k = (cflat[sel, None] + edge_base[e] @ strides) * 3 + (e >> 2)
        idx = np.searchsorted(key, k)
        assert (key[np.minimum(idx, len(key) - 1)] == k).all()
        faces.append(idx)
        order.append(cflat[sel] * 8 + t)
    faces, order = np.concatenate(faces), np.concatenate(order)
    o = np.argsort(order, kind='stable')
    return faces[o].astype(np.int32), order[o] // 8


def ulp_bar(ref):
    return np.spacing(np.float32(np.abs(ref).max()))


def assert_closed(faces, V):
    """every directed edge (a, b) occurs exactly once, and (b, a) exactly once"""
    f = faces.astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code, rev = d[:, 0] * V + d[:, 1], d[:, 1] * V + d[:, 0]
    u, n = np.unique(code, return_counts=True)
    assert (n == 1).all(), 'a directed edge occurs twice'
    assert np.array_equal(u, np.unique(rev)), 'a directed edge has no opposite'


def signed_volume(verts, faces):
    v = verts.astype(np.float64)[faces.astype(np.int64)]
    return np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0


def run_mc(vol, level=0.0, **kw):
    from neurecon_amd.mesh_util import marching_cubes
    v, f = marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).cuda(), level=level, **kw)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    return v.cpu().numpy(), f.cpu().numpy()


def check_mesh(vol, level=0.0, **kw):
    """verts vs the reference list (count exact, order, positions equal), faces vs the table-derived list"""
    key, ref = ref_vertices(vol, level, **kw)
    verts, faces = run_mc(vol, level, **kw)
    assert verts.shape == ref.shape, (verts.shape, ref.shape)
    err = np.abs(verts.astype(np.float64) - ref.astype(np.float64)).max()
    print(f'{np.asarray(vol).shape} level {level}: V={len(verts)} F={len(faces)} max |dpos| {err:.3e} '
          f'({int((verts != ref).sum())} coordinates differ)')
    assert np.array_equal(verts, ref)
    want, _ = ref_faces(vol, level, key)
    assert faces.shape == want.shape and np.array_equal(faces, want)
    return key, ref, verts, faces


# ------------------------------------------------------------------------------------------------
def test_all_256_cases_in_isolation():
    """a 2x2x2 volume per case: corners +-(0.25 + 0.5 k / 8) by class"""
    _, cnt = mc_table()
    for case in range(1, 255):
        vol = np.zeros(8, np.float32)
        for c in range(8):
            mag = 0.25 + 0.5 * c / 8
            vol[c] = -mag if (case >> c) & 1 else mag
        vol = vol.reshape(2, 2, 2)                                   # flat index 4 d0 + 2 d1 + d2 = corner id
        assert cell_cases(vol)[0, 0, 0] == case
        n_cross = sum(((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1 for e in range(12))
        key, ref = ref_vertices(vol)
        verts, faces = run_mc(vol)
        assert len(verts) == n_cross == len(key), case
        assert len(faces) == cnt[case], case
        assert np.abs(verts.astype(np.float64) - ref).max() <= ulp_bar(ref), case
        assert np.array_equal(faces, ref_faces(vol, 0.0, key)[0]), case
    for case, fill in ((0, 1.0), (255, -1.0)):
        from neurecon_amd.mesh_util import marching_cubes
        with pytest.raises(ValueError, match='Surface level must be within volume data range'):
            marching_cubes(torch.full((2, 2, 2), fill, device='cuda'))


def _owner_from_position(verts):
    """(3 * flat point index + axis) decoded from index-space positions (spacing 1, origin 0): the one
    fractional coordinate is the edge's axis, the floors are the owning point"""
    fl = np.floor(verts.astype(np.float64))
    frac = verts != fl
    assert (frac.sum(1) == 1).all()
    return fl.astype(np.int64), frac.argmax(1)


@pytest.mark.parametrize('level', [0.0, 0.3])
@pytest.mark.parametrize('shape', [(2, 2, 2), (3, 5, 130), (9, 18, 33), (2, 300, 3)])
def test_shapes_that_straddle_lanes_and_workgroups(shape, level):
    vol = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
    key, ref, verts, faces = check_mesh(vol, level)
    # V and the per-vertex owning edge, exactly
    ijk, axis = _owner_from_position(verts)
    assert np.array_equal(np.ravel_multi_index(ijk.T, shape) * 3 + axis, key)
    # every face's three vertices lie on edges of one cell; cells non-decreasing along faces
    strides = np.array([shape[1] * shape[2], shape[2], 1], np.int64)
    p, a = ijk[faces.astype(np.int64)], axis[faces.astype(np.int64)]          # [F, 3, 3], [F, 3]
    lo, hi = p.copy(), p.copy()                                               # a cell's min corner c: c[a] = p[a],
    for q in range(3):                                                        # c[b] in {p[b] - 1, p[b]} otherwise
        other = a != q
        lo[..., q] -= other
    lo, hi = lo.max(1), hi.min(1)                                             # intersection over the 3 vertices
    hi = np.minimum(hi, np.array(shape) - 2)
    lo = np.maximum(lo, 0)
    assert (lo <= hi).all()
    cmin, cmax = lo @ strides, hi @ strides
    prev = -1
    for x, y in zip(cmin.tolist(), cmax.tolist()):                            # a non-decreasing choice exists
        prev = max(prev, x)
        assert prev <= y
    # a second run is bit-identical
    v2, f2 = run_mc(vol, level)
    assert v2.tobytes() == verts.tobytes() and f2.tobytes() == faces.tobytes()


def test_more_workgroups_than_scan_threads():
    """1138 workgroups of 256 points: the single scan workgroup's 1024 threads own strips of 2 workgroups, the
    last strips partly or wholly empty (every other shape here has one workgroup per scan thread at most)"""
    shape = (70, 64, 65)
    vol = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    vol += 4 * _sphere(shape, (0.1, -0.2, 0.05), 0.7)                          # fewer crossings than pure noise
    check_mesh(vol, 0.25)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_product_and_sum_are_rounded_separately(axis):
    """vol = index along `axis` - 2.3, rounded to fp32: every vertex sits on an edge from 2 to 3 of that axis, at
    t = 0.30000001192092896, idx = 2.300000011920929 in float64 from the fp32 ends.  origin[axis] =
    -(idx * spacing[axis]) cancels the rounded product exactly, so the position is 0.0 on that axis for all
    25 vertices; one fused multiply-add keeps the product's rounding error instead (1.7e-18, -3.3e-18,
    -1.3e-17 for spacings 0.1, 0.3, 0.7)."""
    shape = [1, 1, 1]
    shape[axis] = 5
    line = (np.arange(5) - 2.3).astype(np.float32)
    vol = np.broadcast_to(line.reshape(shape), (5, 5, 5))
    v0, v1 = np.float64(line[2]), np.float64(line[3])
    idx = np.float64(2.0) + (np.float64(0.0) - v0) / (v1 - v0)
    assert idx == 2.300000011920929
    spacing = np.array([0.1, 0.3, 0.7])
    origin = np.zeros(3)
    origin[axis] = -(idx * spacing[axis])
    _, ref, verts, _ = check_mesh(vol, 0.0, spacing=spacing, origin=origin)
    assert len(ref) == 25 and (ref[:, axis] == 0.0).all()
    assert np.array_equal(verts, ref)


def test_watertight_and_oriented_on_every_case():
    v = np.ones((20, 21, 22), np.float32)
    v[1:-1, 1:-1, 1:-1] = np.random.default_rng(0).standard_normal((18, 19, 20))
    seen = np.bincount(cell_cases(v).ravel(), minlength=256)
    assert seen.min() >= 9, 'the volume must contain every cell case'
    _, _, verts, faces = check_mesh(v)
    assert_closed(faces, len(verts))


def _sphere(shape, centre, r):
    ax = [np.linspace(-1, 1, n) for n in shape]
    g = np.stack(np.meshgrid(*ax, indexing='ij'), -1)
    return (np.linalg.norm(g - np.asarray(centre), axis=-1) - r).astype(np.float32)


def _no_ambiguous_face(vol):
    ins = vol < np.float32(0)
    for a in range(3):
        m = np.moveaxis(ins, a, 0)
        c00, c01, c10, c11 = m[:, :-1, :-1], m[:, :-1, 1:], m[:, 1:, :-1], m[:, 1:, 1:]
        if ((c00 == c11) & (c01 == c10) & (c00 != c01)).any():
            return False
    return True


def test_sphere_volume_and_euler():
    shape, r, c = (40, 36, 33), 0.6, (0.07, -0.11, 0.03)
    vol = _sphere(shape, c, r)
    sp = [2.0 / (n - 1) for n in shape]
    _, _, verts, faces = check_mesh(vol, 0.0, spacing=sp, origin=-1.0)
    assert_closed(faces, len(verts))
    assert len(verts) - len(faces) / 2 == 2
    h = max(sp)
    vol_mesh = signed_volume(verts - np.float32(c), faces)  # volume is translation invariant; centred: better conditioned
    lo, hi = 4 / 3 * np.pi * (r - 3 ** 0.5 * h) ** 3, 4 / 3 * np.pi * (r + 3 ** 0.5 * h) ** 3
    print(f'sphere: signed volume {vol_mesh:.6f} in [{lo:.6f}, {hi:.6f}] (exact {4 / 3 * np.pi * r ** 3:.6f})')
    assert vol_mesh > 0 and lo <= vol_mesh <= hi


def test_torus_and_two_spheres_euler():
    n = 48
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    torus = (np.sqrt((np.sqrt(x * x + y * y) - 0.5) ** 2 + z * z) - 0.2).astype(np.float32)
    assert _no_ambiguous_face(torus), 'the topology must not depend on the table'
    sp = 2.0 / (n - 1)
    _, _, verts, faces = check_mesh(torus, 0.0, spacing=sp, origin=-1.0)
    assert_closed(faces, len(verts))
    assert len(verts) - len(faces) / 2 == 0
    assert signed_volume(verts, faces) > 0
    two = np.minimum(_sphere((n, n, n), (-0.45, 0.02, 0.01), 0.3), _sphere((n, n, n), (0.47, -0.03, 0.04), 0.3))
    assert _no_ambiguous_face(two)
    _, _, verts, faces = check_mesh(two, 0.0, spacing=sp, origin=-1.0)
    assert_closed(faces, len(verts))
    assert len(verts) - len(faces) / 2 == 4


@pytest.mark.parametrize('N, s, n_cross', [(16, 2.0, 90), (24, 1.5, 394)])
def test_reference_produced_volumes(golden, N, s, n_cross):
    """the SDF volumes the reference's extract_mesh handed to its writer, with its spacing s / N and
    origin -s / 2 (mesh_util.py:84, 112)"""
    vol = golden('surface')[f'grid{N}'].astype(np.float32)
    assert vol.shape == (N, N, N) and not (vol == 0).any()
    ins = vol < 0
    assert not (ins[0].any() or ins[-1].any() or ins[:, 0].any() or ins[:, -1].any() or ins[:, :, 0].any()
                or ins[:, :, -1].any())
    key, _, verts, faces = check_mesh(vol, 0.0, spacing=[s / N] * 3, origin=[-s / 2] * 3)
    assert len(key) == n_cross == len(verts)
    assert_closed(faces, len(verts))
    assert signed_volume(verts, faces) > 0


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_extract_mesh_end_to_end(tmp_path, precision):
    from neurecon_amd.mesh_util import extract_mesh, sdf_grid
    m = neus_model(wg.neus_state(seed=1), precision=precision)
    N, s = 24, 1.5
    path = tmp_path / 'm.ply'
    assert extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=path, marching='native') is None
    hdr, verts, faces = read_ply(path)
    assert hdr == HEADER.format(V=len(verts), F=len(faces))
    with torch.no_grad():
        vol = sdf_grid(m.implicit_surface, s, N).cpu().numpy()      # this build's own grid: deterministic
    key, ref = ref_vertices(vol, 0.0, spacing=[s / N] * 3, origin=[-s / 2] * 3)
    assert verts.shape == ref.shape
    assert np.abs(verts.astype(np.float64) - ref).max() <= ulp_bar(ref)
    assert np.array_equal(faces, ref_faces(vol, 0.0, key)[0])
    assert_closed(faces, len(verts))
    # 'auto' without scikit-image / plyfile takes the native path too and writes the same file
    from neurecon_amd import mesh_util
    if not mesh_util._have_skimage_and_plyfile():
        extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=tmp_path / 'auto.ply')
        assert open(tmp_path / 'auto.ply', 'rb').read() == open(path, 'rb').read()


def test_convert_uploads_numpy_and_applies_scale_offset(tmp_path):
    from neurecon_amd.mesh_util import convert_sigma_samples_to_ply
    vol = _sphere((12, 13, 14), (0.1, 0.0, -0.1), 0.5) + 5.0          # the reference's default level is 5.0
    sp, org, scale, off = [0.2, 0.19, 0.18], [-1.0, -1.1, -1.2], 1.7, np.array([0.3, -0.2, 0.1])
    convert_sigma_samples_to_ply(vol, org, sp, tmp_path / 'c.ply', offset=off, scale=scale, marching='native')
    _, verts, faces = read_ply(tmp_path / 'c.ply')
    key, ref = ref_vertices(vol, 5.0, spacing=sp, origin=org, scale=scale, offset=off)
    assert verts.shape == ref.shape and np.abs(verts.astype(np.float64) - ref).max() <= ulp_bar(ref)
    assert np.array_equal(faces, ref_faces(vol, 5.0, key)[0])
    with pytest.raises(ValueError):
        convert_sigma_samples_to_ply(vol, org, sp, tmp_path / 'x.ply', marching='cpu')


def test_errors():
    from neurecon_amd import _lib
    from neurecon_amd.mesh_util import marching_cubes
    lib = _lib.lib()
    vol = torch.from_numpy(_sphere((8, 9, 10), (0, 0, 0), 0.5)).cuda()
    with pytest.raises(ValueError, match='Surface level must be within volume data range'):
        marching_cubes(vol, level=float(vol.max()) + 1.0)
    with pytest.raises(RuntimeError, match='GPU'):
        marching_cubes(vol.cpu())
    with pytest.raises(ValueError):
        marching_cubes(vol[:1])
    with pytest.raises(ValueError):
        marching_cubes(vol[0])
    # nr_mc_emit directly: too-small capacities / workspace are refused before any launch
    n0, n1, n2 = vol.shape
    ws_bytes = lib.nr_mc_workspace_bytes(n0, n1, n2)
    assert 0 < ws_bytes <= 6 * vol.numel() + (1 << 20)
    assert lib.nr_mc_workspace_bytes(512, 512, 512) <= 6 * 512 ** 3 + (1 << 20)
    assert lib.nr_mc_workspace_bytes(1, 9, 10) == 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device='cuda')
    totals = torch.zeros(2, dtype=torch.int64, device='cuda')
    st = _lib.stream_of(vol.device)
    P = _lib.ptr
    assert lib.nr_mc_count(P(vol), n0, n1, n2, 0.0, P(ws), ws_bytes - 1, P(totals), st) == -4
    assert lib.nr_mc_count(P(vol), n0, 1, n2, 0.0, P(ws), ws_bytes, P(totals), st) == -1
    _lib.check(lib.nr_mc_count(P(vol), n0, n1, n2, 0.0, P(ws), ws_bytes, P(totals), st))
    V, F = (int(x) for x in totals.cpu())
    assert V > 0 and F > 0
    verts = torch.full((V, 3), -7.0, device='cuda')
    faces = torch.full((F, 3), -7, dtype=torch.int32, device='cuda')
    d3 = ctypes.c_double * 3
    one, zero = d3(1, 1, 1), d3(0, 0, 0)

    def emit(wsb, nv, nf, vcap, fcap):
        return lib.nr_mc_emit(P(vol), n0, n1, n2, 0.0, one, zero, 1.0, zero, P(ws), wsb, nv, nf, P(verts), vcap,
                              P(faces), fcap, st)
    assert emit(ws_bytes, V, F, V - 1, F) == -1 and 'capacity' in lib.nr_last_error().decode()
    assert emit(ws_bytes, V, F, V, F - 1) == -1
    assert emit(ws_bytes, 2 ** 31, F, 2 ** 31, F) == -1
    assert emit(ws_bytes - 1, V, F, V, F) == -4
    torch.cuda.synchronize()
    assert bool((verts == -7.0).all()) and bool((faces == -7).all())     # nothing was launched
    _lib.check(emit(ws_bytes, V, F, V, F))
    key, ref = ref_vertices(vol.cpu().numpy())
    assert np.abs(verts.cpu().numpy().astype(np.float64) - ref).max() <= ulp_bar(ref)
    assert np.array_equal(faces.cpu().numpy(), ref_faces(vol.cpu().numpy(), 0.0, key)[0])


def test_against_skimage():
    """only where scikit-image is installed: same vertex set (skimage interpolates in fp32: 2 ulps), same winding"""
    measure = pytest.importorskip('skimage.measure')
    shape, r, c = (40, 36, 33), 0.6, (0.07, -0.11, 0.03)
    vol = _sphere(shape, c, r)
    sp = tuple(2.0 / (n - 1) for n in shape)
    verts, faces = run_mc(vol, 0.0, spacing=sp)
    sv, sf, _, _ = measure.marching_cubes(vol, 0.0, spacing=sp)
    assert sv.shape == verts.shape

    def srt(a):
        """by grid edge: the axis with the fractional index coordinate, floor on it, nearest integer on the others"""
        idx = a.astype(np.float64) / np.array(sp)
        ax = np.abs(idx - np.round(idx)).argmax(1)
        own = np.round(idx).astype(np.int64)
        rows = np.arange(len(a))
        own[rows, ax] = np.floor(idx[rows, ax]).astype(np.int64)
        return a[np.lexsort((ax, own[:, 2], own[:, 1], own[:, 0]))]
    bar = 2 * np.spacing(np.float32(np.abs(sv).max()))
    assert np.abs(srt(verts).astype(np.float64) - srt(sv.astype(np.float32))).max() <= bar
    ctr = np.float32(1.0) + np.float32(c)
    assert np.sign(signed_volume(verts - ctr, faces)) == np.sign(signed_volume(sv.astype(np.float32) - ctr, sf))
