"""GPU tests of the mesh metrics: the exact nearest-neighbour search (nr_nn_build / nr_nn_query,
neurecon_amd/csrc/nr_nn.hip), the surface sampler (nr_mesh_face_cdf / nr_mesh_sample, nr_meshsample.hip) and
`evaluate_mesh` with its command line.

The reference is the numpy restatement in tests/mesh_metrics_ref.py; indices, squared distances, face ids and
points are compared by equality (bit for bit), never by a tolerance.  Run as a script
(`python tests/test_gpu_mesh_metrics.py rings`) the file runs the many-ring searches (two clusters far apart,
queries in the empty middle and far outside the box) and prints their result as JSON: test_many_rings starts
that in a child process under a timeout, so a search that does not end fails the test and does not stall the
suite."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clusters():
    """two clusters 10 apart, 1500 points each; queries inside them, in the empty middle and far outside"""
    rng = np.random.default_rng(11)
    a = rng.uniform(-0.1, 0.1, (1500, 3))
    b = rng.uniform(-0.1, 0.1, (1500, 3)) + [10.0, 0.0, 0.0]
    pts = np.concatenate([a, b]).astype(np.float32)
    mid = rng.uniform(-0.1, 0.1, (64, 3)) + [5.0, 0.0, 0.0]
    mid[0] = [5.0, 0.0, 0.0]
    far = np.array([[100, 100, 100], [-1e6, 3, 2], [5, 1e4, 0], [1e30, -1e30, 1e30], [10.05, 0.02, -50],
                    [-3e38, 3e38, 0]])
    q = np.concatenate([pts[::100], mid, far, rng.uniform(-0.3, 10.3, (64, 3))]).astype(np.float32)
    return pts, q


def _rings_main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import torch
    import mesh_metrics_ref as ref
    from neurecon_amd.mesh_metrics import nearest_points
    pts, q = clusters()
    out = {}
    # cell sizes that keep the grid within 64^3: 61 x 2 x 2 cells, and a coarser one; then bounded searches
    for name, kw in (('h017', dict(cell_size=0.17)), ('h05', dict(cell_size=0.5)),
                     ('h017_md4', dict(cell_size=0.17, max_dist=4.95)), ('h017_md6', dict(cell_size=0.17, max_dist=6.0)),
                     ('default', dict())):
        idx, dist, d2 = nearest_points(torch.from_numpy(pts).cuda(), torch.from_numpy(q).cuda(), **kw)
        i2, _, d22 = nearest_points(torch.from_numpy(pts).cuda(), torch.from_numpy(q).cuda(), **kw)
        ridx, rd2 = ref.brute_nn(pts, q, kw.get('max_dist'))
        out[name] = dict(index=bool(np.array_equal(idx.cpu().numpy(), ridx)),
                         d2=bool(np.array_equal(d2.cpu().numpy(), rd2)),
                         same=bool(torch.equal(idx, i2) and torch.equal(d2, d22)),
                         found=int((ridx >= 0).sum()))
    print('RINGS ' + json.dumps(out))


if __name__ == '__main__':
    assert sys.argv[1:] == ['rings']
    _rings_main()
    sys.exit(0)

import math

import pytest
import torch

import mesh_metrics_ref as ref
from test_gpu_mcubes import _sphere

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------
# nearest neighbour: index and d2 equal to the brute force, bit for bit
# ------------------------------------------------------------------------------------------------
def check_nn(points, queries, max_dist=None, cell_size=None):
    from neurecon_amd.mesh_metrics import nearest_points
    points = np.asarray(points, np.float32).reshape(-1, 3)
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    idx, dist, d2 = nearest_points(gpu(points), gpu(queries), max_dist=max_dist, cell_size=cell_size)
    assert idx.is_cuda and idx.dtype == torch.int64 and dist.dtype == torch.float64 and d2.dtype == torch.float64
    assert idx.shape == dist.shape == d2.shape == (len(queries),)
    ridx, rd2 = ref.brute_nn(points, queries, max_dist)
    g_idx, g_d2, g_dist = idx.cpu().numpy(), d2.cpu().numpy(), dist.cpu().numpy()
    bad = np.flatnonzero((g_idx != ridx) | (g_d2 != rd2))
    assert bad.size == 0, (bad[:5], g_idx[bad[:5]], ridx[bad[:5]], g_d2[bad[:5]], rd2[bad[:5]])
    fin = np.isfinite(rd2)
    assert np.isinf(g_dist[~fin]).all() and np.all(np.abs(g_dist[fin] - np.sqrt(rd2[fin])) <= np.spacing(g_dist[fin]))
    i2, t2, s2 = nearest_points(gpu(points), gpu(queries), max_dist=max_dist, cell_size=cell_size)
    assert torch.equal(idx, i2) and torch.equal(d2, s2) and torch.equal(dist, t2), 'a second run differs'
    return ridx, rd2


def test_nn_empty_and_single():
    q = np.random.default_rng(0).standard_normal((5, 3))
    ridx, rd2 = check_nn(np.zeros((0, 3)), q)                            # N = 0
    assert (ridx == -1).all() and np.isinf(rd2).all()
    check_nn(q, np.zeros((0, 3)))                                        # M = 0
    check_nn(np.zeros((0, 3)), np.zeros((0, 3)))
    ridx, _ = check_nn([[0.25, -1.5, 3.0]], q)                           # N = 1: a degenerate box, dims 1
    assert (ridx == 0).all()
    check_nn([[0.25, -1.5, 3.0]], q, max_dist=0.5)
    check_nn([[0.25, -1.5, 3.0]], [[0.25, -1.5, 3.0]], max_dist=0.0)     # d2 == 0 <= 0: kept


def test_nn_identical_and_duplicated_points():
    rng = np.random.default_rng(1)
    q = rng.standard_normal((300, 3))
    ridx, _ = check_nn(np.tile([[0.5, 0.25, -2.0]], (700, 1)), q)        # all identical: index 0
    assert (ridx == 0).all()
    p = rng.standard_normal((400, 3)).astype(np.float32)
    dup = np.concatenate([p, p[::-1], p])[rng.permutation(1200)]         # every point three times
    ridx, rd2 = check_nn(dup, np.concatenate([q, dup[:200]]))
    assert (rd2[300:] == 0).all()
    first = {}
    for i, row in enumerate(map(bytes, dup)):
        first.setdefault(row, i)
    assert all(first[bytes(dup[i])] == i for i in ridx)                  # the smallest index of each triple


def test_nn_integer_lattice_ties():
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    h = np.arange(7, dtype=np.float32) + 0.5
    half = np.stack(np.meshgrid(h, h, h, indexing='ij'), -1).reshape(-1, 3)
    q = np.concatenate([half, lattice, half * [1, 1, 0] + [0, 0, 3]])    # 8-way and 4-way exact ties, exact hits
    for cs in (None, 1.0, 0.5, 3.0):
        ridx, rd2 = check_nn(lattice, q, cell_size=cs)
        assert (rd2[:343] == 0.75).all() and (rd2[343:343 + 512] == 0).all()
    check_nn(lattice[np.random.default_rng(2).permutation(512)], q, cell_size=1.0)
    check_nn(lattice, q, max_dist=math.sqrt(0.75), cell_size=1.0)


def test_nn_cell_boundaries_and_box_maximum():
    """points exactly on cell boundaries (multiples of the cell size) and on the box maximum"""
    g = np.arange(9, dtype=np.float32) * 0.25
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    rng = np.random.default_rng(3)
    q = np.concatenate([rng.uniform(-0.5, 2.5, (500, 3)), pts[::7], pts[::11] + np.float32(1e-7),
                        [[2, 2, 2], [2, 0, 2], [0, 0, 0], [2.0000002, 2, 2], [-1e-30, 0, 0]]])
    for cs in (0.25, 0.125, 0.3, None):
        check_nn(pts, q, cell_size=cs)
    check_nn(pts - np.float32(1.0), q - 1.0, cell_size=0.25)


def test_nn_plane_and_line():
    rng = np.random.default_rng(4)
    plane = rng.uniform(-1, 1, (3000, 3))
    plane[:, 2] = 0.125                                                   # dims 1 along z
    line = np.zeros((500, 3))
    line[:, 0] = rng.uniform(-4, 4, 500)                                  # dims 1 along y and z
    q = rng.uniform(-1.5, 1.5, (700, 3))
    for pts in (plane, plane[:, [2, 0, 1]], line, line[:, [1, 2, 0]]):
        check_nn(pts, q)
        check_nn(pts, q, max_dist=0.3)


def test_nn_forced_cell_sizes():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 1, (1000, 3))
    q = np.concatenate([rng.uniform(-0.2, 1.2, (400, 3)), pts[:100]])
    check_nn(pts, q, cell_size=10.0)        # one cell
    check_nn(pts, q, cell_size=0.6)         # 2 x 2 x 2 cells
    check_nn(pts, q, cell_size=0.02)        # 125 000 cells asked: 0.008 points per cell, over the cap of 4 N
    check_nn(pts, q, cell_size=1e-3)        # 10^9 cells asked
    check_nn(pts, q, cell_size=1e-300)      # the division overflows
    check_nn(pts, q, cell_size=0.05, max_dist=0.04)


def test_nn_max_dist_boundary():
    """d2 == max_dist^2 is kept; the next float64 above it is dropped"""
    t = np.float32(2.0 ** -26)
    pts = np.array([[1, 0, 0], [101, t, 0]], np.float32)
    q = np.array([[0, 0, 0], [100, 0, 0]], np.float32)
    ridx, rd2 = check_nn(pts, q, max_dist=1.0)
    assert ridx.tolist() == [0, -1] and rd2[0] == 1.0
    ridx, rd2 = check_nn(pts, q)
    assert ridx.tolist() == [0, 1] and rd2[1] == np.nextafter(1.0, 2.0)
    ridx, _ = check_nn(pts, q, max_dist=np.nextafter(1.0, 0.0))
    assert ridx.tolist() == [-1, -1]
    ridx, _ = check_nn([[0, 0, 0]], [[3, 4, 0], [3, 4, 12]], max_dist=5.0)
    assert ridx.tolist() == [0, -1]


def test_nn_non_finite_input():
    rng = np.random.default_rng(6)
    pts = rng.standard_normal((900, 3)).astype(np.float32)
    pts[5, 0], pts[77, 1], pts[300, 2], pts[899] = np.nan, np.inf, -np.inf, np.nan
    q = rng.standard_normal((300, 3)).astype(np.float32)
    q[0, 2], q[10, 0], q[299, 1] = np.nan, np.inf, -np.inf
    q[20], q[21] = pts[6], [0, 0, 0]
    ridx, rd2 = check_nn(pts, q)
    assert not np.isin(ridx, [5, 77, 300, 899]).any() and ridx[[0, 10, 299]].tolist() == [-1, -1, -1]
    check_nn(pts, q, max_dist=0.2)
    bad = np.full((4, 3), np.nan, np.float32)
    ridx, _ = check_nn(bad, q)                                           # no finite point at all
    assert (ridx == -1).all()


def test_nn_many_workgroups():
    """N = 70 000, M = 4096: 274 workgroups bin the points, the cell table takes several scan workgroups"""
    rng = np.random.default_rng(7)
    pts = rng.standard_normal((70000, 3)).astype(np.float32)
    q = (rng.standard_normal((4096, 3)) * 1.2).astype(np.float32)
    check_nn(pts, q)


def test_nn_surface_cloud_with_max_dist():
    """the shape of the metric's own call: two clouds on nearby spheres, bounded search, both directions"""
    rng = np.random.default_rng(8)
    a = rng.standard_normal((20000, 3))
    a = (a / np.linalg.norm(a, axis=1, keepdims=True) * 0.6).astype(np.float32)
    b = rng.standard_normal((3000, 3))
    b = (b / np.linalg.norm(b, axis=1, keepdims=True) * 0.65).astype(np.float32)
    check_nn(a, b, max_dist=0.06)
    check_nn(b, a[:3000], max_dist=0.06)


def test_many_rings():
    """two clusters far apart, queries in the empty middle and far outside the box (up to 61 rings each), in a child
    process under a timeout"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), 'rings'], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith('RINGS ')][-1]
    res = json.loads(line[len('RINGS '):])
    assert set(res) == {'h017', 'h05', 'h017_md4', 'h017_md6', 'default'}
    for kind, r in res.items():
        assert r['index'] and r['d2'] and r['same'], (kind, r)
    n = len(clusters()[1])
    assert res['h017']['found'] == n and res['h017_md6']['found'] > res['h017_md4']['found']


# ------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------
def check_sampler(verts, faces, n, seed=0, want_status=0):
    from neurecon_amd.mesh_metrics import sample_mesh_surface
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    F = len(faces)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    u = torch.rand((n, 3), dtype=torch.float64, device='cuda', generator=gen)
    pts, fid, cdf = sample_mesh_surface(gpu(verts), gpu(faces), n, u=u)
    assert pts.dtype == torch.float32 and fid.dtype == torch.int32 and cdf.dtype == torch.float64
    assert pts.shape == (n, 3) and fid.shape == (n,) and cdf.shape == (F,)
    p2, f2, c2 = sample_mesh_surface(gpu(verts), gpu(faces), n, u=u)
    assert torch.equal(pts.view(torch.int32), p2.view(torch.int32)) and torch.equal(fid, f2)
    assert torch.equal(cdf.view(torch.int64), c2.view(torch.int64)), 'a second run differs'
    pts, fid, cdf = pts.cpu().numpy(), fid.cpu().numpy(), cdf.cpu().numpy()
    # cdf against the correctly rounded prefix sums
    areas, status = ref.face_areas(verts, faces)
    assert status == want_status
    exact = ref.exact_prefix(areas)
    total = exact[-1]
    err = np.abs(cdf - exact).max()
    print(f'F={F} n={n}: total {total:.6g}, max cdf error {err:.3e} (bound {F * 2.0 ** -53 * total:.3e})')
    assert err <= F * 2.0 ** -53 * total
    assert (np.diff(cdf) >= 0).all() and cdf[0] >= 0
    # points and faces against the rule, given that cdf
    rp, rf = ref.sample_ref(verts, faces, cdf, u.cpu().numpy())
    assert np.array_equal(fid, rf)
    assert np.array_equal(pts.view(np.int32), rp.view(np.int32))
    # never a face without area; stratification
    assert (areas[fid] > 0).all()
    count = np.bincount(fid, minlength=F)
    dev = np.abs(count - n * areas / total).max()
    print(f'    max |count - n a / total| = {dev:.4f}')
    assert dev <= 2 + n * F * 2.0 ** -53
    return pts, fid, cdf


def test_sampler_single_triangle():
    pts, fid, cdf = check_sampler([[0, 0, 0], [2, 0, 0], [0, 1, 0.5]], [[0, 1, 2]], 1000)
    assert (fid == 0).all() and cdf[0] == 0.5 * math.sqrt(5.0)
    check_sampler([[0, 0, 0], [2, 0, 0], [0, 1, 0.5]], [[0, 1, 2]], 1)


def test_sampler_marching_cubes_sphere():
    from neurecon_amd.mesh_util import marching_cubes
    n = 24
    verts, faces = marching_cubes(gpu(_sphere((n, n, n), (0.05, -0.02, 0.01), 0.6)), 0.0, spacing=2.0 / (n - 1),
                                  origin=-1.0)
    assert 512 < faces.shape[0] <= 4096
    pts, fid, _ = check_sampler(verts.cpu().numpy(), faces.cpu().numpy(), 20000, seed=1)
    r = np.linalg.norm(pts - np.float32([0.05, -0.02, 0.01]), axis=1)
    assert 0.58 < r.min() and r.max() < 0.61


def test_sampler_awkward_mesh():
    """degenerate faces, faces naming vertices outside [0, V), and a giant face next to tiny ones"""
    rng = np.random.default_rng(9)
    verts = rng.uniform(-1e-3, 1e-3, (300, 3)).astype(np.float32)
    verts[0], verts[1], verts[2] = [0, 0, 0], [4e3, 0, 0], [0, 4e3, 0]
    faces = rng.integers(3, 300, (600, 3)).astype(np.int32)
    faces[0] = [0, 1, 2]                                 # area 8e6 beside areas of about 1e-6
    faces[5], faces[6], faces[7] = [7, 7, 9], [8, 8, 8], [10, 11, 10]
    faces[100], faces[101], faces[599] = [3, 300, 4], [-1, 3, 4], [2 ** 31 - 1, 5, 6]
    pts, fid, cdf = check_sampler(verts, faces, 5000, seed=2, want_status=1)
    assert not np.isin(fid, [5, 6, 7, 100, 101, 599]).any()
    assert (fid == 0).sum() >= 4998
    # the giant face last: the tiny ones get their share first, then are absorbed in the giant's rounding
    faces[[0, 598]] = faces[[598, 0]]
    check_sampler(verts, faces, 5000, seed=3, want_status=1)
    # a non-finite vertex: its faces have no area
    verts[50, 1] = np.inf
    _, fid, _ = check_sampler(verts, faces, 3000, seed=4, want_status=3)
    assert not (faces[fid] == 50).any()


def test_sampler_many_workgroups():
    """F = 70 000: 35 workgroups of 2048 faces, so the chain over the workgroup sums and the fix-up run"""
    rng = np.random.default_rng(10)
    verts = rng.standard_normal((9000, 3)).astype(np.float32)
    base = rng.integers(0, 9000 - 40, 70000)
    faces = np.stack([base, base + rng.integers(1, 20, 70000), base + rng.integers(20, 40, 70000)], 1).astype(np.int32)
    faces[::1000, 2] = faces[::1000, 1]                 # some degenerate ones
    check_sampler(verts, faces, 100000, seed=5)


def test_sampler_nothing_to_sample():
    from neurecon_amd.mesh_metrics import sample_mesh_surface
    verts = gpu(np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]]))
    for faces, n in ((np.int32([[0, 1, 2]]), 10), (np.zeros((0, 3), np.int32), 10), (np.int32([[0, 1, 1]]), 0)):
        pts, fid, cdf = sample_mesh_surface(verts, gpu(faces), n)
        assert pts.shape == (0, 3) and fid.shape == (0,) and cdf.shape == (len(faces),) and not cdf.any()
    pts, fid, cdf = sample_mesh_surface(gpu(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])), gpu(np.int32([[0, 1, 2]])), 0)
    assert pts.shape == (0, 3) and cdf.tolist() == [0.5]
    pts, fid, _ = sample_mesh_surface(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int64([[0, 1, 2]]), 7)
    assert pts.is_cuda and pts.shape == (7, 3) and (fid == 0).all()      # host input, default uniforms


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
R, DELTA, N_GT, N_S = 0.6, 0.05, 5000, 6000


@pytest.fixture(scope='module')
def sphere_case():
    """a marching-cubes sphere of radius R, exact points on the sphere of radius R + DELTA, and the float64 brute
    force on the device's own samples"""
    from neurecon_amd.mesh_metrics import sample_mesh_surface
    from neurecon_amd.mesh_util import marching_cubes
    n = 48
    verts, faces = marching_cubes(gpu(_sphere((n, n, n), (0, 0, 0), R)), 0.0, spacing=2.0 / (n - 1), origin=-1.0)
    k = np.arange(N_GT) + 0.5                                            # a Fibonacci lattice on the sphere
    z, phi = 1 - 2 * k / N_GT, k * math.pi * (3 - math.sqrt(5))
    s = np.sqrt(1 - z * z)
    gt = ((R + DELTA) * np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)).astype(np.float32)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(12)
    u = torch.rand((N_S, 3), dtype=torch.float64, device='cuda', generator=gen)
    pred = sample_mesh_surface(verts, faces, N_S, u=u)[0].cpu().numpy()
    d_pg = np.sqrt(ref.brute_nn(gt, pred)[1])
    d_gp = np.sqrt(ref.brute_nn(pred, gt)[1])
    return dict(verts=verts, faces=faces, gt=gt, u=u, pred=pred, d_pg=d_pg, d_gp=d_gp)


def _same(a, b, rel=1e-12):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, list):
            assert len(x) == len(y) and all(abs(p - q) <= rel * abs(q) for p, q in zip(x, y)), k
        elif isinstance(x, float):
            assert abs(x - y) <= rel * abs(y), (k, x, y)
        else:
            assert x == y, (k, x, y)


def test_evaluate_mesh_against_offset_sphere(sphere_case):
    from neurecon_amd.mesh_metrics import evaluate_mesh, metrics_from_distances
    c = sphere_case
    kw = dict(max_dist=0.2, thresholds=(0.03, DELTA + 0.005, 0.1))
    got = evaluate_mesh(c['verts'], c['faces'], gpu(c['gt']), N_S, u=c['u'], **kw)
    want = metrics_from_distances(c['d_pg'], c['d_gp'], **kw)
    _same(got, want)
    assert got['n_pred'] == N_S and got['n_gt'] == N_GT and got['n_pred_excluded'] == 0 and got['n_gt_excluded'] == 0
    # accuracy and completeness are DELTA to within the discretisation, taken in float64 from the same samples:
    #   e_r  how far a sample's radius is from R (the mesh is a polyhedron inside / around the sphere)
    #   a sample p and a cloud point g at angle t: |p - g|^2 = (|g| - |p|)^2 + 4 |p| |g| sin^2(t / 2)
    #   pred -> gt: at least the radial gap, at most the distance to the cloud point nearest to p pushed out to
    #     radius R + DELTA (p', the lateral term is then at most |p' - g|): sqrt(gap^2 + lateral^2), per sample
    #   gt -> pred: at least the radial gap to the outermost sample, at most DELTA + the distance from g pulled in
    #     to radius R (g') to its nearest sample (triangle inequality), per cloud point
    pred, gt = c['pred'].astype(np.float64), c['gt'].astype(np.float64)
    rad = np.linalg.norm(pred, axis=1)
    gap = (R + DELTA) - rad
    lateral = np.sqrt(ref.brute_nn(gt, (pred * ((R + DELTA) / rad)[:, None]).astype(np.float32))[1])
    slack = 1e-6                                                         # fp32 coordinates of p', g', the cloud
    lo, hi = gap.mean() - slack, np.sqrt(gap * gap + lateral * lateral).mean() + slack
    print(f'accuracy {got["accuracy"]:.6f} in [{lo:.6f}, {hi:.6f}]; radii {rad.min():.5f} .. {rad.max():.5f}')
    assert lo <= got['accuracy'] <= hi and abs(got['accuracy'] - DELTA) <= (hi - lo) + np.abs(rad - R).max()
    pulled = np.sqrt(ref.brute_nn(c['pred'], (gt * (R / (R + DELTA))).astype(np.float32))[1])
    lo, hi = (R + DELTA) - rad.max() - slack, DELTA + pulled.mean() + slack
    print(f'completeness {got["completeness"]:.6f} in [{lo:.6f}, {hi:.6f}]')
    assert lo <= got['completeness'] <= hi
    assert got['chamfer'] == (got['accuracy'] + got['completeness']) / 2
    assert got['precision'][0] == 0.0 and got['recall'][0] == 0.0 and got['fscore'][0] == 0.0
    assert got['precision'][2] == 1.0 and got['recall'][2] == 1.0 and got['fscore'][2] == 1.0
    # a mask on the cloud: the same as handing over the masked cloud; a threshold beyond max_dist: unbounded search
    mask = c['gt'][:, 2] > 0
    a = evaluate_mesh(c['verts'], c['faces'], c['gt'], N_S, u=c['u'], gt_mask=mask, max_dist=0.1, thresholds=(0.5,))
    b = evaluate_mesh(c['verts'], c['faces'], c['gt'][mask], N_S, u=c['u'], max_dist=0.1, thresholds=(0.5,))
    assert a == b and a['n_gt'] == int(mask.sum()) and a['n_pred_excluded'] > 0
    dm = np.sqrt(ref.brute_nn(c['gt'][mask], c['pred'])[1])
    _same(a, metrics_from_distances(dm, np.sqrt(ref.brute_nn(c['pred'], c['gt'][mask])[1]), max_dist=0.1,
                                    thresholds=(0.5,)))


def test_command_line(sphere_case, tmp_path):
    from neurecon_amd.mesh_metrics import evaluate_mesh
    from neurecon_amd.mesh_util import write_ply
    c = sphere_case
    pred_ply, gt_ply = tmp_path / 'pred.ply', tmp_path / 'gt.ply'
    write_ply(pred_ply, c['verts'], c['faces'])
    gt_ply.write_bytes(f'ply\nformat binary_little_endian 1.0\nelement vertex {N_GT}\nproperty float x\n'
                       'property float y\nproperty float z\nend_header\n'.encode() + c['gt'].astype('<f4').tobytes())
    p = subprocess.run([sys.executable, '-m', 'neurecon_amd.mesh_metrics', str(pred_ply), str(gt_ply), '--samples',
                        '4000', '--max-dist', '0.2', '--threshold', '0.03', '--threshold', '0.06', '--seed', '5'],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    got = json.loads(lines[0])
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    u = torch.rand((4000, 3), dtype=torch.float64, device='cuda', generator=gen)
    want = evaluate_mesh(c['verts'], c['faces'], c['gt'], 4000, max_dist=0.2, thresholds=(0.03, 0.06), u=u)
    for k, v in want.items():
        assert got[k] == v, k
    assert got['samples'] == 4000 and got['seed'] == 5 and abs(got['accuracy'] - DELTA) < 0.01
