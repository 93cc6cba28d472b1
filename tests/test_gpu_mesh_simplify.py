"""GPU tests of mesh simplification by vertex clustering (neurecon_amd.mesh_simplify: nr_mesh_simplify_count /
nr_mesh_simplify_emit, neurecon_amd/csrc/nr_meshsimplify.hip).  The reference is the numpy restatement of the
rule, tests/mesh_simplify_ref.py; the device's five outputs (vertices, faces, index, vertex_cluster,
cluster_size) are compared to it by equality, in both position modes."""
import numpy as np
import pytest
import torch

import weightgen as wg
from helpers import neus_model
from mesh_simplify_ref import simplify_ref
from test_gpu_mcubes import _sphere

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


def run(verts, faces, h, position):
    """simplify_mesh twice (the runs must agree bit for bit) -> the five outputs as numpy arrays"""
    from neurecon_amd.mesh_simplify import simplify_mesh
    v = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).cuda()
    a = simplify_mesh(v, f, h, position=position, return_clusters=True)
    b = simplify_mesh(v, f, h, position=position, return_clusters=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'a second run differs'
    v2, f2, index, vclu, size = a
    assert v2.is_cuda and v2.dtype == torch.float32 and f2.dtype == torch.int32 and index.dtype == torch.int64
    assert vclu.dtype == torch.int32 and size.dtype == torch.int32
    three = simplify_mesh(v, f, h, position=position)
    assert len(three) == 3 and all(torch.equal(x, y) for x, y in zip(three, a[:3]))
    return [x.cpu().numpy() for x in a]


def check(verts, faces, h, positions=('average', 'nearest')):
    """device == restatement on all five outputs; -> the restatement's result of the last mode"""
    for position in positions:
        want = simplify_ref(verts, faces, h, position=position)
        v2, f2, index, vclu, size = run(verts, faces, h, position)
        assert v2.shape == want['verts'].shape and f2.shape == want['faces'].shape, \
            (position, v2.shape, want['verts'].shape, f2.shape, want['faces'].shape)
        assert np.array_equal(index, want['index']), position
        assert np.array_equal(vclu, want['vertex_cluster']) and np.array_equal(size, want['cluster_size']), position
        assert v2.tobytes() == want['verts'].tobytes(), position
        assert np.array_equal(f2, want['faces']), position
    return want


def cloud(V, seed, corners=True):
    v = np.random.default_rng(seed).random((V, 3)).astype(np.float32)
    if corners and V >= 2:      # the box is [0, 1]^3 exactly, so the cell size fixes the grid
        v[0], v[-1] = 0.0, 1.0
    return v


def soup(V, F, seed):
    return np.random.default_rng(seed).integers(0, V, size=(F, 3)).astype(np.int32)


@pytest.mark.parametrize('V, F', [(1, 0), (3, 1), (50, 200), (5000, 20000)])
@pytest.mark.parametrize('grid', ['2x2x2', 'V cells'])
def test_random_face_soups(V, F, grid):
    """2 x 2 x 2 cells: at most 56 distinct keys, so nearly all faces meet in a few slots of the duplicate table
    (the contended path); about V cells: mostly small clusters and few repeats"""
    v, f = cloud(V, seed=V), soup(V, F, seed=V + 1)
    n = 2 if grid == '2x2x2' else max(1, round(V ** (1 / 3)))
    h = 0.6 if n == 2 else 1.0 / (n - 0.5) if n > 1 else 2.0
    want = check(v, f, h)
    if V >= 2:
        assert want['dim'].tolist() == [n, n, n]
    print(f'V={V} F={F} {grid}: h={h:.4f} dim={want["dim"].tolist()} K={len(want["verts"])} F\'={len(want["faces"])}')
    if grid == '2x2x2' and F >= 200:
        assert len(want['verts']) <= 8 and 0 < len(want['faces']) <= 56


def test_vertices_on_cell_boundaries_and_at_hi():
    """h = 2^-2 and coordinates k / 8: t is an integer or a half, floor and the clamp at hi decide the cell"""
    rng = np.random.default_rng(11)
    v = (rng.integers(0, 9, size=(400, 3)) / 8.0).astype(np.float32)
    v[0], v[1] = 0.0, 1.0
    want = check(v, soup(400, 900, seed=12), 0.25)
    assert want['dim'].tolist() == [5, 5, 5]
    assert want['cell'][1] == 5 ** 3 - 1 and (v == 1.0).any(1).sum() > 10     # t = 4 at hi: clamped into the last cell
    # an origin off the lattice of the coordinates
    check(v + np.float32(0.3), soup(400, 900, seed=13), 0.25)


def test_coincident_vertices_tie_to_the_smaller_index():
    rng = np.random.default_rng(21)
    base = rng.random((12, 3)).astype(np.float32)
    pick = rng.integers(0, 12, size=90)
    v = base[pick]
    want = check(v, soup(90, 300, seed=22), 0.4)
    # among coincident members the representative is the first
    for k, src in enumerate(want['index']):
        same = np.flatnonzero((v == v[src]).all(1) & (want['vertex_cluster'] == k))
        assert src == same.min()
    # every vertex the same point: one cluster, no face, index 0
    one = np.repeat(base[:1], 40, 0)
    want = check(one, soup(40, 60, seed=23), 0.1)
    assert len(want['verts']) == 1 and len(want['faces']) == 0 and want['index'].tolist() == [0]
    assert want['verts'].tobytes() == one[:1].tobytes()


@pytest.fixture(scope='module')
def mc_sphere():
    from neurecon_amd.mesh_util import marching_cubes
    vol = _sphere((64, 64, 64), (0.03, -0.05, 0.02), 0.85)
    verts, faces = marching_cubes(torch.from_numpy(vol).cuda(), 0.0)      # index space: a voxel is 1
    return verts.cpu().numpy(), faces.cpu().numpy()


@pytest.mark.parametrize('cell', [1.5, 3.0, 0.4])
def test_marching_cubes_sphere(mc_sphere, cell):
    """a closed surface of ~ 27 voxels radius: tens of workgroups of vertices, faces and cells.  cell = 0.4 voxel
    gives more than 1024 x 256 cells, so the scan workgroup's threads own strips of several workgroups (the face
    scan gets there in test_more_workgroups_than_scan_threads)."""
    v, f = mc_sphere
    want = check(v, f, cell)
    K, Fk = len(want['verts']), len(want['faces'])
    cells = int(np.prod(want['dim']))
    print(f'sphere V={len(v)} F={len(f)} cell={cell}: dim={want["dim"].tolist()} K={K} F\'={Fk}')
    assert len(v) > 256 * 16 and len(f) > 256 * 32
    if cell == 0.4:
        assert (cells + 255) // 256 > 1024
    else:
        assert K < len(v) and 0 < Fk < len(f)
        tri = want['faces']
        assert len(np.unique(np.sort(tri, 1), axis=0)) == Fk


def test_more_workgroups_than_scan_threads():
    """1172 workgroups of vertices, 2344 of faces and 1340 of cells: the strips of both scans hold several"""
    V, F = 300001, 600001
    v, f = cloud(V, seed=31), soup(V, F, seed=32)
    want = check(v, f, 1.0 / 69.5, positions=('average',))
    assert want['dim'].tolist() == [70, 70, 70] and (70 ** 3 + 255) // 256 == 1340 and (F + 255) // 256 == 2344
    assert len(want['faces']) > 1024 * 256


def test_bad_input_is_refused():
    from neurecon_amd.mesh_simplify import simplify_mesh
    V, F = 1000, 600
    v, f = cloud(V, seed=41), soup(V, F, seed=42)
    vt = torch.from_numpy(v).cuda()
    for bad in (V, -1, 2 ** 31 - 1, -2 ** 31):
        g = f.copy()
        g[F // 2, 1] = bad
        with pytest.raises(ValueError, match='outside'):
            simplify_mesh(vt, torch.from_numpy(g).cuda(), 0.1)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[V // 3, 2] = bad
        with pytest.raises(ValueError, match='not finite'):
            simplify_mesh(torch.from_numpy(w).cuda(), torch.from_numpy(f).cuda(), 0.1)
    with pytest.raises(ValueError, match='larger cell'):
        simplify_mesh(vt, torch.from_numpy(f).cuda(), 1e-3)        # 1001^3 cells
    check(v, f, 0.1)                                               # the next call on the stream is correct
    # int64 faces come back as int64; the read_ply dict is taken as is
    a = simplify_mesh(vt, torch.from_numpy(f).cuda().long(), 0.1)
    b = simplify_mesh(dict(verts=v, faces=f, normals=None, colors=None), None, 0.1)
    assert a[1].dtype == torch.int64 and torch.equal(a[1].int(), b[1]) and torch.equal(a[0], b[0])


# ------------------------------------------------------------------------------------------------
# the model side: snapping and extract_mesh
# ------------------------------------------------------------------------------------------------
N_EX, S_EX = 64, 2.0
CELL_EX = 3 * S_EX / N_EX


@pytest.fixture(scope='module')
def model():
    return neus_model(wg.neus_state(seed=1), precision='fp32')


def test_snap_to_surface(model):
    from neurecon_amd.mesh_simplify import simplify_mesh, snap_to_surface
    from neurecon_amd.mesh_util import grid_sample_positions, marching_cubes, sdf_grid
    surface = model.implicit_surface
    with torch.no_grad():
        vol = sdf_grid(surface, S_EX, N_EX)
    idx, faces = marching_cubes(vol, 0.0)
    p0, _, _ = simplify_mesh(grid_sample_positions(idx, S_EX, N_EX), faces, CELL_EX)
    assert 0 < len(p0) < len(idx)
    got = snap_to_surface(surface, p0)
    p = p0
    with torch.no_grad():
        before = float(surface.forward_with_nablas(p0)[0].abs().max())
        for _ in range(2):
            sdf, nablas = surface.forward_with_nablas(p)[:2]
            p = p - sdf[:, None] * nablas / (nablas * nablas).sum(-1, keepdim=True).clamp_min(1e-12)
        after = float(surface.forward_with_nablas(got)[0].abs().max())
    print(f'snap: {len(p0)} vertices, max |sdf| {before:.3e} -> {after:.3e}')
    assert torch.equal(got, p)
    assert after < before
    assert torch.equal(snap_to_surface(model, p0), got)                      # the model that owns the surface
    assert torch.equal(snap_to_surface(surface, p0, chunk=100), got)         # several launches, one ragged
    assert torch.equal(snap_to_surface(surface, p0, iters=0), p0)


def test_extract_mesh_with_simplify(tmp_path, model):
    from neurecon_amd.mesh_simplify import simplify_mesh, snap_to_surface
    from neurecon_amd.mesh_util import (extract_mesh, grid_sample_positions, marching_cubes, read_ply, sdf_grid,
                                        vertex_attributes, write_ply)
    surface = model.implicit_surface
    kw = dict(volume_size=S_EX, N=N_EX, marching='native', vertex_normals=True, vertex_colors=True, model=model)
    extract_mesh(surface, filepath=tmp_path / 'full.ply', **kw)
    extract_mesh(surface, filepath=tmp_path / 'small.ply', simplify=CELL_EX, **kw)
    full, small = read_ply(tmp_path / 'full.ply'), read_ply(tmp_path / 'small.ply')
    V, F = len(small['verts']), len(small['faces'])
    print(f'extract_mesh N={N_EX}: V {len(full["verts"])} -> {V}, F {len(full["faces"])} -> {F}')
    assert 0 < V < len(full['verts']) and 0 < F < len(full['faces'])
    tri = small['faces']
    assert tri.min() >= 0 and tri.max() < V
    assert ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])).all()
    assert small['normals'] is not None and small['colors'] is not None
    assert small['normals'].shape == (V, 3) and small['colors'].shape == (V, 3)
    assert np.abs(np.linalg.norm(small['normals'].astype(np.float64), axis=1) - 1).max() < 1e-5
    assert len(np.unique(small['colors'])) > 1
    # the pieces by hand: the written vertices are simplify_mesh's, the attributes its source vertices'
    with torch.no_grad():
        vol = sdf_grid(surface, S_EX, N_EX)
    idx, faces = marching_cubes(vol, 0.0)
    verts_ref, _ = marching_cubes(vol, 0.0, spacing=[S_EX / N_EX] * 3, origin=[-S_EX / 2] * 3)
    v2, f2, src = simplify_mesh(verts_ref, faces, CELL_EX)
    n2, c2 = vertex_attributes(model, grid_sample_positions(idx.index_select(0, src), S_EX, N_EX), colors=True)
    assert np.array_equal(small['verts'], v2.cpu().numpy()) and np.array_equal(tri, f2.cpu().numpy())
    assert np.array_equal(small['normals'], n2.cpu().numpy())
    # coords='sampled': the averaged vertices are snapped, the attributes evaluated where they are written
    extract_mesh(surface, filepath=tmp_path / 'sampled.ply', simplify=CELL_EX, coords='sampled', **kw)
    sampled = read_ply(tmp_path / 'sampled.ply')
    v3, f3, _ = simplify_mesh(grid_sample_positions(idx, S_EX, N_EX), faces, CELL_EX)
    v3 = snap_to_surface(surface, v3)
    n3, _ = vertex_attributes(model, v3, colors=True)
    assert np.array_equal(sampled['verts'], v3.cpu().numpy()) and np.array_equal(sampled['faces'], f3.cpu().numpy())
    assert np.array_equal(sampled['normals'], n3.cpu().numpy())
    # 'nearest': input vertices, unchanged
    extract_mesh(surface, filepath=tmp_path / 'nearest.ply', simplify=CELL_EX, simplify_position='nearest', **kw)
    nearest = read_ply(tmp_path / 'nearest.ply')
    v4, _, src4 = simplify_mesh(verts_ref, faces, CELL_EX, position='nearest')
    assert np.array_equal(nearest['verts'], verts_ref.index_select(0, src4).cpu().numpy())
    assert np.array_equal(nearest['verts'], v4.cpu().numpy())
    # without the new keywords, and with them at their defaults: today's bytes
    extract_mesh(surface, volume_size=S_EX, N=N_EX, filepath=tmp_path / 'default.ply', marching='native')
    extract_mesh(surface, volume_size=S_EX, N=N_EX, filepath=tmp_path / 'none.ply', marching='native', simplify=None,
                 simplify_position='average')
    write_ply(tmp_path / 'pieces.ply', verts_ref, faces)
    default = open(tmp_path / 'default.ply', 'rb').read()
    assert default == open(tmp_path / 'none.ply', 'rb').read() == open(tmp_path / 'pieces.ply', 'rb').read()
    extract_mesh(surface, filepath=tmp_path / 'full2.ply', simplify=None, **kw)
    assert open(tmp_path / 'full2.ply', 'rb').read() == open(tmp_path / 'full.ply', 'rb').read()
    # a second run writes the same file
    extract_mesh(surface, filepath=tmp_path / 'again.ply', simplify=CELL_EX, **kw)
    assert open(tmp_path / 'again.ply', 'rb').read() == open(tmp_path / 'small.ply', 'rb').read()
    with pytest.raises(ValueError, match='simplify'):
        extract_mesh(surface, volume_size=S_EX, N=N_EX, filepath=tmp_path / 'x.ply', marching='skimage',
                     simplify=CELL_EX)
    with pytest.raises(ValueError, match='position'):
        extract_mesh(surface, volume_size=S_EX, N=N_EX, filepath=tmp_path / 'x.ply', marching='native',
                     simplify=CELL_EX, simplify_position='median')


def test_command_line(tmp_path, capsys):
    import json
    from neurecon_amd.mesh_simplify import main
    from neurecon_amd.mesh_util import read_ply, write_ply
    from test_mesh_render import icosphere, sphere_attributes
    v, f = icosphere(3)
    n, c = sphere_attributes(v)
    write_ply(tmp_path / 'in.ply', v, f, normals=n, colors=c)
    mesh = read_ply(tmp_path / 'in.ply')
    for position in ('average', 'nearest'):
        assert main([str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply'), '--cell', '0.31', '--position', position]) == 0
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        want = simplify_ref(v, f, 0.31, position=position)
        out = read_ply(tmp_path / 'out.ply')
        assert (line['verts_in'], line['faces_in']) == (len(v), len(f))
        assert (line['verts_out'], line['faces_out']) == (len(want['verts']), len(want['faces']))
        assert out['verts'].tobytes() == want['verts'].tobytes() and np.array_equal(out['faces'], want['faces'])
        assert np.array_equal(out['normals'], mesh['normals'][want['index']])
        assert np.array_equal(out['colors'], mesh['colors'][want['index']])
