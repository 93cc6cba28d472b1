"""CPU checks of mesh simplification by vertex clustering (neurecon_amd.mesh_simplify, nr_meshsimplify.hip): the
numpy restatement the GPU tests compare the device against (tests/mesh_simplify_ref.py), on inputs whose answer
is known, and the argument checks of the C entries.  No GPU: the library loads without one."""
import ctypes
import os

import numpy as np
import pytest

from mesh_simplify_ref import grid_of, simplify_ref
from test_mesh_render import icosphere


def _in_own_cell(out, h):
    """every output vertex lies in the cell of its cluster (closed on the upper side: a mean may round up to it)"""
    lo, dim = out['lo'], out['dim']
    occupied = np.unique(out['cell'])
    c = np.stack([occupied % dim[0], (occupied // dim[0]) % dim[1], occupied // (dim[0] * dim[1])], 1).astype(np.float64)
    t = (out['verts'].astype(np.float64) - lo) / h
    eps = 2.0 ** -22 * np.maximum(np.abs(out['verts']), 1.0) / h     # the fp32 rounding of the written vertex
    return bool(((t >= c - eps) & (t <= c + 1.0 + eps)).all())


def test_cell_larger_than_the_box_gives_one_vertex_at_the_quantised_mean():
    verts = np.array([[0, 0, 0], [1, 2, 3], [2, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    out = simplify_ref(verts, faces, 4.0)
    assert out['dim'].tolist() == [1, 1, 1] and out['lo'].tolist() == [0, 0, 0]
    assert out['verts'].shape == (1, 3) and out['faces'].shape == (0, 3)
    assert out['cluster_size'].tolist() == [3] and out['vertex_cluster'].tolist() == [0, 0, 0]
    # t = x / 4 and t 2^20 are exact, S = (3/4, 3/4, 3/4) 2^20, S / (3 2^20) = 1/4: the mean is (1, 1, 1) exactly
    assert out['mean'].tolist() == [[1.0, 1.0, 1.0]] and out['verts'].tolist() == [[1.0, 1.0, 1.0]]
    # d2 = 3, 5, 2: vertex 2 is nearest
    assert out['index'].tolist() == [2]
    assert simplify_ref(verts, faces, 4.0, position='nearest')['verts'].tolist() == [[2.0, 1.0, 0.0]]
    # a random cloud: within the quantisation step of the float64 mean
    v = np.random.default_rng(0).random((500, 3)).astype(np.float32)
    out = simplify_ref(v, np.zeros((0, 3), np.int32), 2.0)
    assert len(out['verts']) == 1
    err = np.abs(out['mean'][0] - v.astype(np.float64).mean(0))
    print('one cell, 500 vertices: |mean - float64 mean| =', err)
    assert (err <= 2.0 ** -20 * 2.0).all() and (out['mean'][0] <= v.astype(np.float64).mean(0) + 1e-12).all()


def test_tiny_cells_leave_every_vertex_alone():
    rng = np.random.default_rng(1)
    v = rng.random((20, 3)).astype(np.float32)
    f = rng.integers(0, 20, size=(40, 3)).astype(np.int32)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    f = f[np.unique(np.sort(f, 1), axis=0, return_index=True)[1]]     # no repeats, so every face must survive
    h = 1.0 / 400
    near = simplify_ref(v, f, h, position='nearest')
    order = np.argsort(near['cell'], kind='stable')
    assert len(np.unique(near['cell'])) == 20, 'the cloud must have one vertex per cell'
    assert np.array_equal(near['verts'], v[order]) and np.array_equal(near['index'], order)
    assert len(near['faces']) == len(f) and np.array_equal(near['faces'], near['vertex_cluster'][f])
    avg = simplify_ref(v, f, h)
    assert np.array_equal(avg['faces'], near['faces']) and np.array_equal(avg['index'], order)
    err = np.abs(avg['verts'].astype(np.float64) - v[order].astype(np.float64))
    bound = 2.0 ** -20 * h + 2.0 ** -24 * np.abs(v[order]) + 1e-12    # the quantisation step + one fp32 rounding
    print('alone: max |average - input| =', err.max(), 'bound', bound.min())
    assert (err <= bound).all()
    assert (avg['cluster_size'] == 1).all()


def test_repeated_and_flipped_faces_keep_the_first():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32)
    f = np.array([[3, 3, 1],       # degenerate in the input
                  [2, 1, 0],       # first of its set {0, 1, 2}
                  [0, 1, 2],       # the opposite orientation
                  [1, 2, 3],
                  [1, 0, 2],       # a rotation of the flip
                  [2, 1, 0],       # an exact repeat
                  [3, 2, 1]], np.int32)
    out = simplify_ref(v, f, 0.25)
    assert len(out['verts']) == 5
    assert out['kept_faces'].tolist() == [1, 3]
    assert np.array_equal(out['faces'], out['vertex_cluster'][f[[1, 3]]])


@pytest.mark.parametrize('h', [0.17, 0.31, 0.77])
@pytest.mark.parametrize('position', ['average', 'nearest'])
def test_icosphere(h, position):
    v, f = icosphere(3)
    out = simplify_ref(v, f, h, position=position)
    K, tri = len(out['verts']), out['faces']
    print(f'icosphere(3) V={len(v)} F={len(f)} h={h}: K={K} F\'={len(tri)}')
    assert 1 < K < len(v) and 0 < len(tri) < len(f)
    assert tri.min() >= 0 and tri.max() < K
    assert ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])).all()
    assert len(np.unique(np.sort(tri, 1), axis=0)) == len(tri)
    assert _in_own_cell(out, h)
    assert np.array_equal(out['vertex_cluster'][out['index']], np.arange(K))
    assert out['cluster_size'].sum() == len(v) and (out['cluster_size'] > 0).all()
    # the representative is a nearest member
    d = np.linalg.norm(v.astype(np.float64) - out['mean'][out['vertex_cluster']], axis=1)
    best = np.full(K, np.inf)
    np.minimum.at(best, out['vertex_cluster'], d)
    assert np.allclose(d[out['index']], best, rtol=1e-12, atol=0)


def test_permuting_the_vertices_changes_nothing():
    v, f = icosphere(2)
    p = np.random.default_rng(5).permutation(len(v))
    inv = np.empty_like(p)
    inv[p] = np.arange(len(v))
    for h in (0.2, 0.5):
        a = simplify_ref(v, f, h)
        b = simplify_ref(v[p], inv[f].astype(np.int32), h)
        assert a['verts'].tobytes() == b['verts'].tobytes() and a['mean'].tobytes() == b['mean'].tobytes()
        assert np.array_equal(a['faces'], b['faces']) and np.array_equal(a['cluster_size'], b['cluster_size'])
        assert np.array_equal(b['vertex_cluster'], a['vertex_cluster'][p])
        # 'nearest' names the same point of space unless two members tie
        an, bn = simplify_ref(v, f, h, position='nearest'), simplify_ref(v[p], inv[f], h, position='nearest')
        assert np.array_equal(an['faces'], bn['faces'])


def test_grid_of_counts_the_cell_holding_the_maximum():
    v = np.array([[0, 0, 0], [1, 0.5, 0.25]], np.float32)
    lo, dim = grid_of(v, 0.25)
    assert lo.tolist() == [0, 0, 0] and dim.tolist() == [5, 3, 2]
    out = simplify_ref(v, np.zeros((0, 3), np.int32), 0.25)
    assert out['cell'].tolist() == [0, (1 * 3 + 2) * 5 + 4]


# ------------------------------------------------------------------------------------------------
# the C entries' argument checks
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from neurecon_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def _a256(x):
    return (x + 255) & ~255


def test_workspace_formula(lib):
    def want(V, F, cells):
        k, T = min(V, cells), 64
        while T < 2 * F:
            T *= 2
        return (256 + _a256(4 * cells) + _a256(4 * ((cells + 255) // 256)) + _a256(4 * V) + _a256(4 * k) + _a256(4 * k) +
                _a256(24 * k) + _a256(8 * k) + _a256(4 * k) + _a256(24 * k) + _a256(4 * T) + _a256(4 * F) +
                _a256(4 * ((F + 255) // 256)))
    for V, F, cells in ((0, 0, 1), (1, 0, 1), (3, 1, 8), (5000, 20000, 8), (5000, 20000, 4913), (300001, 600001, 1 << 27)):
        assert lib.nr_mesh_simplify_workspace_bytes(V, F, cells) == want(V, F, cells), (V, F, cells)
    for V, F, cells in ((-1, 0, 1), (0, -1, 1), (2 ** 31, 0, 1), (1, 2 ** 30 + 1, 1), (1, 1, 0), (1, 1, 2 ** 27 + 1)):
        assert lib.nr_mesh_simplify_workspace_bytes(V, F, cells) == 0, (V, F, cells)


def test_entries_reject_bad_arguments_without_gpu(lib):
    """fake device pointers: every case returns before any HIP call"""
    D3, I3 = ctypes.c_double * 3, ctypes.c_int64 * 3
    VERTS, FACES, WS, TOT = 0x1000, 0x2000, 0x3000, 0x4000
    big = 1 << 40

    def count(verts=VERTS, V=10, faces=FACES, F=4, h=0.5, lo=(0, 0, 0), dim=(2, 2, 2), ws=WS, nb=big, tot=TOT):
        rc = lib.nr_mesh_simplify_count(verts, V, faces, F, h, None if lo is None else D3(*lo),
                                        None if dim is None else I3(*dim), ws, nb, tot, None)
        return rc, lib.nr_last_error().decode()
    for kw, text in ((dict(h=0.0), 'h must be'), (dict(h=-1.0), 'h must be'), (dict(h=float('nan')), 'h must be'),
                     (dict(h=float('inf')), 'h must be'), (dict(dim=(0, 2, 2)), 'dim'), (dict(dim=(2, 2, -1)), 'dim'),
                     (dict(dim=(512, 512, 513)), 'larger cell'), (dict(dim=(1 << 40, 1 << 40, 1 << 40)), 'larger cell'),
                     (dict(lo=None), 'null'), (dict(dim=None), 'null'), (dict(tot=None), 'null'),
                     (dict(verts=None), 'null'), (dict(faces=None), 'null'), (dict(lo=(0, float('nan'), 0)), 'origin'),
                     (dict(V=-1), 'INT32_MAX'), (dict(F=2 ** 30 + 1), '2^30')):
        rc, msg = count(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    need = lib.nr_mesh_simplify_workspace_bytes(10, 4, 8)
    for kw in (dict(ws=None), dict(nb=need - 1), dict(nb=0)):
        rc, msg = count(**kw)
        assert rc == -4 and 'workspace' in msg, (kw, rc, msg)

    def emit(verts=VERTS, V=10, faces=FACES, F=4, cells=8, position=0, ws=WS, nb=big, K=8, Fk=2, vo=0x5000, idx=0x6000,
             size=0x7000, vcap=8, fo=0x8000, fcap=2, vc=0x9000):
        rc = lib.nr_mesh_simplify_emit(verts, V, faces, F, cells, position, ws, nb, K, Fk, vo, idx, size, vcap, fo, fcap,
                                       vc, None)
        return rc, lib.nr_last_error().decode()
    for kw, text in ((dict(cells=0), 'cells'), (dict(cells=2 ** 27 + 1), 'cells'), (dict(position=2), 'position'),
                     (dict(K=9), 'counts'), (dict(K=-1), 'counts'), (dict(Fk=5), 'counts'), (dict(vcap=7), 'capacity'),
                     (dict(fcap=1), 'capacity'), (dict(verts=None), 'null'), (dict(faces=None), 'null'),
                     (dict(vo=None), 'null output'), (dict(idx=None), 'null output'), (dict(size=None), 'null output'),
                     (dict(fo=None), 'null output'), (dict(vc=None), 'null output')):
        rc, msg = emit(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    for kw in (dict(ws=None), dict(nb=need - 1)):
        rc, msg = emit(**kw)
        assert rc == -4 and 'workspace' in msg, (kw, rc, msg)


def test_simplify_mesh_refuses_bad_input_before_any_work():
    import torch
    from neurecon_amd.mesh_simplify import simplify_mesh, snap_to_surface
    with pytest.raises(RuntimeError, match='GPU'):
        simplify_mesh(torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32), 0.5)
    with pytest.raises(ValueError, match='position'):
        simplify_mesh(torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32), 0.5, position='median')
    with pytest.raises(ValueError, match='cell'):
        simplify_mesh(torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32), 0.0)
    with pytest.raises(ValueError, match='cell'):
        simplify_mesh(torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='GPU'):
        snap_to_surface(None, torch.zeros(4, 3))
