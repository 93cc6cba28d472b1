"""GPU tests of the mesh-finishing stage: connected components and order-preserving filtering
(nr_mesh_components / nr_mesh_filter_count / nr_mesh_filter_emit, neurecon_amd/csrc/nr_meshops.hip), per-vertex
normals and colours, and extract_mesh with the new options.

The reference for labels, counts, maps and faces is the short numpy union-find below; those comparisons are
exact integer equality.  Run as a script (`python tests/test_gpu_mesh_finish.py chains`) the file runs the
long-chain cases and prints their result as JSON: test_chains starts that in a child process under a
timeout, so a labelling loop that does not end fails the test and does not stall the suite."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_V = 70000   # 274 workgroups of 256 faces: more than the chip has CUs, one component through all of them


def chain_faces(kind):
    i = np.arange(CHAIN_V - 2, dtype=np.int64)
    f = np.stack([i, i + 1, i + 2], 1)
    if kind == 'descending':
        f = f[::-1]
    elif kind == 'permuted':
        f = np.random.default_rng(7).permutation(CHAIN_V)[f]
    return np.ascontiguousarray(f).astype(np.int32)


def _chains_main():
    sys.path.insert(0, ROOT)
    import torch
    from neurecon_amd.mesh_util import mesh_components
    out = {}
    for kind in ('ascending', 'descending', 'permuted'):
        faces = torch.from_numpy(chain_faces(kind)).cuda()
        labels, count, n, (big, big_faces) = mesh_components(faces, CHAIN_V, return_largest=True)
        l2, c2, n2 = mesh_components(faces, CHAIN_V)
        out[kind] = dict(n=n, largest=big, largest_faces=big_faces, labels_zero=bool((labels == 0).all()),
                         count0=int(count[0]), count_rest=int(count[1:].abs().sum()),
                         same=bool(torch.equal(labels, l2) and torch.equal(count, c2) and n == n2))
    print('CHAINS ' + json.dumps(out))


if __name__ == '__main__':
    assert sys.argv[1:] == ['chains']
    _chains_main()
    sys.exit(0)

import pytest
import torch

import weightgen as wg
from helpers import neus_model, report, unisurf_model, volsdf_model
from test_gpu_mcubes import _sphere, assert_closed, signed_volume

pytestmark = pytest.mark.gpu
RT, AT = 1e-4, 1e-6


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


# ------------------------------------------------------------------------------------------------
# numpy reference
# ------------------------------------------------------------------------------------------------
def ref_components(faces, V):
    """-> labels [V] (smallest vertex index of the component), face_count [V] (at the label), n, largest label"""
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for a, b, c in np.asarray(faces).tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    labels = np.array([find(v) for v in range(V)], np.int64).reshape(V)
    count = np.bincount(labels[np.asarray(faces, np.int64).reshape(-1, 3)[:, 0]], minlength=V).astype(np.int64)
    n = int((labels == np.arange(V)).sum())
    largest = int(np.argmax(count)) if V else -1           # first maximum: a tie goes to the smaller label
    return labels, count, n, largest


def ref_filter(faces, keep):
    """-> index (new -> old, ascending), remapped kept faces"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    index = np.flatnonzero(keep)
    new = np.full(len(keep), -1, np.int64)
    new[index] = np.arange(len(index))
    return index, new[faces[keep[faces].all(1)]]


def run_components(faces, V):
    from neurecon_amd.mesh_util import mesh_components
    t = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).cuda()
    labels, count, n, (big, big_faces) = mesh_components(t, V, return_largest=True)
    assert labels.is_cuda and labels.dtype == torch.int32 and count.dtype == torch.int32 and isinstance(n, int)
    l2, c2, n2 = mesh_components(t, V)
    assert torch.equal(labels, l2) and torch.equal(count, c2) and n == n2, 'a second run differs'
    return labels.cpu().numpy().astype(np.int64), count.cpu().numpy().astype(np.int64), n, big, big_faces


def check_components(faces, V):
    labels, count, n, big, big_faces = run_components(faces, V)
    rl, rc, rn, rbig = ref_components(faces, V)
    assert np.array_equal(labels, rl) and np.array_equal(count, rc)
    assert n == rn and big == rbig and big_faces == (rc[rbig] if V else 0)
    return rl, rc, rn, rbig


def soup(V, F, seed=0):
    return np.random.default_rng(seed).integers(0, V, size=(F, 3)).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# components
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V, F', [(1, 0), (3, 1), (64, 40), (257, 300), (1000, 600), (5000, 20000)])
def test_random_face_soups(V, F):
    """random indices: degenerate and repeated faces, isolated vertices, one wave up to many workgroups"""
    labels, count, n, _ = check_components(soup(V, F), V)
    print(f'V={V} F={F}: {n} components, largest {count.max()} faces')
    assert count.sum() == F


def test_chains():
    """V = 70 000, faces (i, i+1, i+2): one component that spans every workgroup, in ascending and descending
    face order and with permuted vertex ids.  The input on which fixed-round label propagation gives wrong
    labels and a find that re-reads stale parents loops: run in a child process under a timeout."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), 'chains'], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith('CHAINS ')][-1]
    for kind, r in json.loads(line[len('CHAINS '):]).items():
        assert r == dict(n=1, largest=0, largest_faces=CHAIN_V - 2, labels_zero=True, count0=CHAIN_V - 2,
                         count_rest=0, same=True), (kind, r)


def test_bad_indices_are_refused_and_write_nothing():
    """a face naming V and one naming -1: ValueError, nothing outside the arrays is touched, and the next call
    on the same stream is correct"""
    from neurecon_amd import _lib
    from neurecon_amd.mesh_util import mesh_components
    V, F = 1000, 600
    faces = soup(V, F)
    for bad in (V, -1, 2 ** 31 - 1, -2 ** 31):
        f = faces.copy()
        f[F // 2, 1] = bad
        with pytest.raises(ValueError, match='outside'):
            mesh_components(torch.from_numpy(f).cuda(), V)
    # the raw entry, outputs between guard words
    lib, P = _lib.lib(), _lib.ptr
    f = faces.copy()
    f[3, 0], f[F - 1, 2] = V, -1
    ft = torch.from_numpy(f).cuda()
    G = 64
    labels = torch.full((V + 2 * G,), -7, dtype=torch.int32, device='cuda')
    count = torch.full((V + 2 * G,), -7, dtype=torch.int32, device='cuda')
    totals = torch.zeros(4, dtype=torch.int64, device='cuda')
    ws_bytes = lib.nr_mesh_workspace_bytes(V, F)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device='cuda')
    _lib.check(lib.nr_mesh_components(P(ft), F, V, P(labels[G:]), P(count[G:]), P(totals), P(ws), ws_bytes,
                                      _lib.stream_of(ft.device)))
    assert int(totals[3]) == 1
    for a in (labels, count):
        assert bool((a[:G] == -7).all()) and bool((a[V + G:] == -7).all())
    # the two bad faces are skipped, the others labelled as without them
    good = np.delete(faces, [3, F - 1], 0)
    rl, rc, rn, rbig = ref_components(good, V)
    assert np.array_equal(labels[G:V + G].cpu().numpy(), rl) and np.array_equal(count[G:V + G].cpu().numpy(), rc)
    assert [int(x) for x in totals[:3]] == [rn, rbig, rc[rbig]]
    check_components(faces, V)


# ------------------------------------------------------------------------------------------------
# marching-cubes meshes
# ------------------------------------------------------------------------------------------------
def mc_mesh(vol):
    from neurecon_amd.mesh_util import marching_cubes
    return marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).cuda(), 0.0)


def three_spheres():
    shape = (40, 36, 44)
    return np.minimum(np.minimum(_sphere(shape, (-0.5, -0.4, -0.4), 0.35), _sphere(shape, (0.45, 0.4, 0.3), 0.3)),
                      _sphere(shape, (-0.3, 0.5, 0.55), 0.2))


def tube_and_sphere():
    """distance to a polyline that folds back and forth in the plane z = 0, minus 0.12; a small sphere above it"""
    n = 32
    ax = np.linspace(-1, 1, n)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1)
    pts = []
    for r, y in enumerate((-0.6, -0.2, 0.2, 0.6)):
        xs = (-0.6, 0.6) if r % 2 == 0 else (0.6, -0.6)
        pts += [(xs[0], y, 0.0), (xs[1], y, 0.0)]
    pts = np.array(pts)
    d = np.full(g.shape[:-1], np.inf)
    for a, b in zip(pts[:-1], pts[1:]):
        ab = b - a
        t = np.clip(((g - a) @ ab) / (ab @ ab), 0, 1)
        d = np.minimum(d, np.linalg.norm(g - (a + t[..., None] * ab), axis=-1))
    return np.minimum(d - 0.12, _sphere((n, n, n), (0.0, 0.0, 0.7), 0.2)).astype(np.float32)


def check_filtered(verts, faces, keep_mask, got):
    """got = filter_mesh's (verts', faces', index) vs the numpy remap of keep_mask"""
    v2, f2, index = got
    want_index, want_faces = ref_filter(faces.cpu().numpy(), keep_mask)
    assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), want_index)
    assert bool((index[1:] > index[:-1]).all())
    assert v2.dtype == verts.dtype and torch.equal(v2, verts[index])
    assert f2.dtype == faces.dtype and np.array_equal(f2.cpu().numpy(), want_faces)
    return v2.cpu().numpy(), f2.cpu().numpy()


@pytest.mark.parametrize('name, n_want', [('three_spheres', 3), ('tube_and_sphere', 2)])
def test_marching_cubes_meshes(name, n_want):
    from neurecon_amd.mesh_util import filter_mesh
    verts, faces = mc_mesh(globals()[name]())
    V = len(verts)
    labels, count, n, big = check_components(faces.cpu().numpy(), V)
    sizes = np.sort(count[count > 0])
    print(f'{name}: V={V} F={len(faces)} component faces {sizes.tolist()}')
    assert n == n_want == len(sizes) and len(set(sizes.tolist())) == n
    # the largest component alone: a closed, outward-oriented surface
    v2, f2 = check_filtered(verts, faces, labels == big, filter_mesh(verts, faces, keep='largest'))
    assert len(f2) == sizes[-1]
    assert_closed(f2, len(v2))
    assert signed_volume(v2 - v2.mean(0), f2) > 0
    # a bar between two component sizes drops exactly the smaller ones
    for lo, hi in zip(sizes[:-1], sizes[1:]):
        k = int((lo + hi + 1) // 2)
        assert lo < k <= hi
        _, f3 = check_filtered(verts, faces, count[labels] >= k, filter_mesh(verts, faces, min_faces=k))
        assert len(f3) == sizes[sizes >= k].sum()
    # both at once, and a second run
    a = filter_mesh(verts, faces, keep='largest', min_faces=int(sizes[0]))
    b = filter_mesh(verts, faces, keep='largest', min_faces=int(sizes[0]))
    check_filtered(verts, faces, labels == big, a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # nothing asked: the inputs themselves
    v0, f0, i0 = filter_mesh(verts, faces)
    assert v0 is verts and f0 is faces and torch.equal(i0, torch.arange(V, device='cuda'))
    with pytest.raises(ValueError, match='no vertex'):
        filter_mesh(verts, faces, min_faces=int(sizes[-1]) + 1)


def test_tie_goes_to_the_smaller_label():
    """two congruent spheres, the second a copy of the first 12 voxels further along axis 0"""
    from neurecon_amd.mesh_util import filter_mesh
    g = np.stack(np.meshgrid(np.arange(26.), np.arange(20.), np.arange(20.), indexing='ij'), -1)
    c = np.array([6.3, 9.6, 10.2])
    vol = np.minimum(np.linalg.norm(g - c, axis=-1), np.linalg.norm(g - (c + [12, 0, 0]), axis=-1)) - 4.4
    verts, faces = mc_mesh(vol)
    labels, count, n, big = check_components(faces.cpu().numpy(), len(verts))
    roots = np.flatnonzero(count)
    assert n == 2 == len(roots) and count[roots[0]] == count[roots[1]] > 0
    assert big == roots.min() == 0
    v2, f2 = check_filtered(verts, faces, labels == big, filter_mesh(verts, faces, keep='largest'))
    assert v2[:, 0].max() < 12.3 < verts[:, 0].max()          # the sphere at the lower axis-0 indices stayed


def test_vertex_mask_path():
    from neurecon_amd.mesh_util import filter_mesh
    V, F = 1000, 600
    faces = torch.from_numpy(soup(V, F)).cuda()
    verts = torch.from_numpy(np.random.default_rng(1).standard_normal((V, 3)).astype(np.float32)).cuda()
    mask = np.random.default_rng(2).random(V) < 0.6
    got = filter_mesh(verts, faces, vertex_mask=torch.from_numpy(mask).cuda())
    _, f2 = check_filtered(verts, faces, mask, got)
    assert 0 < len(f2) < F
    # int64 faces come back as int64; a mask and a component bar combine with `and`
    labels, count, _, _ = ref_components(faces.cpu().numpy(), V)
    got = filter_mesh(verts, faces.long(), min_faces=3, vertex_mask=torch.from_numpy(mask).cuda())
    check_filtered(verts, faces.long(), mask & (count[labels] >= 3), got)
    with pytest.raises(ValueError, match='no vertex'):
        filter_mesh(verts, faces, vertex_mask=torch.zeros(V, dtype=torch.bool, device='cuda'))
    with pytest.raises(ValueError):
        filter_mesh(verts, faces, vertex_mask=torch.ones(V - 1, dtype=torch.bool, device='cuda'))


def test_filter_with_more_workgroups_than_scan_threads():
    """1172 workgroups of 256 vertices and 2344 of 256 faces: each scan workgroup's 1024 threads own strips of
    2 and 3 workgroups, the last strips partly or wholly empty (every other case here has one workgroup per
    scan thread at most)"""
    from neurecon_amd.mesh_util import filter_mesh
    V, F = 300001, 600001
    assert ((V + 255) // 256, (F + 255) // 256) == (1172, 2344)
    faces = torch.from_numpy(soup(V, F, seed=3)).cuda()
    verts = torch.from_numpy(np.random.default_rng(4).standard_normal((V, 3)).astype(np.float32)).cuda()
    mask = np.random.default_rng(5).random(V) < 0.6
    _, f2 = check_filtered(verts, faces, mask, filter_mesh(verts, faces, vertex_mask=torch.from_numpy(mask).cuda()))
    assert 0 < len(f2) < F


# ------------------------------------------------------------------------------------------------
# attributes
# ------------------------------------------------------------------------------------------------
N_ATTR, S_ATTR = 24, 1.5


def read_full_ply(path, normals, colors):
    data = open(path, 'rb').read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    hdr = data[:end].decode('ascii')
    V = int([l for l in hdr.split('\n') if l.startswith('element vertex')][0].split()[-1])
    F = int([l for l in hdr.split('\n') if l.startswith('element face')][0].split()[-1])
    fields = [('p', '<f4', (3,))] + ([('n', '<f4', (3,))] if normals else []) + ([('c', 'u1', (3,))] if colors else [])
    assert ('property float nx' in hdr) == normals and ('property uchar red' in hdr) == colors
    vrec = np.frombuffer(data, np.dtype(fields), V, end)
    frec = np.frombuffer(data, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), F, end + V * vrec.dtype.itemsize)
    assert end + V * vrec.dtype.itemsize + F * 13 == len(data) and (frec['n'] == 3).all()
    return vrec, frec['v']


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_vertex_attributes(tmp_path, precision):
    """Normals and colours at the sampled positions of the N = 24, s = 1.5 NeuS mesh.
    (1) The stage adds no arithmetic: equal, bit for bit, to forward_with_nablas / model.forward by hand.
    (2) Normals vs the oracle SDF net's normalised nablas: RT and 1e-4 absolute, the per-ray normals bar.
    (3) Colours vs the oracle radiance net on the oracle's own nablas and feature, the view directions being
        the input both sides are given (-normals of the build under test): RT, AT.
    (4) |normal| = 1 within 4 fp32 ulp (2^-21): the division and the norm each round once per component.
    (5) The oracle's |sdf| is smaller on average at the coords='sampled' vertices than at coords='reference'."""
    from oracle.nets import RadianceNet, SDFNet
    from neurecon_amd.mesh_util import (extract_mesh, grid_sample_positions, marching_cubes, sdf_grid,
                                        vertex_attributes)
    sd = wg.neus_state(seed=1)
    m = neus_model(sd, precision=precision)
    N, s = N_ATTR, S_ATTR
    with torch.no_grad():
        vol = sdf_grid(m.implicit_surface, s, N)
    idx, faces = marching_cubes(vol, 0.0)
    pos = grid_sample_positions(idx, s, N)
    assert pos.is_cuda and pos.dtype == torch.float32
    assert torch.equal(pos.cpu(), grid_sample_positions(idx.cpu(), s, N))
    normals, colors = vertex_attributes(m, pos, normals=True, colors=True)
    with torch.no_grad():
        n_hand = torch.nn.functional.normalize(m.implicit_surface.forward_with_nablas(pos)[1], dim=-1)
        c_hand = m.forward(pos, -n_hand)[0]
    assert torch.equal(normals, n_hand) and torch.equal(colors, c_hand)
    n_only, none = vertex_attributes(m.implicit_surface, pos)
    assert none is None and torch.equal(n_only, n_hand)
    n_chunked, c_chunked = vertex_attributes(m, pos, colors=True, chunk=100)      # several launches, one ragged
    assert torch.equal(n_chunked, n_hand) and torch.equal(c_chunked, c_hand)
    with pytest.raises(ValueError, match='radiance'):
        vertex_attributes(m.implicit_surface, pos, colors=True)
    # oracle
    p = pos.cpu()
    _, nab_ref, h = SDFNet(sd).forward_with_nablas(p)
    n_ref = torch.nn.functional.normalize(nab_ref, dim=-1)
    ok_n, _ = report(f'{precision} vertex normals', normals, n_ref, RT, 1e-4)
    c_ref = RadianceNet(sd).forward(p, -normals.cpu(), nab_ref, h)
    ok_c, _ = report(f'{precision} vertex colours', colors, c_ref, RT, AT)
    length = normals.double().norm(dim=-1)
    print(f'{precision} | |n| - 1 | max {float((length - 1).abs().max()):.3e}')
    # the written positions: sampled vs reference lattice
    sdf_at = {}
    for coords in ('sampled', 'reference'):
        path = tmp_path / f'{coords}.ply'
        extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=path, marching='native', coords=coords,
                     vertex_normals=True)
        vrec, f = read_full_ply(path, True, False)
        assert np.array_equal(f, faces.cpu().numpy()) and np.array_equal(vrec['n'], normals.cpu().numpy())
        sdf_at[coords] = float(SDFNet(sd).sdf(torch.from_numpy(vrec['p'].copy())).abs().mean())
        if coords == 'sampled':
            assert np.array_equal(vrec['p'], pos.cpu().numpy())
    print(f'{precision} mean |sdf| at the written vertices: {sdf_at}')
    assert ok_n.all()
    assert ok_c.all()
    assert float((length - 1).abs().max()) <= 4 * 2.0 ** -23
    assert sdf_at['sampled'] < sdf_at['reference']


def _model(kind, precision='f16x3'):
    if kind == 'neus':
        return neus_model(wg.neus_state(seed=1), precision=precision), 1.5
    if kind == 'volsdf':
        return volsdf_model(wg.volsdf_state(seed=2), 0.1, precision=precision), 2.5
    return unisurf_model(wg.unisurf_state(seed=3), precision=precision), 2.5


@pytest.mark.parametrize('kind', ['neus', 'volsdf', 'unisurf'])
def test_extract_mesh_with_everything_on(tmp_path, kind):
    from neurecon_amd.mesh_util import (extract_mesh, filter_mesh, grid_sample_positions, marching_cubes, sdf_grid,
                                        vertex_attributes, write_ply)
    m, s = _model(kind)
    N = N_ATTR
    full = tmp_path / 'full.ply'
    assert extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=full, marching='native', keep='largest',
                        min_faces=4, vertex_normals=True, vertex_colors=True, model=m, coords='sampled') is None
    vrec, f = read_full_ply(full, True, True)
    # the pieces
    with torch.no_grad():
        vol = sdf_grid(m.implicit_surface, s, N)
    idx, faces = marching_cubes(vol, 0.0)
    verts_ref, faces_ref = marching_cubes(vol, 0.0, spacing=[s / N] * 3, origin=[-s / 2] * 3)
    assert torch.equal(faces, faces_ref)
    pos, f2, index = filter_mesh(grid_sample_positions(idx, s, N), faces, keep='largest', min_faces=4)
    normals, colors = vertex_attributes(m, pos, colors=True)
    print(f'{kind}: V={len(idx)} F={len(faces)} -> V={len(pos)} F={len(f2)}')
    assert len(vrec) == len(pos) and len(f) == len(f2)
    assert np.array_equal(vrec['p'], pos.cpu().numpy()) and np.array_equal(f, f2.cpu().numpy())
    assert np.array_equal(vrec['n'], normals.cpu().numpy())
    q = torch.floor(colors.double().clamp(0, 1) * 255 + 0.5).to(torch.uint8)
    assert np.array_equal(vrec['c'], q.cpu().numpy())
    assert colors.min() >= 0 and colors.max() <= 1 and len(np.unique(vrec['c'])) > 1
    if kind == 'neus':          # the 0.5 sphere lies inside the volume; the other two surfaces reach its border
        assert_closed(f, len(vrec))
    # coords='reference' with attributes: the default call's vertices, attributes still at the sampled points
    extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=tmp_path / 'ref.ply', marching='native',
                 vertex_colors=True, model=m)
    vrec2, f3 = read_full_ply(tmp_path / 'ref.ply', False, True)
    _, c_all = vertex_attributes(m, grid_sample_positions(idx, s, N), normals=False, colors=True)
    assert np.array_equal(vrec2['p'], verts_ref.cpu().numpy()) and np.array_equal(f3, faces.cpu().numpy())
    assert np.array_equal(vrec2['c'], torch.floor(c_all.double().clamp(0, 1) * 255 + 0.5).to(torch.uint8).cpu().numpy())
    # the default call: today's bytes
    extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=tmp_path / 'default.ply', marching='native')
    write_ply(tmp_path / 'pieces.ply', verts_ref, faces)
    assert open(tmp_path / 'default.ply', 'rb').read() == open(tmp_path / 'pieces.ply', 'rb').read()
    # a second run writes the same file
    extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=tmp_path / 'again.ply', marching='native',
                 keep='largest', min_faces=4, vertex_normals=True, vertex_colors=True, model=m, coords='sampled')
    assert open(tmp_path / 'again.ply', 'rb').read() == open(full, 'rb').read()
    with pytest.raises(ValueError, match='model'):
        extract_mesh(m.implicit_surface, volume_size=s, N=N, filepath=tmp_path / 'x.ply', marching='native',
                     vertex_colors=True)
