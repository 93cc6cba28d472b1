"""CPU checks of the mesh-finishing stage (neurecon_amd.mesh_util): the PLY writer with per-vertex normals
and colours, the index-space -> sample-space map of extract_mesh's grid, and the argument checks of the
nr_mesh_* entries (nr_meshops.hip).  No GPU: the library loads without one."""
import os
import struct

import numpy as np
import pytest
import torch

from test_mc_table import HEADER, read_ply

HEADER_FULL = ('ply\nformat binary_little_endian 1.0\nelement vertex {V}\nproperty float x\nproperty float y\n'
               'property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\n'
               'property uchar green\nproperty uchar blue\nelement face {F}\n'
               'property list uchar int vertex_indices\nend_header\n')

VERTS = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, -2.25], [1.5, 1, 1e-3]], np.float32)
FACES = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
NORMALS = np.array([[0, 0, 1], [0.6, 0, 0.8], [-1, 0, 0], [0, -0.28, 0.96]], np.float32)


def _split(path, vertex_bytes):
    data = open(path, 'rb').read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    hdr = data[:end].decode('ascii')
    V = int([l for l in hdr.split('\n') if l.startswith('element vertex')][0].split()[-1])
    F = int([l for l in hdr.split('\n') if l.startswith('element face')][0].split()[-1])
    assert len(data) == end + V * vertex_bytes + F * 13
    return hdr, data[end:end + V * vertex_bytes], data[end + V * vertex_bytes:]


def test_write_ply_with_normals_and_colours(tmp_path):
    """exact header, 27 bytes per vertex (3 float + 3 float + 3 uchar, packed), the quantisation rule
    floor(clamp(c, 0, 1) * 255 + 0.5) at 0, 1, 0.5 / 255 (the first value that rounds up to 1) and its
    neighbours, and outside [0, 1]"""
    from neurecon_amd.mesh_util import write_ply
    half = 0.5 / 255
    colors = np.array([[0.0, 1.0, half], [np.nextafter(half, 0), np.nextafter(half, 1), -3.0],
                       [7.5, 254.5 / 255 + 1e-9, 254.5 / 255 - 1e-9], [0.2, 0.5, 0.999]], np.float64)
    want_rgb = np.array([[0, 255, 1], [0, 1, 0], [255, 255, 254], [51, 128, 255]], np.uint8)
    want = HEADER_FULL.format(V=4, F=2).encode('ascii')
    want += b''.join(struct.pack('<ffffffBBB', *map(float, v), *map(float, n), *map(int, c))
                     for v, n, c in zip(VERTS, NORMALS, want_rgb))
    want += b''.join(struct.pack('<Biii', 3, *map(int, f)) for f in FACES)
    for name, args in (('np.ply', (VERTS, FACES, NORMALS, colors)),
                       ('t.ply', tuple(torch.from_numpy(a) for a in (VERTS, FACES, NORMALS, colors))),
                       ('u8.ply', (VERTS, FACES, NORMALS, want_rgb))):
        write_ply(tmp_path / name, args[0], args[1], normals=args[2], colors=args[3])
        assert open(tmp_path / name, 'rb').read() == want, name
    hdr, vbytes, _ = _split(tmp_path / 'np.ply', 27)
    assert hdr == HEADER_FULL.format(V=4, F=2)
    rec = np.frombuffer(vbytes, np.dtype([('p', '<f4', (3,)), ('n', '<f4', (3,)), ('c', 'u1', (3,))]))
    assert rec.dtype.itemsize == 27
    assert np.array_equal(rec['p'], VERTS) and np.array_equal(rec['n'], NORMALS) and np.array_equal(rec['c'], want_rgb)
    # fp32 colours go through the same rule
    c32 = np.array([[0.0, 1.0, 0.25]] * 4, np.float32)
    write_ply(tmp_path / 'c32.ply', VERTS, FACES, colors=c32)
    hdr, vbytes, _ = _split(tmp_path / 'c32.ply', 15)
    assert 'nx' not in hdr and 'property uchar blue\nelement face' in hdr
    rec = np.frombuffer(vbytes, np.dtype([('p', '<f4', (3,)), ('c', 'u1', (3,))]))
    assert np.array_equal(rec['c'], np.array([[0, 255, 64]] * 4, np.uint8))
    # normals alone: 24 bytes
    write_ply(tmp_path / 'n.ply', VERTS, FACES, normals=NORMALS)
    hdr, vbytes, _ = _split(tmp_path / 'n.ply', 24)
    assert 'red' not in hdr and 'property float nz\nelement face' in hdr
    assert np.array_equal(np.frombuffer(vbytes, '<f4').reshape(4, 6)[:, 3:], NORMALS)
    with pytest.raises(ValueError):
        write_ply(tmp_path / 'bad.ply', VERTS, FACES, normals=NORMALS[:3])
    with pytest.raises(ValueError):
        write_ply(tmp_path / 'bad.ply', VERTS, FACES, colors=np.zeros((4, 3), np.int32))


def test_write_ply_without_attributes_is_unchanged(tmp_path):
    from neurecon_amd.mesh_util import write_ply
    want = HEADER.format(V=4, F=2).encode('ascii')
    want += b''.join(struct.pack('<fff', *map(float, v)) for v in VERTS)
    want += b''.join(struct.pack('<Biii', 3, *map(int, f)) for f in FACES)
    write_ply(tmp_path / 'a.ply', VERTS, FACES, normals=None, colors=None)
    assert open(tmp_path / 'a.ply', 'rb').read() == want
    _, v, f = read_ply(tmp_path / 'a.ply')
    assert np.array_equal(v, VERTS) and np.array_equal(f, FACES)


def reference_grid_points(N, s):
    """the float64 point array of the reference's extract_mesh (mesh_util.py:87-100), np.int64 for np.int"""
    voxel_grid_origin = [-s / 2., -s / 2., -s / 2.]
    overall_index = np.arange(0, N ** 3, 1).astype(np.int64)
    xyz = np.zeros([N ** 3, 3])
    xyz[:, 2] = overall_index % N
    xyz[:, 1] = (overall_index / N) % N
    xyz[:, 0] = ((overall_index / N) / N) % N
    xyz[:, 0] = (xyz[:, 0] * (s / (N - 1))) + voxel_grid_origin[2]
    xyz[:, 1] = (xyz[:, 1] * (s / (N - 1))) + voxel_grid_origin[1]
    xyz[:, 2] = (xyz[:, 2] * (s / (N - 1))) + voxel_grid_origin[0]
    return xyz


@pytest.mark.parametrize('N, s', [(5, 2.0), (16, 1.5), (16, 2.0)])
def test_grid_sample_positions_at_every_integer_index(N, s):
    from neurecon_amd.mesh_util import grid_sample_positions
    want = reference_grid_points(N, s).astype(np.float32)
    ax = torch.arange(N)
    idx = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)       # row = flat index
    for dtype in (torch.int64, torch.float32, torch.float64):
        got = grid_sample_positions(idx.to(dtype), s, N)
        assert got.dtype == torch.float32 and got.shape == (N ** 3, 3)
        assert np.array_equal(got.numpy(), want), dtype
    # the sheared lattice is not the s / N lattice the writer assumes, nor the un-sheared s / (N - 1) one
    plain = (idx.double() * (s / (N - 1)) - s / 2).float().numpy()
    assert not np.array_equal(plain, want)


def test_grid_sample_positions_between_lattice_points():
    """N = 5, s = 2: step = 0.5.  Index (1, 2, 3.5) lies halfway on the axis-2 edge from (1, 2, 3) to (1, 2, 4):
    lattice (1, 2, 3) -> ((1 + 2/5 + 3/25) 0.5 - 1, (2 + 3/5) 0.5 - 1, 3 * 0.5 - 1) = (-0.24, 0.3, 0.5),
    lattice (1, 2, 4) -> ((1 + 2/5 + 4/25) 0.5 - 1, (2 + 4/5) 0.5 - 1, 4 * 0.5 - 1) = (-0.22, 0.4, 1.0),
    midpoint (-0.23, 0.35, 0.75); a quarter along axis 0 from (1, 2, 3): (-0.24 + 0.125, 0.3, 0.5)."""
    from neurecon_amd.mesh_util import grid_sample_positions
    got = grid_sample_positions(torch.tensor([[1, 2, 3.5], [1.25, 2, 3], [4, 4, 4], [3.75, 4, 4]]), 2.0, 5).double()
    want = torch.tensor([[-0.23, 0.35, 0.75], [-0.115, 0.3, 0.5], [(4 + 4 / 5 + 4 / 25) * 0.5 - 1, 1.4, 1.0],
                         [(3.75 + 4 / 5 + 4 / 25) * 0.5 - 1, 1.4, 1.0]], dtype=torch.float64)
    assert (got - want).abs().max() <= 2 ** -24            # half an fp32 ulp at |x| < 2 (one rounding)
    # affine: parameter t on an edge maps to parameter t between the two sampled points
    a, b = grid_sample_positions(torch.tensor([[2., 1, 3], [2., 2, 3]]), 1.5, 16).double()
    for t in (0.125, 0.5, 0.8125):
        mid = grid_sample_positions(torch.tensor([[2., 1 + t, 3]]), 1.5, 16).double()[0]
        assert (mid - ((1 - t) * a + t * b)).abs().max() <= 2 ** -23
    with pytest.raises(ValueError):
        grid_sample_positions(torch.zeros(4, 2), 2.0, 5)


@pytest.fixture(scope='module')
def lib():
    from neurecon_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def test_mesh_entries_check_arguments_without_gpu(lib):
    """every argument check comes before any HIP call (fake device pointers: nothing is dereferenced on the
    error paths): bad counts, null pointers, a small workspace, small capacities"""
    def err():
        return lib.nr_last_error().decode()
    assert lib.nr_mesh_workspace_bytes(-1, 0) == 0
    assert lib.nr_mesh_workspace_bytes(0, -1) == 0
    assert lib.nr_mesh_workspace_bytes(1 << 31, 0) == 0 and lib.nr_mesh_workspace_bytes(0, 1 << 31) == 0
    assert lib.nr_mesh_workspace_bytes(0, 0) > 0
    for V, F in ((1, 0), (1000, 600), (120644, 241284), ((1 << 31) - 1, (1 << 31) - 1)):
        assert 4 * V <= lib.nr_mesh_workspace_bytes(V, F) <= 4 * V + (V + F) // 64 + 2048, (V, F)
    V, F = 1000, 600
    ws = lib.nr_mesh_workspace_bytes(V, F)
    faces, labels, counts, tot, wsp, keep, out = 0x1000, 0x2000, 0x3000, 0x4000, 0x100000, 0x5000, 0x6000

    assert lib.nr_mesh_components(faces, -1, V, labels, counts, tot, wsp, ws, None) == -1 and 'counts' in err()
    assert lib.nr_mesh_components(faces, F, -1, labels, counts, tot, wsp, ws, None) == -1
    assert lib.nr_mesh_components(faces, 1 << 31, V, labels, counts, tot, wsp, 1 << 40, None) == -1
    assert lib.nr_mesh_components(None, F, V, labels, counts, tot, wsp, ws, None) == -1 and 'null' in err()
    assert lib.nr_mesh_components(faces, F, V, None, counts, tot, wsp, ws, None) == -1
    assert lib.nr_mesh_components(faces, F, V, labels, None, tot, wsp, ws, None) == -1
    assert lib.nr_mesh_components(faces, F, V, labels, counts, None, wsp, ws, None) == -1
    assert lib.nr_mesh_components(faces, F, V, labels, counts, tot, wsp, ws - 1, None) == -4 and 'workspace' in err()
    assert lib.nr_mesh_components(faces, F, V, labels, counts, tot, None, ws, None) == -4

    assert lib.nr_mesh_filter_count(faces, F, -1, keep, wsp, ws, tot, None) == -1 and 'counts' in err()
    assert lib.nr_mesh_filter_count(faces, -1, V, keep, wsp, ws, tot, None) == -1
    assert lib.nr_mesh_filter_count(None, F, V, keep, wsp, ws, tot, None) == -1 and 'null' in err()
    assert lib.nr_mesh_filter_count(faces, F, V, None, wsp, ws, tot, None) == -1
    assert lib.nr_mesh_filter_count(faces, F, V, keep, wsp, ws, None, None) == -1
    assert lib.nr_mesh_filter_count(faces, F, V, keep, wsp, ws - 1, tot, None) == -4 and 'workspace' in err()
    assert lib.nr_mesh_filter_count(faces, F, V, keep, None, ws, tot, None) == -4

    def emit(f=faces, nf=F, nv=V, vk=10, fk=20, vcap=10, fcap=20, wsb=ws, vkeep=keep, vsrc=out, fo=out):
        return lib.nr_mesh_filter_emit(f, nf, nv, vkeep, wsp, wsb, vk, fk, vsrc, vcap, fo, fcap, None)
    assert emit(nv=-1) == -1 and 'counts' in err()
    assert emit(nf=-1) == -1
    assert emit(f=None) == -1 and 'null' in err()
    assert emit(vkeep=None) == -1
    assert emit(vk=-1) == -1 and emit(fk=-1) == -1
    assert emit(vk=V + 1, vcap=V + 1) == -1 and emit(fk=F + 1, fcap=F + 1) == -1
    assert emit(vcap=9) == -1 and 'capacity' in err()
    assert emit(fcap=19) == -1 and 'capacity' in err()
    assert emit(vsrc=None) == -1 and 'null output' in err()
    assert emit(fo=None) == -1
    assert emit(wsb=ws - 1) == -4 and 'workspace' in err()
    assert emit(vk=0, fk=0, vcap=0, fcap=0, vsrc=None, fo=None) == 0          # nothing kept: no launch


def test_extract_mesh_refuses_bad_options_before_any_work():
    """the option checks need no GPU: they come before the grid"""
    from neurecon_amd import mesh_util
    with pytest.raises(ValueError, match='coords'):
        mesh_util.extract_mesh(None, coords='grid')
    for kw in (dict(keep='largest'), dict(min_faces=10), dict(vertex_normals=True), dict(vertex_colors=True),
               dict(coords='sampled')):
        with pytest.raises(ValueError, match=next(iter(kw))):
            mesh_util.extract_mesh(None, marching='skimage', **kw)
    with pytest.raises(ValueError, match='model'):
        mesh_util.extract_mesh(None, marching='native', vertex_colors=True)
    with pytest.raises(ValueError, match='keep'):
        mesh_util.filter_mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), keep='biggest')
