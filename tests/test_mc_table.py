"""CPU checks of the marching-cubes case table (nr_mc_table, generated in nr_mcubes.hip) and of the
built-in binary PLY writer (neurecon_amd.mesh_util.write_ply).  No GPU: the library loads without one.

Cube numbering (nr_mcubes.hip): corner c = 4 d0 + 2 d1 + d2; cube edge e = 4 a + 2 u + w along axis a,
base corner (0,u,w) / (u,0,w) / (u,w,0) for a = 0 / 1 / 2; case bit c set iff corner c is inside."""
import ctypes
import os
import struct

import numpy as np
import pytest


def edge_corners(e):
    a, u, w = e >> 2, (e >> 1) & 1, e & 1
    base = [(0, u, w), (u, 0, w), (u, w, 0)][a]
    end = list(base)
    end[a] = 1
    return 4 * base[0] + 2 * base[1] + base[2], 4 * end[0] + 2 * end[1] + end[2]


def crossing_edges(case):
    return [e for e in range(12) if ((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1]


def edge_faces(e):
    """the two cube faces (axis, side) a cube edge lies on"""
    a, u, w = e >> 2, (e >> 1) & 1, e & 1
    o = [x for x in range(3) if x != a]
    return {(o[0], u), (o[1], w)}


@pytest.fixture(scope='module')
def table():
    from neurecon_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.lib()
    tri = np.zeros((256, 16), np.int8)
    cnt = np.zeros(256, np.int32)
    assert lib.nr_mc_table(ctypes.c_void_p(tri.ctypes.data), ctypes.c_void_p(cnt.ctypes.data)) == 0, lib.nr_last_error()
    return tri, cnt


def _tris(tri, cnt, case):
    row = tri[case]
    n = int(cnt[case])
    assert (row[3 * n:] == -1).all() and (row[:3 * n] >= 0).all() and (row[:3 * n] < 12).all(), case
    return row[:3 * n].reshape(n, 3).tolist()


def test_table_null_arguments(table):
    from neurecon_amd import _lib
    assert _lib.lib().nr_mc_table(None, None) == -1


def test_mc_entries_check_arguments_without_gpu(table):
    """nr_mc_workspace_bytes keeps the memory condition (<= 6 bytes per voxel + 1 MiB); nr_mc_count and
    nr_mc_emit refuse bad dims, null pointers, small workspaces and small capacities before any HIP call
    (fake device pointers: nothing is dereferenced on the error paths)"""
    from neurecon_amd import _lib
    lib = _lib.lib()
    for dims in ((2, 2, 2), (3, 5, 130), (512, 512, 512), (2, 3, 1 << 30)):
        n = dims[0] * dims[1] * dims[2]
        assert n + 4 * n <= lib.nr_mc_workspace_bytes(*dims) <= 6 * n + (1 << 20), dims
    for dims in ((1, 9, 9), (9, 9, 0), (2, 2, (1 << 30) + 1), (1 << 20, 1 << 20, 2)):
        assert lib.nr_mc_workspace_bytes(*dims) == 0, dims
    ws = lib.nr_mc_workspace_bytes(8, 9, 10)
    vol, wsp, tot, out = 0x1000, 0x100000, 0x2000, 0x3000
    d3 = ctypes.c_double * 3
    one, zero = d3(1, 1, 1), d3(0, 0, 0)

    def err():
        return lib.nr_last_error().decode()
    assert lib.nr_mc_count(vol, 8, 1, 10, 0.0, wsp, ws, tot, None) == -1 and 'dims' in err()
    assert lib.nr_mc_count(None, 8, 9, 10, 0.0, wsp, ws, tot, None) == -1 and 'null' in err()
    assert lib.nr_mc_count(vol, 8, 9, 10, 0.0, wsp, ws, None, None) == -1
    assert lib.nr_mc_count(vol, 8, 9, 10, 0.0, wsp, ws - 1, tot, None) == -4 and 'workspace' in err()
    assert lib.nr_mc_count(vol, 8, 9, 10, 0.0, None, ws, tot, None) == -4

    def emit(nv=10, nf=20, vcap=10, fcap=20, wsb=ws, dims=(8, 9, 10), sp=one, verts=out):
        return lib.nr_mc_emit(vol, *dims, 0.0, sp, zero, 1.0, zero, wsp, wsb, nv, nf, verts, vcap, out, fcap, None)
    assert emit(dims=(8, 9, 1)) == -1 and 'dims' in err()
    assert emit(sp=None) == -1 and 'null' in err()
    assert emit(vcap=9) == -1 and 'capacity' in err()
    assert emit(fcap=19) == -1 and 'capacity' in err()
    assert emit(nv=1 << 31, vcap=1 << 31) == -1 and 'int32' in err()
    assert emit(nv=-1) == -1
    assert emit(verts=None) == -1 and 'null output' in err()
    assert emit(wsb=ws - 1) == -4 and 'workspace' in err()
    assert emit(nv=0, nf=0, vcap=0, fcap=0) == 0                    # empty: no launch


def test_table_counts_and_edges(table):
    tri, cnt = table
    assert cnt[0] == 0 and cnt[255] == 0
    assert (tri[0] == -1).all() and (tri[255] == -1).all()
    assert cnt.min() >= 0 and cnt.max() <= 5
    for case in range(256):
        used = {e for t in _tris(tri, cnt, case) for e in t}
        assert used == set(crossing_edges(case)), case
        if 0 < case < 255:
            assert cnt[case] >= 1


def test_table_loops_are_closed_and_on_faces(table):
    """Within a case an undirected vertex pair occurs at most twice (an interior fan edge, once in each
    direction); a pair that occurs once is a boundary segment: it lies on one cube face, and with
    direction these segments form closed loops (every vertex once as a start, once as an end)."""
    tri, cnt = table
    for case in range(256):
        directed = []
        for a, b, c in _tris(tri, cnt, case):
            assert len({a, b, c}) == 3, case
            directed += [(a, b), (b, c), (c, a)]
        und = {}
        for a, b in directed:
            und.setdefault(frozenset((a, b)), []).append((a, b))
        boundary = []
        for pair, lst in und.items():
            assert len(lst) <= 2, (case, pair)
            if len(lst) == 2:
                assert lst[0] == lst[1][::-1], (case, pair)      # shared by two triangles: opposite directions
                a, b = lst[0]
                # an interior diagonal never lies in a cube face (the neighbouring cell could double it)
                assert not edge_faces(a) & edge_faces(b), (case, pair)
            else:
                a, b = lst[0]
                assert edge_faces(a) & edge_faces(b), (case, pair)
                boundary.append((a, b))
        nxt = dict(boundary)
        assert len(nxt) == len(boundary), case                     # one segment out of every vertex
        assert sorted(nxt.values()) == sorted(nxt.keys()), case    # and one in
        assert set(nxt) == set(crossing_edges(case)), case
        seen = set()
        for s in nxt:
            x, n = s, 0
            while x not in seen:
                seen.add(x)
                x = nxt[x]
                n += 1
            assert n == 0 or n >= 3, case


def test_table_faces_agree_between_neighbours(table):
    """The segments on a cube face depend on that face's four corner classes only, and mirror exactly
    (same undirected segments, opposite direction) on the neighbouring cell's opposite face: what makes
    the mesh watertight."""
    tri, cnt = table

    def face_segments(case, axis, side):
        segs = set()
        for a, b, c in _tris(tri, cnt, case):
            for x, y in ((a, b), (b, c), (c, a)):
                if (axis, side) in edge_faces(x) & edge_faces(y):
                    segs.add((x, y))
        # drop fan-interior pairs (both directions present)
        return {(x, y) for x, y in segs if (y, x) not in segs}

    def mirror(e, axis):
        """the same grid edge seen from the neighbour across `axis`: side 1 <-> side 0"""
        a, u, w = e >> 2, (e >> 1) & 1, e & 1
        o = [x for x in range(3) if x != a]
        if o[0] == axis:
            u ^= 1
        else:
            w ^= 1
        return 4 * a + 2 * u + w

    for axis in range(3):
        bit = [4, 2, 1][axis]
        hi = [c for c in range(8) if c & bit]
        for case in range(256):
            s1 = face_segments(case, axis, 1)
            # a neighbour whose side-0 face carries this cell's side-1 classes (its far corners: all outside)
            nb = 0
            for c in hi:
                if (case >> c) & 1:
                    nb |= 1 << (c ^ bit)
            s0 = face_segments(nb, axis, 0)
            assert {(mirror(y, axis), mirror(x, axis)) for x, y in s1} == s0, (axis, case)


HEADER = ('ply\nformat binary_little_endian 1.0\nelement vertex {V}\nproperty float x\nproperty float y\n'
          'property float z\nelement face {F}\nproperty list uchar int vertex_indices\nend_header\n')


def read_ply(path):
    """minimal reader of the one layout write_ply produces"""
    data = open(path, 'rb').read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    lines = data[:end].decode('ascii').split('\n')
    V = int([l for l in lines if l.startswith('element vertex')][0].split()[-1])
    F = int([l for l in lines if l.startswith('element face')][0].split()[-1])
    verts = np.frombuffer(data, '<f4', V * 3, end).reshape(V, 3)
    rec = np.frombuffer(data, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), F, end + V * 12)
    assert end + V * 12 + F * 13 == len(data)
    assert (rec['n'] == 3).all()
    return data[:end].decode('ascii'), verts, rec['v']


def test_write_ply_bytes_and_roundtrip(tmp_path):
    import torch
    from neurecon_amd.mesh_util import write_ply
    verts = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, -2.25], [1.5, 1, 1e-3]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    want = HEADER.format(V=4, F=2).encode('ascii')
    want += b''.join(struct.pack('<fff', *map(float, v)) for v in verts)
    want += b''.join(struct.pack('<Biii', 3, *map(int, f)) for f in faces)
    for name, v, f in (('np.ply', verts, faces), ('t.ply', torch.from_numpy(verts), torch.from_numpy(faces)),
                       ('wide.ply', verts.astype(np.float64), faces.astype(np.int64))):
        p = tmp_path / name
        write_ply(p, v, f)
        assert open(p, 'rb').read() == want, name
    hdr, v, f = read_ply(tmp_path / 'np.ply')
    assert hdr == HEADER.format(V=4, F=2)
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    with pytest.raises(ValueError):
        write_ply(tmp_path / 'bad.ply', verts[:, :2], faces)
