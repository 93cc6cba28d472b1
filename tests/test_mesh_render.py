"""CPU checks of the mesh renderer (neurecon_amd.mesh_util.render_mesh / read_ply, nr_meshrender.hip): the two
numpy references the GPU tests compare the device against, checked against each other here, the PLY
reader, the fill rule and the argument checks of nr_mesh_render.  No GPU: the library loads without one.

(A) `ref_raster`: the rule in the header of nr_meshrender.hip restated operation for operation in float64
    and int64 (numpy rounds every elementwise operation on its own; the kernel file forbids contraction).
(B) `ref_cast`: an independent float64 Moeller-Trumbore ray cast over all rays x faces, nearest hit."""
import ctypes
import os
import struct

import numpy as np
import pytest

RT, AT = 1e-4, 1e-6           # the project's per-ray bar
H_STD, W_STD = 37, 53         # neither a multiple of anything
DELTA = 1.0 / 64              # robust pixels: the casts through (u +- DELTA, v +- DELTA) agree with the centre's


# ------------------------------------------------------------------------------------------------
# the standard scene
# ------------------------------------------------------------------------------------------------
def std_intrinsics():
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1] = 61, 57, 25.3, 17.9, 0.8
    return K


def std_pose(dist=3.2, a=0.7, b=-0.4, offset=(0.05, -0.03, 0.02)):
    """camera rotated about y then x, looking at the origin along its +z axis from `dist`, plus a small offset"""
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    R = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    c2w = np.eye(4)
    c2w[:3, :3] = R
    c2w[:3, 3] = -dist * R[:, 2] + np.asarray(offset)
    return c2w.astype(np.float32)


def icosphere(subdiv):
    """unit icosphere: 20 * 4^subdiv faces, outward orientation -> verts float32 [V, 3], faces int32 [F, 3]"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(subdiv):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v, np.float32), np.array(f, np.int32)


def sphere_attributes(verts):
    """vertex normals (the unit sphere's) and smooth colours in [0, 1]"""
    n = verts / np.linalg.norm(verts, axis=1, keepdims=True)
    return n.astype(np.float32), (0.5 + 0.5 * np.sin(3 * verts + [0.0, 1.0, 2.0])).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# (A) the rule, operation for operation
# ------------------------------------------------------------------------------------------------
def _cam(c2w, K):
    c2w = np.asarray(c2w).astype(np.float64)
    K = np.asarray(K).astype(np.float64)
    return np.linalg.inv(c2w), c2w[:3, :3], K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]


def _lift(i, j, fx, fy, cx, cy, sk):
    """nr_rays.hip:20-21 in float64: i = column, j = row (arrays)"""
    xl = (((i - cx) + (cy * sk) / fy) - (sk * j) / fy) / fx
    yl = (j - cy) / fy
    return xl, yl


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _edge(xa, ya, xb, yb, px, py):
    dx, dy = xb - xa, yb - ya
    e = dx * (py - ya) - dy * (px - xa)
    return (e > 0) | ((e == 0) & (bool(dy < 0) | bool(dy == 0 and dx > 0)))


def ref_raster(verts, faces, c2w, K, H, W, normals=None, colors=None, near=1e-4, ambient=0.3,
               base=(0.7, 0.7, 0.7), background=(1.0, 1.0, 1.0)):
    """-> dict like render_mesh's, numpy, plus cover [H, W]: how many faces cover each sample (before depth), and
    n_drawn: faces with a non-empty clipped box (the ones either rasteriser path walks)"""
    w2c, M, fx, fy, cx, cy, sk = _cam(c2w, K)
    v = np.asarray(verts).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    V = len(v)
    with np.errstate(all='ignore'):
        pc = np.stack([((w2c[k, 0] * v[:, 0] + w2c[k, 1] * v[:, 1]) + w2c[k, 2] * v[:, 2]) + w2c[k, 3]
                       for k in range(3)], 1) if V else np.zeros((0, 3))
        xp, yp = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
        uu = (fx * xp + sk * yp) + cx
        vv = fy * yp + cy
        ok = (np.isfinite(pc[:, 2]) & np.isfinite(uu) & np.isfinite(vv) & (pc[:, 2] >= near) &
              (np.abs(uu) <= 2.0 ** 20) & (np.abs(vv) <= 2.0 ** 20))
        X = np.where(ok, np.rint(256.0 * np.where(ok, uu, 0)), 0).astype(np.int64)
        Y = np.where(ok, np.rint(256.0 * np.where(ok, vv, 0)), 0).astype(np.int64)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    xl, yl = _lift(ii, jj, fx, fy, cx, cy, sk)
    miss = np.uint64(2 ** 64 - 1)
    keys = np.full((H, W), miss, np.uint64)
    cover = np.zeros((H, W), np.int64)
    n_clipped = n_degenerate = n_drawn = 0

    def plane(a, b, c):
        v0, e1, e2 = pc[a], pc[b] - pc[a], pc[c] - pc[a]
        n = _cross(e1, e2)
        return v0, e1, e2, n, _dot(n, v0)

    for f, (a, b, c) in enumerate(faces.tolist()):
        if not all(0 <= q < V for q in (a, b, c)):
            n_degenerate += 1
            continue
        if not (ok[a] and ok[b] and ok[c]):
            n_clipped += 1
            continue
        x0, y0, x1, y1, x2, y2 = (int(q) for q in (X[a], Y[a], X[b], Y[b], X[c], Y[c]))
        a2 = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if a2 == 0:
            n_degenerate += 1
            continue
        if a2 < 0:
            x1, y1, x2, y2 = x2, y2, x1, y1
        i0, i1 = max(-(-min(x0, x1, x2) // 256), 0), min(max(x0, x1, x2) // 256, W - 1)
        j0, j1 = max(-(-min(y0, y1, y2) // 256), 0), min(max(y0, y1, y2) // 256, H - 1)
        if i0 > i1 or j0 > j1:
            continue
        n_drawn += 1
        py, px = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64) * 256, np.arange(i0, i1 + 1, dtype=np.int64) * 256,
                             indexing='ij')
        cov = _edge(x0, y0, x1, y1, px, py) & _edge(x1, y1, x2, y2, px, py) & _edge(x2, y2, x0, y0, px, py)
        box = (slice(j0, j1 + 1), slice(i0, i1 + 1))
        cover[box] += cov
        _, _, _, n, num = plane(a, b, c)
        with np.errstate(all='ignore'):
            tz = num / ((n[0] * xl[box] + n[1] * yl[box]) + n[2])
        valid = cov & np.isfinite(tz) & (tz > 0)
        with np.errstate(all='ignore'):
            bits = tz.astype(np.float32).view(np.uint32).astype(np.uint64)
        key = (bits << np.uint64(32)) | np.uint64(f)
        keys[box] = np.where(valid & (key < keys[box]), key, keys[box])

    hit = keys != miss
    face_id = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    out = dict(face_id=face_id, mask=hit, cover=cover, n_clipped=n_clipped, n_degenerate=n_degenerate, n_drawn=n_drawn,
               depth=np.zeros((H, W), np.float32), depth_z=np.zeros((H, W), np.float32),
               normal=np.zeros((H, W, 3), np.float32), bary=np.zeros((H, W, 3), np.float32),
               rgb=np.tile(np.broadcast_to(np.asarray(background, np.float64), (3,)).astype(np.float32), (H, W, 1)))
    if not hit.any():
        return out
    fa = faces[face_id[hit]]
    v0, e1, e2 = pc[fa[:, 0]], pc[fa[:, 1]] - pc[fa[:, 0]], pc[fa[:, 2]] - pc[fa[:, 0]]
    n = _cross(e1, e2)
    x, y = xl[hit], yl[hit]
    tz = _dot(n, v0) / ((n[:, 0] * x + n[:, 1] * y) + n[:, 2])
    dw = np.stack([(M[k, 0] * x + M[k, 1] * y) + M[k, 2] for k in range(3)], 1)
    ln = np.sqrt(_dot(dw, dw))
    w = np.stack([tz * x, tz * y, tz], 1) - v0
    nn = _dot(n, n)
    b1 = _dot(_cross(w, e2), n) / nn
    b2 = _dot(_cross(e1, w), n) / nn
    b0 = (1.0 - b1) - b2

    def blend(attr):
        at = np.asarray(attr).astype(np.float64)
        p, q, r = at[fa[:, 0]], at[fa[:, 1]], at[fa[:, 2]]
        return (b0[:, None] * p + b1[:, None] * q) + b2[:, None] * r
    if normals is not None:
        m = blend(normals)
    else:
        m = _cross(v[fa[:, 1]] - v[fa[:, 0]], v[fa[:, 2]] - v[fa[:, 0]])
    ml = np.sqrt(_dot(m, m))
    with np.errstate(all='ignore'):
        nh = np.where(((ml > 0) & np.isfinite(ml))[:, None], m / ml[:, None], 0.0)
    shade = ambient + (1.0 - ambient) * np.abs(_dot(nh, dw) / ln)
    bs = blend(colors) if colors is not None else np.broadcast_to(np.asarray(base, np.float64), (len(fa), 3))
    out['depth'][hit] = (tz * ln).astype(np.float32)
    out['depth_z'][hit] = tz.astype(np.float32)
    out['bary'][hit] = np.stack([b0, b1, b2], 1).astype(np.float32)
    out['normal'][hit] = nh.astype(np.float32)
    out['rgb'][hit] = (bs * shade[:, None]).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------
# (B) ray casting
# ------------------------------------------------------------------------------------------------
def pixel_rays(c2w, K, H, W, du=0.0, dv=0.0):
    """world rays through the pixel coordinates (column + du, row + dv) -> origin [3], dirs [H * W, 3] (float64,
    not normalised)"""
    _, M, fx, fy, cx, cy, sk = _cam(c2w, K)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64) + dv, np.arange(W, dtype=np.float64) + du, indexing='ij')
    xl, yl = _lift(ii.reshape(-1), jj.reshape(-1), fx, fy, cx, cy, sk)
    return np.asarray(c2w).astype(np.float64)[:3, 3], np.stack([xl, yl, np.ones_like(xl)], 1) @ M.T


def ref_cast(verts, faces, origin, dirs, chunk=1 << 22):
    """Moeller-Trumbore, two-sided, nearest hit -> face [R] (-1: miss), depth [R]: distance along the
    normalised ray (inf at a miss)"""
    v = np.asarray(verts).astype(np.float64)[np.asarray(faces).astype(np.int64).reshape(-1, 3)]
    d = np.asarray(dirs).astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.asarray(origin).astype(np.float64), d.shape)
    R, F = len(d), len(v)
    face, depth = np.full(R, -1, np.int64), np.full(R, np.inf)
    if F == 0:
        return face, depth
    v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    step = max(1, chunk // F)
    for r0 in range(0, R, step):
        dd, oo = d[r0:r0 + step, None], o[r0:r0 + step, None]
        with np.errstate(all='ignore'):
            pv = np.cross(dd, e2[None])
            det = (e1[None] * pv).sum(-1)
            tv = oo - v0[None]
            bu = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1[None])
            bv = (dd * qv).sum(-1) / det
            t = (e2[None] * qv).sum(-1) / det
        good = (np.abs(det) > 1e-300) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0) & np.isfinite(t)
        t = np.where(good, t, np.inf)
        k = t.argmin(1)
        tk = t[np.arange(len(k)), k]
        face[r0:r0 + step] = np.where(np.isfinite(tk), k, -1)
        depth[r0:r0 + step] = tk
    return face, depth


def five_casts(verts, faces, c2w, K, H, W, centre=None):
    """the cast through every pixel and through its four DELTA corners -> faces [5, H, W], depths [5, H, W];
    `centre`: (origin, dirs) to use for the middle cast instead of the numpy rays"""
    fs, ds = [], []
    for du, dv in ((0, 0), (-DELTA, -DELTA), (DELTA, -DELTA), (-DELTA, DELTA), (DELTA, DELTA)):
        o, d = centre if (centre is not None and du == 0 and dv == 0) else pixel_rays(c2w, K, H, W, du, dv)
        f, t = ref_cast(verts, faces, o, d)
        fs.append(f.reshape(H, W))
        ds.append(t.reshape(H, W))
    return np.stack(fs), np.stack(ds)


def robust_pixels(fs):
    """-> (robust [H, W]: all five casts name the same face or all miss; touched [H, W]: any cast hits)"""
    return (fs == fs[0]).all(0), (fs >= 0).any(0)


def check_against_casts(name, face_id, depth, fs, ds):
    """on robust pixels the face equals B's and the depth is within the bar; non-robust pixels <= 5 % of the
    touched ones"""
    robust, touched = robust_pixels(fs)
    frac = float((touched & ~robust).sum()) / max(int(touched.sum()), 1)
    hit = robust & (fs[0] >= 0)
    err = np.abs(depth[hit].astype(np.float64) - ds[0][hit])
    bar = RT * np.abs(ds[0][hit]) + AT
    print(f'{name}: {int(touched.sum())} touched pixels, {frac * 100:.2f} % not robust, {int(hit.sum())} robust hits, '
          f'face mismatches {int((face_id[robust] != fs[0][robust]).sum())}, max depth err {err.max() if err.size else 0:.3e}')
    assert frac <= 0.05
    assert hit.sum() > 0.5 * touched.sum()
    assert np.array_equal(face_id[robust], fs[0][robust])
    assert (err <= bar).all()


@pytest.mark.parametrize('subdiv', [1, 2])
def test_rule_against_ray_cast(subdiv):
    verts, faces = icosphere(subdiv)
    assert len(faces) == 20 * 4 ** subdiv
    c2w, K = std_pose(), std_intrinsics()
    a = ref_raster(verts, faces, c2w, K, H_STD, W_STD)
    fs, ds = five_casts(verts, faces, c2w, K, H_STD, W_STD)
    check_against_casts(f'{len(faces)} faces', a['face_id'], a['depth'], fs, ds)
    assert a['n_clipped'] == 0 and 0 < a['mask'].sum() < H_STD * W_STD
    assert (a['cover'][a['mask']] >= 1).all()
    # depth_z is the camera-space z of the hit: depth = depth_z |d_w|
    _, d = pixel_rays(c2w, K, H_STD, W_STD)
    ln = np.linalg.norm(d, axis=1).reshape(H_STD, W_STD)
    assert np.allclose(a['depth'], a['depth_z'] * ln, rtol=1e-6, atol=0)
    assert np.abs(a['bary'][a['mask']].astype(np.float64).sum(1) - 1).max() <= 4 * 2.0 ** -23
    assert np.abs(np.linalg.norm(a['normal'][a['mask']].astype(np.float64), axis=1) - 1).max() <= 4 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------
# fill rule
# ------------------------------------------------------------------------------------------------
def fan_scene():
    """identity pose, fx = fy = 8, cx = cy = 4, no skew, 9 x 9 pixels; a fan of 8 faces in the plane z = 1 around
    the vertex that projects to pixel (4, 4), ring vertices at pixels (1|4|7, 1|4|7): every edge from the
    centre runs along a pixel row, column or diagonal, so the 8 shared edges and the shared vertex fall
    exactly on pixel samples.  Every other face is stored with the opposite winding."""
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 8
    K[0, 2] = K[1, 2] = 4
    pix = [(4, 4), (1, 1), (4, 1), (7, 1), (7, 4), (7, 7), (4, 7), (1, 7), (1, 4)]
    verts = np.array([((i - 4) / 8, (j - 4) / 8, 1.0) for i, j in pix], np.float32)
    faces = [(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)]
    faces = np.array([f if k % 2 == 0 else (f[0], f[2], f[1]) for k, f in enumerate(faces)], np.int32)
    return verts, faces, np.eye(4, dtype=np.float32), K, 9, 9


def fan_expected_mask():
    """the union is the square [1, 7]^2; its top and left edges are top / left edges, its bottom and right are not"""
    m = np.zeros((9, 9), bool)
    m[1:7, 1:7] = True
    return m


def test_fill_rule_shared_edges_and_vertex():
    verts, faces, c2w, K, H, W = fan_scene()
    a = ref_raster(verts, faces, c2w, K, H, W)
    assert a['n_clipped'] == 0 and a['n_degenerate'] == 0
    assert np.array_equal(a['cover'], fan_expected_mask().astype(np.int64))      # exactly one face per covered sample
    assert np.array_equal(a['mask'], fan_expected_mask())
    assert np.allclose(a['depth_z'][a['mask']], 1.0, rtol=0, atol=1e-6)
    # the samples on shared edges and the shared vertex: covered, once
    for i, j in ((4, 4), (2, 2), (3, 3), (4, 2), (4, 3), (5, 5), (2, 4), (5, 3), (3, 5), (4, 6), (6, 4)):
        assert a['cover'][j, i] == 1, (i, j)
    # one face alone covers its own samples whichever winding it is stored with
    for k in range(8):
        one = ref_raster(verts, faces[k:k + 1], c2w, K, H, W)['cover']
        flip = ref_raster(verts, faces[k:k + 1, ::-1], c2w, K, H, W)['cover']
        assert np.array_equal(one, flip) and one.max() == 1
    assert sum(ref_raster(verts, faces[k:k + 1], c2w, K, H, W)['cover'].sum() for k in range(8)) == 36


# ------------------------------------------------------------------------------------------------
# read_ply
# ------------------------------------------------------------------------------------------------
PLY_V = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, -2.25], [1.5, 1, 1e-3], [-7.125, 3e-8, 2.5e6]], np.float32)
PLY_F = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 3]], np.int32)
PLY_N = np.array([[0, 0, 1], [0.6, 0, 0.8], [-1, 0, 0], [0, -0.28, 0.96], [0.1, 0.2, 0.3]], np.float32)
PLY_C = np.array([[0, 255, 1], [0, 1, 0], [255, 255, 254], [51, 128, 255], [9, 8, 7]], np.uint8)


def _same(got, verts, faces, normals, colors):
    assert set(got) == {'verts', 'faces', 'normals', 'colors'}
    assert got['verts'].dtype == np.float32 and got['faces'].dtype == np.int32
    assert np.array_equal(got['verts'], verts) and np.array_equal(got['faces'], faces)
    for key, want, dtype in (('normals', normals, np.float32), ('colors', colors, np.uint8)):
        if want is None:
            assert got[key] is None
        else:
            assert got[key].dtype == dtype and np.array_equal(got[key], want)


@pytest.mark.parametrize('with_n, with_c, nbytes', [(False, False, 12), (True, False, 24), (False, True, 15),
                                                    (True, True, 27)])
def test_read_ply_round_trip(tmp_path, with_n, with_c, nbytes):
    from neurecon_amd.mesh_util import read_ply, write_ply
    n, c = (PLY_N if with_n else None), (PLY_C if with_c else None)
    path = tmp_path / 'm.ply'
    write_ply(path, PLY_V, PLY_F, normals=n, colors=c)
    data = open(path, 'rb').read()
    assert len(data) - data.index(b'end_header\n') - 11 == len(PLY_V) * nbytes + len(PLY_F) * 13
    _same(read_ply(path), PLY_V, PLY_F, n, c)
    # the same elements as ASCII (9 significant digits carry an fp32 value exactly), with a comment line
    hdr = data[:data.index(b'end_header\n')].decode().replace('binary_little_endian', 'ascii')
    hdr = hdr.replace('format ascii 1.0\n', 'format ascii 1.0\ncomment made by a test\n')
    rows = []
    for k in range(len(PLY_V)):
        row = ['%.9g' % x for x in PLY_V[k]] + (['%.9g' % x for x in PLY_N[k]] if with_n else [])
        rows.append(' '.join(row + ([str(int(x)) for x in PLY_C[k]] if with_c else [])))
    rows += ['3 %d %d %d' % tuple(f) for f in PLY_F]
    apath = tmp_path / 'a.ply'
    apath.write_text(hdr + 'end_header\n' + '\n'.join(rows) + '\n')
    _same(read_ply(apath), PLY_V, PLY_F, n, c)


def test_read_ply_skips_unknown_properties_and_empty_meshes(tmp_path):
    from neurecon_amd.mesh_util import read_ply, write_ply
    hdr = ('ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty double quality\nproperty float x\n'
           'property float y\nproperty uchar flag\nproperty float z\nproperty short s\nelement face 3\n'
           'property list uchar uint vertex_index\nend_header\n')
    body = b''.join(struct.pack('<dffBfh', 0.25 * k, v[0], v[1], k, v[2], -k) for k, v in enumerate(PLY_V.tolist()))
    body += b''.join(struct.pack('<BIII', 3, *f) for f in PLY_F.tolist())
    path = tmp_path / 'x.ply'
    path.write_bytes(hdr.encode() + body)
    _same(read_ply(path), PLY_V, PLY_F, None, None)
    write_ply(tmp_path / 'e.ply', np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    got = read_ply(tmp_path / 'e.ply')
    assert got['verts'].shape == (0, 3) and got['faces'].shape == (0, 3)


def test_read_ply_rejections(tmp_path):
    from neurecon_amd.mesh_util import read_ply, write_ply
    good = tmp_path / 'good.ply'
    write_ply(good, PLY_V, PLY_F, normals=PLY_N, colors=PLY_C)
    data = open(good, 'rb').read()
    end = data.index(b'end_header\n') + 11

    def bad(name, payload, match):
        p = tmp_path / name
        p.write_bytes(payload)
        with pytest.raises(ValueError, match=match):
            read_ply(p)
    # quads, binary and ASCII
    hdr = ('ply\nformat {} 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
           'element face 1\nproperty list uchar int vertex_indices\nend_header\n')
    quad = b''.join(struct.pack('<fff', *v) for v in PLY_V[:4].tolist()) + struct.pack('<Biiii', 4, 0, 1, 3, 2)
    bad('quad.ply', hdr.format('binary_little_endian').encode() + quad, 'triangle')
    bad('quad_a.ply', (hdr.format('ascii') + '0 0 0\n1 0 0\n0 1 0\n1 1 0\n4 0 1 3 2\n').encode(), 'triangle')
    # a triangle first, a quad second: the record sizes no longer add up
    mixed = hdr.replace('element face 1', 'element face 2').format('binary_little_endian').encode()
    bad('mixed.ply', mixed + quad[:48] + struct.pack('<Biii', 3, 0, 1, 2) + quad[48:], 'triangle')
    # truncated: in the faces, in the vertices, in the header
    bad('cut_f.ply', data[:-5], 'truncated')
    bad('cut_v.ply', data[:end + 40], 'truncated')
    bad('cut_h.ply', data[:end - 15], 'end_header')
    bad('cut_a.ply', (hdr.format('ascii') + '0 0 0\n1 0 0\n0 1 0\n1 1 0\n3 0 1\n').encode(), 'truncated')
    # bytes after the last face: said as such, like the ASCII reader's extra values
    bad('tail.ply', data + b'\0\0', 'extra bytes')
    bad('tail_a.ply', (hdr.format('ascii') + '0 0 0\n1 0 0\n0 1 0\n1 1 0\n3 0 1 3\n7\n').encode(), 'extra values')
    # big-endian, and not a PLY
    bad('big.ply', data.replace(b'binary_little_endian', b'binary_big_endian'), 'big-endian')
    bad('not.ply', b'solid cube\n', 'not a PLY')
    bad('type.ply', data.replace(b'property float nx', b'property half nx'), 'unknown property type')


# ------------------------------------------------------------------------------------------------
# argument checks
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from neurecon_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def _args(lib, V=100, F=50, H=H_STD, W=W_STD):
    """valid arguments with fake device pointers: the checks come before any HIP call"""
    from neurecon_amd import _lib
    a = _lib.NrMeshRenderArgs()
    a.verts, a.faces, a.V, a.F, a.H, a.W = 0x1000, 0x2000, V, F, H, W
    a.w2c[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    a.m[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    a.fx, a.fy, a.cx, a.cy, a.skew, a.near, a.large_threshold, a.ambient = 61, 57, 25.3, 17.9, 0.8, 1e-4, 64, 0.3
    a.depth, a.counters, a.workspace = 0x3000, 0x4000, 0x100000
    a.workspace_bytes = lib.nr_mesh_render_workspace_bytes(max(V, 0), max(F, 0), max(H, 1), max(W, 1))
    return a


def test_mesh_render_checks_arguments_without_gpu(lib):
    def call(a):
        return lib.nr_mesh_render(None if a is None else ctypes.byref(a), None), lib.nr_last_error().decode()
    rc, msg = call(None)
    assert rc == -1 and 'null argument' in msg
    a = _args(lib)
    a.verts = None
    rc, msg = call(a)
    assert rc == -1 and 'null verts' in msg
    a = _args(lib)
    a.faces = None
    assert call(a)[0] == -1
    for H, W in ((0, W_STD), (-3, W_STD), (H_STD, 0)):
        rc, msg = call(_args(lib, H=H, W=W))
        assert rc == -1 and 'H and W' in msg
    rc, msg = call(_args(lib, F=-1))
    assert rc == -1 and 'negative' in msg
    assert call(_args(lib, V=-1))[0] == -1
    rc, msg = call(_args(lib, F=2 ** 31 - 1))
    assert rc == -1 and 'INT32_MAX' in msg
    rc, msg = call(_args(lib, H=1 << 16, W=1 << 15))                     # H W = 2^31
    assert rc == -1 and '2^31' in msg
    a = _args(lib)
    a.workspace_bytes -= 1
    rc, msg = call(a)
    assert rc == -4 and 'workspace' in msg
    a = _args(lib)
    a.workspace = None
    assert call(a)[0] == -4
    for field, value in (('near', 0.0), ('near', float('nan')), ('fx', 0.0), ('cy', float('inf')), ('large_threshold', -1)):
        a = _args(lib)
        setattr(a, field, value)
        assert call(a)[0] == -1, field
    a = _args(lib)
    a.w2c[5] = float('nan')
    assert call(a)[0] == -1


def test_mesh_render_workspace_size(lib):
    ws = lib.nr_mesh_render_workspace_bytes
    assert ws(-1, 0, 1, 1) == 0 and ws(0, -1, 1, 1) == 0 and ws(0, 0, 0, 1) == 0 and ws(0, 0, 1, 0) == 0
    assert ws(0, 2 ** 31 - 1, 1, 1) == 0 and ws(0, 0, 1 << 16, 1 << 15) == 0
    assert ws(0, 0, 1, 1) > 0
    for V, F, H, W in ((1, 1, 1, 1), (42, 80, H_STD, W_STD), (1_500_000, 3_000_000, 600, 800)):
        want = 32 * V + 4 * F + 8 * H * W
        assert want <= ws(V, F, H, W) <= want + 5 * 256


def test_render_mesh_refuses_bad_input_before_any_work():
    """the option checks need no GPU"""
    from neurecon_amd.mesh_util import render_mesh
    verts, faces = icosphere(0)
    with pytest.raises(ValueError, match='needs'):
        render_mesh(verts, faces)
    with pytest.raises(ValueError, match='H, W'):
        render_mesh(verts, faces, std_pose(), std_intrinsics(), 0, 5)
    with pytest.raises(ValueError, match='H, W'):
        render_mesh(verts, faces, std_pose(), std_intrinsics(), 1 << 16, 1 << 15)
