"""numpy restatement of the two rules of the mesh metrics (neurecon_amd/csrc/nr_nn.hip, nr_meshsample.hip):
a dense brute-force nearest-neighbour search and the stratified surface sampler, float64, operation for
operation (numpy never fuses a product into a sum), so device results are compared by equality."""
import numpy as np

INF = np.inf


def brute_nn(points, queries, max_dist=None, chunk=128):
    """-> (index int64 [M], d2 float64 [M]): the point with the smallest (d2, index); d2 = (dx dx + dy dy) + dz dz
    from the fp32 coordinates widened to float64; -1 / +inf for a non-finite query, when no finite point exists,
    and when d2 > max_dist max_dist.  Points with a non-finite coordinate are never neighbours."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    q = np.asarray(queries, np.float32).reshape(-1, 3).astype(np.float64)
    M = q.shape[0]
    index = np.full(M, -1, np.int64)
    d2 = np.full(M, INF)
    pf = np.isfinite(p).all(1)
    if not pf.any() or M == 0:
        return index, d2
    ids = np.flatnonzero(pf)          # ascending: argmin's first minimum is the smallest original index
    p = p[pf]
    for s in range(0, M, chunk):
        qc = q[s:s + chunk]
        qf = np.isfinite(qc).all(1)
        qc = np.where(qf[:, None], qc, 0.0)
        acc = qc[:, 0:1] - p[None, :, 0]
        acc *= acc                     # dx dx
        t = qc[:, 1:2] - p[None, :, 1]
        t *= t
        acc += t                       # (dx dx) + (dy dy)
        t = qc[:, 2:3] - p[None, :, 2]
        t *= t
        acc += t                       # ... + (dz dz)
        j = acc.argmin(1)
        best = acc[np.arange(len(qc)), j]
        index[s:s + chunk] = np.where(qf, ids[j], -1)
        d2[s:s + chunk] = np.where(qf, best, INF)
    if max_dist is not None:
        md = np.float64(max_dist)
        drop = ~(d2 <= md * md)
        index[drop] = -1
        d2[drop] = INF
    return index, d2


def face_areas(verts, faces):
    """-> (areas float64 [F], status): 0.5 |e1 x e2| in float64; an index outside [0, V) gives 0 (bit 0), a
    non-finite area 0 (bit 1)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < len(v))).all(1)
    g = np.where(valid[:, None], f, 0)
    status = 0 if valid.all() else 1
    if len(v) == 0:
        return np.zeros(len(f)), status
    v0, v1, v2 = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(invalid='ignore', over='ignore'):
        e1, e2 = v1 - v0, v2 - v0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        a = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    bad = valid & ~np.isfinite(a)
    if bad.any():
        status |= 2
    return np.where(valid & np.isfinite(a), a, 0.0), status


_SCALE = 1 << 1074  # every float64 times 2^1074 is an integer


def exact_prefix(areas):
    """the correctly rounded inclusive prefix sums (exact integer sums, one rounding each): what math.fsum of
    every prefix gives"""
    out, s = np.empty(len(areas)), 0
    for i, a in enumerate(areas.tolist()):
        n, d = a.as_integer_ratio()
        s += n * (_SCALE // d)
        out[i] = s / _SCALE
    return out


def sample_ref(verts, faces, cdf, u):
    """the sampler, given the device's cdf -> (points fp32 [n, 3], face_id int32 [n])"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cdf = np.asarray(cdf, np.float64)
    u = np.asarray(u, np.float64).reshape(-1, 3)
    n, F = len(u), len(cdf)
    total = cdf[-1]
    t = ((np.arange(n, dtype=np.float64) + u[:, 0]) / np.float64(n)) * total
    face = np.searchsorted(cdf, t, side='right')                       # the first f with cdf[f] > t
    face[face == F] = np.searchsorted(cdf, total, side='left')        # the first f with cdf[f] >= total
    a, b = u[:, 1].copy(), u[:, 2].copy()
    flip = a + b > 1.0
    a[flip], b[flip] = 1.0 - a[flip], 1.0 - b[flip]
    b0 = (1.0 - a) - b
    tri = v[f[face]]                                                  # [n, 3 vertices, 3]
    p = (b0[:, None] * tri[:, 0] + a[:, None] * tri[:, 1]) + b[:, None] * tri[:, 2]
    return p.astype(np.float32), face.astype(np.int32)
