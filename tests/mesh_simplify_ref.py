"""numpy restatement of the vertex-clustering rule in the header comment of neurecon_amd/csrc/nr_meshsimplify.hip
(neurecon_amd.mesh_simplify.simplify_mesh), operation for operation: numpy rounds every elementwise float64
operation on its own, the kernel file forbids contraction, and every sum is an integer sum.  The device is
compared to this by equality.

    verts fp32 [V, 3], faces int [F, 3], h > 0, lo[3] float64, dim[3] ints
    t = (x - lo) / h;  c = clamp(floor(t), 0, dim - 1);  cell = (c_z dim_y + c_y) dim_x + c_x
    cluster id = rank of the cell among the occupied cells, ascending
    f = clamp(t - c, 0, 1);  q = min(floor(f 2^20), 2^20 - 1);  S = sum q, n = count (integers)
    m = lo + (c + S / (n 2^20)) h
    d2 = ((dx dx) + (dy dy)) + (dz dz), dx = x - m_x;  index[k] = the member with the smallest (d2, index)
    'average': vertex k = (float) m;  'nearest': vertex k = verts[index[k]]
    face f survives iff its clusters (A, B, C) are pairwise distinct and no g < f with pairwise distinct clusters
    has the same unordered set; survivors in ascending f as (A, B, C) in the original order."""
import numpy as np

Q = 2.0 ** 20


def grid_of(verts, h):
    """the wrapper's grid: lo / hi the exact per-axis min / max, dim = floor((hi - lo) / h) + 1 in float64"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    dim = (np.floor((hi - lo) / np.float64(h)) + 1.0).astype(np.int64)
    return lo, dim


def simplify_ref(verts, faces, h, position='average', lo=None, dim=None):
    """-> dict(verts [K, 3] float32, faces [F', 3] int64, index [K], vertex_cluster [V], cluster_size [K], mean
    [K, 3] float64, cell [V], lo, dim)"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    if not np.isfinite(v).all():
        raise ValueError('a vertex coordinate is not finite')
    if fc.size and (fc.min() < 0 or fc.max() >= V):
        raise ValueError(f'faces name a vertex outside [0, {V})')
    h = np.float64(h)
    if lo is None:
        lo, dim = grid_of(v, h)
    lo, dim = np.asarray(lo, np.float64), np.asarray(dim, np.int64)
    x = v.astype(np.float64)
    t = (x - lo) / h
    c = np.clip(np.floor(t), 0.0, (dim - 1).astype(np.float64))
    ci = c.astype(np.int64)
    cell = (ci[:, 2] * dim[1] + ci[:, 1]) * dim[0] + ci[:, 0]
    f = np.clip(t - c, 0.0, 1.0)
    q = np.minimum(np.floor(f * Q), Q - 1.0).astype(np.int64)
    occupied, vclu = np.unique(cell, return_inverse=True)            # ascending cell: the rank is the id
    vclu = vclu.reshape(-1).astype(np.int64)
    K = len(occupied)
    n = np.bincount(vclu, minlength=K).astype(np.int64)
    S = np.zeros((K, 3), np.int64)
    np.add.at(S, vclu, q)
    cc = np.stack([occupied % dim[0], (occupied // dim[0]) % dim[1], occupied // (dim[0] * dim[1])], 1)
    den = n.astype(np.float64) * Q
    m = lo + (cc.astype(np.float64) + S.astype(np.float64) / den[:, None]) * h
    d = x - m[vclu]
    d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
    order = np.lexsort((np.arange(V), d2, vclu))                     # by cluster, then d2, then index
    first = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if K else np.zeros(0, np.int64)
    index = order[first]
    out_v = m.astype(np.float32) if position == 'average' else v[index]
    if position not in ('average', 'nearest'):
        raise ValueError(position)
    # faces
    t3 = vclu[fc] if len(fc) else np.zeros((0, 3), np.int64)
    distinct = (t3[:, 0] != t3[:, 1]) & (t3[:, 1] != t3[:, 2]) & (t3[:, 0] != t3[:, 2])
    ids = np.flatnonzero(distinct)
    key = np.sort(t3[ids], 1)
    o = np.lexsort((ids, key[:, 2], key[:, 1], key[:, 0]))           # equal keys: ascending face index
    ks = key[o]
    head = np.ones(len(o), bool)
    head[1:] = (ks[1:] != ks[:-1]).any(1)
    keep = np.sort(ids[o[head]])
    return dict(verts=out_v, faces=t3[keep], index=index, vertex_cluster=vclu, cluster_size=n, mean=m, cell=cell,
                lo=lo, dim=dim, kept_faces=keep)
