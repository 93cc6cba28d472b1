"""numpy restatement of the two rules of mesh culling (neurecon_amd/csrc/nr_meshcull.hip): the dilation of a
mask by a square and the per-vertex, per-view test, float64, operation for operation (numpy never fuses a
product into a sum), so device results are compared by equality."""
import numpy as np

IN_IMAGE, IN_MASK, VISIBLE = 1, 2, 4


def ref_dilate(masks, radius):
    """masks [..., H, W] (non-zero is set) -> bool, same shape: set iff a set in-image pixel lies within `radius`
    in both row and column.  Rows then columns; each pass ORs the 2 r + 1 shifts of the zero-padded line (shifts
    beyond the image add nothing and are left out)."""
    m = np.asarray(masks) != 0
    r = int(radius)
    assert r >= 0
    for axis in (m.ndim - 1, m.ndim - 2):
        n = m.shape[axis]
        rr = min(r, n)
        pad = [(0, 0)] * m.ndim
        pad[axis] = (rr, rr)
        p = np.pad(m, pad)
        out = np.zeros_like(m)
        for s in range(2 * rr + 1):
            out |= np.take(p, np.arange(s, s + n), axis=axis)
        m = out
    return m


def ref_project(verts, c2w, K):
    """the renderer's vertex stage for one camera -> (p_c.z, u, v), float64 [V]"""
    w2c = np.linalg.inv(np.asarray(c2w).astype(np.float64))
    K = np.asarray(K).astype(np.float64)
    fx, fy, cx, cy, sk = K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all='ignore'):
        pc = [((w2c[k, 0] * v[:, 0] + w2c[k, 1] * v[:, 1]) + w2c[k, 2] * v[:, 2]) + w2c[k, 3] for k in range(3)]
        xp, yp = pc[0] / pc[2], pc[1] / pc[2]
        u = (fx * xp + sk * yp) + cx
        vv = fy * yp + cy
    return pc[2], u, vv


def ref_view_test(verts, c2w, K, H, W, masks=None, zdepth=None, face_id=None, depth_tol=0.0, near=1e-4):
    """-> dict(flags uint8 [B, V], counts int32 [V, 3], zmax float64 [B, V] (NaN where not in image or without
    depth)).  c2w [B, 4, 4], K one or one per camera; masks [B, H, W] (already dilated), zdepth / face_id [B, H, W]:
    the depth frames the visibility is judged against."""
    poses = np.asarray(c2w).reshape(-1, 4, 4)
    B = len(poses)
    Ks = np.asarray(K)
    Ks = np.broadcast_to(Ks.reshape(-1, *Ks.shape[-2:]), (B, *Ks.shape[-2:]))
    V = len(np.asarray(verts).reshape(-1, 3))
    flags = np.zeros((B, V), np.uint8)
    zmaxs = np.full((B, V), np.nan)
    for b in range(B):
        z, u, v = ref_project(verts, poses[b], Ks[b])
        with np.errstate(all='ignore'):
            ok = (np.isfinite(z) & np.isfinite(u) & np.isfinite(v) & (z >= near) & (u >= 0.0) & (u <= float(W - 1)) &
                  (v >= 0.0) & (v <= float(H - 1)))
        us, vs = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        bits = ok.astype(np.uint8) * IN_IMAGE
        if masks is not None:
            i, j = np.rint(us).astype(np.int64), np.rint(vs).astype(np.int64)
            bits |= (ok & (np.asarray(masks)[b][j, i] != 0)).astype(np.uint8) * IN_MASK
        if zdepth is not None:
            i0, j0 = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
            i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
            zd, fid = np.asarray(zdepth)[b], np.asarray(face_id)[b]
            zmax = None
            for jj, ii in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)):
                s = np.where(fid[jj, ii] < 0, np.inf, zd[jj, ii].astype(np.float64))
                zmax = s if zmax is None else np.where(s > zmax, s, zmax)
            with np.errstate(all='ignore'):
                vis = ok & (z <= zmax + float(depth_tol))
            bits |= vis.astype(np.uint8) * VISIBLE
            zmaxs[b] = np.where(ok, zmax, np.nan)
        flags[b] = bits
    counts = np.stack([((flags & bit) != 0).sum(0) for bit in (IN_IMAGE, IN_MASK, VISIBLE)], 1).astype(np.int32)
    return dict(flags=flags, counts=counts.reshape(V, 3), zmax=zmaxs)
