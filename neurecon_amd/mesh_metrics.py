"""Evaluate an extracted mesh against a ground-truth point cloud, on the device.

NeuS, VolSDF and UNISURF are published against one number: the Chamfer distance of the extracted mesh to a
ground-truth cloud (the DTU protocol), with precision, recall and F-score at a threshold as its companions.
This module closes train -> extract -> finish -> render -> evaluate without leaving the package or the device:

* `sample_mesh_surface`: area-weighted, stratified points on the mesh (libnrhip `nr_mesh_face_cdf` +
  `nr_mesh_sample`, neurecon_amd/csrc/nr_meshsample.hip).
* `nearest_points`: the exact nearest neighbour of every query in a point set on a uniform grid (libnrhip
  `nr_nn_build` + `nr_nn_query`, neurecon_amd/csrc/nr_nn.hip), in place of a host k-d tree over millions of
  points.  The result is the one a dense float64 brute force gives, bit for bit (a distance tie goes to the
  smaller index).
* `metrics_from_distances`: accuracy, completeness, Chamfer, precision / recall / F-score from two distance
  arrays; a pure function, host or device input.
* `evaluate_mesh`: the three chained.  `read_ply_points` reads a ground-truth cloud (a PLY without faces,
  which `mesh_util.read_ply` rightly refuses).

    python -m neurecon_amd.mesh_metrics pred.ply gt.ply --samples N [--max-dist D] [--threshold T ...] [--seed S]

prints the metrics as one JSON line.

Both kernels' results are pure functions of their inputs (two runs are bit-identical); the rules are stated in
the header comments of the two .hip files and restated in numpy in tests/mesh_metrics_ref.py.

Out of scope: DTU's greedy radius thinning of the sampled cloud (the stratified sampler gives an even cloud
instead), reading DTU's `.mat` ObsMask / plane files (pass the mask you derived from them as `gt_mask`),
point-to-triangle distance (distances are between points: sample densely), sharding across ranks.  Culling
the mesh by the cameras' masks and visibility before it is scored, as the published DTU figures do, is
`neurecon_amd.mesh_cull`.
"""
import argparse
import ctypes
import json
import math
import sys

import numpy as np
import torch

from . import _lib as L
from .mesh_util import _mesh_faces, _ply_header, _PLY_TYPES, read_ply

_MAX_CELLS = 1 << 26  # the library's cap on grid cells is max(1, min(4 N, 2^26))


def _device_of(*xs):
    dev = next((t.device for t in xs if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError('neurecon_amd: mesh_metrics needs a GPU (ROCm) device; the path is HIP-only')
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _points(a, dev, name):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f'{name} must be [N, 3], got {tuple(t.shape)}')
    if t.shape[0] >= 2 ** 31:
        raise ValueError(f'{name}: {t.shape[0]} rows do not fit int32 indices')
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def sample_mesh_surface(verts, faces, n, u=None, generator=None):
    """n points on the surface of an indexed triangle mesh, area-weighted and stratified, on the device ->
    (points [n, 3] fp32, face_id [n] int32, cdf [F] float64), device tensors.

    verts [V, 3], faces [F, 3] (tensors or arrays); u: float64 [n, 3] uniforms in [0, 1) on the device,
    default `torch.rand` with `generator`.  Sample k lies at t = ((k + u[k,0]) / n) total on the cumulative
    face area `cdf` (so face f receives n a_f / total samples to within 2), in face `face_id[k]` at the
    barycentrics given by u[k,1], u[k,2] (reflected into the triangle; no square root).  Faces of area 0, faces
    naming a vertex outside [0, V) (never dereferenced) and faces with a non-finite vertex are never chosen.
    Every output is a pure function of (verts, faces, u).  A mesh of total area 0, or n == 0, gives empty
    points and face_id: no error.  The rule in full: neurecon_amd/csrc/nr_meshsample.hip."""
    n = int(n)
    if not 0 <= n < 2 ** 31:
        raise ValueError(f'sample_mesh_surface: n must be in [0, 2^31), got {n}')
    dev = _device_of(verts, faces, u)
    v = _points(verts, dev, 'verts')
    ft = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
    f, V = _mesh_faces(ft.reshape(-1, 3).to(dev) if ft.numel() == 0 else ft.to(dev), v.shape[0])
    F = f.shape[0]
    if u is None:
        u = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=generator)
    else:
        L.require_gpu(u, 'u')
        if u.dtype != torch.float64 or tuple(u.shape) != (n, 3):
            raise ValueError(f'sample_mesh_surface: u must be float64 [{n}, 3], got {u.dtype} {tuple(u.shape)}')
        u = u.detach().to(dev).contiguous()
    lib = L.lib()
    with torch.cuda.device(dev):
        ws_bytes = lib.nr_mesh_sample_workspace_bytes(F)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        cdf = torch.empty(F, dtype=torch.float64, device=dev)
        info = torch.empty(2, dtype=torch.float64, device=dev)
        st = L.stream_of(dev)
        L.check(lib.nr_mesh_face_cdf(L.ptr(v) if V else None, V, L.ptr(f) if F else None, F,
                                     L.ptr(cdf) if F else None, L.ptr(info), L.ptr(ws), ws_bytes, st))
        total = float(info[0].item())  # the one host read: 16 bytes
        if not math.isfinite(total):
            raise ValueError('sample_mesh_surface: the total face area is not finite')
        if n == 0 or total <= 0.0:
            return (torch.empty((0, 3), dtype=torch.float32, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev), cdf)
        points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        face_id = torch.empty(n, dtype=torch.int32, device=dev)
        L.check(lib.nr_mesh_sample(L.ptr(v), V, L.ptr(f), F, L.ptr(cdf), L.ptr(u), n, L.ptr(points), L.ptr(face_id),
                                   st))
    return points, face_id, cdf


def default_cell_size(lo, hi, n):
    """The cell size `nearest_points` uses when none is given, from the box [lo, hi] of n points: about 8
    points per occupied cell for points that lie on a surface (h^2 = 8 A / n with A = half the box's surface
    area; a line: 8 points per cell along it), not below the size at which the grid reaches the library's cap
    of min(4 n, 2^26) cells (which is what binds for large clouds)."""
    e = [max(float(b) - float(a), 0.0) for a, b in zip(lo, hi)]
    cap = max(1, min(4 * int(n), _MAX_CELLS))
    n = max(int(n), 1)
    area = e[0] * e[1] + e[1] * e[2] + e[2] * e[0]
    if area > 0.0:
        h = math.sqrt(8.0 * area / n)
    elif max(e) > 0.0:
        h = 8.0 * max(e) / n
    else:
        return 1.0
    h = max(h, max(e) * 2.0 ** -40)
    for _ in range(4096):  # the +1 per axis makes this a search; it ends once h exceeds the largest extent
        if (math.floor(e[0] / h) + 1) * (math.floor(e[1] / h) + 1) * (math.floor(e[2] / h) + 1) <= cap:
            break
        h *= 1.03
    return h


def nearest_points(points, queries, max_dist=None, cell_size=None):
    """Exact nearest neighbour of every query among `points`, on the device -> (index int64 [M], dist float64
    [M], d2 float64 [M]), device tensors; dist = sqrt(d2).

    points [N, 3], queries [M, 3]: fp32 (tensors or arrays; other dtypes are converted).  d2 is the squared
    distance evaluated in float64 as (dx dx + dy dy) + dz dz; the neighbour is the point with the smallest
    (d2, index), so a tie goes to the smaller index and the result is the one a dense brute force gives, bit
    for bit, two runs alike.  max_dist: the neighbour is kept iff d2 <= max_dist^2, otherwise index -1 and
    dist = d2 = +inf (and the search stops early: give it whenever the metric has one).  Points with a
    non-finite coordinate are never neighbours; a query with one, and every query when there is no finite point,
    gets -1 / +inf.  cell_size: the grid's cell size (default `default_cell_size`); it changes the speed, never
    the result.  The rule in full and why the ring search is exact: neurecon_amd/csrc/nr_nn.hip."""
    dev = _device_of(points, queries)
    p, q = _points(points, dev, 'points'), _points(queries, dev, 'queries')
    N, M = p.shape[0], q.shape[0]
    md = math.inf if max_dist is None else float(max_dist)
    if not md >= 0.0:
        raise ValueError(f'nearest_points: max_dist must be >= 0, got {max_dist}')
    if cell_size is not None and not (0.0 < float(cell_size) < math.inf):
        raise ValueError(f'nearest_points: cell_size must be finite and > 0, got {cell_size}')
    lib = L.lib()
    with torch.cuda.device(dev):
        ws_bytes = lib.nr_nn_workspace_bytes(N, M)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = L.stream_of(dev)
        if cell_size is None:
            bounds = torch.empty(8, dtype=torch.float64, device=dev)
            L.check(lib.nr_nn_bounds(L.ptr(p) if N else None, N, L.ptr(bounds), L.ptr(ws), ws_bytes, st))
            b = bounds.cpu().tolist()  # a host read of 64 bytes
            h = default_cell_size(b[0:3], b[3:6], N)
        else:
            h = float(cell_size)
        index = torch.empty(M, dtype=torch.int32, device=dev)
        d2 = torch.empty(M, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int64, device=dev)
        L.check(lib.nr_nn_build(L.ptr(p) if N else None, N, ctypes.c_double(h), L.ptr(ws), ws_bytes, st))
        L.check(lib.nr_nn_query(N, L.ptr(q) if M else None, M, ctypes.c_double(md),
                                L.ptr(index) if M else None, L.ptr(d2) if M else None, L.ptr(status), L.ptr(ws),
                                ws_bytes, st))
        s = int(status.item())
    if s & ~1:
        raise L.NrError(f'nr_nn_query: status {s} (bit 1: the ring cap was reached; bit 2: no build in the workspace)')
    return index.long(), torch.sqrt(d2), d2


def _host64(d):
    if isinstance(d, torch.Tensor):
        d = d.detach().cpu().numpy()
    return np.asarray(d, dtype=np.float64).reshape(-1)


def metrics_from_distances(d_pred_to_gt, d_gt_to_pred, max_dist=None, thresholds=()):
    """Accuracy, completeness, Chamfer distance and precision / recall / F-score from two arrays of distances
    (numpy or torch, host or device) -> dict of Python numbers and lists.

    accuracy / completeness: the mean of the pred -> gt / gt -> pred distances that are < max_dist (DTU's
    convention: the far ones are excluded, not clipped; without max_dist every finite distance counts);
    chamfer = (accuracy + completeness) / 2.  Per threshold t: precision = the share of ALL pred -> gt distances
    that are <= t, recall the same of gt -> pred, fscore their harmonic mean (0 when both are 0).  n_pred / n_gt:
    the array lengths; n_*_used / n_*_excluded: the distances that entered the mean and those that did not.  An
    empty side (or one with nothing < max_dist) gives NaN for its mean and shares; nothing raises."""
    dp, dg = _host64(d_pred_to_gt), _host64(d_gt_to_pred)
    md = math.inf if max_dist is None else float(max_dist)
    out = {}
    means = []
    for name, key, d in (('accuracy', 'pred', dp), ('completeness', 'gt', dg)):
        used = d[d < md]
        mean = float(used.mean()) if used.size else math.nan
        means.append(mean)
        out[name] = mean
        out[f'n_{key}'] = int(d.size)
        out[f'n_{key}_used'] = int(used.size)
        out[f'n_{key}_excluded'] = int(d.size - used.size)
    out['chamfer'] = (means[0] + means[1]) / 2.0
    out['max_dist'] = None if max_dist is None else md
    out['thresholds'] = [float(t) for t in thresholds]
    out['precision'], out['recall'], out['fscore'] = [], [], []
    for t in out['thresholds']:
        pr = float((dp <= t).sum()) / dp.size if dp.size else math.nan
        rc = float((dg <= t).sum()) / dg.size if dg.size else math.nan
        out['precision'].append(pr)
        out['recall'].append(rc)
        out['fscore'].append(0.0 if pr == 0.0 and rc == 0.0 else 2.0 * pr * rc / (pr + rc))
    return out


def evaluate_mesh(verts, faces, gt_points, n_samples, max_dist=None, thresholds=(), gt_mask=None, u=None):
    """Sample `n_samples` points on the mesh, search both ways against the ground-truth cloud, and return
    `metrics_from_distances` of the two distance arrays -- all on the device but the final reductions.

    gt_points [N, 3]; gt_mask: bool [N], drops ground-truth points before both searches (a visibility mask such
    as DTU's ObsMask, derived by the caller); u: the sampler's uniforms (float64 [n_samples, 3], device), default
    fresh `torch.rand`.  The searches are bounded by max_dist when every threshold is <= max_dist."""
    dev = _device_of(verts, faces, gt_points)
    gt = _points(gt_points, dev, 'gt_points')
    if gt_mask is not None:
        m = torch.as_tensor(gt_mask, device=dev).reshape(-1)
        if m.dtype != torch.bool or m.shape[0] != gt.shape[0]:
            raise ValueError(f'evaluate_mesh: gt_mask must be bool [{gt.shape[0]}], got {m.dtype} {tuple(m.shape)}')
        gt = gt[m].contiguous()
    pred, _, _ = sample_mesh_surface(verts, faces, n_samples, u=u)
    thresholds = tuple(float(t) for t in thresholds)
    bound = max_dist if max_dist is not None and all(t <= float(max_dist) for t in thresholds) else None
    _, d_pg, _ = nearest_points(gt, pred, max_dist=bound)
    _, d_gp, _ = nearest_points(pred, gt, max_dist=bound)
    return metrics_from_distances(d_pg, d_gp, max_dist=max_dist, thresholds=thresholds)


def read_ply_points(path):
    """Read the points of a PLY file -> dict(points [V, 3] float32, normals [V, 3] float32 or None), numpy arrays:
    x y z (and nx ny nz when all three are there) of the `vertex` element, which must come first; every other
    scalar vertex property is skipped by its declared size, and whatever follows the vertices (a `face` element
    or none: ground-truth clouds have no faces) is not read.  binary_little_endian and ascii.  Raises ValueError
    for a file without a leading vertex element, a list property among the vertex properties, missing x / y / z,
    a big-endian file and a truncated body."""
    with open(path, 'rb') as f:
        data = f.read()
    fmt, elements, pos = _ply_header(data, path)
    if not elements or elements[0][0] != 'vertex':
        raise ValueError(f'read_ply_points: {path}: the first element must be vertex, got {[e[0] for e in elements]}')
    _, V, vprops = elements[0]
    if V < 0 or any(p[0] == 'list' for p in vprops):
        raise ValueError(f'read_ply_points: {path}: needs scalar vertex properties')
    names = [p[1] for p in vprops]
    if len(set(names)) != len(names) or not all(k in names for k in 'xyz'):
        raise ValueError(f'read_ply_points: {path}: vertex properties {names} must be distinct and hold x, y, z')
    if fmt == 'ascii':
        tok = data[pos:].split()
        nv = V * len(names)
        if len(tok) < nv:
            raise ValueError(f'read_ply_points: {path} is truncated')
        try:
            vtab = np.array(tok[:nv], dtype=np.float64).reshape(V, len(names))
        except ValueError as e:
            raise ValueError(f'read_ply_points: {path}: bad number in the body') from e
        col = {n: vtab[:, k] for k, n in enumerate(names)}
    else:
        vdt = np.dtype([(n, '<' + _PLY_TYPES[p[0]]) for n, p in zip(names, vprops)])
        if len(data) - pos < V * vdt.itemsize:
            raise ValueError(f'read_ply_points: {path} is truncated')
        vrec = np.frombuffer(data, vdt, V, pos)
        col = {n: vrec[n] for n in names}

    def cols(keys):
        return np.stack([col[k] for k in keys], 1).astype(np.float32) if all(k in col for k in keys) else None
    return dict(points=cols('xyz'), normals=cols(('nx', 'ny', 'nz')))


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m neurecon_amd.mesh_metrics',
                                 description='Chamfer distance, precision, recall and F-score of a mesh (PLY) against '
                                             'a ground-truth point cloud (PLY), on the device; prints one JSON line.')
    ap.add_argument('pred', help='the extracted mesh (a PLY with vertex and face elements)')
    ap.add_argument('gt', help='the ground-truth cloud (a PLY; only its vertex element is read)')
    ap.add_argument('--samples', type=int, required=True, help='points to sample on the mesh')
    ap.add_argument('--max-dist', type=float, default=None, help='distances >= this are left out of the means')
    ap.add_argument('--threshold', type=float, action='append', default=[], help='F-score threshold (repeatable)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the sampler')
    a = ap.parse_args(argv)
    mesh = read_ply(a.pred)
    gt = read_ply_points(a.gt)['points']
    dev = _device_of()
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    u = torch.rand((a.samples, 3), dtype=torch.float64, device=dev, generator=gen)
    out = evaluate_mesh(mesh['verts'], mesh['faces'], gt, a.samples, max_dist=a.max_dist, thresholds=a.threshold, u=u)
    out.update(pred=a.pred, gt=a.gt, samples=a.samples, seed=a.seed)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
