#!/usr/bin/env python
"""Timing of the mesh metrics (neurecon_amd/mesh_metrics.py; nr_meshsample.hip, nr_nn.hip) on the marching-cubes
mesh of an analytic sphere volume at --grid-n^3 (512):

  sample     sample_mesh_surface at n = --points (2^20)
  nn_bounded nearest_points, N = M = --points surface points (mesh samples against an exact cloud on a sphere
             --offset farther out), with max_dist
  nn_free    the same without max_dist

Prints one JSON line.  Per case: the call time (device events around --reps Python calls after a warm-up, three
windows; the calls include their small host reads), the per-kernel times from the library's own event timers
in a pass of their own, the build / query split, the bytes the stage has to move at least (computed from the
shapes, below) and their share of the 8 TB/s HBM peak over the kernel time, and whether a second run is
bit-identical.  Where scipy imports, the cKDTree time (build + query, float64, all cores) for the same arrays:
the host step these calls replace."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurecon_amd import _lib  # noqa: E402
from neurecon_amd.mesh_metrics import nearest_points, sample_mesh_surface  # noqa: E402
from neurecon_amd.mesh_util import marching_cubes  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def sphere_mesh(N, r):
    ax = torch.linspace(-1, 1, N, device='cuda')
    vol = torch.empty((N, N, N), device='cuda')
    for i in range(N):  # slab by slab: no N^3 coordinate arrays
        vol[i] = torch.sqrt((ax[i] - 0.01) ** 2 + (ax[:, None] + 0.02) ** 2 + (ax[None, :] - 0.03) ** 2) - r
    return marching_cubes(vol, 0.0, spacing=[2 / (N - 1)] * 3, origin=[-1.0] * 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid-n', type=int, default=512)
    ap.add_argument('--points', type=int, default=1 << 20)
    ap.add_argument('--radius', type=float, default=0.8)
    ap.add_argument('--offset', type=float, default=0.01)
    ap.add_argument('--max-dist', type=float, default=0.05)
    ap.add_argument('--reps', type=int, default=20, help='calls per timed window')
    ap.add_argument('--profile-reps', type=int, default=5, help='calls of a per-kernel pass')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_metrics needs a GPU (ROCm) device: no time is reported without one')
    n = args.points
    verts, faces = sphere_mesh(args.grid_n, args.radius)
    V, F = len(verts), len(faces)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    u = torch.rand((n, 3), dtype=torch.float64, device='cuda', generator=gen)
    pred = sample_mesh_surface(verts, faces, n, u=u)[0]
    d = torch.randn((n, 3), dtype=torch.float64, device='cuda', generator=gen)
    centre = torch.tensor([0.01, -0.02, 0.03], dtype=torch.float64, device='cuda')
    gt = (d / d.norm(dim=1, keepdim=True) * (args.radius + args.offset) + centre).float()

    def window(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.reps, 4)

    def kernels(fn, prefix):
        _lib.profile_enable(True, prefix)
        for _ in range(args.profile_reps):
            fn()
        stats = _lib.profile_read()
        _lib.profile_enable(False)
        return {k: round(v[1] / args.profile_reps, 5) for k, v in stats.items()}

    def same(a, b):
        return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))

    res = dict(workload=f'mesh metrics, sphere mesh of a {args.grid_n}^3 volume', verts=V, faces=F, points=n,
               max_dist=args.max_dist, offset=args.offset)

    # sampler.  Least bytes: the faces (12 F) and vertices (12 V) once, cdf written and fixed up (8 F + 16 F);
    # per sample u (24), the point (12) and the face id (4)
    def sample():
        return sample_mesh_surface(verts, faces, n, u=u)
    k = kernels(sample, 'mesh_')
    cdf_ms = sum(v for name, v in k.items() if name.startswith('mesh_area'))
    res['sample'] = dict(call_ms=[window(sample) for _ in range(3)], kernel_ms=k, cdf_ms=round(cdf_ms, 5),
                         sample_ms=k.get('mesh_sample'),
                         min_bytes=dict(cdf=36 * F + 12 * V, sample=40 * n),
                         hbm_share=dict(cdf=round((36 * F + 12 * V) / (cdf_ms * 1e-3) / HBM_PEAK, 4),
                                        sample=round(40 * n / (k['mesh_sample'] * 1e-3) / HBM_PEAK, 4)),
                         second_run_bit_identical=same(sample(), sample()))

    # neighbour search.  Least bytes: build reads the points (12 N) and writes the records (16 N); the query reads
    # the queries (12 M) and the records once (16 N) and writes index and d2 (12 M)
    for name, md in (('nn_bounded', args.max_dist), ('nn_free', None)):
        def nn():
            return nearest_points(gt, pred, max_dist=md)
        k = kernels(nn, 'nn_')
        build_ms = sum(k.get(x, 0.0) for x in ('nn_bounds', 'nn_hist', 'nn_scan', 'nn_scatter'))
        query_ms = sum(k.get(x, 0.0) for x in ('nn_qhist', 'nn_qscan', 'nn_qscatter', 'nn_query'))
        out = nn()
        case = dict(call_ms=[window(nn) for _ in range(3)], kernel_ms=k, build_ms=round(build_ms, 5),
                    query_ms=round(query_ms, 5), min_bytes=dict(build=28 * n, query=40 * n),
                    hbm_share=dict(build=round(28 * n / (build_ms * 1e-3) / HBM_PEAK, 4),
                                   query=round(40 * n / (query_ms * 1e-3) / HBM_PEAK, 4)),
                    found=int((out[0] >= 0).sum()), mean_dist=float(out[1][out[0] >= 0].mean()),
                    workspace_bytes=_lib.lib().nr_nn_workspace_bytes(n, n), second_run_bit_identical=same(out, nn()))
        try:
            from scipy.spatial import cKDTree
            p64, q64 = gt.cpu().numpy().astype(np.float64), pred.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(p64)
            t1 = time.perf_counter()
            dist, _ = tree.query(q64, workers=-1, **({} if md is None else dict(distance_upper_bound=md)))
            t2 = time.perf_counter()
            case['ckdtree_ms'] = dict(build=round((t1 - t0) * 1e3, 1), query=round((t2 - t1) * 1e3, 1))
            fin = np.isfinite(dist)
            case['ckdtree_max_abs_diff'] = float(np.abs(dist[fin] - out[1].cpu().numpy()[fin]).max())
        except ImportError:
            case['ckdtree_ms'] = None
        res[name] = case
    print(json.dumps(res))


if __name__ == '__main__':
    main()
