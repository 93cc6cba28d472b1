#!/usr/bin/env python
"""Timing of neurecon_amd.mesh_simplify.simplify_mesh (nr_meshsimplify.hip) on the mesh `extract_mesh` gives for a
geometric-init surface net (a sphere of radius 0.5) at --grid-n^3 (512), at cells of 2 and 4 voxels.

Prints one JSON line and writes it to profiles/mesh_simplify/bench_mesh_simplify.json: per cell size the
end-to-end `simplify_mesh` time (host clock around synchronised calls, so it holds the two host reads, the
workspace allocation and the memsets; warm-up, then the median of --reps runs), the count and the emit step
separately from the library's own event timers (per kernel, in a pass of its own), the workspace bytes, the
sizes before and after and whether a second run is bit-identical; beside them the SDF grid and marching
cubes the step follows, timed the same way."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurecon_amd import _lib  # noqa: E402
from neurecon_amd.base import ImplicitSurface  # noqa: E402
from neurecon_amd.mesh_simplify import _grid, simplify_mesh  # noqa: E402
from neurecon_amd.mesh_util import marching_cubes, sdf_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid-n', type=int, default=512)
    ap.add_argument('--reps', type=int, default=7, help='timed runs per figure (the median is reported)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_simplify', 'bench_mesh_simplify.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_simplify needs a GPU (ROCm) device: no time is reported without one')
    if args.reps < 5:
        raise SystemExit('bench_mesh_simplify: --reps must be at least 5')
    N, s = args.grid_n, 2.0
    torch.manual_seed(0)
    surface = ImplicitSurface(radius_init=0.5, geometric_init=True).cuda().eval()
    voxel = s / N

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(round((time.perf_counter() - t0) * 1e3, 3))
        return dict(median=statistics.median(ts), runs=ts)

    def kernels(fn):
        fn()
        torch.cuda.synchronize()
        _lib.profile_enable(True, 'simplify_')
        for _ in range(args.reps):
            fn()
        stats = _lib.profile_read()
        _lib.profile_enable(False)
        per = {k: round(v[1] / args.reps, 5) for k, v in stats.items()}   # ms per call (the scan runs twice)
        emit = sum(v for k, v in per.items() if k.startswith('simplify_emit'))
        return dict(per_call=per, count_ms=round(sum(per.values()) - emit, 5), emit_ms=round(emit, 5))

    with torch.no_grad():
        vol = sdf_grid(surface, s, N)
        res = dict(workload=f'geometric-init sphere (radius 0.5), {N}^3 grid over {s}',
                   sdf_grid_wall_ms=wall(lambda: sdf_grid(surface, s, N)))
    mc = lambda: marching_cubes(vol, 0.0, spacing=[voxel] * 3, origin=[-s / 2] * 3)  # noqa: E731
    res['marching_cubes_wall_ms'] = wall(mc)
    verts, faces = mc()
    del vol
    res['verts'], res['faces'] = int(verts.shape[0]), int(faces.shape[0])
    for k in (2, 4):
        cell = k * voxel
        _, dim = _grid(verts, cell)
        run = lambda position='average': simplify_mesh(verts, faces, cell, position=position, return_clusters=True)  # noqa: E731
        a, b = run(), run()
        r = dict(cell=cell, dim=dim, verts_out=int(a[0].shape[0]), faces_out=int(a[1].shape[0]),
                 workspace_bytes=int(_lib.lib().nr_mesh_simplify_workspace_bytes(verts.shape[0], faces.shape[0],
                                                                                 dim[0] * dim[1] * dim[2])),
                 second_run_bit_identical=all(torch.equal(x, y) for x, y in zip(a, b)))
        r['simplify_mesh_wall_ms'] = wall(run)
        r['simplify_mesh_nearest_wall_ms'] = wall(lambda: run('nearest'))
        r['kernel_ms'] = kernels(run)
        res[f'cell_{k}_voxels'] = r
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
