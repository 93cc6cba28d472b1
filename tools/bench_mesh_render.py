#!/usr/bin/env python
"""Timing of neurecon_amd.mesh_util.render_mesh (nr_meshrender.hip): the marching-cubes mesh of an analytic
sphere volume at --grid-n^3 (512: 1.6 M sub-pixel faces), one --width x --height frame (800 x 600).

Prints one JSON line: the frame time (device events around --reps calls after a warm-up, three windows), the
per-kernel times from the library's own event timers in a pass of their own, the same with vertex normals
and colours, the frame time at several large_threshold values (alternated), and whether the outputs of the
two rasteriser paths and of a second run are bit-identical at this size."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurecon_amd import _lib  # noqa: E402
from neurecon_amd.mesh_util import marching_cubes, render_mesh  # noqa: E402


def sphere_mesh(N):
    ax = torch.linspace(-1, 1, N, device='cuda')
    vol = torch.empty((N, N, N), device='cuda')
    for i in range(N):  # slab by slab: no N^3 coordinate arrays
        vol[i] = torch.sqrt((ax[i] - 0.01) ** 2 + (ax[:, None] + 0.02) ** 2 + (ax[None, :] - 0.03) ** 2) - 0.8
    return marching_cubes(vol, 0.0, spacing=[2 / (N - 1)] * 3, origin=[-1.0] * 3)


def camera(H, W, dist=3.2, a=0.7, b=-0.4):
    """rotated about y then x, looking at the origin; the sphere (radius 0.8) fills 0.9 of the frame's height"""
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    R = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = R, -dist * R[:, 2] + [0.05, -0.03, 0.02]
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 0.45 * H * dist / 0.8
    K[0, 2], K[1, 2] = (W - 1) / 2 + 0.3, (H - 1) / 2
    return c2w.astype(np.float32), K.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid-n', type=int, default=512)
    ap.add_argument('--height', type=int, default=600)
    ap.add_argument('--width', type=int, default=800)
    ap.add_argument('--reps', type=int, default=1000, help='frames per timed window')
    ap.add_argument('--profile-reps', type=int, default=50, help='frames of a per-kernel pass')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_render needs a GPU (ROCm) device: no time is reported without one')
    H, W = args.height, args.width
    verts, faces = sphere_mesh(args.grid_n)
    attrs = dict(normals=torch.nn.functional.normalize(verts, dim=-1), colors=0.5 + 0.5 * torch.sin(3 * verts))
    c2w, K = camera(H, W)

    def frame(**kw):
        return render_mesh(verts, faces, c2w, K, H, W, **kw)

    def window(**kw):
        for _ in range(3):
            frame(**kw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            frame(**kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def kernels(**kw):
        _lib.profile_enable(True, 'mr_')
        for _ in range(args.profile_reps):
            frame(**kw)
        stats = _lib.profile_read()
        _lib.profile_enable(False)
        per = {k: round(v[1] / v[0], 5) for k, v in stats.items()}
        return dict(per, total=round(sum(per.values()), 5))

    out = frame()
    res = dict(workload=f'render_mesh {W}x{H}, sphere mesh of a {args.grid_n}^3 volume', verts=len(verts),
               faces=len(faces), hit_pixels=int(out['mask'].sum()), n_clipped=int(out['n_clipped']),
               workspace_bytes=_lib.lib().nr_mesh_render_workspace_bytes(len(verts), len(faces), H, W),
               frame_ms=[round(window(), 5) for _ in range(3)],
               frame_ms_normals_colors=[round(window(**attrs), 5) for _ in range(3)])
    by_lt = {}
    for _ in range(2):
        for lt in (16, 64, 256, 1024):
            by_lt.setdefault(lt, []).append(round(window(large_threshold=lt), 5))
    res['frame_ms_by_large_threshold'] = by_lt
    res['kernel_ms'] = kernels()
    res['kernel_ms_normals_colors'] = kernels(**attrs)
    a, b = frame(large_threshold=0), frame(large_threshold=2 ** 40)
    res['n_large'] = {'default': int(out['n_large']), '0': int(a['n_large']), '2^40': int(b['n_large'])}
    res['paths_bit_identical'] = all(torch.equal(out[k], a[k]) and torch.equal(out[k], b[k]) for k in out
                                     if k != 'n_large')  # the one output that says which path a face took
    res['second_run_bit_identical'] = all(torch.equal(out[k], v) for k, v in frame().items())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
