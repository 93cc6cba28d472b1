#!/usr/bin/env python
"""Timing of neurecon_amd.mesh_cull (nr_meshcull.hip): the marching-cubes mesh of an analytic sphere volume at
--grid-n^3 (512: 1.6 M faces) against --views orbit cameras at --width x --height (64 at 1600 x 1200), with
the sphere's own silhouettes as masks.

Prints one JSON line and writes it to profiles/mesh_cull/bench_mesh_cull.json: per-kernel times from the
library's own event timers (each in a pass of its own) for the dilation at radius 5 and 50 and for the view
test with and without depth, the end-to-end `cull_mesh` time (host timer around synchronised calls: it holds
the renders, the uploads and `filter_mesh`'s host reads), and whether a second run is bit-identical."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from neurecon_amd import _lib  # noqa: E402
from neurecon_amd.mesh_cull import cull_mesh, dilate_masks, vertex_views  # noqa: E402
from neurecon_amd.mesh_util import render_mesh  # noqa: E402
from bench_mesh_render import camera, sphere_mesh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid-n', type=int, default=512)
    ap.add_argument('--height', type=int, default=1200)
    ap.add_argument('--width', type=int, default=1600)
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5, help='calls per timed figure')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_cull', 'bench_mesh_cull.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh_cull needs a GPU (ROCm) device: no time is reported without one')
    H, W, B = args.height, args.width, args.views
    verts, faces = sphere_mesh(args.grid_n)
    cams = [camera(H, W, a=0.7 + 2 * np.pi * k / B, b=-0.4 + 0.25 * np.sin(k)) for k in range(B)]
    c2w, K = np.stack([c for c, _ in cams]), cams[0][1]
    masks = torch.stack([render_mesh(verts, faces, c2w[k], K, H, W)['mask'] for k in range(B)])   # bool [B, H, W]

    def kernels(prefix, fn):
        fn()
        torch.cuda.synchronize()
        _lib.profile_enable(True, prefix)
        for _ in range(args.reps):
            fn()
        stats = _lib.profile_read()
        _lib.profile_enable(False)
        per = {k: round(v[1] / v[0], 5) for k, v in stats.items()}   # ms per launch
        return dict(per, total_per_call=round(sum(v[1] for v in stats.values()) / args.reps, 5))

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(round((time.perf_counter() - t0) * 1e3, 3))
        return ts

    res = dict(workload=f'{B} views {W}x{H}, sphere mesh of a {args.grid_n}^3 volume', verts=len(verts), faces=len(faces),
               mask_bytes=int(masks.numel()), set_share=round(float(masks.float().mean()), 4))
    for r in (5, 50):
        res[f'dilate_r{r}_kernel_ms'] = kernels('md_', lambda: dilate_masks(masks, r))
        res[f'dilate_r{r}_wall_ms'] = wall(lambda: dilate_masks(masks, r))
    res['view_test_kernel_ms'] = kernels('mc_', lambda: vertex_views(verts, None, c2w, K, H, W, masks=masks))
    res['view_test_depth_kernel_ms'] = kernels('mc_', lambda: vertex_views(verts, faces, c2w, K, H, W, masks=masks,
                                                                            depth_tol=1e-3))
    res['depth_frames_kernel_ms'] = kernels('mr_', lambda: vertex_views(verts, faces, c2w, K, H, W, depth_tol=1e-3))
    res['vertex_views_wall_ms'] = wall(lambda: vertex_views(verts, None, c2w, K, H, W, masks=masks))
    res['vertex_views_depth_wall_ms'] = wall(lambda: vertex_views(verts, faces, c2w, K, H, W, masks=masks, depth_tol=1e-3))

    def cull():
        return cull_mesh(verts, faces, c2w, K, H, W, masks=masks, dilate=5, depth_tol=1e-3)
    res['cull_mesh_wall_ms'] = wall(cull)
    a, b = cull(), cull()
    res['verts_kept'], res['faces_kept'] = int(a['verts'].shape[0]), int(a['faces'].shape[0])
    res['second_run_bit_identical'] = all(torch.equal(a[k], b[k]) for k in ('verts', 'faces', 'index', 'kept', 'n_in_image',
                                                                            'n_in_mask', 'n_visible'))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
