"""Minimal driver for profiling the fused SDF MLP kernels: ImplicitSurface.forward_with_nablas on
P points (default 524288 = one config-(b) step's samples), N launches.  Used under rocprofv3.
--mode render: the benchmark's config-(b) step instead (4096 rays x 128 samples = 524288 sample points), whose
sample launches <true,false,1>, compacted reverse launch <true,false,4> and mid-point launch <true,true,0>
--stamps then reports one by one."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=524288)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--precision', default='f16x3')
    ap.add_argument('--mode', default='nabla', choices=['nabla', 'nabla0', 'fwd', 'radiance', 'render'])
    ap.add_argument('--stamps', action='store_true', help='print sdf4_kernel phase totals (stamps build)')
    a = ap.parse_args()
    from neurecon_amd.base import ImplicitSurface, RadianceNet
    torch.manual_seed(0)
    what = f'{a.points} points'
    if a.mode != 'render':
        s = ImplicitSurface(W=256, D=8, skips=[4], W_geo_feat=256, radius_init=0.5, embed_multires=6,
                            precision=a.precision).cuda().eval()
        x = (torch.rand(a.points, 3, device='cuda') * 2 - 1) * 0.9
    with torch.no_grad():
        if a.mode == 'radiance':
            r = RadianceNet(D=4, W=256, W_geo_feat=256, embed_multires=-1, embed_multires_view=4,
                            precision=a.precision).cuda().eval()
            _, n, h = s.forward_with_nablas(x)
            fn = lambda: r.forward(x, x, n, h)
        elif a.mode == 'render':
            import bench
            from neurecon_amd import rend_util
            from neurecon_amd.frameworks.neus import volume_render
            m = bench.make_model('cuda', a.precision)
            ro, rd, _ = rend_util.get_rays(*bench.camera('cuda'), 64, 64)
            fn = lambda: volume_render(ro, rd, m, **bench.render_kwargs())
            what = f'{ro.shape[1]} rays x 128 samples'
        elif a.mode == 'nabla0':  # sdf + nablas without the geometry feature (the sample launches)
            fn = lambda: s._run(x, nabla=True, feature=False)
        elif a.mode == 'fwd':
            fn = lambda: s.forward(x)
        else:
            fn = lambda: s.forward_with_nablas(x)
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / a.iters
    print(f'{a.mode} {a.precision}: {what}, {dt * 1e3:.3f} ms/launch-set')
    if a.stamps:
        import ctypes
        import numpy as np
        from neurecon_amd import _lib as L
        # values per wave (kStampPh) from the library: the calls return waves per workgroup x values per wave
        one = np.zeros(1, dtype=np.uint64)
        NPH = L.lib().nr_exp_stamps(one.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(1)) // 8
        assert NPH >= 9, 'this library stamps no whole-tile phases'
        names = ['vmem issue', 'mfma loop', 'bias+vmcnt', 'barrier']
        # (label, STAGE_ slot or None = the last launch)
        slots = ([('<true,false,1> sample forward', 1), ('<true,false,4> compacted reverse', 4),
                 ('<true,true,0> mid-points', 0)] if a.mode == 'render' else [(a.mode, None)])
        for label, stage in slots:
            buf = np.zeros(2048 * 8 * NPH, dtype=np.uint64)
            bp, bn = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(buf.size)
            nw = L.lib().nr_exp_stamps(bp, bn) if stage is None else L.lib().nr_exp_stamps_stage(stage, bp, bn)
            v = buf.reshape(-1, NPH)
            v = v[v[:, 4] > 0].astype(np.float64)
            tot = v[:, :4].sum(1)
            print(f'{label}: waves {len(v)} (per WG {nw // NPH}), chunk iterations/wave {v[:, 4].mean():.0f}, '
                  f'clocks/iteration {tot.mean() / v[:, 4].mean():.0f}')
            for i, n in enumerate(names):
                print(f'  {n:12s} {v[:, i].mean() / v[:, 4].mean():8.0f} clk/iter  {100 * v[:, i].sum() / tot.sum():5.1f} %')
            # the whole tile (sdf4_kernel): per wave, and as a share of the tiles' time
            tile = v[:, 8].sum()
            if tile > 0:
                rest = tile - tot.sum() - v[:, 6].sum() - v[:, 7].sum()
                for n, x in (('tile start', v[:, 6].sum()), ('chunk iterations', tot.sum()),
                             ('op boundaries + turn', rest), ('tile end', v[:, 7].sum())):
                    print(f'  {n:22s} {x / len(v):10.0f} clk/wave  {100 * x / tile:5.1f} % of the tiles')


if __name__ == '__main__':
    main()
