#!/usr/bin/env python
"""Timing of the image metrics (neurecon_amd/image_metrics.py; nr_imgmetrics.hip) on an 800 x 600 x 3 frame and
on a stack of 8, device tensors in:

  ssim        image_metrics.ssim (Gaussian window of 11), the mean of every frame read back
  psnr        image_metrics.psnr
  torch_ssim  the plain-torch float64 formulation on the same device: the five fields materialised, each
              through two F.conv2d (1 x 11, then 11 x 1, one group per channel), the formula, the mean

Prints one JSON line and writes it to profiles/image_metrics/bench_image_metrics.json.  Per case: the call time
(the median of --reps calls after a warm-up, host clock; every call ends in a read of its result, so the device
has finished), the per-kernel times from the library's own event timers in a pass of their own, the bytes the
kernels have to move at least (computed from the shapes, below) and their share of the 8 TB/s HBM peak over the
kernel time, the largest difference between the two SSIM means, and whether a second run is bit-identical."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurecon_amd import _lib  # noqa: E402
from neurecon_amd import image_metrics as im  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def torch_ssim(x, y, w, C1, C2):
    """x, y fp32 [F, H, W, C] on the device -> the mean SSIM of every frame (float64 tensor [F])"""
    C, win = x.shape[-1], w.numel()
    x, y = x.permute(0, 3, 1, 2).double(), y.permute(0, 3, 1, 2).double()
    kh = w.reshape(1, 1, 1, win).repeat(C, 1, 1, 1)
    kv = w.reshape(1, 1, win, 1).repeat(C, 1, 1, 1)

    def filt(a):
        return F.conv2d(F.conv2d(a, kh, groups=C), kv, groups=C)
    mx, my = filt(x), filt(y)
    vx, vy, cxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    S = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return S.mean(dim=(1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=600)
    ap.add_argument('--width', type=int, default=800)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--reps', type=int, default=30, help='timed calls per case')
    ap.add_argument('--profile-reps', type=int, default=5, help='calls of a per-kernel pass')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'image_metrics', 'bench_image_metrics.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_image_metrics needs a GPU (ROCm) device: no time is reported without one')
    H, W, C, win = args.height, args.width, 3, 11
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    w = torch.from_numpy(im.gaussian_window()).cuda()
    C1, C2 = 0.01 ** 2, 0.03 ** 2

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))

    def kernels(fn):
        _lib.profile_enable(True, 'img_')
        for _ in range(args.profile_reps):
            fn()
        stats = _lib.profile_read()
        _lib.profile_enable(False)
        return {k: round(v[1] / args.profile_reps, 5) for k, v in stats.items()}

    res = dict(workload=f'image metrics, {W} x {H} x {C} frames, Gaussian window of {win}', reps=args.reps)
    for name, nf in (('frame', 1), (f'stack{args.frames}', args.frames)):
        gt = torch.rand((nf, H, W, C), device='cuda', generator=gen)
        pred = (gt + 0.05 * torch.randn((nf, H, W, C), device='cuda', generator=gen)).clamp(0, 1)
        values = nf * H * W * C
        case = dict(frames=nf)
        k = kernels(lambda: im.ssim(pred, gt))
        # least bytes: both images once (8 per value) and one partial per tile
        case['ssim'] = dict(call=timed(lambda: im.ssim(pred, gt)), kernel_ms=k, min_bytes=8 * values,
                            hbm_share=round(8 * values / (sum(k.values()) * 1e-3) / HBM_PEAK, 4))
        k = kernels(lambda: im.psnr(pred, gt))
        case['psnr'] = dict(call=timed(lambda: im.psnr(pred, gt)), kernel_ms=k, min_bytes=8 * values,
                            hbm_share=round(8 * values / (sum(k.values()) * 1e-3) / HBM_PEAK, 4))
        case['torch_ssim'] = dict(call=timed(lambda: torch_ssim(pred, gt, w, C1, C2).cpu()))
        a, b = im.ssim_sums(pred, gt, return_map=True), im.ssim_sums(pred, gt, return_map=True)
        case['second_run_bit_identical'] = bool(torch.equal(a['map'].view(torch.int64), b['map'].view(torch.int64))
                                                and (a['sum'] == b['sum']).all())
        mean = a['sum'] / a['n_used']
        case['ssim_mean'] = [float(v) for v in mean]
        case['psnr_db'] = [float(v) for v in im.psnr(pred, gt)]
        case['max_abs_diff_to_torch'] = float(abs(torch_ssim(pred, gt, w, C1, C2).cpu().numpy() - mean).max())
        case['speedup_vs_torch'] = round(case['torch_ssim']['call']['median_ms'] / case['ssim']['call']['median_ms'], 2)
        res[name] = case
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
