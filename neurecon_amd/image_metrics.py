"""Evaluate rendered frames against ground truth on the device: PSNR, SSIM, depth and normal error.

NeuS and VolSDF report the PSNR of rendered views beside the Chamfer distance of the mesh, and SSIM is its
standard companion.  `mesh_metrics` scores the geometry; this module scores the images, without leaving the
package or the device:

* `image_error` / `psnr`: the per-frame error sums (libnrhip `nr_img_error`) and the PSNR from them.
* `ssim` / `ssim_sums`: Wang et al.'s structural similarity with a caller-chosen 1-D window, over the valid
  region (libnrhip `nr_img_ssim`); equals scikit-image's `structural_similarity(gaussian_weights=True,
  use_sample_covariance=False)` with the default window.
* `depth_error`: L1 and RMSE between two depth maps where both are finite and > 0 (a miss of `render_mesh`
  is 0), through `nr_img_error` with one channel.
* `normal_error`: mean and median angle between two normal maps (libnrhip `nr_img_normal_cos`, then
  `torch.acos` in float64).
* `evaluate_frames`: PSNR and SSIM of a stack of frames and their means, as Python numbers.

    python -m neurecon_amd.image_metrics PRED GT [--mask M] [--data-range L]

prints `evaluate_frames` as one JSON line (PRED, GT, M: `.npy` / `.npz` stacks, or directories of images).

Images are [H, W, C] or [F, H, W, C] (channel last, 1 <= C <= 4: what `render_mesh` returns, and
`volume_render`'s rgb after a reshape); [H, W] is one single-channel frame.  Device or host tensors, or
arrays; uint8 images become float32(v) / float32(255).  A mask is [H, W] or [F, H, W], true (non-zero) where a
pixel counts.  A single frame in gives Python numbers out, a stack gives numpy arrays of length F.

The kernels' results are pure functions of their inputs (two runs are bit-identical); the rules are stated in
the header comment of neurecon_amd/csrc/nr_imgmetrics.hip and restated in numpy in tests/image_metrics_ref.py.

Out of scope: LPIPS, multi-scale SSIM, reading EXR, sharding frames across ranks.
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

from . import _lib as L

_MAX_WIN = 33


def _device_of(*xs):
    dev = next((t.device for t in xs if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError('neurecon_amd: image_metrics needs a GPU (ROCm) device; the path is HIP-only')
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _tensor(a):
    return a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def _frames_shape(t, name):
    """-> ((F, H, W, C), batched) of an image [H, W], [H, W, C] or [F, H, W, C]"""
    s = tuple(t.shape)
    if len(s) == 2:
        full, batched = (1,) + s + (1,), False
    elif len(s) == 3:
        full, batched = (1,) + s, False
    elif len(s) == 4:
        full, batched = s, True
    else:
        raise ValueError(f'{name} must be [H, W], [H, W, C] or [F, H, W, C], got {s}')
    if not 1 <= full[3] <= 4:
        raise ValueError(f'{name}: the channel count must be in 1..4 (channel last), got {s}')
    if min(full) < 1:
        raise ValueError(f'{name}: empty image {s}')
    if math.prod(full) >= 2 ** 31:
        raise ValueError(f'{name}: {s} has 2^31 values or more; score the frames in smaller stacks')
    return full, batched


def _pair(pred, gt, mask, who):
    """the shape checks, before a device is needed -> (pred, gt, mask tensors as given, (F, H, W, C), batched)"""
    p, g = _tensor(pred), _tensor(gt)
    if tuple(p.shape) != tuple(g.shape):
        raise ValueError(f'{who}: pred {tuple(p.shape)} and gt {tuple(g.shape)} must have the same shape')
    full, batched = _frames_shape(p, f'{who}: pred')
    m = None
    if mask is not None:
        m = _tensor(mask)
        want = full[:3] if batched else full[1:3]
        if tuple(m.shape) != want:
            raise ValueError(f'{who}: mask must be {list(want)}, got {tuple(m.shape)}')
    return p, g, m, full, batched


def _image(t, full, dev):
    t = t.to(dev)
    if t.dtype == torch.uint8:
        t = t.to(torch.float32)
        t = t / torch.full_like(t, 255.0)  # a true division (by a scalar it would multiply by 1 / 255)
    return t.to(torch.float32).reshape(full).contiguous()


def _mask8(m, full, dev):
    return None if m is None else (m.to(dev) != 0).to(torch.uint8).reshape(full[:3]).contiguous()


def _out(x, batched):
    return x if batched else x[0].item()


def gaussian_window(win=11, sigma=1.5):
    """The 1-D Gaussian window of SSIM -> float64 [win]: w[k] = exp(-(k - win // 2)^2 / (2 sigma^2)), divided by
    the `math.fsum` of the values.  win = 11, sigma = 1.5: Wang et al.'s window, scikit-image's with
    gaussian_weights=True."""
    win = int(win)
    if win < 1 or win > _MAX_WIN or win % 2 == 0:
        raise ValueError(f'gaussian_window: win must be odd and in 1..{_MAX_WIN}, got {win}')
    if not float(sigma) > 0.0:
        raise ValueError(f'gaussian_window: sigma must be > 0, got {sigma}')
    w = [math.exp(-((k - win // 2) ** 2) / (2.0 * float(sigma) ** 2)) for k in range(win)]
    s = math.fsum(w)
    return np.array([v / s for v in w], dtype=np.float64)


def _window(window):
    w = gaussian_window() if window is None else np.asarray(
        window.detach().cpu().numpy() if isinstance(window, torch.Tensor) else window, dtype=np.float64)
    if w.ndim != 1 or w.size < 1 or w.size > _MAX_WIN or w.size % 2 == 0:
        raise ValueError(f'ssim: window must be 1-D of odd length in 1..{_MAX_WIN}, got shape {w.shape}')
    if not np.isfinite(w).all():
        raise ValueError('ssim: window must be finite')
    return np.ascontiguousarray(w)


def _data_range(data_range, who):
    r = float(data_range)
    if not (0.0 < r < math.inf):
        raise ValueError(f'{who}: data_range must be finite and > 0, got {data_range}')
    return r


def _error_sums(p, g, m8, full, dev):
    """nr_img_error on prepared device tensors -> float64 [F, 4] on the host"""
    F, H, W, C = full
    lib = L.lib()
    with torch.cuda.device(dev):
        ws_bytes = lib.nr_img_workspace_bytes(F, H, W, C, 1)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((F, 4), dtype=torch.float64, device=dev)
        L.check(lib.nr_img_error(L.ptr(p), L.ptr(g), L.ptr(m8), F, H, W, C, L.ptr(out), L.ptr(ws), ws_bytes,
                                 L.stream_of(dev)))
        return out.cpu().numpy()


def image_error(pred, gt, mask=None):
    """The error sums of every frame, on the device -> dict(sum_sq, sum_abs float64; n_used, n_excluded int64).

    A pixel counts iff the mask passes it and all its values in both images are finite; one the mask passes
    that holds a non-finite value adds to n_excluded.  sum_sq / sum_abs: the sums of d^2 and |d| over the
    counted values, d = pred - gt in float64 (n_used C values).  Identical images give exactly 0."""
    p, g, m, full, batched = _pair(pred, gt, mask, 'image_error')
    dev = _device_of(pred, gt, mask)
    o = _error_sums(_image(p, full, dev), _image(g, full, dev), _mask8(m, full, dev), full, dev)
    return dict(sum_sq=_out(o[:, 0].copy(), batched), sum_abs=_out(o[:, 1].copy(), batched),
                n_used=_out(o[:, 2].astype(np.int64), batched), n_excluded=_out(o[:, 3].astype(np.int64), batched))


def _psnr_of(sum_sq, n_values, L2):
    """10 log10(L^2 / mse) on the host: inf at mse 0, NaN without a counted value"""
    if n_values == 0:
        return math.nan
    mse = sum_sq / n_values
    return math.inf if mse == 0.0 else 10.0 * math.log10(L2 / mse)


def psnr(pred, gt, mask=None, data_range=1.0):
    """Peak signal-to-noise ratio per frame: mse = sum_sq / (n_used C), psnr = 10 log10(data_range^2 / mse), the
    sums from `image_error` and the logarithm on the host.  inf for identical images, NaN when no pixel
    counts."""
    r = _data_range(data_range, 'psnr')
    p, _, _, full, batched = _pair(pred, gt, mask, 'psnr')
    e = image_error(pred, gt, mask)
    ss, nu = np.atleast_1d(e['sum_sq']), np.atleast_1d(e['n_used'])
    return _out(np.array([_psnr_of(float(s), int(n) * full[3], r * r) for s, n in zip(ss, nu)]), batched)


def ssim_sums(pred, gt, mask=None, data_range=1.0, window=None, k1=0.01, k2=0.03, return_map=False):
    """The SSIM sums of every frame, on the device -> dict(sum float64, n_used, n_nan int64, map).

    window: 1-D, odd length <= 33 (default `gaussian_window()`; e.g. np.full(7, 1 / 7) for a uniform one),
    applied along the rows and then along the columns.  C1 = (k1 data_range)^2, C2 = (k2 data_range)^2.  The
    SSIM map covers the valid region, [F, H - win + 1, W - win + 1, C] (a device float64 tensor when
    return_map, else None; without the frame axis for a single frame); a value is NaN exactly where its window
    covers a non-finite input.  sum / n_used: the sum and the count of the map values that are not NaN and whose
    centre pixel the mask passes; n_nan: the NaN ones among those the mask passes.  An image smaller than the
    window gives an empty map and n_used 0: no error."""
    r = _data_range(data_range, 'ssim')
    w = _window(window)
    p, g, m, full, batched = _pair(pred, gt, mask, 'ssim')
    dev = _device_of(pred, gt, mask)
    F, H, W, C = full
    win = int(w.size)
    c1, c2 = (float(k1) * r) ** 2, (float(k2) * r) ** 2
    if not (0.0 <= c1 < math.inf and 0.0 <= c2 < math.inf):
        raise ValueError(f'ssim: k1 and k2 must be finite, got {k1}, {k2}')
    p, g, m8 = _image(p, full, dev), _image(g, full, dev), _mask8(m, full, dev)
    lib = L.lib()
    with torch.cuda.device(dev):
        wd = torch.from_numpy(w).to(dev)
        ws_bytes = lib.nr_img_workspace_bytes(F, H, W, C, win)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((F, 3), dtype=torch.float64, device=dev)
        smap = None
        if return_map:
            smap = torch.empty((F, max(H - win + 1, 0), max(W - win + 1, 0), C), dtype=torch.float64, device=dev)
        L.check(lib.nr_img_ssim(L.ptr(p), L.ptr(g), L.ptr(m8), F, H, W, C, L.ptr(wd), win, ctypes.c_double(c1),
                                ctypes.c_double(c2), L.ptr(smap) if smap is not None and smap.numel() else None,
                                L.ptr(out), L.ptr(ws), ws_bytes, L.stream_of(dev)))
        o = out.cpu().numpy()
    if smap is not None and not batched:
        smap = smap[0]
    return dict(sum=_out(o[:, 0].copy(), batched), n_used=_out(o[:, 1].astype(np.int64), batched),
                n_nan=_out(o[:, 2].astype(np.int64), batched), map=smap)


def ssim(pred, gt, mask=None, data_range=1.0, window=None, k1=0.01, k2=0.03, return_map=False):
    """Mean structural similarity per frame: the sum of `ssim_sums` over n_used, NaN when n_used is 0.
    return_map: -> (mean, map), the map a device float64 tensor (see `ssim_sums`)."""
    s = ssim_sums(pred, gt, mask, data_range, window, k1, k2, return_map)
    batched = isinstance(s['sum'], np.ndarray)
    mean = np.array([float(a) / int(n) if n else math.nan
                     for a, n in zip(np.atleast_1d(s['sum']), np.atleast_1d(s['n_used']))])
    mean = _out(mean, batched)
    return (mean, s['map']) if return_map else mean


def _depth_shape(t, name):
    if t.dim() not in (2, 3):
        raise ValueError(f'{name} must be [H, W] or [F, H, W], got {tuple(t.shape)}')
    return ((1,) + tuple(t.shape) if t.dim() == 2 else tuple(t.shape)) + (1,), t.dim() == 3


def depth_error(pred, gt, mask=None):
    """L1 and RMSE between two depth maps [H, W] or [F, H, W], on the device -> dict(l1, rmse float64; n_used,
    n_excluded int64).  A pixel is valid where the mask passes it and both depths are finite and > 0 (a miss of
    `render_mesh` is 0); n_excluded: the pixels the mask passes that are not valid.  NaN when nothing is valid.
    `render_mesh`'s depth and `volume_render`'s depth_volume are both distances along the normalised ray through
    the same pixels, so they compare pixel for pixel."""
    p, g = _tensor(pred), _tensor(gt)
    if tuple(p.shape) != tuple(g.shape):
        raise ValueError(f'depth_error: pred {tuple(p.shape)} and gt {tuple(g.shape)} must have the same shape')
    full, batched = _depth_shape(p, 'depth_error: pred')
    if min(full) < 1 or math.prod(full) >= 2 ** 31:
        raise ValueError(f'depth_error: needs 0 < F H W < 2^31, got {tuple(p.shape)}')
    m = None
    if mask is not None:
        m = _tensor(mask)
        if tuple(m.shape) != tuple(p.shape):
            raise ValueError(f'depth_error: mask must be {list(p.shape)}, got {tuple(m.shape)}')
    dev = _device_of(pred, gt, mask)
    p, g = _image(p, full, dev), _image(g, full, dev)
    user = torch.ones(full[:3], dtype=torch.bool, device=dev) if m is None else (m.to(dev) != 0).reshape(full[:3])
    m8 = (user & (p[..., 0] > 0) & (g[..., 0] > 0)).to(torch.uint8).contiguous()
    n_mask = user.reshape(full[0], -1).sum(1).cpu().numpy().astype(np.int64)
    o = _error_sums(p, g, m8, full, dev)
    nu = o[:, 2].astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        l1 = np.where(nu > 0, o[:, 1] / nu, np.nan)
        rmse = np.where(nu > 0, np.sqrt(o[:, 0] / nu), np.nan)
    return dict(l1=_out(l1, batched), rmse=_out(rmse, batched), n_used=_out(nu, batched),
                n_excluded=_out(n_mask - nu, batched))


def normal_cosine(pred, gt, mask=None):
    """The cosine between two normal maps [..., 3], on the device -> float64 tensor of the leading shape:
    dot / sqrt(|a|^2 |b|^2) in float64, clamped to [-1, 1]; NaN where the mask is 0, a component is not finite or
    a normal has length 0.  The normals need not be unit."""
    p, g = _tensor(pred), _tensor(gt)
    if tuple(p.shape) != tuple(g.shape) or p.dim() < 1 or p.shape[-1] != 3:
        raise ValueError(f'normal_error: pred and gt must both be [..., 3], got {tuple(p.shape)} and {tuple(g.shape)}')
    lead = tuple(p.shape[:-1])
    P = math.prod(lead)
    if 3 * P >= 2 ** 31:
        raise ValueError(f'normal_error: {tuple(p.shape)} has 2^31 values or more')
    m = None
    if mask is not None:
        m = _tensor(mask)
        if tuple(m.shape) != lead:
            raise ValueError(f'normal_error: mask must be {list(lead)}, got {tuple(m.shape)}')
    dev = _device_of(pred, gt, mask)
    p = p.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    g = g.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    m8 = None if m is None else (m.to(dev) != 0).to(torch.uint8).reshape(-1).contiguous()
    out = torch.empty(P, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().nr_img_normal_cos(L.ptr(p) if P else None, L.ptr(g) if P else None, L.ptr(m8), P,
                                          L.ptr(out) if P else None, L.stream_of(dev)))
    return out.reshape(lead)


def normal_error(pred, gt, mask=None):
    """Mean and median angle in degrees between two normal maps [H, W, 3] or [F, H, W, 3] -> dict(mean_deg,
    median_deg float64; n_used, n_excluded int64): `torch.acos` of `normal_cosine` in float64 on the device, over
    the pixels where it is not NaN.  The median of an even count is the mean of the two middle angles.
    n_excluded: the pixels the mask passes whose cosine is NaN (a miss of `render_mesh` has a zero normal).
    NaN when no pixel counts."""
    p = _tensor(pred)
    if p.dim() not in (3, 4):
        raise ValueError(f'normal_error: pred must be [H, W, 3] or [F, H, W, 3], got {tuple(p.shape)}')
    batched = p.dim() == 4
    cos = normal_cosine(pred, gt, mask)
    F = cos.shape[0] if batched else 1
    cos = cos.reshape(F, -1)
    ang = torch.rad2deg(torch.acos(cos))
    n_mask = np.full(F, cos.shape[1], np.int64) if mask is None else \
        (_tensor(mask).to(cos.device) != 0).reshape(F, -1).sum(1).cpu().numpy().astype(np.int64)
    mean, med, nu = np.full(F, np.nan), np.full(F, np.nan), np.zeros(F, np.int64)
    for f in range(F):
        v = ang[f][~torch.isnan(ang[f])]
        n = int(v.numel())
        nu[f] = n
        if n:
            s = torch.sort(v).values
            mean[f] = float(v.mean())
            med[f] = float((s[(n - 1) // 2] + s[n // 2]) / 2)
    return dict(mean_deg=_out(mean, batched), median_deg=_out(med, batched), n_used=_out(nu, batched),
                n_excluded=_out(n_mask - nu, batched))


def evaluate_frames(pred, gt, mask=None, data_range=1.0):
    """PSNR and SSIM (default window) of a stack of frames -> dict of Python numbers and per-frame lists:
    frames, channels, data_range; psnr, mse, mae, ssim (lists); n_used / n_excluded (pixels of the error sums),
    ssim_n_used / ssim_n_nan (SSIM map values); psnr_mean, mse_mean, mae_mean, ssim_mean: the plain means over
    the frames (an inf or NaN frame shows in its mean)."""
    r = _data_range(data_range, 'evaluate_frames')
    _, _, _, full, _ = _pair(pred, gt, mask, 'evaluate_frames')
    C = full[3]
    e = image_error(pred, gt, mask)
    s = ssim_sums(pred, gt, mask, r)
    ss, sa = np.atleast_1d(e['sum_sq']).tolist(), np.atleast_1d(e['sum_abs']).tolist()
    nu, ne = np.atleast_1d(e['n_used']).tolist(), np.atleast_1d(e['n_excluded']).tolist()
    su, sn = np.atleast_1d(s['n_used']).tolist(), np.atleast_1d(s['n_nan']).tolist()
    out = dict(frames=full[0], channels=C, data_range=r)
    out['psnr'] = [_psnr_of(a, n * C, r * r) for a, n in zip(ss, nu)]
    out['mse'] = [a / (n * C) if n else math.nan for a, n in zip(ss, nu)]
    out['mae'] = [a / (n * C) if n else math.nan for a, n in zip(sa, nu)]
    out['ssim'] = [a / n if n else math.nan for a, n in zip(np.atleast_1d(s['sum']).tolist(), su)]
    out['n_used'], out['n_excluded'], out['ssim_n_used'], out['ssim_n_nan'] = nu, ne, su, sn
    for k in ('psnr', 'mse', 'mae', 'ssim'):
        out[k + '_mean'] = math.fsum(out[k]) / len(out[k])
    return out


def _load_stack(path, what):
    """a .npy / .npz stack, or a directory of images (sorted by name)"""
    if os.path.isdir(path):
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError(f'image_metrics: reading a directory of {what} images needs PIL (pillow); save the '
                               'stack as a .npy file instead') from e
        names = sorted(n for n in os.listdir(path) if not n.startswith('.'))
        if not names:
            raise ValueError(f'image_metrics: {path} holds no {what} image')
        if what == 'mask':
            return np.stack([np.asarray(Image.open(os.path.join(path, n)).convert('L'), dtype=np.float32) > 127.5
                             for n in names])
        return np.stack([np.asarray(Image.open(os.path.join(path, n)).convert('RGB'), dtype=np.uint8) for n in names])
    data = np.load(path)
    if isinstance(data, np.lib.npyio.NpzFile):
        with data:
            if len(data.files) != 1:
                raise ValueError(f'image_metrics: {path} must hold one array, got {data.files}')
            data = data[data.files[0]]
    return np.ascontiguousarray(data != 0) if what == 'mask' else np.ascontiguousarray(data)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m neurecon_amd.image_metrics',
                                 description='PSNR and SSIM of rendered frames against ground truth, on the device; '
                                             'prints one JSON line.')
    ap.add_argument('pred', help='the rendered frames: a .npy / .npz stack [F, H, W, C] (or one frame [H, W, C]), '
                                 'or a directory of images')
    ap.add_argument('gt', help='the ground-truth frames, the same way')
    ap.add_argument('--mask', default=None, help='a .npy / .npz stack [F, H, W], or a directory of mask images')
    ap.add_argument('--data-range', type=float, default=1.0, help='the value range L of the images (uint8: 1)')
    a = ap.parse_args(argv)
    pred, gt = _load_stack(a.pred, 'pred'), _load_stack(a.gt, 'gt')
    mask = None if a.mask is None else _load_stack(a.mask, 'mask')
    out = evaluate_frames(pred, gt, mask=mask, data_range=a.data_range)
    out.update(pred=a.pred, gt=a.gt, mask=a.mask)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
