"""numpy restatement of the three rules of the image metrics (neurecon_amd/csrc/nr_imgmetrics.hip): the SSIM
map, the error sums and the normal cosine, float64, operation for operation with explicit tap loops in the
stated order (numpy never fuses a product into a sum), so the device's maps are compared by equality.  The
sums are taken with math.fsum: the device adds in a fixed tree of its own, compared within the bound that holds
for any summation order.  Also the case generators the CPU and the GPU tests share."""
import math

import numpy as np


def gaussian(win=11, sigma=1.5):
    """w[k] = exp(-(k - win // 2)^2 / (2 sigma^2)) divided by the fsum of the values"""
    w = [math.exp(-((k - win // 2) ** 2) / (2.0 * sigma ** 2)) for k in range(win)]
    s = math.fsum(w)
    return np.array([v / s for v in w])


def constants(data_range=1.0, k1=0.01, k2=0.03):
    return (k1 * data_range) ** 2, (k2 * data_range) ** 2


def to_float(img):
    """uint8 -> float32(v) / float32(255); everything else -> float32"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(np.float32) / np.float32(255)
    return img.astype(np.float32)


def _filter(a, w):
    """the separable window over the valid region of a [..., H, W, C] float64 field: horizontal first, then
    vertical, each sum sequential in ascending tap order starting from w[0] a[0]"""
    win = len(w)
    H, W = a.shape[-3], a.shape[-2]
    Wo, Ho = W - win + 1, H - win + 1
    h = w[0] * a[..., :, 0:Wo, :]
    for i in range(1, win):
        h = h + w[i] * a[..., :, i:i + Wo, :]
    m = w[0] * h[..., 0:Ho, :, :]
    for j in range(1, win):
        m = m + w[j] * h[..., j:j + Ho, :, :]
    return m


def ssim_map(x, y, w=None, C1=None, C2=None):
    """-> float64 [..., H - win + 1, W - win + 1, C]; x, y [..., H, W, C] (fp32 values); empty when the image is
    smaller than the window"""
    w = gaussian() if w is None else np.asarray(w, np.float64)
    if C1 is None:
        C1, C2 = constants()
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    win = len(w)
    if x.shape[-3] < win or x.shape[-2] < win:
        return np.zeros(x.shape[:-3] + (max(x.shape[-3] - win + 1, 0), max(x.shape[-2] - win + 1, 0), x.shape[-1]))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        mx, my = _filter(x, w), _filter(y, w)
        exx, eyy, exy = _filter(x * x, w), _filter(y * y, w), _filter(x * y, w)
        mxx, myy, mxy = mx * mx, my * my, mx * my
        vx, vy, cxy = exx - mxx, eyy - myy, exy - mxy
        return ((2.0 * mxy + C1) * (2.0 * cxy + C2)) / (((mxx + myy) + C1) * ((vx + vy) + C2))


def ssim_counted(smap, mask, win):
    """one frame: smap [Ho, Wo, C], mask [H, W] or None -> (the counted values, n_used, n_nan): the values whose
    centre pixel passes the mask, split into not NaN / NaN"""
    Ho, Wo, C = smap.shape
    if mask is None:
        ok = np.ones((Ho, Wo), bool)
    else:
        ok = np.asarray(mask)[win // 2:win // 2 + Ho, win // 2:win // 2 + Wo] != 0
    v = smap[ok]
    nan = np.isnan(v)
    return v[~nan], int((~nan).sum()), int(nan.sum())


def error_terms(pred, gt, mask=None):
    """one frame: pred, gt [H, W, C], mask [H, W] or None -> (d float64 [n_used, C], n_used, n_excluded)"""
    p, g = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    ok = np.ones(p.shape[:2], bool) if mask is None else np.asarray(mask) != 0
    fin = np.isfinite(p).all(-1) & np.isfinite(g).all(-1)
    use = ok & fin
    d = p[use].astype(np.float64) - g[use].astype(np.float64)
    return d, int(use.sum()), int((ok & ~fin).sum())


def normal_cos(a, b, mask=None):
    """a, b [..., 3] -> float64 [...]: dot / sqrt(na nb) clamped to [-1, 1]; NaN where the mask is 0, a value is
    not finite or na nb == 0"""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ok = np.isfinite(a32).all(-1) & np.isfinite(b32).all(-1)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        na = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
        nb = (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]
        den = na * nb
        c = dot / np.sqrt(den)
    c = np.where(c > 1.0, 1.0, np.where(c < -1.0, -1.0, c))
    return np.where(ok & (den != 0.0), c, np.nan)


def psnr_of(sum_sq, n_values, data_range=1.0):
    if n_values == 0:
        return math.nan
    mse = sum_sq / n_values
    return math.inf if mse == 0.0 else 10.0 * math.log10(data_range * data_range / mse)


def sum_bound(values):
    """how far any fixed summation tree of n float64 values may be from their exact sum: n 2^-53 sum |v|
    (each of the n - 1 additions is off by at most 2^-53 of a partial sum, itself at most (1 + n 2^-53) sum |v|;
    fsum's own rounding, 2^-53 of the sum, takes the one addition that is left)"""
    v = np.abs(np.asarray(values, np.float64)).ravel().tolist()
    return len(v) * 2.0 ** -53 * math.fsum(v)


# ------------------------------------------------------------------------------------------------
# case generators
# ------------------------------------------------------------------------------------------------
def random_pair(shape, seed, scale=1.0, noise=0.1):
    """a random image in [0, scale] and a noisy copy clipped to the same range, fp32"""
    rng = np.random.default_rng(seed)
    x = rng.random(shape)
    y = np.clip(x + noise * rng.standard_normal(shape), 0.0, 1.0)
    return (x * scale).astype(np.float32), (y * scale).astype(np.float32)


def smooth_pair(shape, seed, noise=0.05):
    """a smooth field (products of sines over the pixel grid, per channel) plus noise, in [0, 1], fp32"""
    rng = np.random.default_rng(seed)
    H, W, C = shape[-3:]
    v, u = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing='ij')
    x = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * (1.3 + c) * u + c) * np.cos(2 * np.pi * (0.7 + 0.5 * c) * v)
                  for c in range(C)], -1)
    x = np.broadcast_to(x, shape).copy()
    y = np.clip(x + noise * rng.standard_normal(shape), 0.0, 1.0)
    return x.astype(np.float32), y.astype(np.float32)


def uint8_pair(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    y = np.clip(x.astype(np.int64) + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)
    return x, y
