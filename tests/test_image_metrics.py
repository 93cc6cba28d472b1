"""CPU tests of the image metrics (neurecon_amd/image_metrics.py): the numpy restatement of the SSIM rule
(tests/image_metrics_ref.py) against an independent formulation and against exact facts of the rule, the PSNR
closed forms, `gaussian_window`, the C-ABI argument checks and the workspace formula with fake pointers (the
checks come before any HIP call), and the Python refusals that come before a device is needed.  The device
itself is compared with the restatement in tests/test_gpu_image_metrics.py."""
import math
import os

import numpy as np
import pytest

import image_metrics_ref as ref

# Tolerance of the SSIM restatement against another formulation of the same filter, for data in [0, 1] with
# L = 1: each of the five moments is a sum of 121 products of weights that add up to 1 and values <= 1, taken as
# two passes of 11 taps: at most 2 x (11 products + 10 additions) + the roundings of the field and of the
# normalised weights = at most 44 roundings of values <= 1, each <= 2^-53: about 5e-15 per moment.  The formula
# divides by (mx^2 + my^2 + C1) (vx + vy + C2), whose factors can be as small as C1 = 1e-4 and C2 = 9e-4, and the
# numerator's factors are no larger than the denominator's, so an error of 5e-15 in a moment moves S by at most
# about 5e-15 / C1 = 5e-11 per factor, 1e-10 for the two.  1e-9 leaves a factor of 10 on top of that.
SSIM_TOL = 1e-9


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _scipy_ssim(x, y, C1, C2):
    """Wang et al. through scipy's reflected Gaussian filter on the five fields, cropped by the 5 pixels the
    reflection touches: what scikit-image computes with gaussian_weights=True, use_sample_covariance=False"""
    ndimage = pytest.importorskip('scipy.ndimage')
    x, y = x.astype(np.float64), y.astype(np.float64)

    def filt(a):
        return np.stack([ndimage.gaussian_filter(a[..., c], 1.5, truncate=3.5) for c in range(a.shape[-1])], -1)
    mx, my = filt(x), filt(y)
    vx, vy, cxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    S = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return S[5:-5, 5:-5]


def _cases():
    yield 'random 37x53', ref.random_pair((37, 53, 3), 1)
    yield 'smooth 70x150', ref.smooth_pair((70, 150, 3), 2)
    yield 'values <= 1e-3', ref.random_pair((37, 53, 3), 3, scale=1e-3)
    yield 'uint8-valued', tuple(ref.to_float(a) for a in ref.uint8_pair((37, 53, 3), 4))


def test_ssim_restatement_against_scipy():
    pytest.importorskip('scipy.ndimage')
    C1, C2 = ref.constants()
    worst = 0.0
    for name, (x, y) in _cases():
        got = ref.ssim_map(x, y)
        want = _scipy_ssim(x, y, C1, C2)
        assert got.shape == want.shape == (x.shape[0] - 10, x.shape[1] - 10, 3)
        err = float(np.abs(got - want).max())
        print(f'{name}: max |restatement - scipy| = {err:.3e}')
        worst = max(worst, err)
        assert err <= SSIM_TOL, (name, err)
    print(f'worst {worst:.3e} against the bound {SSIM_TOL:.0e}')


def test_ssim_identical_images_are_exactly_one():
    for name, (x, _) in _cases():
        assert (ref.ssim_map(x, x) == 1.0).all(), name
    x, _ = ref.random_pair((20, 23, 4), 5)
    assert (ref.ssim_map(x, x, np.full(7, 1 / 7)) == 1.0).all()
    assert (ref.ssim_map(x, x, np.ones(1)) == 1.0).all()


def test_ssim_of_two_constant_images():
    C1, C2 = ref.constants()
    for a, b in ((0.25, 0.75), (0.0, 1.0), (1.0, 1.0), (0.1, 0.100001)):
        x, y = np.full((15, 17, 1), a, np.float32), np.full((15, 17, 1), b, np.float32)
        a64, b64 = float(np.float32(a)), float(np.float32(b))
        want = (2 * a64 * b64 + C1) / (a64 * a64 + b64 * b64 + C1)
        got = ref.ssim_map(x, y)
        assert got.shape == (5, 7, 1) and np.abs(got - want).max() <= SSIM_TOL, (a, b)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_one_non_finite_pixel_gives_win_squared_nans(bad):
    x, y = ref.random_pair((40, 45, 3), 6)
    x[20, 22, 1] = bad
    m = ref.ssim_map(x, y)
    nan = np.isnan(m)
    assert nan[..., 1].sum() == 121 and not nan[..., 0].any() and not nan[..., 2].any()
    assert nan[10:21, 12:23, 1].all()                        # the 11 x 11 windows that cover pixel (20, 22)
    y[5, 5, 0] = bad
    assert np.isnan(ref.ssim_map(x, y, np.full(7, 1 / 7)))[..., 0].sum() == 36   # rows 0..5, cols 0..5 exist
    assert ref.ssim_map(x[:10], y[:10]).shape == (0, 35, 3)                      # smaller than the window: empty


def test_counted_values_follow_the_centre_pixel():
    x, y = ref.random_pair((20, 24, 2), 7)
    m = ref.ssim_map(x, y)
    mask = np.zeros((20, 24), bool)
    mask[5, 5] = mask[14, 18] = mask[4, 5] = mask[15, 18] = True          # centres (5,5) and (14,18) exist
    v, nu, nn = ref.ssim_counted(m, mask, 11)
    assert (nu, nn) == (4, 0) and sorted(v.tolist()) == sorted(m[0, 0].tolist() + m[9, 13].tolist())
    border = np.ones((20, 24), bool)
    border[5:-5, 5:-5] = False
    assert ref.ssim_counted(m, border, 11)[1:] == (0, 0)
    assert ref.ssim_counted(m, None, 11)[1] == m.size


# ------------------------------------------------------------------------------------------------
# psnr, gaussian_window
# ------------------------------------------------------------------------------------------------
def test_psnr_closed_forms():
    for delta in (0.5, 0.125, 2.0 ** -10):                  # gt + delta exactly: d = delta at every value
        g = (np.random.default_rng(8).integers(0, 64, (9, 11, 3)) / 128.0).astype(np.float32)
        d, nu, ne = ref.error_terms(g + np.float32(delta), g)
        assert (d == delta).all() and (nu, ne) == (99, 0)
        got = ref.psnr_of(math.fsum((d * d).ravel().tolist()), d.size)
        assert got == pytest.approx(-20 * math.log10(delta), abs=1e-12)
    assert ref.psnr_of(0.0, 297) == math.inf                # identical images
    assert math.isnan(ref.psnr_of(0.0, 0))                   # an all-false mask
    d, nu, ne = ref.error_terms(g, g, np.zeros((9, 11), bool))
    assert d.size == 0 and (nu, ne) == (0, 0)
    from neurecon_amd import image_metrics as im
    assert im._psnr_of(297 * 0.25, 297, 1.0) == pytest.approx(-20 * math.log10(0.5), abs=1e-12)
    assert im._psnr_of(0.0, 297, 1.0) == math.inf and math.isnan(im._psnr_of(0.0, 0, 1.0))
    assert im._psnr_of(297 * 4.0, 297, 255.0 ** 2) == pytest.approx(20 * math.log10(255 / 2), abs=1e-12)


def test_gaussian_window():
    from neurecon_amd.image_metrics import gaussian_window
    for win, sigma in ((11, 1.5), (7, 1.0), (33, 5.0), (1, 1.5), (3, 0.5)):
        w = gaussian_window(win, sigma)
        assert w.dtype == np.float64 and w.shape == (win,)
        assert np.array_equal(w, w[::-1]) and (w > 0).all() and w.argmax() == win // 2
        assert abs(math.fsum(w.tolist()) - 1.0) <= 2.0 ** -52
        assert np.array_equal(w, ref.gaussian(win, sigma))
    assert np.array_equal(gaussian_window(), gaussian_window(11, 1.5))
    for kw in (dict(win=10), dict(win=0), dict(win=35), dict(sigma=0.0), dict(sigma=-1.0)):
        with pytest.raises(ValueError):
            gaussian_window(**kw)


# ------------------------------------------------------------------------------------------------
# C ABI: the argument checks come before any HIP call, so fake pointers are never dereferenced
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from neurecon_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


A, B, M, WIN, MAP, OUT, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x100000


def _err(lib):
    return lib.nr_last_error().decode()


def _a256(x):
    return (x + 255) // 256 * 256


def _tile_rows(win):
    return min(32, 64512 // (8 * (31 + win) + 1280) - (win - 1))


def test_workspace_formula(lib):
    ws = lib.nr_img_workspace_bytes
    assert [_tile_rows(w) for w in (1, 7, 9, 11, 33)] == [32, 32, 32, 29, 4]
    for F, H, W, C, win in ((1, 1, 1, 1, 1), (1, 11, 11, 3, 11), (2, 37, 53, 3, 11), (8, 600, 800, 3, 11),
                            (8, 600, 800, 3, 33), (1, 2048, 2049, 4, 7), (3, 70, 150, 1, 1)):
        want = _a256(8 * max(4 * F * -(-H * W // 2048), 3 * F * -(-H // _tile_rows(win)) * -(-W // 32)))
        assert ws(F, H, W, C, win) == want, (F, H, W, C, win)
    for bad in ((0, 8, 8, 3, 11), (1, 0, 8, 3, 11), (1, 8, 0, 3, 11), (1, 8, 8, 0, 11), (1, 8, 8, 5, 11),
                (1, 8, 8, 3, 0), (1, 8, 8, 3, 10), (1, 8, 8, 3, 35), (1, 8, 8, 3, -1), (-1, 8, 8, 3, 11),
                (1, 1 << 16, 1 << 15, 1, 11), (2, 1 << 15, 1 << 15, 1, 11), (1, 1 << 15, 1 << 14, 4, 11),
                (2 ** 31, 1, 1, 1, 1)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1 << 15, (1 << 14) - 1, 4, 11) > 0                      # the largest: just below 2^31 values
    # monotone in every argument
    base = dict(F=2, H=100, W=120, C=2, win=5)
    for key, values in (('F', range(1, 40)), ('H', range(1, 300)), ('W', range(1, 300)), ('C', range(1, 5)),
                        ('win', range(1, 34, 2))):
        sizes = [ws(*{**base, key: v}.values()) for v in values]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), key


def test_error_entry_checks_arguments_without_gpu(lib):
    need = lib.nr_img_workspace_bytes(2, 37, 53, 3, 1)

    def call(pred=A, gt=B, mask=M, F=2, H=37, W=53, C=3, out=OUT, ws=WS, nbytes=need):
        return lib.nr_img_error(pred, gt, mask, F, H, W, C, out, ws, nbytes, None)
    for kw in (dict(pred=None), dict(gt=None)):
        assert call(**kw) == -1 and 'null argument' in _err(lib), kw
    assert call(out=None) == -1 and 'null output' in _err(lib)
    for kw in (dict(C=0), dict(C=5), dict(C=-3)):
        assert call(**kw) == -1 and 'C must be in 1..4' in _err(lib), kw
    for kw in (dict(F=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == -1 and 'positive' in _err(lib), kw
    for kw in (dict(H=1 << 15, W=1 << 15, F=1, C=2), dict(F=2 ** 31, H=1, W=1, C=1),
               dict(F=1 << 20, H=1 << 20, W=1 << 20)):
        assert call(**kw) == -1 and '2^31' in _err(lib), kw
    assert call(nbytes=need - 1) == -4 and 'workspace' in _err(lib)
    assert call(ws=None) == -4 and 'workspace' in _err(lib)
    assert call(H=600, W=800) == -4                                        # a larger frame needs more


def test_ssim_entry_checks_arguments_without_gpu(lib):
    need = lib.nr_img_workspace_bytes(2, 37, 53, 3, 11)

    def call(pred=A, gt=B, mask=M, F=2, H=37, W=53, C=3, window=WIN, win=11, C1=1e-4, C2=9e-4, smap=MAP, out=OUT,
             ws=WS, nbytes=need):
        return lib.nr_img_ssim(pred, gt, mask, F, H, W, C, window, win, C1, C2, smap, out, ws, nbytes, None)
    for kw in (dict(pred=None), dict(gt=None)):
        assert call(**kw) == -1 and 'null argument' in _err(lib), kw
    assert call(window=None) == -1 and 'null window' in _err(lib)
    assert call(out=None) == -1 and 'null output' in _err(lib)
    for kw in (dict(C=0), dict(C=5)):
        assert call(**kw) == -1 and 'C must be in 1..4' in _err(lib), kw
    for win in (0, -1, 2, 10, 34, 35, 101):
        assert call(win=win) == -1 and 'win must be odd' in _err(lib), win
    for kw in (dict(C1=-1.0), dict(C2=float('nan')), dict(C1=float('inf'))):
        assert call(**kw) == -1 and 'C1 and C2' in _err(lib), kw
    assert call(F=4, H=1 << 15, W=1 << 14, C=1) == -1 and '2^31' in _err(lib)
    assert call(nbytes=need - 1) == -4 and 'workspace' in _err(lib)
    assert call(ws=None) == -4
    assert call(win=33) == -4                                               # flatter tiles: more partials


def test_normal_entry_checks_arguments_without_gpu(lib):
    def call(a=A, b=B, mask=M, P=100, out=OUT):
        return lib.nr_img_normal_cos(a, b, mask, P, out, None)
    for kw in (dict(P=-1), dict(P=(2 ** 31) // 3 + 1), dict(P=2 ** 40)):
        assert call(**kw) == -1 and '2^31' in _err(lib), kw
    for kw in (dict(a=None), dict(b=None)):
        assert call(**kw) == -1 and 'null argument' in _err(lib), kw
    assert call(out=None) == -1 and 'null output' in _err(lib)
    assert call(P=0, a=None, b=None, out=None) == 0                         # nothing to do: no launch


# ------------------------------------------------------------------------------------------------
# Python: what is refused before a device is needed
# ------------------------------------------------------------------------------------------------
def test_python_refusals_before_any_work():
    import torch
    from neurecon_amd import image_metrics as im
    a = np.zeros((12, 13, 3), np.float32)
    for fn in (im.image_error, im.psnr, im.ssim, im.ssim_sums, im.evaluate_frames):
        with pytest.raises(ValueError, match='same shape'):
            fn(a, np.zeros((12, 14, 3), np.float32))
        with pytest.raises(ValueError, match='channel count'):
            fn(np.zeros((12, 13, 5), np.float32), np.zeros((12, 13, 5), np.float32))
        with pytest.raises(ValueError, match='mask must be'):
            fn(a, a, mask=np.ones((13, 12), bool))
        with pytest.raises(ValueError, match='mask must be'):
            fn(a[None], a[None], mask=np.ones((12, 13), bool))
        with pytest.raises(ValueError, match=r'\[H, W\]'):
            fn(np.zeros(5, np.float32), np.zeros(5, np.float32))
    for fn in (im.psnr, im.ssim, im.evaluate_frames):
        for r in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='data_range'):
                fn(a, a, data_range=r)
    for w in (np.ones(4) / 4, np.ones((3, 3)) / 9, np.ones(35) / 35, np.array([0.5, np.nan, 0.5]), np.zeros(0)):
        with pytest.raises(ValueError, match='window'):
            im.ssim(a, a, window=w)
    with pytest.raises(ValueError, match='same shape'):
        im.depth_error(np.zeros((4, 5)), np.zeros((5, 4)))
    with pytest.raises(ValueError, match=r'\[H, W\] or \[F, H, W\]'):
        im.depth_error(np.zeros((2, 4, 5, 1)), np.zeros((2, 4, 5, 1)))
    with pytest.raises(ValueError, match='mask must be'):
        im.depth_error(np.zeros((4, 5)), np.zeros((4, 5)), mask=np.ones((5, 4), bool))
    with pytest.raises(ValueError, match=r'\[\.\.\., 3\]'):
        im.normal_cosine(np.zeros((4, 5, 2)), np.zeros((4, 5, 2)))
    with pytest.raises(ValueError, match='mask must be'):
        im.normal_error(np.zeros((4, 5, 3)), np.zeros((4, 5, 3)), mask=np.ones((4, 5, 3), bool))
    with pytest.raises(ValueError, match=r'\[H, W, 3\]'):
        im.normal_error(np.zeros((5, 3)), np.zeros((5, 3)))
    if not torch.cuda.is_available():                      # no fallback: host input without a device is refused
        for fn in (im.image_error, im.psnr, im.ssim, im.evaluate_frames):
            with pytest.raises(RuntimeError, match='GPU'):
                fn(a, a)
        with pytest.raises(RuntimeError, match='GPU'):
            im.depth_error(a[..., 0], a[..., 0])
        with pytest.raises(RuntimeError, match='GPU'):
            im.normal_error(a, a)


def test_command_line_loader(tmp_path):
    from neurecon_amd import image_metrics as im
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 4, 1)
    np.save(tmp_path / 'a.npy', x)
    np.savez(tmp_path / 'b.npz', frames=x)
    np.savez(tmp_path / 'two.npz', p=x, q=x)
    assert np.array_equal(im._load_stack(str(tmp_path / 'a.npy'), 'pred'), x)
    assert np.array_equal(im._load_stack(str(tmp_path / 'b.npz'), 'gt'), x)
    assert im._load_stack(str(tmp_path / 'a.npy'), 'mask').dtype == bool
    with pytest.raises(ValueError, match='one array'):
        im._load_stack(str(tmp_path / 'two.npz'), 'pred')
    (tmp_path / 'empty').mkdir()
    try:
        import PIL  # noqa: F401
        with pytest.raises(ValueError, match='holds no pred image'):
            im._load_stack(str(tmp_path / 'empty'), 'pred')
    except ImportError:
        with pytest.raises(RuntimeError, match='needs PIL'):
            im._load_stack(str(tmp_path / 'empty'), 'pred')
