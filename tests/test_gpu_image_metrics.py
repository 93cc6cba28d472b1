"""GPU tests of the image metrics (neurecon_amd/image_metrics.py; nr_img_error, nr_img_ssim, nr_img_normal_cos,
neurecon_amd/csrc/nr_imgmetrics.hip).

The reference is the numpy restatement in tests/image_metrics_ref.py.  The SSIM map and the cosine map are
compared by equality (bit for bit, NaNs in the same places), the counts by equality, the sums with math.fsum of
the reference's counted values within n 2^-53 sum |v|, the bound of any fixed summation tree.  Every case runs
twice and the two runs must be bit-identical.  The shapes are the smallest that can break the kernel: single
values, empty maps, every remainder at the tile edges (tiles are at most 64 pixels in either dimension, so a
sweep over 131 output rows or columns crosses every remainder twice), wave and workgroup boundaries of the
error kernel."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_metrics_ref as ref
from test_gpu_mcubes import _sphere
from test_mesh_render import std_intrinsics, std_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

UNIFORM7 = np.full(7, 1.0 / 7.0)
WINDOWS = {'gauss11': None, 'uniform7': UNIFORM7, 'one': np.ones(1)}


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------
# SSIM
# ------------------------------------------------------------------------------------------------
def check_ssim(x, y, mask=None, window=None, data_range=1.0, on_device=True):
    """x, y [F, H, W, C] (float arrays), mask [F, H, W] or None -> the device's result dict, the map on the host"""
    from neurecon_amd import image_metrics as im
    w = ref.gaussian() if window is None else np.asarray(window, np.float64)
    win = len(w)
    F, H, W, C = x.shape
    args = (gpu(x), gpu(y)) if on_device else (x, y)
    m = None if mask is None else (gpu(mask) if on_device else mask)
    runs = [im.ssim_sums(*args, mask=m, data_range=data_range, window=window, return_map=True) for _ in range(2)]
    a, b = runs
    got = a['map'].cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (F, max(H - win + 1, 0), max(W - win + 1, 0), C)
    assert same_bits(got, b['map'].cpu().numpy()), 'two runs differ in the map'
    for k in ('sum', 'n_used', 'n_nan'):
        assert same_bits(a[k], b[k]), f'two runs differ in {k}'
    want = ref.ssim_map(ref.to_float(x), ref.to_float(y), w, *ref.constants(data_range))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), 'NaNs in other places'
    bad = (got != want) & ~nan
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(got - want)[bad].max()))
    mean = im.ssim(*args, mask=m, data_range=data_range, window=window)
    for f in range(F):
        v, nu, nn = ref.ssim_counted(want[f], None if mask is None else mask[f], win)
        assert (int(a['n_used'][f]), int(a['n_nan'][f])) == (nu, nn), f
        assert abs(float(a['sum'][f]) - math.fsum(v.tolist())) <= ref.sum_bound(v), f
        if nu:
            assert mean[f] == float(a['sum'][f]) / nu
        else:
            assert math.isnan(mean[f]) and float(a['sum'][f]) == 0.0
    a['map'] = got
    return a


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('shape', [(11, 11), (10, 40), (40, 10), (11, 75), (37, 53), (70, 150)])
def test_ssim_map_equals_the_restatement(shape, C):
    x, y = ref.smooth_pair((2,) + shape + (C,), 100 + C) if shape == (70, 150) else \
        ref.random_pair((2,) + shape + (C,), 100 + C)
    out = check_ssim(x, y)
    if min(shape) < 11:                                      # empty map, n_used 0, mean NaN, no error
        assert out['map'].size == 0 and out['n_used'].tolist() == [0, 0] and out['n_nan'].tolist() == [0, 0]
    else:
        assert out['n_used'].tolist() == [(shape[0] - 10) * (shape[1] - 10) * C] * 2


def test_ssim_at_every_tile_edge():
    """every H from win to win + 130 at W = win + 3 and every W likewise at H = win + 3: 1 .. 131 output rows /
    columns cross every remainder of a tile of at most 64 twice; one random image, cropped"""
    win = 11
    big_x, big_y = ref.random_pair((2, win + 130, win + 130, 3), 7)
    for n in range(win, win + 131):
        check_ssim(big_x[:, :n, :win + 3], big_y[:, :n, :win + 3])
        check_ssim(big_x[:, :win + 3, :n], big_y[:, :win + 3, :n])


@pytest.mark.parametrize('name', ['uniform7', 'one', 'gauss33', 'gauss5'])
def test_ssim_windows(name):
    """other windows take other tile heights (32 rows up to win 9, 29 at 11, 4 at 33)"""
    w = {'gauss33': ref.gaussian(33, 5.0), 'gauss5': ref.gaussian(5, 1.0)}.get(name, WINDOWS.get(name))
    win = len(w)
    for shape in ((win, win), (win + 3, 75), (37, 53), (70, 150)):
        if shape[0] < win:
            continue
        x, y = ref.random_pair((2,) + shape + (3,), 20 + win)
        check_ssim(x, y, window=w)
    x, y = ref.random_pair((1, win + 70, win + 2, 1), 21)
    for n in range(win, win + 71, 3):                        # tile edges of this window's tile height
        check_ssim(x[:, :n], y[:, :n], window=w)


def test_ssim_values():
    shape = (2, 37, 53, 3)
    zeros, ones = np.zeros(shape, np.float32), np.ones(shape, np.float32)
    for x, y in ((zeros, zeros), (ones, ones), (zeros, ones)):
        check_ssim(x, y)
    check_ssim(*ref.random_pair(shape, 30, scale=1e-3))
    x, y = ref.uint8_pair(shape, 31)
    check_ssim(x.astype(np.float32), y.astype(np.float32), data_range=255.0)     # 0 .. 255 as floats
    out = check_ssim(x, y)                                                       # uint8 in: v / 255
    assert 0.0 < out['sum'][0] / out['n_used'][0] < 1.0
    check_ssim(x, y, on_device=False)                                            # host arrays in


def test_ssim_masks():
    shape = (2, 37, 53, 3)
    x, y = ref.random_pair(shape, 40)
    rng = np.random.default_rng(41)
    out = check_ssim(x, y, mask=rng.random(shape[:3]) < 0.4)
    assert 0 < out['n_used'][0] < 27 * 43 * 3
    out = check_ssim(x, y, mask=np.zeros(shape[:3], bool))
    assert out['n_used'].tolist() == [0, 0] and out['sum'].tolist() == [0.0, 0.0]
    border = np.ones(shape[:3], bool)
    border[:, 5:-5, 5:-5] = False                            # true only where no window is centred
    out = check_ssim(x, y, mask=border)
    assert out['n_used'].tolist() == [0, 0]
    check_ssim(x, y, mask=rng.random(shape[:3]) < 0.5, window=UNIFORM7)


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_ssim_one_non_finite_value(bad):
    x, y = ref.random_pair((2, 40, 45, 3), 50)
    x[0, 20, 22, 1] = bad
    y[1, 3, 41, 2] = bad
    out = check_ssim(x, y)
    nan = np.isnan(out['map'])
    # pixel (3, 41) of a 40 x 45 frame lies in the windows of output rows 0..3 and columns 31..34 (the last)
    assert nan[0, ..., 1].sum() == 121 and nan[0].sum() == 121 and nan[1].sum() == nan[1, ..., 2].sum() == 4 * 4
    assert out['n_nan'].tolist() == [121, 16]
    mask = np.ones((2, 40, 45), bool)
    mask[0, 25, :] = False                                   # centres of output row 20: 11 of the NaN values
    assert check_ssim(x, y, mask=mask)['n_nan'].tolist() == [110, 16]


def test_ssim_identical_images():
    from neurecon_amd import image_metrics as im
    for shape, window in (((2, 37, 53, 3), None), ((2, 70, 150, 4), None), ((2, 37, 53, 1), UNIFORM7)):
        x, _ = ref.random_pair(shape, 60)
        out = check_ssim(x, x, window=window)
        assert (out['map'] == 1.0).all()
        mean = im.ssim(gpu(x), gpu(x), window=window)
        assert mean.tolist() == [1.0, 1.0]
    mean, smap = im.ssim(gpu(x[0]), gpu(x[0]), return_map=True)                  # one frame: a number, a 3-D map
    assert mean == 1.0 and isinstance(mean, float) and smap.shape == (27, 43, 1) and smap.is_cuda


def test_ssim_frames_are_independent():
    """F = 3 with different masks equals three single-frame calls, bit for bit"""
    from neurecon_amd import image_metrics as im
    x, y = ref.random_pair((3, 45, 70, 3), 70)
    rng = np.random.default_rng(71)
    mask = rng.random((3, 45, 70)) < np.array([0.2, 0.5, 0.9])[:, None, None]
    whole = im.ssim_sums(gpu(x), gpu(y), mask=gpu(mask), return_map=True)
    for f in range(3):
        one = im.ssim_sums(gpu(x[f]), gpu(y[f]), mask=gpu(mask[f]), return_map=True)
        assert torch.equal(one['map'].view(torch.int64), whole['map'][f].view(torch.int64))
        assert same_bits(np.float64(one['sum']), whole['sum'][f])
        assert one['n_used'] == whole['n_used'][f] and one['n_nan'] == whole['n_nan'][f]


# ------------------------------------------------------------------------------------------------
# error sums
# ------------------------------------------------------------------------------------------------
def check_error(p, g, mask=None):
    from neurecon_amd import image_metrics as im
    m = None if mask is None else gpu(mask)
    a, b = (im.image_error(gpu(p), gpu(g), mask=m) for _ in range(2))
    for k in ('sum_sq', 'sum_abs', 'n_used', 'n_excluded'):
        assert same_bits(a[k], b[k]), f'two runs differ in {k}'
    C = p.shape[-1]
    psnr = im.psnr(gpu(p), gpu(g), mask=m)
    for f in range(p.shape[0]):
        d, nu, ne = ref.error_terms(p[f], g[f], None if mask is None else mask[f])
        assert (int(a['n_used'][f]), int(a['n_excluded'][f])) == (nu, ne), f
        sq, ab = (d * d).ravel(), np.abs(d).ravel()
        assert abs(float(a['sum_sq'][f]) - math.fsum(sq.tolist())) <= ref.sum_bound(sq), f
        assert abs(float(a['sum_abs'][f]) - math.fsum(ab.tolist())) <= ref.sum_bound(ab), f
        want = ref.psnr_of(float(a['sum_sq'][f]), nu * C)
        assert psnr[f] == want or (math.isnan(psnr[f]) and math.isnan(want))
    return a


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('shape', [(1, 1), (1, 63), (1, 64), (1, 65), (257, 3), (70, 150)])
def test_error_sums(shape, C):
    """1, 63, 64, 65, 771 and 10500 pixels: lanes, waves, and the 2048 pixels of a workgroup"""
    full = (2,) + shape + (C,)
    p, g = ref.random_pair(full, 80 + C)
    out = check_error(p, g)
    assert out['n_used'].tolist() == [shape[0] * shape[1]] * 2 and out['n_excluded'].tolist() == [0, 0]
    rng = np.random.default_rng(81)
    mask = rng.random(full[:3]) < 0.6
    check_error(p, g, mask)
    out = check_error(p, g, np.zeros(full[:3], bool))
    assert out['n_used'].tolist() == [0, 0] and out['sum_sq'].tolist() == [0.0, 0.0]
    q = p.copy()
    flat = q.reshape(2, -1, C)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):      # non-finite values, in either image
        flat[0, (k * 37) % flat.shape[1], k % C] = bad
    h = g.copy()
    h.reshape(2, -1, C)[1, -1, C - 1] = np.nan
    out = check_error(q, h, mask)
    out = check_error(q, h)
    assert out['n_excluded'][1] == 1 and 1 <= out['n_excluded'][0] <= 3
    out = check_error(p, p)                                  # identical images: exactly 0
    assert out['sum_sq'].tolist() == [0.0, 0.0] and out['sum_abs'].tolist() == [0.0, 0.0]


def test_psnr_closed_forms_on_the_device():
    from neurecon_amd import image_metrics as im
    g = (np.random.default_rng(8).integers(0, 64, (2, 19, 23, 3)) / 128.0).astype(np.float32)
    for delta in (0.5, 0.125, 2.0 ** -10):
        got = im.psnr(gpu(g + np.float32(delta)), gpu(g))
        assert got.shape == (2,) and np.abs(got - (-20 * math.log10(delta))).max() <= 1e-12
    assert im.psnr(gpu(g), gpu(g)).tolist() == [math.inf, math.inf]
    assert np.isnan(im.psnr(gpu(g), gpu(g + 1), mask=np.zeros((2, 19, 23), bool))).all()
    u8 = (g * 128).astype(np.uint8)
    # uint8: v / 255 in fp32, host arrays, one frame: a number.  The two quotients are each off by at most 2^-25
    # (values <= 0.26), their difference 2 / 255 by at most 2^-24: 7.6e-6 of it, 6.6e-5 dB; the bound is 1e-4
    got = im.psnr(u8[0], u8[0] + np.uint8(2))
    assert isinstance(got, float) and abs(got - 20 * math.log10(255 / 2)) <= 1e-4
    assert abs(im.psnr(u8[0].astype(np.float32), (u8[0] + 2).astype(np.float32), data_range=255.0)
               - 20 * math.log10(255 / 2)) <= 1e-12


# ------------------------------------------------------------------------------------------------
# normal cosine
# ------------------------------------------------------------------------------------------------
def test_normal_cosine_map():
    from neurecon_amd import image_metrics as im
    rng = np.random.default_rng(90)
    a = rng.standard_normal((2, 23, 29, 3)).astype(np.float32)
    b = (a + 0.3 * rng.standard_normal(a.shape)).astype(np.float32)
    a /= np.linalg.norm(a, axis=-1, keepdims=True)
    a[0, 0, 0] = 0.0                                         # a zero-length normal
    b[0, 0, 1] = 0.0
    a[0, 0, 2, 1] = np.nan                                   # non-finite components
    b[0, 0, 3, 2] = np.inf
    b[0, 1] = a[0, 1]                                        # identical unit normals: cos exactly 1
    b[0, 2] = -a[0, 2]                                       # antiparallel: exactly -1
    a[1, 0] *= 1e-20                                         # tiny and huge, not unit
    b[1, 1] *= 1e18
    mask = rng.random(a.shape[:3]) < 0.7
    for m in (None, mask):
        got, again = (im.normal_cosine(gpu(a), gpu(b), None if m is None else gpu(m)).cpu().numpy() for _ in range(2))
        want = ref.normal_cos(a, b, m)
        assert got.shape == want.shape == a.shape[:3] and got.dtype == np.float64
        assert same_bits(got, again)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])
        assert np.nanmax(got) <= 1.0 and np.nanmin(got) >= -1.0
    assert np.isnan(got[0, 0, :4]).all() and (np.isnan(got) == (~mask | np.isnan(ref.normal_cos(a, b)))).all()
    got = im.normal_cosine(gpu(a), gpu(b)).cpu().numpy()
    assert (got[0, 1, 4:] == 1.0).all() and (got[0, 2, 4:] == -1.0).all()
    assert im.normal_cosine(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).shape == (0,)
    e = im.normal_error(gpu(a), gpu(b), gpu(mask))
    for f in range(2):
        ang = np.degrees(np.arccos(want[f][~np.isnan(want[f])]))
        assert e['n_used'][f] == ang.size and e['n_excluded'][f] == mask[f].sum() - ang.size
        assert abs(e['mean_deg'][f] - ang.mean()) <= 1e-9 and abs(e['median_deg'][f] - np.median(ang)) <= 1e-9


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
H_E, W_E = 48, 64


@pytest.fixture(scope='module')
def renders():
    """the marching-cubes sphere, with the sphere's own normals at its vertices (blended per pixel, so two views
    of one face differ), rendered from two cameras a small angle apart"""
    from neurecon_amd.mesh_util import marching_cubes, render_mesh
    n = 32
    verts, faces = marching_cubes(gpu(_sphere((n, n, n), (0, 0, 0), 0.6)), 0.0, spacing=2.0 / (n - 1), origin=-1.0)
    normals = verts / verts.norm(dim=1, keepdim=True)
    K = std_intrinsics()
    K[0, 2], K[1, 2] = 31.3, 23.9
    return [render_mesh(verts, faces, std_pose(a=a), K, H_E, W_E, normals=normals) for a in (0.7, 0.73)]


def test_end_to_end_on_two_renders(renders):
    from neurecon_amd import image_metrics as im
    A, B = renders
    mask = A['mask'] & B['mask']
    n_mask = int(mask.sum())
    assert 200 < n_mask < H_E * W_E and not torch.equal(A['rgb'], B['rgb'])
    got = im.evaluate_frames(A['rgb'], B['rgb'], mask=mask)
    assert got == im.evaluate_frames(A['rgb'], B['rgb'], mask=mask)
    assert all(isinstance(got[k], float) for k in ('psnr_mean', 'ssim_mean', 'mse_mean', 'mae_mean'))
    pa, pb, m = A['rgb'].cpu().numpy(), B['rgb'].cpu().numpy(), mask.cpu().numpy()
    d, nu, ne = ref.error_terms(pa, pb, m)
    assert (got['frames'], got['channels'], got['n_used'], got['n_excluded']) == (1, 3, [nu], [ne]) and nu == n_mask
    sq = (d * d).ravel()
    assert abs(got['mse'][0] * nu * 3 - math.fsum(sq.tolist())) <= 2 * ref.sum_bound(sq)
    want_psnr = ref.psnr_of(math.fsum(sq.tolist()), nu * 3)
    assert abs(got['psnr'][0] - want_psnr) <= 1e-9 and got['psnr_mean'] == got['psnr'][0] and 10 < want_psnr < 100
    smap = ref.ssim_map(pa, pb)
    v, su, sn = ref.ssim_counted(smap, m, 11)
    assert (got['ssim_n_used'], got['ssim_n_nan']) == ([su], [sn]) and su > 0
    assert abs(got['ssim'][0] * su - math.fsum(v.tolist())) <= 2 * ref.sum_bound(v) and 0 < got['ssim'][0] < 1
    mean, dmap = im.ssim(A['rgb'], B['rgb'], mask=mask, return_map=True)
    assert np.array_equal(dmap.cpu().numpy(), smap) and mean == got['ssim'][0]
    # depth and normals of the two renders, where both hit
    de = im.depth_error(A['depth'], B['depth'], mask=mask)
    dd, dn, _ = ref.error_terms(A['depth'].cpu().numpy()[..., None], B['depth'].cpu().numpy()[..., None], m)
    assert de['n_used'] == dn == n_mask and de['n_excluded'] == 0
    assert abs(de['l1'] - math.fsum(np.abs(dd).ravel().tolist()) / dn) <= 1e-12
    assert abs(de['rmse'] - math.sqrt(math.fsum((dd * dd).ravel().tolist()) / dn)) <= 1e-12
    assert 0 < de['l1'] <= de['rmse']
    de = im.depth_error(A['depth'], B['depth'])              # no mask: a miss (depth 0) is not valid
    assert de['n_used'] == n_mask and de['n_excluded'] == H_E * W_E - n_mask
    cos = im.normal_cosine(A['normal'], B['normal'], mask).cpu().numpy()
    want = ref.normal_cos(A['normal'].cpu().numpy(), B['normal'].cpu().numpy(), m)
    assert np.array_equal(np.isnan(cos), np.isnan(want)) and np.array_equal(cos[m], want[m])
    ne_ = im.normal_error(A['normal'], B['normal'], mask)
    ang = np.degrees(np.arccos(want[m]))
    assert ne_['n_used'] == n_mask and ne_['n_excluded'] == 0
    assert abs(ne_['mean_deg'] - ang.mean()) <= 1e-9 and abs(ne_['median_deg'] - np.median(ang)) <= 1e-9
    assert 0 < ne_['median_deg'] < 30


def test_a_frame_against_itself(renders):
    from neurecon_amd import image_metrics as im
    A = renders[0]
    got = im.evaluate_frames(A['rgb'], A['rgb'], mask=A['mask'])
    assert got['psnr'] == [math.inf] and got['ssim'] == [1.0] and got['mse'] == [0.0] and got['ssim_mean'] == 1.0
    de = im.depth_error(A['depth'], A['depth'])
    assert de['l1'] == 0.0 and de['rmse'] == 0.0 and de['n_used'] == int(A['mask'].sum())
    ne_ = im.normal_error(A['normal'], A['normal'])          # misses have a zero normal: excluded
    assert ne_['mean_deg'] == 0.0 and ne_['median_deg'] == 0.0 and ne_['n_used'] == int(A['mask'].sum())
    assert ne_['n_excluded'] == H_E * W_E - ne_['n_used']


def test_command_line(tmp_path):
    from neurecon_amd import image_metrics as im
    x, y = ref.smooth_pair((2, 24, 31, 3), 95)
    mask = np.random.default_rng(96).random((2, 24, 31)) < 0.8
    np.save(tmp_path / 'pred.npy', x)
    np.save(tmp_path / 'gt.npy', y)
    np.save(tmp_path / 'mask.npy', mask)
    p = subprocess.run([sys.executable, '-m', 'neurecon_amd.image_metrics', str(tmp_path / 'pred.npy'),
                        str(tmp_path / 'gt.npy'), '--mask', str(tmp_path / 'mask.npy'), '--data-range', '1.0'],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    got = json.loads(lines[0])
    want = im.evaluate_frames(x, y, mask=mask, data_range=1.0)
    for k, v in want.items():
        assert got[k] == v, k
    assert got['frames'] == 2 and len(got['psnr']) == 2 and got['pred'].endswith('pred.npy')
