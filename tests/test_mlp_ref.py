"""The float64 references and input classes of tests/mlp_ref.py are fit for purpose (CPU only).

1. The float64 reference is the oracle's float64 evaluation, to 1e-12, on every configuration: two independent
   statements of each net.
2. Condition A: on every configuration and input class the oracle evaluated in fp32 on the CPU lies within half the
   bar of the float64 reference, so a kernel that misses the bar there is wrong and not merely rounding.  This is a
   condition on the inputs; mlp_ref.MIXED_GAIN and NERF_GAIN are the largest gains that meet it with room for
   another BLAS build's summation order, and the values tried are recorded beside them.  The same is asserted of
   mlp_ref.sequential_fp32_*, fp32 arithmetic in a fixed order, whose figure no BLAS build moves.
3. The comparison has teeth: each of four deliberate errors applied to the reference puts more than 10 % of the
   points outside the bar on the class named (NeRF: three errors)."""
import numpy as np
import pytest
import torch

import mlp_ref as R

IDS = [R.cfg_id(c) for c in R.RAD_CONFIGS]


@pytest.fixture(scope='module')
def rad():
    """configuration -> (float64 layers, fp32 CPU oracle, float64 oracle); weights do not depend on the precision"""
    from oracle.nets import RadianceNet
    cache = {}

    def get(c):
        if c not in cache:
            layers = R.radiance_layers(R.radiance_module(c, 'fp32'))
            mk = lambda dt: RadianceNet(R.oracle_radiance_state(layers, dt), prefix='', D=c.D, multires=-1,
                                        multires_view=c.mv, use_view_dirs=c.view, siren=c.siren)
            cache[c] = layers, mk(torch.float32), mk(torch.float64)
        return cache[c]
    return get


@pytest.fixture(scope='module')
def nerf():
    from oracle.nets import NeRFNet
    layers = R.nerf_layers(R.nerf_module('fp32'))
    return (layers, NeRFNet(R.oracle_nerf_state(layers, torch.float32), prefix=''),
            NeRFNet(R.oracle_nerf_state(layers, torch.float64), prefix=''))


def _classes(c):
    return (('unit', R.unit()), ('mixed_scale', R.mixed_scale(R.MIXED_GAIN[c.siren])), ('zeros', R.zeros()),
            ('view_edges', R.view_edges(c.mv if c.view else -1)))


NERF_CLASSES = (('nerf_unit', R.nerf_unit), ('nerf_edges', R.nerf_edges))


def test_classes_hold_300_distinct_points():
    for mv in R.VIEW_MULTIRES:
        for name, t in _classes(R.RadCfg(mv, True, 4, False)):
            assert all(len(a) == R.N_POINTS for a in t) and R.all_distinct(*t), (name, mv)
    for name, build in NERF_CLASSES:
        t = build()
        assert all(len(a) == R.N_POINTS for a in t) and R.all_distinct(*t), name
    x, _, _, f = R.zeros()
    assert not f[R.ZERO_ROWS].any() and not x[R.ZERO_ROWS].any() and torch.signbit(x[R.ZERO_ROWS]).any()
    k = torch.log2(R.mixed_scale(1.0)[3][:, 0] / R.unit()[3][:, 0]).round()
    assert k.min() == -6 and k.max() == 6 and (k[1:] != k[:-1]).float().mean() > 0.8  # neighbours differ


def test_view_edges_reach_every_band():
    """every band of every view multires has components within 2 ulp of each of its four turning points"""
    for mv in (1, 3, 4, 7):
        v = R.view_edges(mv)[1].numpy()
        for band in range(mv):
            for k in range(1, 5):
                t = np.float32(k * np.pi / 2 ** (band + 1))
                assert (np.abs(v - t) <= 2 * np.spacing(t)).sum() >= 5, (mv, band, k)
    x4 = R.nerf_edges()[0].numpy()
    assert set(np.unique(x4[200:, 3])) == {np.float32(1.0), np.float32(0.05), np.float32(1e-3), np.float32(0.0)}
    for band in range(10):
        t = np.float32(np.pi / 2 ** (band + 1))
        assert (np.abs(x4 - t) <= 2 * np.spacing(t)).sum() >= 5, band


@pytest.mark.parametrize('c', R.RAD_CONFIGS, ids=IDS)
def test_radiance_reference_is_the_oracle_in_float64(rad, c):
    layers, _, o64 = rad(c)
    for name, (x, v, n, f) in _classes(c):
        ref = R.float64_rgb(layers, c, x, v, n, f)
        with torch.no_grad():
            want = o64.forward(x.double(), v.double(), n.double(), f.double()).numpy()
        assert np.abs(ref - want).max() <= 1e-12, name


def test_nerf_reference_is_the_oracle_in_float64(nerf):
    layers, _, o64 = nerf
    for name, build in NERF_CLASSES:
        x4, v = build()
        sigma, rgb = R.float64_nerf(layers, x4, v)
        with torch.no_grad():
            s, c = o64.forward(x4.double(), v.double())
        assert np.abs(sigma - s.numpy()).max() <= 1e-12 and np.abs(rgb - c.numpy()).max() <= 1e-12, name


@pytest.mark.parametrize('c', R.RAD_CONFIGS, ids=IDS)
def test_condition_a_radiance(rad, c):
    layers, o32, _ = rad(c)
    for name, (x, v, n, f) in _classes(c):
        ref = R.float64_rgb(layers, c, x, v, n, f)
        with torch.no_grad():
            w = R.worst(o32.forward(x, v, n, f), ref, *R.bar(c))
        ws = R.worst(R.sequential_fp32_rgb(layers, c, x, v, n, f), ref, *R.bar(c))
        print(f'{R.cfg_id(c)} {name}: fp32 CPU worst err / (atol + rtol |ref|) = {w:.3f}, sequential {ws:.3f}')
        assert w <= 0.5 and ws <= 0.5, name


def test_condition_a_nerf(nerf):
    """at the fp32 bar, the tighter of the two"""
    layers, o32, _ = nerf
    for name, build in NERF_CLASSES:
        x4, v = build()
        sigma, rgb = R.float64_nerf(layers, x4, v)
        with torch.no_grad():
            s, c = o32.forward(x4, v)
        ws, wc = R.worst(s, sigma, *R.BAR_NERF['fp32']), R.worst(c, rgb, *R.BAR_NERF['fp32'])
        s, c = R.sequential_fp32_nerf(layers, x4, v)
        qs, qc = R.worst(s, sigma, *R.BAR_NERF['fp32']), R.worst(c, rgb, *R.BAR_NERF['fp32'])
        print(f'nerf {name}: fp32 CPU worst err / (atol + rtol |ref|): sigma {ws:.3f}, rgb {wc:.3f}; sequential: sigma '
              f'{qs:.3f}, rgb {qc:.3f}; rgb in [{rgb.min():.3f}, {rgb.max():.3f}], max |sigma| {np.abs(sigma).max():.2f}')
        assert max(ws, wc, qs, qc) <= 0.5, name


def test_nerf_gain_spreads_the_outputs(nerf):
    """what the gain is for: rgb leaves sigmoid(0) and sigma leaves 0; at gain 1 rgb spans 0.06 and |sigma| stays
    below 0.03, and the gain must buy at least twice the one and five times the other"""
    sigma, rgb = R.float64_nerf(nerf[0], *R.nerf_unit())
    assert rgb.max() - rgb.min() > 0.12 and np.abs(sigma).max() > 0.15


# -- deliberate errors ------------------------------------------------------------------------------------------
def _swap_pairs(v):
    return v[torch.arange(len(v)) ^ 1]


def _caught(name, wrong, ref, bar):
    frac = R.frac_outside(wrong, ref, *bar)
    print(f'{name}: {frac * 100:.1f} % of the points outside the bar')
    return frac > 0.10


@pytest.mark.parametrize('c', R.RAD_CONFIGS, ids=IDS)
def test_radiance_errors_are_caught(rad, c):
    layers = rad(c)[0]
    x, v, n, f = R.unit()
    ref = R.float64_rgb(layers, c, x, v, n, f)
    tag = R.cfg_id(c)
    if c.view:  # 1. view dirs of points p and p + 1 swapped
        assert _caught(f'{tag} swapped view dirs', R.float64_rgb(layers, c, x, _swap_pairs(v), n, f), ref, R.bar(c))
    # 2. the last small-input column dropped: n_z with view dirs, x_z without
    W0 = layers[0][0].clone()
    W0[:, R.n_small(c) - 1] = 0.0
    assert _caught(f'{tag} last small column dropped',
                   R.float64_rgb([(W0, layers[0][1])] + layers[1:], c, x, v, n, f), ref, R.bar(c))
    # 3. layer 1's bias rotated by one row
    rot = layers[:1] + [(layers[1][0], torch.roll(layers[1][1], 1))] + layers[2:]
    assert _caught(f'{tag} layer-1 bias rotated', R.float64_rgb(rot, c, x, v, n, f), ref, R.bar(c))
    # 4. the per-point operand scale taken from the previous point
    x, v, n, f = R.mixed_scale(R.MIXED_GAIN[c.siren])
    assert _caught(f'{tag} scale of the previous point', R.float64_rgb(layers, c, x, v, n, f, scale_from_previous=True),
                   R.float64_rgb(layers, c, x, v, n, f), R.bar(c))


def test_nerf_errors_are_caught(nerf):
    """at the f16x3 bar, the wider of the two"""
    layers = nerf[0]
    x4, v = R.nerf_unit()
    ref = np.concatenate([R.float64_nerf(layers, x4, v)[0][:, None], R.float64_nerf(layers, x4, v)[1]], 1)
    both = lambda out: np.concatenate([out[0][:, None], out[1]], 1)
    bar = R.BAR_NERF['f16x3']
    assert _caught('nerf swapped view dirs', both(R.float64_nerf(layers, x4, _swap_pairs(v))), ref, bar)
    rot = dict(layers, pts=layers['pts'][:1] + [(layers['pts'][1][0], torch.roll(layers['pts'][1][1], 1))] +
               layers['pts'][2:])
    assert _caught('nerf layer-1 bias rotated', both(R.float64_nerf(rot, x4, v)), ref, bar)
    assert _caught('nerf skip concatenated in the wrong order', both(R.float64_nerf(layers, x4, v, skip_swapped=True)),
                   ref, bar)
