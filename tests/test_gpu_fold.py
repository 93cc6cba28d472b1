"""NeuS render fold: the SDF net's geometry-feature layer (no activation) folded into the radiance net's
layer 0 (nr_neus_fold_pack; sdf4_kernel runs F8' in F8's place, rad4_kernel<KBS, true> adds u in layer
0's epilogue).

The bar on rgb is the one the unfolded f16x3 radiance kernel is held to (test_f16x3_radiance_vs_golden):
rtol 1e-5, atol 1e-6, here against a float64 evaluation points -> h7 -> f -> layer 0 -> ... -> rgb on the CPU
from the model's effective fp32 weights.  Both routes run on the same points and both worst ratios
err / (atol + rtol |ref|) are printed."""
import ctypes

import numpy as np
import pytest
import torch

import weightgen as wg
from helpers import neus_model

pytestmark = pytest.mark.gpu

RT, AT = 1e-5, 1e-6
SIZES = (1, 16, 17, 128, 129, 300)  # a column, a column + 1, a tile, a tile + 1, a ragged third tile


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()  # must load: no fallback exists


def _effective(layers):
    return [(l.effective_weight().detach().cpu().double(), l.bias.detach().cpu().double()) for l in layers]


def _float64_rgb(m, x, v, n):
    """points -> h7 -> feature -> radiance layers -> rgb in float64 (base.py:243-263, :372-391)"""
    import math
    from oracle.nets import embed, softplus100
    x, v, n = x.double(), v.double(), n.double()
    sl = _effective(m.implicit_surface.surface_fc_layers)
    xe = embed(x, 6)
    h = xe
    for i in range(8):
        if i == 4:
            h = torch.cat([h, xe], -1) / math.sqrt(2)
        h = softplus100(h @ sl[i][0].T + sl[i][1])
    f = (h @ sl[8][0].T + sl[8][1])[:, 1:]
    rl = _effective(m.radiance_net.layers)
    h = torch.cat([x, embed(v, 4), n, f], -1)
    for i in range(4):
        h = torch.relu(h @ rl[i][0].T + rl[i][1])
    return torch.sigmoid(h @ rl[4][0].T + rl[4][1]).numpy()


def _folded_rgb(m, x, v, n):
    from neurecon_amd import _lib as L
    dev = x.device
    sdesc, spk = m.implicit_surface.nr_packed(dev)
    rdesc, rpk = m.radiance_net.nr_packed(dev)
    fpk = m.radiance_net.nr_fold_packed(m.implicit_surface, dev)
    assert fpk is not None
    P = x.shape[0]
    u = torch.empty(P, 256, device=dev)
    sdf = torch.empty(P, device=dev)
    rgb = torch.empty(P, 3, device=dev)
    L.check(L.lib().nr_neus_fold_forward(ctypes.byref(sdesc), L.ptr(spk), ctypes.byref(rdesc), L.ptr(rpk), L.ptr(fpk),
                                         L.ptr(x), L.ptr(v), 1, L.ptr(n), P, L.ptr(u), L.ptr(sdf), L.ptr(rgb),
                                         L.stream_of(dev)))
    return rgb.cpu().numpy()


def _unfolded_rgb(m, x, v, n):
    _, f = m.implicit_surface.forward(x, return_h=True)
    return m.radiance_net.forward(x, v, n, f).cpu().numpy()


@pytest.fixture(scope='module')
def pair():
    """one model, 300 points inside the unit sphere with unit view dirs and normals, and their float64 rgb"""
    m = neus_model(wg.neus_state(seed=11), precision='f16x3')
    rs = np.random.RandomState(5)
    x = rs.randn(300, 3)
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * rs.uniform(0.05, 0.98, (300, 1)) ** (1 / 3)
    v = rs.randn(300, 3)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    n = rs.randn(300, 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    x, v, n = (torch.from_numpy(a.astype(np.float32)) for a in (x, v, n))
    with torch.no_grad():
        ref = _float64_rgb(m, x, v, n)
    return m, x.cuda(), v.cuda(), n.cuda(), ref


def _worst(a, ref):
    return float((np.abs(a.astype(np.float64) - ref) / (AT + RT * np.abs(ref))).max())


@pytest.mark.parametrize('P', SIZES)
def test_folded_pair_vs_float64(pair, P):
    m, x, v, n, ref = pair
    xs, vs, ns = (t[:P].contiguous() for t in (x, v, n))
    with torch.no_grad():
        fold = _worst(_folded_rgb(m, xs, vs, ns), ref[:P])
        plain = _worst(_unfolded_rgb(m, xs, vs, ns), ref[:P])
    print(f'P={P}: worst err / (atol + rtol |ref|): folded {fold:.4f}, unfolded {plain:.4f}')
    assert fold <= 1.0


def _rays64():
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'neus_b.npz'))
    return torch.from_numpy(g['rays_o'][:, :64]).cuda(), torch.from_numpy(g['rays_d'][:, :64]).cuda(), int(g['seed'])


def _render(m, ro, rd, **kw):
    from neurecon_amd.frameworks.neus import volume_render
    with torch.no_grad():
        return volume_render(ro, rd, m, batched=True, calc_normal=True, detailed_output=True, N_samples=64,
                             N_importance=64, **kw)


def test_fold_leaves_sampling_bit_identical():
    """config (b), 64 rays, detailed: everything ahead of the radiance net is bit-identical with and without
    the fold pack; radiance and rgb within twice the radiance bar of each other"""
    ro, rd, seed = _rays64()
    m = neus_model(wg.neus_state(seed=seed), precision='f16x3')
    assert m.radiance_net.nr_fold_packed(m.implicit_surface, ro.device) is not None
    rgb1, _, ex1 = _render(m, ro, rd)
    rgb0, _, ex0 = _render(m, ro, rd, fold_feature=False)
    for k in ('d_final', 'implicit_surface', 'implicit_nablas', 'alpha', 'visibility_weights'):
        assert torch.equal(ex1[k], ex0[k]), k
    for name, a, b in (('radiance', ex1['radiance'], ex0['radiance']), ('rgb', rgb1, rgb0)):
        a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        r = (np.abs(a - b) / (2 * (AT + RT * np.abs(b)))).max()
        print(f'{name}: folded vs unfolded worst err / (2 (atol + rtol |unfolded|)) = {r:.4f}')
        assert r <= 1.0, name


def test_fp32_mode_has_no_fold_pack():
    """the fp32 precision mode yields no fold pack and renders by the unfolded route either way"""
    from neurecon_amd import _lib as L
    ro, rd, seed = _rays64()
    m = neus_model(wg.neus_state(seed=seed), precision='fp32')
    assert m.radiance_net.nr_fold_packed(m.implicit_surface, ro.device) is None
    sdesc, rdesc = m.implicit_surface.nr_desc(), m.radiance_net.nr_desc()
    assert L.lib().nr_neus_fold_packed_bytes(ctypes.byref(sdesc), ctypes.byref(rdesc)) == 0
    rgb1, dep1, ex1 = _render(m, ro, rd)
    rgb0, dep0, ex0 = _render(m, ro, rd, fold_feature=False)
    assert torch.equal(rgb1, rgb0) and torch.equal(dep1, dep0)
    for k in ('radiance', 'implicit_surface', 'implicit_nablas', 'visibility_weights'):
        assert torch.equal(ex1[k], ex0[k]), k
