"""Lean weight stream of the f16x3 SDF render kernels: sdf4_kernel's reverse ops B7..B0 fetch only the
weight pieces of each chunk (op4's LEAN mode) and take their scalars -- 1 / weight scale and (R, B) -- from
the per-op tables of the pack's tail instead of the chunks' bias slots.

Lean instances: the reverse-only launches of the deferred sample nablas (sdf4_kernel<true, false, 2 / 4>)
and the nabla + feature launch (<true, true, 0>).  The fused nabla launch without the feature
(<true, false, 0>) keeps the slot path, so comparing the two bit for bit holds the table's values to the
slots'.  Every op's every chunk runs at any P.

The forward ops of the launches whose LDS holds the weight ring alone (forward only, narrow tiles, forward +
feature, the deferred sample launch) read bias, scalars and aux from a per-op bias table in LDS (op4's kTab
mode); the fused launches' forward halves keep the slot path.  One sdf across the four launch_sdf instances
therefore holds the table's values to the slots' too.

Config (b)'s architecture; every bias and the sdf row are randomised away from the geometric init, so a
bias, scale or aux entry read from the wrong chunk or op changes the result.

The float64 bars are tests/test_gpu_fold.py's: rtol 1e-5, atol 1e-6, against a CPU evaluation (autograd for
the nablas) from the model's effective fp32 weights."""
import math

import numpy as np
import pytest
import torch

import weightgen as wg
from helpers import neus_model

pytestmark = pytest.mark.gpu

RT, AT = 1e-5, 1e-6
# one lane, one wave, a wave boundary, one tile, a tile boundary, a ragged third tile
SIZES = (1, 16, 17, 128, 129, 300)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()  # must load: no fallback exists


def _randomised_state(seed):
    """wg.neus_state with every SDF-net bias redrawn (sigma 0.03: three times weightgen's, distinct per row)
    and the sdf row of the last layer scaled element-wise by U(0.5, 1.5)"""
    sd = wg.neus_state(seed=seed)
    rs = np.random.RandomState(1000 + seed)
    for l in range(9):
        k = f'implicit_surface.surface_fc_layers.{l}.bias'
        b = rs.normal(0.0, 0.03, size=tuple(sd[k].shape))
        if l == 8:
            b[0] = -0.5 + rs.normal(0.0, 0.05)
        sd[k] = torch.tensor(b, dtype=torch.float32)
    k = 'implicit_surface.surface_fc_layers.8.weight_v'
    v = sd[k].clone()
    v[0] *= torch.tensor(rs.uniform(0.5, 1.5, size=(v.shape[1],)), dtype=torch.float32)
    sd[k] = v
    return sd


def _float64_sdf_nabla(m, x):
    """points -> sdf and d sdf / d x in float64 on the CPU (base.py:243-282)"""
    from oracle.nets import embed, softplus100
    sl = [(l.effective_weight().detach().cpu().double(), l.bias.detach().cpu().double())
          for l in m.implicit_surface.surface_fc_layers]
    x = x.detach().cpu().double().requires_grad_(True)
    xe = embed(x, 6)
    h = xe
    for i in range(8):
        if i == 4:
            h = torch.cat([h, xe], -1) / math.sqrt(2)
        h = softplus100(h @ sl[i][0].T + sl[i][1])
    sdf = (h @ sl[8][0].T + sl[8][1])[:, 0]
    nab, = torch.autograd.grad(sdf.sum(), x)
    return sdf.detach().numpy(), nab.numpy()


@pytest.fixture(scope='module')
def net():
    """one model, 300 points inside the unit sphere, their float64 sdf and nablas"""
    m = neus_model(_randomised_state(seed=11), precision='f16x3')
    rs = np.random.RandomState(5)
    x = rs.randn(300, 3)
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * rs.uniform(0.05, 0.98, (300, 1)) ** (1 / 3)
    x = torch.from_numpy(x.astype(np.float32))
    sdf64, nab64 = _float64_sdf_nabla(m, x)
    return m, x.cuda(), sdf64, nab64


def _worst(a, ref):
    return float((np.abs(a.cpu().numpy().astype(np.float64) - ref) / (AT + RT * np.abs(ref))).max())


def _paths(m, xs):
    """sdf (and nablas) of the launch_sdf instances: forward only (narrow tiles at these sizes), forward +
    feature, fused nabla (slot-path reverse), nabla + feature (lean reverse)"""
    s = m.implicit_surface
    with torch.no_grad():
        fwd, _, _ = s._run(xs, nabla=False, feature=False)
        feat, _, _ = s._run(xs, nabla=False, feature=True)
        nab_sdf, nab, _ = s._run(xs, nabla=True, feature=False)
        nf_sdf, nf_nab, _ = s._run(xs, nabla=True, feature=True)
    torch.cuda.synchronize()
    return dict(fwd=fwd, feat=feat, nabla=nab_sdf, nabla_feat=nf_sdf), dict(nabla=nab, nabla_feat=nf_nab)


@pytest.mark.parametrize('P', SIZES)
def test_one_forward_value_across_paths(net, P):
    m, x, sdf64, _ = net
    sdf, _ = _paths(m, x[:P].contiguous())
    for k, v in sdf.items():
        assert torch.equal(v, sdf['fwd']), (k, float((v - sdf['fwd']).abs().max()))
    w = _worst(sdf['fwd'], sdf64[:P])
    print(f'P={P}: sdf worst err / (atol + rtol |ref|) = {w:.4f}')
    assert w <= 1.0


@pytest.mark.parametrize('P', SIZES)
def test_one_nabla_across_paths(net, P):
    """lean reverse pass (nabla + feature launch) against the slot-path reverse pass (fused nabla launch), bit
    for bit, and both against float64"""
    m, x, _, nab64 = net
    _, nab = _paths(m, x[:P].contiguous())
    assert torch.equal(nab['nabla_feat'], nab['nabla']), float((nab['nabla_feat'] - nab['nabla']).abs().max())
    for k, v in nab.items():
        w = _worst(v, nab64[:P])
        print(f'P={P}: {k} nablas worst err / (atol + rtol |ref|) = {w:.4f}')
        assert w <= 1.0, k


def test_wide_tiles_second_workgroup_iteration(net):
    """128 points per CU and 300 more: the forward-only launch leaves the narrow tiles for the 128-point ones,
    and some workgroups run a second tile, whose first op's table is fetched by the first tile's last op.
    sdf, nablas and feature equal across the instances, bit for bit."""
    m, x, _, _ = net
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    P = 128 * cus + 300
    rs = np.random.RandomState(9)
    xs = rs.randn(P, 3)
    xs = xs / np.linalg.norm(xs, axis=1, keepdims=True) * rs.uniform(0.05, 0.98, (P, 1)) ** (1 / 3)
    xs = torch.from_numpy(xs.astype(np.float32)).cuda()
    s = m.implicit_surface
    with torch.no_grad():
        fwd, _, _ = s._run(xs, nabla=False, feature=False)
        feat_sdf, _, feat = s._run(xs, nabla=False, feature=True)
        nab_sdf, nab, _ = s._run(xs, nabla=True, feature=False)
        nf_sdf, nf_nab, nf_feat = s._run(xs, nabla=True, feature=True)
    for k, v in (('feat', feat_sdf), ('nabla', nab_sdf), ('nabla_feat', nf_sdf)):
        assert torch.equal(v, fwd), (k, float((v - fwd).abs().max()))
    assert torch.equal(nf_nab, nab), float((nf_nab - nab).abs().max())
    assert torch.equal(nf_feat, feat), float((nf_feat - feat).abs().max())


def _rays64():
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'neus_b.npz'))
    return torch.from_numpy(g['rays_o'][:, :64]).cuda(), torch.from_numpy(g['rays_d'][:, :64]).cuda()


def _render(m, ro, rd, **kw):
    from neurecon_amd.frameworks.neus import volume_render
    with torch.no_grad():
        return volume_render(ro, rd, m, batched=True, calc_normal=True, N_samples=64, N_importance=64, **kw)


def test_render_detailed_bit_identical():
    """64 rays of config (b), detailed outputs, with and without defer_sample_nablas"""
    ro, rd = _rays64()
    m = neus_model(_randomised_state(seed=1), precision='f16x3')
    _, _, ex1 = _render(m, ro, rd, detailed_output=True, defer_sample_nablas=True)
    _, _, ex0 = _render(m, ro, rd, detailed_output=True, defer_sample_nablas=False)
    for k in ('implicit_surface', 'implicit_nablas', 'alpha', 'visibility_weights', 'd_final'):
        assert torch.equal(ex1[k], ex0[k]), k


def test_render_deferred_reverse_pass_bit_identical():
    """Detailed outputs ask for every sample's nabla, which switches the deferral off; the maps of the plain
    render are where the deferred samples' reverse-only launch (lean) meets the fused one (slot path)."""
    ro, rd = _rays64()
    m = neus_model(_randomised_state(seed=1), precision='f16x3')
    outs = []
    for defer in (True, False):
        rgb, depth, ex = _render(m, ro, rd, detailed_output=False, defer_sample_nablas=defer)
        outs.append((rgb, depth, ex['mask_volume'], ex['normals_volume']))
    for name, a, b in zip(('rgb', 'depth', 'mask', 'normals'), *outs):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert float(outs[0][3].abs().max()) > 0.0  # some sample's nabla reached the normal map
