"""CPU: pins tests/reintegrate_ref.py and the ray sets of tests/test_gpu_reintegrate.py before any GPU run.

1. In fp32 each `integrate` reproduces its oracle's `render` bit for bit on the oracle's own depths.
2. Conditioning of every ray set at the oracle's depths: the fp32 reference stays within 0.25 x the bar
   of its float64 self (same lines, same inputs) on all but 2 % of the rays for rgb / mask / normals,
   and for depth among the rays with acc >= 1e-3.  These caps are conditions on the inputs.
3. Each full set holds empty rays (acc < 1e-3) and opaque ones (acc > 0.99) where its model can produce
   them (reintegrate_ref.EXTREMES names the sets that cannot, and why).
"""
import numpy as np
import pytest
import torch

import reintegrate_ref as rr
from oracle import rays as orays
from oracle.neus import NeuSOracle
from oracle.unisurf import UNISURFOracle
from oracle.volsdf import VolSDFOracle

KEYS = ('rgb', 'depth_volume', 'mask_volume', 'normals_volume')


@pytest.fixture(scope='module', autouse=True)
def _threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, prev)))
    yield
    torch.set_num_threads(prev)


def _check_set(tag, ref32, ref64):
    """the conditioning caps, on all rays and on each small set's rows"""
    cond = rr.conditioning(ref32, ref64)
    acc = cond['acc']
    print(f'\n[{tag}] rays {acc.size}: acc < 1e-3 on {(acc < 1e-3).sum()}, acc > 0.99 on {(acc > 0.99).sum()}')
    for name, _ in rr.OUTPUTS:
        c = cond[name]
        print(f'[{tag}] {name}: max E_ray {c["E"][c["judged"]].max() if c["judged"].any() else 0:.3e}, ill conditioned '
              f'{(~c["well"] & c["judged"]).sum()} of {c["judged"].sum()} judged')
        assert c['ill_share'] <= rr.ILL_CAP, (tag, name, c['ill_share'])
        for R, rows_ in rr.SMALL_SETS.items():  # rendered on their own: 2 % of 1 or 3 rays is no ray
            assert not (~c['well'] & c['judged'])[rows_].any(), (tag, name, R)
    fw, case = tag.split(' ')
    ends = rr.EXTREMES[fw][case]
    assert 'lo' not in ends or (acc < 1e-3).any(), tag
    assert 'hi' not in ends or (acc > 0.99).any(), tag
    return cond


@pytest.mark.parametrize('name', list(rr.NEUS_CASES))
def test_neus_integrate_pins_render_and_conditioning(name):
    cam, sd, kw = rr.neus_case(name)
    ro, rd = rr.camera_rays(cam)
    with torch.no_grad():
        ref = NeuSOracle(sd, use_outside_nerf=kw['N_outside'] > 0).render(ro, rd, **kw)
    S = kw['N_samples'] + kw['N_importance']
    o, d = rr.prepare_rays(ro, rd)
    near, far = orays.near_far_from_sphere(o, d)
    skw = {k: v for k, v in kw.items() if k not in ('N_outside', 'white_bkgd')}
    with torch.no_grad():
        d_all = NeuSOracle(sd).sample_depths(o, d, near, far, **skw)
    assert d_all.shape[-1] == S
    ikw = dict(N_outside=kw['N_outside'], white_bkgd=kw['white_bkgd'])
    r32 = rr.neus_integrate(sd, o, d, d_all, torch.float32, **ikw)
    for k in KEYS + ('d_final', 'visibility_weights', 'radiance'):
        assert torch.equal(r32[k], ref[k]), (name, k, float((r32[k] - ref[k]).abs().max()))
    r64 = rr.neus_integrate(sd, o, d, d_all, torch.float64, **ikw)
    assert r64['rgb'].dtype == torch.float64 and r64['implicit_surface'].dtype == torch.float64
    _check_set(f'neus {name}', r32, r64)


@pytest.mark.parametrize('name', list(rr.VOLSDF_CASES))
def test_volsdf_integrate_pins_render_and_conditioning(name):
    cam, sd, beta, nerfpp = rr.volsdf_case(name)
    ro, rd = rr.camera_rays(cam)
    with torch.no_grad():
        ref = VolSDFOracle(sd, use_nerfplusplus=nerfpp).render(ro, rd, near=0.0, far=6.0, N_samples=64,
                                                               N_importance=64, max_upsample_steps=6, N_outside=32)
    o, d = rr.prepare_rays(ro, rd)
    d_all = ref['d_vals'][..., :128]
    ikw = dict(use_nerfplusplus=nerfpp, N_outside=32)
    r32 = rr.volsdf_integrate(sd, o, d, d_all, torch.float32, **ikw)
    for k in KEYS + ('d_vals', 'visibility_weights', 'radiance', 'sigma'):
        assert torch.equal(r32[k], ref[k]), (name, k, float((r32[k] - ref[k]).abs().max()))
    r64 = rr.volsdf_integrate(sd, o, d, d_all, torch.float64, **ikw)
    assert r64['rgb'].dtype == torch.float64 and r64['sigma'].dtype == torch.float64
    _check_set(f'volsdf {name}', r32, r64)


@pytest.mark.parametrize('name', list(rr.UNISURF_CASES))
def test_unisurf_integrate_pins_render_and_conditioning(name):
    import weightgen as wg
    sd = wg.unisurf_state(seed=3)
    ro, rd = rr.camera_rays('e')
    c = rr.UNISURF_CASES[name]
    o, d = rr.prepare_rays(ro, rd)
    with torch.no_grad():  # the oracle renders one ray chunk; the chunks of the render loop one by one
        refs = [UNISURFOracle(sd).render(ro[:, i:i + c['rayschunk']], rd[:, i:i + c['rayschunk']], logit_tau=0.0,
                                         netchunk=c['netchunk']) for i in range(0, rr.R_FULL, c['rayschunk'])]
    ref = {k: torch.cat([r[k] for r in refs], 1) for k in KEYS + ('d_all', 'visibility_weights', 'radiance')}
    r32 = rr.unisurf_integrate(sd, o, d, ref['d_all'], torch.float32, **c)
    for k in ref:
        assert torch.equal(r32[k], ref[k]), (name, k, float((r32[k] - ref[k]).abs().max()))
    r64 = rr.unisurf_integrate(sd, o, d, ref['d_all'], torch.float64, **c)
    assert r64['rgb'].dtype == torch.float64
    _check_set(f'unisurf {name}', r32, r64)
    # the small sets render on their own: their points are one normalisation window
    for R, rows in rr.SMALL_SETS.items():
        s32 = rr.unisurf_integrate(sd, o[:, rows], d[:, rows], ref['d_all'][:, rows], torch.float32, **c)
        s64 = rr.unisurf_integrate(sd, o[:, rows], d[:, rows], ref['d_all'][:, rows], torch.float64, **c)
        cond = rr.conditioning(s32, s64)
        for nm, _ in rr.OUTPUTS:
            assert not (~cond[nm]['well'] & cond[nm]['judged']).any(), (name, R, nm)


def test_three_windows_case_has_three_windows_per_chunk():
    c = rr.UNISURF_CASES['three_windows']
    pts = c['rayschunk'] * (64 + 32)
    assert pts == 3 * c['netchunk']
    assert [min(c['rayschunk'], rr.R_FULL - i) for i in range(0, rr.R_FULL, c['rayschunk'])] == [64, 64, 2]
