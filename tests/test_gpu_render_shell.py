"""The Python shell around the three render calls: for tiny inputs, the exact `extras` key order,
shapes and dtypes of volume_render in render mode (no grad) and training mode (grad), written out
here literally from the frameworks' documented returns, and that (rgb, depth) are the dict's own
entries.  Also: a VolSDF render takes its workspace from the stream's shared buffer (_lib.workspace)."""
import ctypes
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as F

import render_host_cases as C
import weightgen as wg
from helpers import neus_model, unisurf_model, volsdf_model
from neurecon_amd import _lib as L

pytestmark = pytest.mark.gpu

f32, boolean = torch.float32, torch.bool
S_NEUS = 8 + 2 * (8 // 2)  # N_samples + N_upsample_iters * (N_importance // N_upsample_iters)
S_VOL = 8 + 8              # N_samples + N_importance
P_UNI = 8 + 4              # N_query + N_freespace
N_OUT = 4

HEAD = [('rgb', (3,), f32), ('depth_volume', (), f32), ('mask_volume', (), f32)]
NORMALS = [('normals_volume', (3,), f32)]


def neus_table(detailed, calc_normal, nerfpp, grad):
    S, M = S_NEUS, S_NEUS - 1 + (N_OUT if nerfpp else 0)
    t = HEAD + (NORMALS if calc_normal else [])
    if detailed:
        # training returns the surface net's colours at the S-1 mid-points, render mode all M merged samples
        t = t + [('implicit_nablas', (S, 3), f32), ('implicit_surface', (S,), f32),
                 ('radiance', (S - 1 if grad else M, 3), f32), ('alpha', (M,), f32), ('cdf', (S,), f32),
                 ('visibility_weights', (M,), f32), ('d_final', (M,), f32)]
        if nerfpp:
            t = t + [('sigma_out', (M,), f32), ('radiance_out', (M, 3), f32)]
    return t


def volsdf_table(detailed, calc_normal, nerfpp, grad):
    S, No = S_VOL, N_OUT if nerfpp else 0
    M = S + No
    t = HEAD + (NORMALS if calc_normal else [])
    if detailed:
        t = t + [('implicit_surface', (S,), f32), ('implicit_nablas', (S, 3), f32), ('radiance', (M, 3), f32),
                 ('alpha', (M - 1,), f32), ('p_i', (M - 1,), f32), ('visibility_weights', (M - 1,), f32),
                 ('d_vals', (M,), f32), ('sigma', (M,), f32), ('beta_map', (1,), f32), ('iter_usage', (), f32)]
        if nerfpp:
            t = t + [('sigma_out', (No,), f32), ('radiance_out', (No, 3), f32)]
    return t


def unisurf_table(detailed, calc_normal, nerfpp, grad):
    P = P_UNI
    t = HEAD + (NORMALS if calc_normal else [])
    if detailed:
        t = t + [('surface_points', (3,), f32), ('mask_surface', (), boolean), ('depth_surface', (), f32),
                 ('radiance', (P, 3), f32), ('implicit_surface', (P,), f32), ('implicit_nablas', (P, 3), f32),
                 ('alpha', (P,), f32), ('visibility_weights', (P,), f32)]
        if grad:  # training also returns the sample depths
            t = t + [('d_all', (P,), f32)]
    return t


@lru_cache(maxsize=None)
def _model(fw, nerfpp):
    if fw == 'neus':
        return neus_model(wg.neus_state(seed=1, use_outside_nerf=nerfpp), use_outside_nerf=nerfpp, precision='f16x3')
    if fw == 'volsdf':
        return volsdf_model(wg.volsdf_state(seed=3, beta_init=0.1, use_nerfplusplus=nerfpp), 0.1, precision='f16x3',
                            use_nerfplusplus=nerfpp)
    return unisurf_model(wg.unisurf_state(seed=3), precision='f16x3')


def _render(fw, rays_o, rays_d, batched, detailed, calc_normal, nerfpp):
    kw = dict(batched=batched, detailed_output=detailed, calc_normal=calc_normal)
    if fw == 'neus':
        from neurecon_amd.frameworks.neus import volume_render
        kw.update(N_samples=8, N_importance=8, N_upsample_iters=2, N_outside=N_OUT if nerfpp else 0)
    elif fw == 'volsdf':
        from neurecon_amd.frameworks.volsdf import volume_render
        kw.update(N_samples=8, N_importance=8, max_upsample_steps=2, use_nerfplusplus=nerfpp, N_outside=N_OUT,
                  obj_bounding_radius=3.0)
    else:
        from neurecon_amd.frameworks.unisurf import volume_render
        kw.update(N_query=8, N_freespace=4)
    return volume_render(rays_o, rays_d, _model(fw, nerfpp), **kw)


def _rays(shape, r):
    g = torch.Generator().manual_seed(3)
    o = F.normalize(torch.randn(*shape, 3, generator=g), dim=-1) * r
    d = 1.7 * F.normalize(0.3 * torch.randn(*shape, 3, generator=g) - o, dim=-1)  # not normalised on purpose
    return o.cuda(), d.cuda()


TABLES = {'neus': neus_table, 'volsdf': volsdf_table, 'unisurf': unisurf_table}
CASES = [(fw, nerfpp) for fw in TABLES for nerfpp in ((False, True) if fw != 'unisurf' else (False,))]


@pytest.mark.parametrize('grad', [False, True], ids=['nograd', 'grad'])
@pytest.mark.parametrize('calc_normal', [False, True], ids=['', 'normals'])
@pytest.mark.parametrize('detailed', [False, True], ids=['maps', 'detailed'])
@pytest.mark.parametrize('batched', [False, True], ids=['37', '2x24'])
@pytest.mark.parametrize('fw,nerfpp', CASES, ids=[f + ('-nerfpp' if n else '') for f, n in CASES])
def test_extras_keys_shapes_dtypes(fw, nerfpp, batched, detailed, calc_normal, grad):
    prefix = (2, 24) if batched else (37,)
    o, d = _rays(prefix, 2.0 if fw == 'volsdf' else 2.5)
    with torch.enable_grad() if grad else torch.no_grad():
        rgb, depth, ex = _render(fw, o, d, batched, detailed, calc_normal, nerfpp)
    torch.cuda.synchronize()
    want = TABLES[fw](detailed, calc_normal, nerfpp, grad)
    got = [(k, tuple(v.shape), v.dtype) for k, v in ex.items()]
    assert got == [(k, prefix + shape, dt) for k, shape, dt in want]
    assert ex['rgb'] is rgb and ex['depth_volume'] is depth
    assert rgb.requires_grad == grad
    assert all(v.is_cuda for v in ex.values())
    assert torch.isfinite(rgb).all() and torch.isfinite(depth).all()


@pytest.mark.parametrize('nerfpp', [False, True], ids=['builtin', 'nerfpp'])
def test_volsdf_render_uses_the_shared_workspace(nerfpp):
    """the render's scratch is the stream's grow-only buffer of _lib.workspace, as for NeuS and UNISURF"""
    o, d = _rays((37,), 2.0)
    L._WS.clear()
    with torch.no_grad():
        _render('volsdf', o, d, False, True, True, nerfpp)
    a = C.volsdf_args(n_rays=37, N_outside=N_OUT if nerfpp else 0, max_upsample_steps=2)
    a.N_samples = a.N_importance = 8
    ws_bytes = L.lib().nr_volsdf_workspace_bytes(ctypes.byref(a))
    assert ws_bytes > 0
    buf = L._WS.get((str(o.device), torch.cuda.current_stream(o.device).cuda_stream))
    assert buf is not None and buf.numel() >= ws_bytes
