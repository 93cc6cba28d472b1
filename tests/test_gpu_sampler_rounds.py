"""GPU: the NeuS and VolSDF samplers held to float64, round by round, on every sample of every ray.

The kernels that decide where the samples go (neus_upsample<1|4>, neus_direct_upsample, neus_merge,
sample_pdf_ray*, volsdf_first / vs_decide / vs_finalize) are checked forwards (tests/sampler_ref.py): the
inputs of a round are the GPU's own -- the sorted depths and the SDF values it read -- the round's CDF is
rebuilt from them in float64 on the host, and evaluated at every depth the GPU emitted it has to return
the uniform that depth was drawn for.  No MLP runs on the host, no ray is excused, no pass rate.

NeuS, the ladder: a render with N_upsample_iters = k, N_importance = 16 k runs exactly the first k rounds
of the shipped 4 x 16 configuration (16 new samples per round, inverse std 64 2^it), so the renders
k = 0..4 give the state (D_k, S_k) after every round: D_k from neus._sample_depths, S_k from the render's
implicit_surface (the sv the sampler read, carried through the merges; tied to D_k by the stored mid
depths).  The library takes k = 0 as it is.  For k = 1..4, per ray: (D_{k-1}, S_{k-1}) is contained in
(D_k, S_k) as a multiset of pairs bit for bit (neus_merge's pairing; a k-round render is the start of a
(k+1)-round one), exactly 16 depths are new, D_k is sorted and finite, and the 16 new depths pass the
forward check at tol = 1e-5 + K 2^-24 L / total64 with K = sampler_ref.K_GPU.  Perturbed: one fixed block
U[4][n][16] goes through rend_util.uniform, rung k receiving the first k blocks in its sample pass and in
its render, chunk by chunk as the library draws them.

VolSDF, the first sampling pass (max_upsample_steps = 0): from d_init (numpy fp32), the GPU's SDF there and
the background sphere's min restated in fp32, every ray's decision (iter_usage, beta_map) outside the
delta band and every ray's fine samples (d_vals minus the bit-exact coarse lerp) against the float64
opacity CDF.  Later VolSDF rounds keep their lists in the workspace and are not held here.

Worst figures are printed per case: residual / tol and the ray it occurred on.
"""
import numpy as np
import pytest
import torch

import reintegrate_ref as rr
import sampler_ref as sr
import weightgen as wg
from helpers import neus_model, volsdf_model

pytestmark = pytest.mark.gpu
CHUNKED = dict(rayschunk=64, max_workspace_gb=4)  # chunks of 64, 64 and 2 rays: a non-zero ray0, a partial wave


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


def _np(t):
    return t.detach().cpu().numpy()


class Draws:
    """stand-in for rend_util.uniform: hands out the given blocks in order, shape-checked"""

    def __init__(self, blocks):
        self.blocks = list(blocks)

    def __call__(self, shape, device=None):
        assert self.blocks, 'more draws than expected'
        u = self.blocks.pop(0)
        assert tuple(u.shape) == tuple(shape), (tuple(u.shape), tuple(shape))
        return u.to(device if device is not None else 'cpu')


def _neus_draws(U, k, n, rayschunk, direct=False):
    """the library draws per ray chunk: k blocks [1, nc, 16] each (direct: one [1, nc, N_importance])"""
    out = []
    for r0 in range(0, n, rayschunk):
        out += [U[r0:r0 + rayschunk][None]] if direct else [U[i, r0:r0 + rayschunk][None] for i in range(k)]
    return Draws(out)


class NeusRig:
    """renders and sample passes of one model on one ray set, with the uniforms replayed"""

    def __init__(self, m, og, dg, monkeypatch):
        self.m, self.og, self.dg, self.mp = m, og, dg, monkeypatch
        self.n = og.shape[1]

    def _patch(self, U, k, rayschunk, direct):
        from neurecon_amd import rend_util
        if U is not None:
            self.mp.setattr(rend_util, 'uniform', _neus_draws(U, k, self.n, rayschunk, direct))

    def _done(self, U):
        from neurecon_amd import rend_util
        assert U is None or not rend_util.uniform.blocks, 'fewer draws than expected'

    def render(self, kw, U=None, k=0, **chunk):
        from neurecon_amd.frameworks import neus
        self._patch(U, k, chunk.get('rayschunk', 65536), kw['upsample_algo'] != 'official_solution')
        with torch.no_grad():
            ex = neus.volume_render(self.og, self.dg, self.m, obj_bounding_radius=1.0, batched=True, calc_normal=True,
                                    perturb=U is not None, detailed_output=True, N_outside=0, **kw, **chunk)[2]
        self._done(U)
        return ex

    def depths(self, kw, U=None, k=0, rayschunk=65536):
        from neurecon_amd.frameworks import neus
        self._patch(U, k, rayschunk, kw['upsample_algo'] != 'official_solution')
        with torch.no_grad():
            d_all, _ = neus._sample_depths(self.og.reshape(-1, 3).contiguous(), self.dg.reshape(-1, 3).contiguous(),
                                           self.m, self.og.device, 1.0, True, 1, rayschunk, None, None, U is not None,
                                           1 / 64., kw['N_samples'], kw['N_importance'], kw['upsample_algo'],
                                           kw.get('N_nograd_samples', 2048), kw.get('N_upsample_iters', 4), 0)
        self._done(U)
        return d_all

    def state(self, kw, U=None, k=0):
        """(D, S) [n, S] numpy fp32 of a configuration: chunked and whole bit-identical, the render's depths
        (its mid depths) those of the sample pass"""
        ex = self.render(kw, U, k, **CHUNKED)
        whole = self.render(kw, U, k)
        for key in ex:
            if torch.is_tensor(ex[key]):
                assert torch.equal(ex[key], whole[key]), ('chunked vs whole', key)
        D = self.depths(kw, U, k, 64)
        assert torch.equal(D, self.depths(kw, U, k)), 'sample pass: chunked vs whole'
        D = _np(D)
        S = _np(ex['implicit_surface'])[0]
        assert D.shape == S.shape and D.dtype == np.float32 and S.dtype == np.float32
        mid = (np.float32(0.5) * (D[:, 1:] + D[:, :-1])).astype(np.float32)
        assert np.array_equal(_np(ex['d_final'])[0], mid), 'the render and the sample pass differ in their depths'
        return D, S, ex


def _rung(k, N_coarse=sr.N_COARSE):
    return dict(upsample_algo='official_solution', N_samples=N_coarse, N_importance=sr.N_UP * k, N_upsample_iters=k)


def _ladder(tag, rig, U, N_coarse=sr.N_COARSE, small=True):
    """the states k = 0..4 and the prefix and forward checks between them; returns the states and the
    float64 total of the first round"""
    n = rig.n
    states, worst, total0 = [], [], None
    for k in range(sr.N_ROUNDS + 1):
        D, S, ex = rig.state(_rung(k, N_coarse), U, k)
        assert D.shape == (n, N_coarse + sr.N_UP * k)
        if small:  # 1 and 3 rays on their own: the rows of the full set, bit for bit
            for R, rows in rr.SMALL_SETS.items():
                sub = NeusRig(rig.m, rig.og[:, rows].contiguous(), rig.dg[:, rows].contiguous(), rig.mp)
                part = sub.render(_rung(k, N_coarse), None if U is None else U[:, rows], k)
                for key in part:
                    if torch.is_tensor(part[key]):
                        assert torch.equal(ex[key][:, rows], part[key]), (tag, f'R={R}', k, key)
        states.append((D, S))
        if k == 0:
            continue
        Dp, Sp = states[k - 1]
        u = sr.det_u(sr.N_UP) if U is None else U[k - 1]
        res, total = sr.neus_round_check(Dp, Sp, D, S, k - 1, u)
        total0 = total if k == 1 else total0
        w, r = sr.worst(res, sr.neus_tol(Dp.shape[-1], total, sr.K_GPU))
        kk = float(sr.neus_k_ratio(res, Dp.shape[-1], total).max())
        print(f'SAMPLER [{tag}] round {k}: worst residual / tol {w:.3f} on ray {r} (K needed {kk:+.3f} of {sr.K_GPU})')
        worst.append((w, k, r))
    assert all(w <= 1.0 for w, _, _ in worst), (tag, 'forward check: (residual / tol, round, ray)', worst)  # NaN misses
    return states, total0


def _neus_setup(precision, monkeypatch, rows=None):
    ro, rd = rr.camera_rays(sr.NEUS_CAM)
    if rows is not None:
        ro, rd = ro[:, rows].contiguous(), rd[:, rows].contiguous()
    m = neus_model(wg.neus_state(seed=sr.NEUS_SEED), precision=precision)
    return NeusRig(m, ro.cuda(), rd.cuda(), monkeypatch)


def _U(mode, rows=None):
    if mode == 'det':
        return None
    U = sr.uniform_block(sr.U_SEED, sr.N_ROUNDS, rr.R_FULL, sr.N_UP)
    return U if rows is None else U[:, rows].contiguous()


@pytest.mark.parametrize('mode', ['det', 'rand'])
@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_neus_ladder(precision, mode, monkeypatch):
    """130 rays in chunks of 64, 64 and 2; 1 and 3 rays; every round of every ray"""
    tag = f'neus ladder {precision} {mode}'
    rig = _neus_setup(precision, monkeypatch)
    states, total0 = _ladder(tag, rig, _U(mode))
    # the set holds rays that hit and rays that miss (sum w of the first round, from its float64 total)
    sw = total0 - (sr.N_COARSE - 1) * 1e-5
    print(f'SAMPLER [{tag}] sum w: {int((sw > 0.5).sum())} rays > 0.5, {int((sw < 1e-3).sum())} rays < 1e-3')
    assert (sw > 0.5).sum() >= 10 and (sw < 1e-3).sum() >= 10


LDS_ROWS = [0, 40, 65, 90, 129]


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
@pytest.mark.parametrize('N_coarse', [755, 756])
def test_neus_ladder_at_the_lds_boundary(N_coarse, precision, monkeypatch):
    """Five rays, 4 rounds of 16.  The upsampling kernel stages 5 S + 1 floats per ray: with S = 819 samples
    (N_samples 755) four rays take exactly 65536 bytes and neus_upsample<4> still runs; with S = 820
    (N_samples 756) it is neus_upsample<1>.  (The staging is sized by the configuration's final S, so only
    rung 4 of each ladder sits on the boundary; the lower rungs supply its inputs.)"""
    for mode in ('det', 'rand'):
        rig = _neus_setup(precision, monkeypatch, LDS_ROWS)
        _ladder(f'neus lds N_samples={N_coarse} {precision} {mode}', rig, _U(mode, LDS_ROWS), N_coarse, small=False)


def _directions(dg):
    """the library's normalised directions [n, 3] (nr_normalize3, as the renders normalise them)"""
    from neurecon_amd import _lib as L
    rd_raw = dg.reshape(-1, 3).contiguous()
    rd = torch.empty_like(rd_raw)
    L.check(L.lib().nr_normalize3(L.ptr(rd_raw), rd_raw.shape[0], L.ptr(rd), L.stream_of(rd_raw.device)))
    return _np(rd)


def _gpu_sdf(surface, og, dg, depths):
    """the GPU's SDF [n, L] at the fp32 points o + d * dir of the depths [n, L]"""
    pts = sr.points32(_np(og)[0], _directions(dg), depths)
    with torch.no_grad():
        return _np(surface.forward(torch.from_numpy(pts).cuda())), pts


def _direct_check(tag, bins, sdf, D, D_coarse, u):
    assert np.isfinite(D).all() and (np.diff(D, axis=-1) >= 0).all(), tag
    new = sr.multiset_split(D, D_coarse)
    cdf, total = sr.pdf_cdf(sr.neus_direct_weights(sdf, 64.0))
    res = sr.forward_residual(bins, cdf, new, u)
    L = bins.shape[-1]
    w, r = sr.worst(res, sr.neus_tol(L, total, sr.K_GPU))
    kk = float(sr.neus_k_ratio(res, L, total.numpy()).max())
    print(f'SAMPLER [{tag}]: worst residual / tol {w:.3f} on ray {r} (K needed {kk:+.3f} of {sr.K_GPU})')
    assert w <= 1.0, (tag, w, r)


@pytest.mark.parametrize('mode', ['det', 'rand'])
@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_neus_direct(precision, mode, monkeypatch):
    """direct_use: one round on the ladder's k = 0 state at s = 64, the 64 new depths are D minus D_0.
    direct_more: the bins are the fp32 lerp of linspace(N_nograd_samples) between the coarse list's ends,
    their SDF the GPU's own at the fp32 points o + d * dir; 256 bins, and 2048 once (fp32, det)."""
    rig = _neus_setup(precision, monkeypatch)
    n = rig.n
    D0, S0, _ = rig.state(_rung(0))
    U = None if mode == 'det' else sr.uniform_block(sr.U_SEED + 1, n, 64)
    u = sr.det_u(64) if U is None else U
    kw = dict(upsample_algo='direct_use', N_samples=sr.N_COARSE, N_importance=64)
    D, _, _ = rig.state(kw, U)
    _direct_check(f'neus direct_use {precision} {mode}', D0, S0, D, D0, u)
    for N in (256, 2048) if (precision, mode) == ('fp32', 'det') else (256,):
        kw = dict(upsample_algo='direct_more', N_samples=sr.N_COARSE, N_importance=64, N_nograd_samples=N)
        D, _, _ = rig.state(kw, U)
        bins = sr.lerp32(D0[:, :1], D0[:, -1:], torch.linspace(0, 1, N).numpy()[None])
        sdf, _ = _gpu_sdf(rig.m.implicit_surface, rig.og, rig.dg, bins)
        _direct_check(f'neus direct_more {N} {precision} {mode}', bins, sdf, D, D0, u)


# ---------------------------------------------------------------------------------------------
# VolSDF: the first sampling pass
# ---------------------------------------------------------------------------------------------
def _norm3(p):
    """|x| as surface_sdf forms it in fp32: sqrt(fma(z, z, fma(y, y, x x)))"""
    x, y, z = (p[..., i].astype(np.float64) for i in range(3))
    s = (x * x).astype(np.float32).astype(np.float64)
    s = (y * y + s).astype(np.float32).astype(np.float64)
    return np.sqrt((z * z + s).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize('mode', ['det', 'rand'])
@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
@pytest.mark.parametrize('name', list(sr.VOLSDF_CASES))
def test_volsdf_first_pass(name, precision, mode, monkeypatch):
    from neurecon_amd import rend_util
    from neurecon_amd.frameworks import volsdf
    Ns, beta_init, nerfpp = sr.VOLSDF_CASES[name]
    tag = f'volsdf first pass {name} {precision} {mode}'
    N0, m_imp, No = 4 * Ns, sr.VOLSDF_N_IMPORTANCE, 32
    S = Ns + m_imp
    sd = wg.volsdf_state(seed=sr.VOLSDF_SEED, beta_init=beta_init, use_nerfplusplus=nerfpp)
    m = volsdf_model(sd, beta_init, precision=precision, use_nerfplusplus=nerfpp)
    ro, rd = rr.camera_rays(sr.VOLSDF_CAM)
    og, dg = ro.cuda(), rd.cuda()
    n = og.shape[1]
    U = None if mode == 'det' else sr.uniform_block(sr.U_SEED + 2, n, m_imp)
    U_out = sr.uniform_block(sr.U_SEED + 3, n, No)

    def render(rows=None):
        o_, d_ = (og, dg) if rows is None else (og[:, rows].contiguous(), dg[:, rows].contiguous())
        if U is not None:  # one [rays, N_importance] block, then the NeRF++ strata
            r_ = slice(None) if rows is None else rows
            monkeypatch.setattr(rend_util, 'uniform', Draws([U[r_]] + ([U_out[r_][None]] if nerfpp else [])))
        with torch.no_grad():
            ex = volsdf.volume_render(o_, d_, m, near=0.0, far=sr.VOLSDF_FAR, obj_bounding_radius=3.0, batched=True,
                                      calc_normal=True, detailed_output=True, perturb=U is not None, N_samples=Ns,
                                      N_importance=m_imp, N_outside=No, use_nerfplusplus=nerfpp, max_upsample_steps=0,
                                      epsilon=sr.VOLSDF_EPS)[2]
        assert U is None or not rend_util.uniform.blocks
        return ex
    ex = render()
    for R, rows in rr.SMALL_SETS.items():
        part = render(rows)
        for key in part:
            if torch.is_tensor(part[key]):
                assert torch.equal(ex[key][:, rows], part[key]), (tag, f'R={R}', key)

    d_all = _np(ex['d_vals'])[0, :, :S]
    assert np.isfinite(d_all).all() and (np.diff(d_all, axis=-1) >= 0).all(), tag
    zero = np.zeros((n, 1), np.float32)
    if nerfpp:  # the sphere exit per ray: the last coarse depth, which no fine sample exceeds
        from oracle import rays as orays
        far = d_all.max(-1, keepdims=True)
        o, d = rr.prepare_rays(ro, rd)
        far_ref = orays.sphere_intersection(o, d, r=3.0)[1][0].numpy()
        assert np.allclose(far, far_ref, rtol=1e-6, atol=0), (tag, 'far', float(np.abs(far - far_ref).max()))
    else:
        far = np.full((n, 1), sr.VOLSDF_FAR, np.float32)
    coarse = sr.lerp32(zero, far, torch.linspace(0, 1, Ns).numpy()[None])
    fine = sr.multiset_split(d_all, coarse)  # the coarse lerp is there bit for bit
    assert fine.shape == (n, m_imp)

    d_init = sr.lerp32(zero, far, torch.linspace(0, 1, N0).numpy()[None])
    sdf, pts = _gpu_sdf(m.implicit_surface, og, dg, d_init)
    if not nerfpp:  # VolSDF.forward_surface: min(sdf, r - |x|)
        sdf = np.minimum(sdf, (np.float32(3.0) - _norm3(pts)).astype(np.float32))
    with torch.no_grad():
        beta_net = torch.exp(m.ln_beta.detach().float().cpu() * m.speed_factor)
        alpha_net = 1. / beta_net
    info = sr.volsdf_first_check(d_init, sdf, float(alpha_net), float(beta_net), sr.volsdf_beta_plus(far, N0),
                                 _np(ex['iter_usage'])[0], _np(ex['beta_map'])[0], fine,
                                 sr.det_u(m_imp) if U is None else U, sr.DELTA_GPU, sr.SWITCH + sr.R_GPU)
    print(f'SAMPLER [{tag}]: converged {info["n_conv"]}, not {info["n_nonc"]}, in the band {info["band"] * 100:.1f} %; '
          f'worst residual / tol {info["worst"]:.4f} (residual {info["res"]:.3e}) on ray {info["ray"]}')
    assert info['band'] <= sr.BAND_CAP, (tag, info['band'])
    assert info['n_conv'] >= 1 and info['n_nonc'] >= 1, (tag, 'one branch only', info['n_conv'], info['n_nonc'])
