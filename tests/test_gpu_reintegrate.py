"""GPU: every render re-integrated in float64 on the GPU's own sample depths.

The full-size render tests compare with the oracle end to end, through the samplers' discrete decisions,
and so end in a pass rate; rays whose samples moved are excused.  Here the sorted sample depths are
taken from the GPU, and tests/reintegrate_ref.py goes from those depths to the image in fp32 and in
float64 on the host.  No discrete decision is left in between, so EVERY ray is held:

a. rgb / depth / mask / normals meet the bar against float64 on every well-conditioned ray (the fp32
   reference within 0.25 x bar of its float64 self on that ray); the ill-conditioned share stays within
   2 % (asserted; depth judged where acc64 >= 1e-3).  The worst (|gpu - f64| - E_ray) / max|f64| is printed.
b. per-sample SDF / logits, nablas, radiance (and VolSDF's sigma) against float64 at the same points,
   for every sample of every ray: a value paired with the wrong depth after a merge or gather shows here.
c. structure, no tolerance: depths finite, sorted, S of them, every coarse depth present, NeuS mid
   depths = 0.5 (d[s] + d[s+1]) bit for bit, stored weights sum to the stored acc, the benchmarked call
   (detailed_output=False: zero-alpha skip, deferred nablas) and the chunked render bit-identical.

130 rays with rayschunk 64 (chunks of 64, 64 and 2: a non-zero ray0, a ragged last chunk, a partial
four-ray wave), and 1 and 3 rays on their own; fp32 and f16x3.  The coarse-depth check reads near back
as the first sample and searches far among the last ones (NeuS, VolSDF); UNISURF's interval and
free-space runs are rebuilt from near, the stored surface depth and a searched end each.

Last: sample_pdf against the oracle's, bit for bit, at its edges.
"""
import numpy as np
import pytest
import torch

import reintegrate_ref as rr
import weightgen as wg
from helpers import neus_model, report, unisurf_model, volsdf_model
from test_gpu_parity import NAB_AT, RT, _assert_bench_call_equal

pytestmark = pytest.mark.gpu
MAPS = ('rgb', 'depth_volume', 'mask_volume', 'normals_volume')


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, prev)))
    yield
    torch.set_num_threads(prev)


def _np(t):
    return t.detach().cpu().numpy()


def _assert_same(a, b, tag):
    """every tensor of two renders' extras bit for bit"""
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), (tag, k, float((a[k].float() - b[k].float()).abs().max()))


def _assert_rows(full, part, rows, tag):
    for k in part:
        if torch.is_tensor(part[k]):
            assert torch.equal(full[k][:, rows], part[k]), (tag, k)


def _structure(tag, d_all, S, w, acc, t_coarse=None):
    d = _np(d_all).reshape(-1, d_all.shape[-1])
    assert d.shape[-1] == S and d.dtype == np.float32, (tag, d.shape)
    assert np.isfinite(d).all(), tag
    assert (np.diff(d, axis=-1) >= 0).all(), tag
    if t_coarse is not None:  # near (1 - t) + far t with separately rounded fp32 ops
        t = t_coarse.numpy().astype(np.float32)[None, :]
        # near is the first sample (u = 0 inverts to the first bin edge exactly).  far is the last coarse
        # sample, but every det round's u = 1 inverts to far give or take an ulp, so far is one of the last
        # few samples: the one with which all coarse depths are present.  For far this is an existence
        # search, not a read-back: a ray passes if one of its last samples, taken as far, puts all the
        # coarse depths among its samples (a false pass would need every one of them to match bit for bit)
        near = d[:, :1]
        ok = np.zeros(d.shape[0], bool)
        for k in range(1, min(8, S) + 1):
            far = d[:, -k:][:, :1]
            coarse = (near * (np.float32(1) - t)).astype(np.float32) + (far * t).astype(np.float32)
            assert coarse.dtype == np.float32
            ok |= (coarse[:, :, None] == d[:, None, :]).any(-1).all(-1)
        assert ok.all(), (tag, 'coarse depths missing on rays', np.nonzero(~ok)[0].tolist())
    wsum = _np(w).astype(np.float64).reshape(d.shape[0], -1).sum(-1)
    err = np.abs(wsum - _np(acc).astype(np.float64).reshape(-1))
    assert (err <= 1e-6).all(), (tag, 'weights do not sum to acc', float(err.max()))


def _lerp32(a, b, t):
    """a (1 - t) + b t in numpy fp32 with separately rounded operations"""
    return (a * (np.float32(1) - t)).astype(np.float32) + (b * t).astype(np.float32)


def _unisurf_runs(tag, d_all, depth_surface, n_query=64, n_free=32, interval=1.0):
    """UNISURF's two runs, bit for bit.  near is the first sample (the free-space run starts on it and the
    interval run starts at d_lo >= near).  d_lo = max(depth_surface - interval, near) is formed exactly
    from the stored surface depth; d_up (the interval run's t = 1) and the free-space run's end (its
    t = 1) are samples of the ray, so each is searched among the ray's samples: an existence search --
    a ray passes if some sample, taken as the run's end, puts every depth of the run among its samples."""
    d = _np(d_all).reshape(-1, d_all.shape[-1])
    near = d[:, :1]
    dc = _np(depth_surface).reshape(-1, 1).astype(np.float32)
    d_lo = np.maximum((dc - np.float32(interval)).astype(np.float32), near)
    for name, start, n in (('interval', d_lo, n_query), ('free-space', near, n_free)):
        t = torch.linspace(0.0, 1.0, n).numpy().astype(np.float32)[None, :]
        ok = np.zeros(d.shape[0], bool)
        for k in range(d.shape[1]):
            end = d[:, k:k + 1]
            run = _lerp32(start, end, t)
            # a run ends above its start (interval > 0; the free-space run ends at or above the too-close
            # threshold): a candidate equal to the start would collapse the run onto one sample
            ok |= (run[:, :, None] == d[:, None, :]).any(-1).all(-1) & (end > start)[:, 0]
        assert ok.all(), (tag, name + ' run: depths missing on rays', np.nonzero(~ok)[0].tolist())


def _bar(tag, got, r32, r64, cap=True):
    """check a: bar on every well-conditioned ray, ill-conditioned share within the cap"""
    for k in MAPS:  # empty rays included: depth's 1e-10 keeps 0 / acc finite
        assert torch.isfinite(got[k]).all(), (tag, k, 'not finite')
    cond = rr.conditioning(r32, r64)
    res = rr.bar_excess({k: got[k] for k in MAPS}, r64, cond)
    line = []
    for name, _ in rr.OUTPUTS:
        c = cond[name]
        n_ill = int((~c['well'] & c['judged']).sum())
        line.append(f'{name} excess {res[name]["excess"]:+.2e} ill {n_ill}/{int(c["judged"].sum())}')
    print(f'EXCESS [{tag}] ' + '; '.join(line))
    for name, _ in rr.OUTPUTS:
        c = cond[name]
        n_ill, n = int((~c['well'] & c['judged']).sum()), int(c['judged'].sum())
        assert n_ill <= int(rr.ILL_CAP * n), (tag, name, 'ill-conditioned share', n_ill, n)
        miss = res[name]['miss']
        assert not miss.any(), (tag, name, 'rays off the bar', np.nonzero(miss)[0].tolist(), res[name]['worst_err'])


# ---------------------------------------------------------------------------------------------
# NeuS
# ---------------------------------------------------------------------------------------------
def _neus_calls(m, kw):
    from neurecon_amd.frameworks import neus

    def render(o, d, detailed, **extra):
        with torch.no_grad():
            return neus.volume_render(o, d, m, obj_bounding_radius=1.0, batched=True, calc_normal=True, perturb=False,
                                      detailed_output=detailed, **kw, **extra)

    def depths(o, d, rayschunk):
        with torch.no_grad():
            d_all, _ = neus._sample_depths(o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), m, o.device,
                                           1.0, True, 1, rayschunk, None, None, False, 1 / 64., kw['N_samples'],
                                           kw['N_importance'], kw['upsample_algo'], kw.get('N_nograd_samples', 2048),
                                           kw.get('N_upsample_iters', 4), kw['N_outside'])
        return d_all
    return render, depths


def _train_points(tag, og, dg, d_all, mid):
    """the training step takes these same depths (_sample_depths) and forms its sample points, mid-points
    and mid depths with nr_neus_points: o + d t and 0.5 (d[s] + d[s+1]) in numpy fp32, bit for bit"""
    from neurecon_amd import _lib as L
    n, S = d_all.shape[1], d_all.shape[2]
    ro = og.reshape(-1, 3).contiguous()
    rd = torch.empty_like(ro)
    st = L.stream_of(ro.device)
    L.check(L.lib().nr_normalize3(L.ptr(dg.reshape(-1, 3).contiguous()), n, L.ptr(rd), st))
    da = d_all.reshape(n, S).contiguous()
    pts, mids = torch.empty(n, S, 3, device=ro.device), torch.empty(n, S - 1, 3, device=ro.device)
    dmid = torch.empty(n, S - 1, device=ro.device)
    L.check(L.lib().nr_neus_points(L.ptr(ro), L.ptr(rd), L.ptr(da), n, S, L.ptr(pts), L.ptr(mids), L.ptr(dmid), st))
    o_, d_ = _np(ro)[:, None, :], _np(rd)[:, None, :]
    assert np.array_equal(_np(dmid), mid), tag
    for name, got, t in (('points', pts, _np(da)), ('mid-points', mids, mid)):
        want = o_ + (d_ * t[:, :, None]).astype(np.float32)
        assert want.dtype == np.float32 and np.array_equal(_np(got), want), (tag, 'training ' + name)


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
@pytest.mark.parametrize('name', list(rr.NEUS_CASES))
def test_neus_reintegrated(name, precision):
    cam, sd, kw = rr.neus_case(name)
    tag = f'neus {name} {precision}'
    ro, rd = rr.camera_rays(cam)
    og, dg = ro.cuda(), rd.cuda()
    nerf = kw['N_outside'] > 0
    m = neus_model(sd, use_outside_nerf=nerf, precision=precision)
    render, depths = _neus_calls(m, kw)
    S = kw['N_samples'] + kw['N_importance']
    # rayschunk is honoured exactly once a workspace budget is set: chunks of 64, 64 and 2 rays
    chunked = dict(rayschunk=64, max_workspace_gb=4)
    det = render(og, dg, True, **chunked)
    _assert_bench_call_equal(det, render(og, dg, False, **chunked), tag)
    whole = render(og, dg, True)
    _assert_same(det[2], whole[2], tag + ' chunked vs whole')
    _assert_bench_call_equal(whole, render(og, dg, False), tag + ' whole')
    ex = det[2]
    d_all = depths(og, dg, 64)
    assert torch.equal(d_all, depths(og, dg, 65536)), tag
    d_all = d_all.reshape(1, rr.R_FULL, -1)

    # c. structure
    _structure(tag, d_all, S, ex['visibility_weights'], ex['mask_volume'], torch.linspace(0, 1, kw['N_samples']))
    dn = _np(d_all)[0]
    mid = (np.float32(0.5) * (dn[:, 1:] + dn[:, :-1])).astype(np.float32)
    assert np.array_equal(_np(ex['d_final'])[0, :, :S - 1], mid), tag
    for R, rows in rr.SMALL_SETS.items():
        o_s, d_s = og[:, rows].contiguous(), dg[:, rows].contiguous()
        part = render(o_s, d_s, True)
        _assert_rows(ex, part[2], rows, f'{tag} R={R}')
        _assert_bench_call_equal(part, render(o_s, d_s, False), f'{tag} R={R}')
    _train_points(tag, og, dg, d_all, mid)

    # a. + b. against float64 on the GPU's depths
    o, d = rr.prepare_rays(ro, rd)
    ikw = dict(N_outside=kw['N_outside'], white_bkgd=kw['white_bkgd'])
    r32 = rr.neus_integrate(sd, o, d, d_all.cpu(), torch.float32, **ikw)
    r64 = rr.neus_integrate(sd, o, d, d_all.cpu(), torch.float64, **ikw)
    _bar(tag, ex, r32, r64)
    assert report(f'{tag} sdf', ex['implicit_surface'], r64['implicit_surface'].numpy(), 1e-5, 1e-6)[0].all()
    assert report(f'{tag} nablas', ex['implicit_nablas'], r64['implicit_nablas'].numpy(), RT, NAB_AT)[0].all()
    # detailed_output=True evaluates every mid-point (the skip only runs when radiance is not asked for)
    assert report(f'{tag} radiance', ex['radiance'][..., :S - 1, :], r64['radiance'][..., :S - 1, :].numpy(), 1e-5,
                  1e-6)[0].all()
    if nerf:  # the background's tolerances are test_volsdf_nerfpp_vs_golden's
        assert report(f'{tag} d_out', ex['d_final'][..., S - 1:], r64['d_final'][..., S - 1:].numpy(), 1e-6, 1e-6)[0].all()
        assert report(f'{tag} sigma_out', ex['sigma_out'], r64['sigma_out'].numpy(), RT, 1e-5)[0].all()
        assert report(f'{tag} radiance_out', ex['radiance_out'], r64['radiance_out'].numpy(), RT, 1e-6)[0].all()


# ---------------------------------------------------------------------------------------------
# VolSDF
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
@pytest.mark.parametrize('name', list(rr.VOLSDF_CASES))
def test_volsdf_reintegrated(name, precision):
    from neurecon_amd.frameworks import volsdf
    cam, sd, beta, nerfpp = rr.volsdf_case(name)
    tag = f'volsdf {name} {precision}'
    ro, rd = rr.camera_rays(cam)
    og, dg = ro.cuda(), rd.cuda()
    m = volsdf_model(sd, beta, precision=precision, use_nerfplusplus=nerfpp)
    S, No = 128, 32 if nerfpp else 0

    def render(o, d, detailed):
        with torch.no_grad():
            return volsdf.volume_render(o, d, m, near=0.0, far=6.0, obj_bounding_radius=3.0, batched=True,
                                        calc_normal=True, detailed_output=detailed, perturb=False, N_samples=64,
                                        N_importance=64, N_outside=32, use_nerfplusplus=nerfpp, max_upsample_steps=6)
    det = render(og, dg, True)
    _assert_bench_call_equal(det, render(og, dg, False), tag)
    ex = det[2]
    # the library has no rayschunk for VolSDF: the caller's ray-chunk loop, as calls of 64, 64 and 2 rays
    parts = [render(og[:, a:a + 64].contiguous(), dg[:, a:a + 64].contiguous(), True)[2] for a in (0, 64, 128)]
    for k in ex:
        assert torch.equal(ex[k], torch.cat([p[k] for p in parts], 1)), (tag, 'chunked', k)
    for R, rows in rr.SMALL_SETS.items():
        o_s, d_s = og[:, rows].contiguous(), dg[:, rows].contiguous()
        part = render(o_s, d_s, True)
        _assert_rows(ex, part[2], rows, f'{tag} R={R}')
        _assert_bench_call_equal(part, render(o_s, d_s, False), f'{tag} R={R}')

    d_all = ex['d_vals'][..., :S]
    _structure(tag, d_all, S, ex['visibility_weights'], ex['mask_volume'], torch.linspace(0, 1, 64))
    assert tuple(ex['d_vals'].shape) == (1, rr.R_FULL, S + No)
    assert (np.diff(_np(ex['d_vals'])[0], axis=-1) >= 0).all(), tag

    o, d = rr.prepare_rays(ro, rd)
    ikw = dict(use_nerfplusplus=nerfpp, N_outside=32)
    r32 = rr.volsdf_integrate(sd, o, d, d_all.cpu(), torch.float32, **ikw)
    r64 = rr.volsdf_integrate(sd, o, d, d_all.cpu(), torch.float64, **ikw)
    _bar(tag, ex, r32, r64)
    assert report(f'{tag} sdf', ex['implicit_surface'], r64['implicit_surface'].numpy(), 1e-5, 1e-6)[0].all()
    assert report(f'{tag} nablas', ex['implicit_nablas'], r64['implicit_nablas'].numpy(), RT, NAB_AT)[0].all()
    assert report(f'{tag} radiance', ex['radiance'][..., :S, :], r64['radiance'][..., :S, :].numpy(), 1e-5, 1e-6)[0].all()
    assert report(f'{tag} sigma', ex['sigma'][..., :S], r64['sigma'][..., :S].numpy(), RT,
                  4e-6 / (2 * beta * beta))[0].all()
    if nerfpp:
        assert report(f'{tag} d_out', ex['d_vals'][..., S:], r64['d_vals'][..., S:].numpy(), 1e-6, 1e-6)[0].all()
        assert report(f'{tag} sigma_out', ex['sigma_out'], r64['sigma_out'].numpy(), RT, 1e-5)[0].all()
        assert report(f'{tag} radiance_out', ex['radiance_out'], r64['radiance_out'].numpy(), RT, 1e-6)[0].all()


# ---------------------------------------------------------------------------------------------
# UNISURF
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
@pytest.mark.parametrize('name', list(rr.UNISURF_CASES))
def test_unisurf_reintegrated(name, precision):
    from neurecon_amd.frameworks import unisurf
    c = rr.UNISURF_CASES[name]
    tag = f'unisurf {name} {precision}'
    sd = wg.unisurf_state(seed=3)
    ro, rd = rr.camera_rays('e')
    m = unisurf_model(sd, precision=precision)
    P = 96

    def render(o, d, detailed, rayschunk=c['rayschunk'], **extra):
        with torch.no_grad():
            return unisurf.volume_render(o, d, m, batched=True, calc_normal=True, detailed_output=detailed,
                                         logit_tau=0.0, radius_of_interest=4.0, interval=1.0, N_query=64, N_freespace=32,
                                         netchunk=c['netchunk'], rayschunk=rayschunk, **extra)

    def check(tag, ro, rd, chunk_invariant):
        og, dg = ro.cuda(), rd.cuda()
        det = render(og, dg, True)
        _assert_bench_call_equal(det, render(og, dg, False), tag)
        ex = det[2]
        if chunk_invariant:  # the windows of the 64-ray chunks coincide with the whole render's
            _assert_same(ex, render(og, dg, True, rayschunk=65536)[2], tag + ' chunked vs whole')
        d_all = render(og, dg, True, _sample_only=True)['d_all'].reshape(1, -1, P)
        _structure(tag, d_all, P, ex['visibility_weights'], ex['mask_volume'])
        _unisurf_runs(tag, d_all, ex['depth_surface'])
        o, d = rr.prepare_rays(ro, rd)
        r32 = rr.unisurf_integrate(sd, o, d, d_all.cpu(), torch.float32, **c)
        r64 = rr.unisurf_integrate(sd, o, d, d_all.cpu(), torch.float64, **c)
        _bar(tag, ex, r32, r64)
        assert report(f'{tag} logits', ex['implicit_surface'], r64['implicit_surface'].numpy(), 1e-5, 1e-6)[0].all()
        assert report(f'{tag} nablas', ex['implicit_nablas'], r64['implicit_nablas'].numpy(), RT, NAB_AT)[0].all()
        assert report(f'{tag} radiance', ex['radiance'], r64['radiance'].numpy(), 1e-5, 1e-6)[0].all()

    check(tag, ro, rd, chunk_invariant=name == 'three_windows')
    for R, rows in rr.SMALL_SETS.items():  # their points are a window of their own: judged on their own
        check(f'{tag} R={R}', ro[:, rows].contiguous(), rd[:, rows].contiguous(), False)


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_unisurf_empty_rays_depth_is_zero(precision):
    """Config (e)'s rays are all opaque, and there acc + 1e-10 == acc in fp32: the depth normaliser's
    1e-10 only shows on empty rays.  The occupancy logit raised by 120 makes alpha = e^-120 / (1 + e^-120)
    underflow to 0 on every sample, so acc is exactly 0 and depth = sum w / (acc + 1e-10) d is exactly 0;
    without the 1e-10 it is 0 / 0."""
    from neurecon_amd.frameworks import unisurf
    sd = {k: v.clone() for k, v in wg.unisurf_state(seed=3).items()}
    sd['implicit_surface.surface_fc_layers.8.bias'][0] += 120.0
    ro, rd = rr.camera_rays('e')
    rows = rr.SMALL_SETS[3]
    m = unisurf_model(sd, precision=precision)
    with torch.no_grad():
        rgb, depth, ex = unisurf.volume_render(ro[:, rows].cuda(), rd[:, rows].cuda(), m, batched=True,
                                               calc_normal=True, detailed_output=True, logit_tau=0.0, N_query=64,
                                               N_freespace=32)
    assert not ex['mask_surface'].any()
    assert float(ex['implicit_surface'].min()) > 100.0
    for name, t in (('rgb', rgb), ('depth', depth), ('mask', ex['mask_volume']), ('normals', ex['normals_volume'])):
        assert torch.equal(t, torch.zeros_like(t)), (precision, name, t)


# ---------------------------------------------------------------------------------------------
# sample_pdf, bit for bit against the oracle's at its edges
# ---------------------------------------------------------------------------------------------
def _pdf_inputs(gen, R, L, weights, repeat):
    bins = torch.sort(torch.rand(R, L, generator=gen) * 3 + 0.5, -1).values
    if repeat and L > 2:
        k = L // 2
        bins[:, k] = bins[:, k - 1]
    elif repeat:
        bins[:, 1] = bins[:, 0]
    if weights == 'random':
        w = torch.rand(R, L - 1, generator=gen)
    elif weights == 'zero':
        w = torch.zeros(R, L - 1)
    elif weights == 'one_hot':
        w = torch.zeros(R, L - 1)
        w[torch.arange(R), torch.randint(0, L - 1, (R,), generator=gen)] = 1.0
    else:  # one weight 1e4 times the rest
        w = torch.rand(R, L - 1, generator=gen) * 0.5 + 0.5
        w[torch.arange(R), torch.randint(0, L - 1, (R,), generator=gen)] *= 1e4
    return bins, w


def _pdf_uniforms(gen, w, N):
    """random u holding exactly 0, exactly 1 and values of the row's own cdf (searchsorted ties)"""
    R = w.shape[0]
    u = torch.rand(R, N, generator=gen)
    pdf = (w + 1e-5) / torch.sum(w + 1e-5, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    pick = torch.randint(0, cdf.shape[-1], (R, N), generator=gen)
    tie = torch.rand(R, N, generator=gen) < 0.4
    u = torch.where(tie, torch.gather(cdf, -1, pick), u)
    u[:, 0] = 0.0
    if N > 1:
        u[:, -1] = 1.0
    return u.contiguous()


@pytest.mark.parametrize('L', [2, 8, 9, 33, 64, 65, 128, 257, 2048])
def test_sample_pdf_bit_exact_at_edges(L, monkeypatch):
    """rend_util.sample_pdf (nr_sample_pdf) equals oracle.rays.sample_pdf by torch.equal: det with the
    shared linspace and per-row u handed through rend_util.uniform.  The row lengths cover every branch
    of aten_row_sum (fewer than a vector, one vector, vector + tail, the ILP groups, the cascade levels
    that direct_more's 2048 samples reach)."""
    from neurecon_amd import rend_util
    from oracle import rays as orays
    gen = torch.Generator().manual_seed(1000 + L)
    bad = []
    for R in (1, 63, 65):
        for weights in ('random', 'zero', 'one_hot', 'spike'):
            for repeat in (False, True):
                bins, w = _pdf_inputs(gen, R, L, weights, repeat)
                bg, wgpu = bins.cuda(), w.cuda()
                for N in (1, 16, 66):
                    ref = orays.sample_pdf(bins, w, N, det=True)
                    got = rend_util.sample_pdf(bg, wgpu, N, det=True).cpu()
                    if not torch.equal(got, ref):
                        bad.append(('det', R, weights, repeat, N, int((got != ref).sum()), float((got - ref).abs().max())))
                    u = _pdf_uniforms(gen, w, N)
                    monkeypatch.setattr(rend_util, 'uniform', lambda shape, device=None, _u=u: _u.to(device))
                    ref = orays.sample_pdf(bins, w, N, u=u)
                    got = rend_util.sample_pdf(bg, wgpu, N, det=False).cpu()
                    if not torch.equal(got, ref):
                        bad.append(('u', R, weights, repeat, N, int((got != ref).sum()), float((got - ref).abs().max())))
    print(f'sample_pdf L={L}: {len(bad)} mismatching calls {bad[:8]}')
    assert not bad, bad
