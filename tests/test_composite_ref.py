"""Pins tests/composite_ref.py (the reference tests/test_gpu_composite.py holds the training compositing
kernels to) to the oracle, and holds the conditioning caps of every case of tests/composite_cases.py, on
the CPU.

  1. composite_ref in fp32 against the corresponding lines of oracle/train.py (neus_train_losses with
     and without the NeRF++ background, volsdf_train_losses with the builtin background sphere and with
     background samples, unisurf_train_losses): the loss functions run on a few rays of the training
     fixtures' nets with recorders on their building blocks (nablas_graph, the nets' forward,
     sdf_to_alpha, alpha_to_w, sdf_to_sigma, F.l1_loss, F.binary_cross_entropy); composite_ref on the
     recorded sdf / radiance / sigma reproduces the recorded alpha, weights, sigma, rgb and acc to 1e-6.
     white_bkgd and depth, which the training losses do not use, against NeuSOracle.integrate.
  2. the caps: where the fp32 reference itself is off, |hip - f64| <= 4 E_ray + 2e-6 scale would pass
     anything, so per case and tensor at most 2 % of the rays may have E_ray > 1e-4 scale; VolSDF and
     UNISURF cases hold at least 10 % of rays with acc < 1e-3 (g_depth = 0 there) and 25 % with
     acc > 0.5; every upstream gradient is non-zero; the inputs have the features the cases are there
     for (equal consecutive depths, an exact sdf = 0, background values taken, inside / outside rows, a
     sigma above softplus's threshold, |logit| < 80).
  3. composite_ref's float64 gradients against finite differences (gradcheck), one small case a kind."""
import pytest
import torch
import torch.nn.functional as F

import composite_cases as CC
import composite_ref as CR
import weightgen as wg

TOL = 1e-6


def _close(name, got, ref, tol=TOL):
    e = float((got - ref).abs().max())
    sc = max(float(ref.abs().max()), 1.0)
    print(f'{name}: max |composite_ref - oracle| {e:.2e} (scale {sc:.3e})')
    assert e <= tol * sc, name


class Rec:
    """records the calls of oracle.train's building blocks while one loss function runs"""

    def __init__(self, mp):
        import oracle.train as OT
        self.log = {}
        for owner, attr, key in ((OT, 'nablas_graph', 'nablas_graph'), (OT, 'sdf_to_alpha', 'sdf_to_alpha'),
                                 (OT, 'alpha_to_w', 'alpha_to_w'), (OT, 'sdf_to_sigma', 'sdf_to_sigma'),
                                 (OT.RadianceNet, 'forward', 'rad'), (OT.NeRFNet, 'forward', 'nerf'),
                                 (F, 'l1_loss', 'l1'), (F, 'binary_cross_entropy', 'bce')):
            mp.setattr(owner, attr, self._wrap(getattr(owner, attr), key))

    def _wrap(self, fn, key):
        def rec(*a, **kw):
            out = fn(*a, **kw)
            self.log.setdefault(key, []).append((a, out))
            return out
        return rec

    def one(self, key, i=0):
        return self.log[key][i]


def _rays(B, n, seed, r=2.5):
    g = torch.Generator().manual_seed(seed)
    o = F.normalize(torch.randn(B, n, 3, generator=g), dim=-1) * r
    d = F.normalize(0.3 * torch.randn(B, n, 3, generator=g) - o, dim=-1)
    return o, d, g


def _sorted_depths(g, shape, lo, hi):
    return (lo + (hi - lo) * torch.rand(*shape, generator=g)).sort(-1)[0]


@pytest.mark.parametrize('N_outside', [0, 4])
def test_neus_vs_oracle_train(monkeypatch, N_outside):
    import oracle.rays as OR
    from oracle.train import neus_train_losses
    sd = wg.neus_state(seed=11, use_outside_nerf=N_outside > 0)
    o, d, g = _rays(1, 6, 3)
    near, far = OR.near_far_from_sphere(o, d, r=1.0)
    S = 12
    d_all = near + (far - near) * _sorted_depths(g, (1, 6, S), 0.0, 1.0)
    tgt, mask = torch.rand(1, 6, 3, generator=g), (torch.rand(1, 6, generator=g) < 0.7).float()
    with monkeypatch.context() as mp:
        rec = Rec(mp)
        with torch.enable_grad():
            neus_train_losses(sd, o, d, tgt, mask, d_all=d_all, N_outside=N_outside, N_samples=S // 2,
                              N_importance=S // 2)
    (sdf, s), (cdf, alpha_in) = rec.one('sdf_to_alpha')
    rad = rec.one('rad')[1]
    (alpha,), w = rec.one('alpha_to_w')
    rgb = rec.one('l1')[0][0]
    acc_clamped = rec.one('bce')[0][0]
    d_mid = 0.5 * (d_all[..., 1:] + d_all[..., :-1])
    bg = None
    if N_outside > 0:
        sig_o, rad_o = rec.one('nerf')[1]
        tt = torch.linspace(0, 1, N_outside + 2)[..., 1:-1].float()
        d_out = torch.cat([d_mid, far / torch.flip(tt, dims=[-1])], -1)
        inside = (o[..., None, :] + d[..., None, :] * d_mid[..., :, None]).norm(dim=-1) <= 1.0
        assert 0 < int(inside.sum()) < inside.numel()
        bg = (sig_o, rad_o, d_out, inside)
    with torch.no_grad():
        out = CR.neus(sdf.detach(), s.detach(), rad.detach(), d_mid, False, bg)
    _close('cdf', out['cdf'], cdf.detach())
    _close('alpha', out['alpha'], alpha.detach())
    _close('weights', out['weights'], w.detach())
    _close('rgb', out['rgb'], rgb.detach())
    _close('acc', torch.clamp(out['acc'], 1e-3, 1 - 1e-3), acc_clamped.detach())


@pytest.mark.parametrize('N_outside', [0, 4])
def test_volsdf_vs_oracle_train(monkeypatch, N_outside):
    from oracle.train import volsdf_train_losses
    sd = wg.volsdf_state(seed=12, beta_init=0.1, use_nerfplusplus=N_outside > 0)
    o, d, g = _rays(1, 6, 4, r=2.0)
    S = 12
    d_in = _sorted_depths(g, (1, 6, S), 0.0, 6.0)
    d_all = torch.cat([d_in, 6.0 + _sorted_depths(g, (1, 6, N_outside), 0.1, 20.0)], -1) if N_outside else d_in
    tgt, eik = torch.rand(1, 6, 3, generator=g), torch.rand(1, 6, 1, 3, generator=g) * 6 - 3
    with monkeypatch.context() as mp:
        rec = Rec(mp)
        with torch.enable_grad():
            volsdf_train_losses(sd, o, d, tgt, eik, d_all=d_all, N_outside=N_outside, N_samples=S // 2,
                                N_importance=S // 2)
    sdf_net = rec.one('nablas_graph')[1][0]
    (sdf_bg, _, beta), sigma = rec.one('sdf_to_sigma')
    rad = rec.one('rad')[1]
    rgb = rec.one('l1')[0][0]
    pts = o[..., None, :] + d[..., None, :] * d_in[..., :, None]
    bg = None
    if N_outside > 0:
        sig_o, rad_o = rec.one('nerf')[1]
        bg = (sig_o.detach(), rad_o.detach(), d_all[..., S:])
    else:
        assert 0 < int((sdf_bg != sdf_net).sum()) < sdf_net.numel()  # some samples take the background value
    with torch.no_grad():
        out = CR.volsdf(sdf_net.detach(), beta.detach(), rad.detach(), pts, d_in, N_outside == 0, 3.0, False, bg)
    _close('sdf_out', out['sdf_out'], sdf_bg.detach())
    _close('sigma', out['sigma'][..., :S], sigma.detach())
    _close('rgb', out['rgb'], rgb.detach())


def test_unisurf_vs_oracle_train(monkeypatch):
    from oracle.train import unisurf_train_losses
    sd = wg.unisurf_state(seed=13)
    o, d, g = _rays(1, 6, 5)
    P = 10
    d_all = _sorted_depths(g, (1, 6, P), 0.5, 4.5)
    tgt, sp, pert = torch.rand(1, 6, 3, generator=g), torch.randn(1, 6, 3, generator=g), \
        0.01 * torch.randn(1, 6, 3, generator=g)
    with monkeypatch.context() as mp:
        rec = Rec(mp)
        with torch.enable_grad():
            unisurf_train_losses(sd, o, d, tgt, pert, d_all=d_all, surface_points=sp)
    logits = rec.one('nablas_graph')[1][0].reshape(1, 6, P)
    rad = rec.one('rad')[1].reshape(1, 6, P, 3)
    rgb = rec.one('l1')[0][0]
    with torch.no_grad():
        out = CR.unisurf(logits.detach(), rad.detach(), d_all, False)
    _close('rgb', out['rgb'], rgb.detach())


@pytest.mark.parametrize('N_outside', [0, 4])
def test_neus_depth_and_white_vs_oracle_integrate(N_outside):
    """depth and white_bkgd are not in the training losses: NeuSOracle.integrate (the render the golden
    suites pin to the reference project) has them"""
    import oracle.rays as OR
    from oracle.neus import NeuSOracle
    sd = wg.neus_state(seed=11, use_outside_nerf=N_outside > 0)
    o, d, g = _rays(1, 6, 7)
    near, far = OR.near_far_from_sphere(o, d, r=1.0)
    d_all = near + (far - near) * _sorted_depths(g, (1, 6, 12), 0.0, 1.0)
    orc = NeuSOracle(sd, use_outside_nerf=N_outside > 0)
    ref = orc.integrate(o, d, near, far, d_all, d, calc_normal=False, N_outside=N_outside, white_bkgd=True)
    ref = {k: v.detach() for k, v in ref.items()}
    d_mid = 0.5 * (d_all[..., 1:] + d_all[..., :-1])
    n1 = d_mid.shape[-1]
    bg = None
    if N_outside > 0:
        inside = (o[..., None, :] + d[..., None, :] * d_mid[..., :, None]).norm(dim=-1) <= 1.0
        bg = (ref['sigma_out'], ref['radiance_out'], ref['d_final'], inside)
    # integrate returns the merged colours: at the inside mid-points they are the radiance net's
    out = CR.neus(ref['implicit_surface'], orc.s(), ref['radiance'][..., :n1, :], d_mid, True, bg)
    for k, rk in (('rgb', 'rgb'), ('depth', 'depth_volume'), ('acc', 'mask_volume'), ('weights', 'visibility_weights'),
                  ('alpha', 'alpha'), ('cdf', 'cdf')):
        _close(k, out[k], ref[rk])


# ---- the caps -----------------------------------------------------------------------------------
def test_case_set_is_the_issue_s():
    """every shape, scalar and white_bkgd value, at every R"""
    names = set(CC.BY_NAME)
    for R in CC.R_SET:
        for w in (0, 1):
            for S in CC.NEUS_S:
                for s in CC.S_SET:
                    assert (f'neus-R{R}-S{S}_s{s:g}-w{w}' in names) == (not (S == 2 and s == 3000.0))
            for (S, N) in CC.NEUS_BG_SN:
                for s in CC.S_SET:
                    assert (f'neus_bg-R{R}-S{S}_N{N}_s{s:g}-w{w}' in names) == (not (S == 2 and s == 3000.0))
            for (S, N) in CC.VOLSDF_SN:
                for beta in CC.BETA_SET:
                    assert f'volsdf-R{R}-S{S}_N{N}_beta{beta:g}_use_bg{int(N == 0)}-w{w}' in names
            assert f'volsdf-R{R}-S65_N3_beta0.01_use_bg1-w{w}' in names
            for P in CC.UNI_P:
                for c in CC.UNI_C:
                    assert f'unisurf-R{R}-P{P}_c{c:g}-w{w}' in names
    assert len(CC.CASES) == 400


@pytest.mark.parametrize('kind', CC.KINDS)
def test_conditioning_caps(kind):
    worst = {}
    for c in CC.cases_of(kind):
        CC.build(c)
        for k, (t32, t64, E, scale) in CC.tensors(c).items():
            assert bool(torch.isfinite(t32).all()) and bool(torch.isfinite(t64).all()), (c, k)
            loose = float((E > CC.LOOSE * scale).double().mean())
            if scale > 0:
                worst[k] = max(worst.get(k, 0.0), float(E.max()) / scale)
            assert loose <= CC.LOOSE_SHARE, (c, k, loose, float(E.max()), scale)
        for k, v in c.g.items():
            live = v if k != 'g_depth' else v[c.acc64 >= CC.ACC_MIN]
            assert bool((live != 0).all()), (c, k)
            assert bool((c.g['g_depth'][c.acc64 < CC.ACC_MIN] == 0).all()), c
        if kind in ('volsdf', 'unisurf') and c.R >= 63:
            lo, hi = float((c.acc64 < CC.ACC_MIN).double().mean()), float((c.acc64 > 0.5).double().mean())
            assert lo >= 0.10 and hi >= 0.25, (c, lo, hi)
        if kind == 'neus_bg':
            assert float(c.acc64.min()) > 0.999, c  # the last distance is 1e10: no depth exception needed
    print(f'{kind}: worst max |fp32 - f64| / scale per tensor over {len(CC.cases_of(kind))} cases:',
          {k: f'{v:.1e}' for k, v in worst.items()})


def test_case_inputs_have_their_features():
    for c in CC.CASES:
        x = CC.build(c).x
        R = c.R
        if c.kind in ('neus', 'neus_bg'):
            step = x['sdf'][:, 1:] - x['sdf'][:, :-1]
            assert bool((x['sdf'][:, 0] > 0.3).all()) and bool((x['sdf'][:, -1] < 0).all()), c
            if c.S >= 64 and R >= 63:
                assert bool((step > 0).any()) and bool((step < 0).any()), c
        if c.kind == 'neus_bg':
            ins = x['inside'].bool()
            assert x['d_out'].shape[1] == c.S - 1 + c.N and bool((x['d_out'][:, 1:] > x['d_out'][:, :-1]).all()), c
            assert bool((x['sigma_out'] > 20).any()) and (R < 63 or bool((x['sigma_out'] < 0).any())), c
            if R >= 3:
                assert bool(ins[0].all()) and not bool(ins[1].any()), c
                if c.S > 2:
                    assert 0.7 < float(ins[2:].float().mean()) < 0.9, c
        if c.kind == 'volsdf':
            empty, thin = CC.volsdf_ray_kinds(c)
            taken = (R_bg_value(x) < x['sdf'])
            if c.use_bg and R >= 63:
                assert float(taken.float().mean()) > (0.1 if c.S > 2 else 0.25), (c, float(taken.float().mean()))
            if c.S > 2:
                assert bool(((x['d_all'][:, 1:] == x['d_all'][:, :-1]).sum(-1) == 1).all()), c
                assert bool(((x['sdf'] == 0).sum(-1) >= 1)[~empty].all()), c   # an empty ray cannot hold one
            assert bool((x['d_all'][:, 1:] >= x['d_all'][:, :-1]).all()), c
            if c.N:
                assert bool((x['d_bg'][:, :1] > x['d_all'][:, -1:]).all()), c
        if c.kind == 'unisurf':
            assert float(x['logits'].abs().max()) < 80, c
            assert bool((x['d_all'][:, 1:] > x['d_all'][:, :-1]).all()), c


def R_bg_value(x):
    return CC.R_BG - x['pts'].norm(dim=-1)


@pytest.mark.parametrize('name', ['neus-R1-S2_s20-w1', 'neus_bg-R1-S2_N1_s20-w1', 'neus_bg-R1-S2_N1_s300-w1',
                                  'volsdf-R1-S2_N0_beta0.1_use_bg1-w1', 'unisurf-R1-P2_c1-w1'])
def test_reference_gradients_vs_finite_differences(name):
    """autograd of composite_ref in float64 is the truth of every gradient check: small cases of each kind
    against central differences (S = 2 / P = 2: away from the clamp, ReLU and min() kinks and the constructed
    delta = 0 and sdf = 0 points; the NeuS + NeRF++ mid-point inside at s = 20, outside at s = 300)"""
    c = CC.BY_NAME[name]
    kind = c.kind
    CC.build(c)
    _, g64 = CC.evaluate(c, torch.float64)

    def loss(x):
        out = CC._forward(c, x)
        tot = 0
        for gk, ok in (('g_rgb', 'rgb'), ('g_depth', 'depth'), ('g_acc', 'acc'), ('g_w', 'weights'), ('g_sdf', 'sdf_out')):
            if gk in c.g:
                tot = tot + (out[ok] * c.g[gk].double()).sum()
        return float(tot)
    x0 = {k: (v.double() if v.is_floating_point() else v) for k, v in c.x.items()}
    scalar = {'neus': 's', 'neus_bg': 's', 'volsdf': 'beta'}.get(kind)
    names = [k for k in CC.DIFF_IN[kind] if k in x0] + ([scalar] if scalar else [])
    for k in names:
        ref = g64[CC.GRAD_OF[k]] if k in CC.GRAD_OF else g64['d_' + k].sum().reshape(1)
        fd = torch.zeros_like(x0[k])
        for i in range(x0[k].numel()):
            h = 1e-6 * max(1.0, abs(float(x0[k].reshape(-1)[i])))
            vals = []
            for sgn in (1, -1):
                x = dict(x0)
                x[k] = x0[k].clone()
                x[k].reshape(-1)[i] += sgn * h
                vals.append(loss(x))
            fd.reshape(-1)[i] = (vals[0] - vals[1]) / (2 * h)
        sc = max(float(ref.abs().max()), 1e-12)
        e = float((fd.reshape(ref.shape) - ref).abs().max())
        print(f'{c} {k}: max |autograd - central difference| {e / sc:.2e} of {sc:.3e}')
        assert e <= 1e-5 * sc, (c, k)
