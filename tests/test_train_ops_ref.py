"""tests/train_ops_ref.py on the CPU: each float64 reference pinned to an independent source (the
oracle's embedding and RadianceNet input, torch's softplus / sin and float64 autograd), and the conditions
tests/test_gpu_train_ops.py relies on: the integer column sums stay exact in fp32, no replica input makes
a subnormal product, the single-band vjp cases are zero outside their band, the case lists hold every
size at which a kernel takes another path."""
import pytest
import torch

import train_ops_ref as R
from oracle import nets

F64 = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize('nfreq', R.EMBED_NFREQ)
def test_embedding_refs_vs_oracle_and_autograd(nfreq):
    x, v = R.points(5)
    x64, v64 = x.double(), v.double()
    emb = lambda t: nets.embed(t, nfreq)
    if nfreq == 0:   # the oracle's linspace(0, -1, 0) is empty as well: x alone
        assert emb(x64).shape == (5, 3)
    _close(R.embed_ref(x, nfreq), emb(x64))
    assert R.embed_ref(x, nfreq).shape[1] == R.nfeat(nfreq)
    _, jv = torch.autograd.functional.jvp(emb, x64, v64)
    _close(R.embed_jvp_ref(x, v, nfreq), jv)
    for s1 in R.VJP_S1:
        _, e0, e1 = R.vjp_inputs(5, nfreq, R.nfeat(nfreq), R.nfeat(nfreq), s1)
        ct = e0.double() if e1 is None else e0.double() + e1.double() * torch.tensor(s1, dtype=torch.float32).double()
        _, vj = torch.autograd.functional.vjp(emb, x64, ct)
        _close(R.embed_vjp_ref(x, e0, e1, s1, nfreq), vj, 1e-11)


def test_activation_refs_vs_torch():
    z = R.softplus_sweep()
    z64 = z.double().requires_grad_(True)
    h_t = torch.nn.functional.softplus(z64, beta=100, threshold=20)
    s_t, = torch.autograd.grad(h_t.sum(), z64)
    h, s = R.softplus100_ref(z)
    _close(h, h_t.detach(), 1e-14)
    _close(s, s_t, 1e-14)
    z = R.sine_sweep()
    z64 = z.double().requires_grad_(True)
    h_t = torch.sin(30 * z64)
    s_t, = torch.autograd.grad(h_t.sum(), z64)
    h, s = R.sine30_ref(z)
    _close(h, h_t.detach(), 1e-14)
    _close(s, s_t, 1e-13)
    y = torch.linspace(-100, 100, 4001)
    _close(R.sigmoid_ref(y), torch.sigmoid(y.double()), 1e-15)


@pytest.mark.parametrize('sine', [False, True], ids=['softplus', 'sine'])
def test_adjoint_refs_vs_autograd(sine):
    """zbar = d/dz [hbar . act(z) + (g zdot) . act'(z)] under float64 autograd (softplus on its smooth
    branch: torch's double backward is 0 on the linear one, as 100 s (1 - s) with s = 1)"""
    g0 = torch.Generator().manual_seed(3)
    z = (torch.rand(7, 39, generator=g0, dtype=F64) * (20.0 if sine else 0.5) - (10.0 if sine else 0.35)).requires_grad_(True)
    hbar, g, zdot = (torch.randn(7, 39, generator=g0, dtype=F64) for _ in range(3))
    act = (lambda t: torch.sin(30 * t)) if sine else (lambda t: torch.nn.functional.softplus(t, beta=100, threshold=20))
    a = act(z)
    d1, = torch.autograd.grad(a.sum(), z, create_graph=True)
    zbar, = torch.autograd.grad((hbar * a).sum() + (g * zdot * d1).sum(), z)
    for with_g in (True, False):
        if not with_g:
            zbar, = torch.autograd.grad((hbar * act(z)).sum(), z)
        gg, zz = (g, zdot) if with_g else (None, None)
        if sine:
            got = R.sine_adjoint_ref(hbar, d1.detach(), a.detach(), gg, zz)
        else:
            got = R.softplus_adjoint_ref(hbar, d1.detach(), gg, zz)
        _close(got, zbar, 1e-12)


@pytest.mark.parametrize('P, uv, nfv, wf', R.RAD_CASES[:18])
def test_radiance_input_ref_vs_oracle(P, uv, nfv, wf):
    """the torch.cat of oracle.nets.RadianceNet.forward (multires = -1: x itself), caught at its first layer"""
    x, v, nrm, feat = R.radiance_inputs(P, wf)
    ld = 3 + (R.nfeat(nfv) + 3 if uv else 0) + wf
    sd = {}
    for l in range(2):   # identity layers: the hidden layer's pre-activation is the input itself
        sd.update({f'l.layers.{l}.weight_v': torch.eye(ld, dtype=F64), f'l.layers.{l}.weight_g': torch.ones(ld, 1, dtype=F64),
                   f'l.layers.{l}.bias': torch.zeros(ld, dtype=F64)})
    net = nets.RadianceNet(sd, prefix='l.', D=1, multires=-1, multires_view=nfv, use_view_dirs=bool(uv))
    z = []
    f = feat.double() if wf else torch.zeros(P, 0, dtype=F64)
    net.forward(x.double(), v.double(), nrm.double(), f, z_out=z)
    ref = R.radiance_input_ref(x, v, nrm, feat, nfv, uv, wf)
    _close(ref, z[0], 0.0)
    copies, emb = R.radiance_input_copies(x, nrm, feat, nfv, uv, wf)
    for sl, val in copies:
        assert torch.equal(ref[:, sl], val.double())
    covered = sum(sl.stop - sl.start for sl, _ in copies) + (emb.stop - emb.start if emb else 0)
    assert covered == ld == ref.shape[1]


def test_integer_column_sums_are_exact_in_fp32():
    a = R.colsum_input('int')
    assert a.shape == (16385, 257) and torch.equal(a, a.round()) and float(a.abs().max()) == 8.0
    # every partial sum of any subset of a column's rows is an integer of magnitude <= sum |a| < 2^24
    assert float(a.abs().double().sum(0).max()) < 2 ** 24
    for P in R.COLSUM_P:
        c = R.colsum_case('int', P, 65)
        assert c.shape == (P, 65) and c.is_contiguous()
        assert float(c.long().sum(0).abs().max()) < 2 ** 24 if P else True
    h = R.colsum_input('heavy')
    assert float(h.abs().max()) > 100 * float(h.abs().median())


def _normal_or_zero(ts):
    for t in ts:
        a = t.abs()
        assert bool(((a == 0) | (a >= R.TINY)).all()) and bool(torch.isfinite(t).all())


def test_replica_inputs_make_no_subnormal_product():
    for P, n, ldh, with_g in R.grid_cases():
        for sine in (False, True):
            d = R.adjoint_inputs(P, n, ldh, 7 * P + n, sine)
            for k in ('s', 'g', 'zdot') + (('h',) if sine else ()):
                assert 1e-3 <= float(d[k].abs().min()) and float(d[k].abs().max()) <= 1e3
            assert bool(torch.isnan(d['hbar'][:, n:]).all())
            tr = []
            hb = d['hbar'][:, :n]
            g, zd = (d['g'], d['zdot']) if with_g else (None, None)
            if sine:
                R.sine_adjoint_replica(hb, d['s'], d['h'], g, zd, tr)
            else:
                R.softplus_adjoint_replica(hb, d['s'], g, zd, tr)
            assert tr
            _normal_or_zero(tr)
    for P, lda, col0, ncols, with_s, scale in R.scale_cols_cases():
        tr = []
        R.scale_cols_replica(R.mag((P, lda), P + lda), col0, ncols, R.mag((P, ncols), 3) if with_s else None, scale, tr)
        _normal_or_zero(tr)
        assert col0 + ncols <= lda
    for n in R.FLAT_N:
        tr = []
        R.mul_replica(R.mag((n,), n), R.mag((n,), n + 1), tr)
        R.activation_replica(R.unit((n,), n), R.mag((n,), n + 2), 3, tr)
        assert len(tr) == 3
        _normal_or_zero(tr)
        y, g = R.relu_inputs(n, n)
        _normal_or_zero([y, g])
    y, _ = R.relu_inputs(1000, 0)
    for v, neg in ((0.0, False), (0.0, True), (R.TINY, False), (R.TINY, True)):
        assert bool(((y.abs() == v) & (torch.signbit(y) == neg)).any())
    assert torch.tensor(R.TINY, dtype=torch.float32).item() == torch.finfo(torch.float32).tiny


def test_single_band_vjp_cases_are_zero_elsewhere():
    nf = R.nfeat(R.VJP_BAND_NFREQ)
    gr = dict(R.groups(R.VJP_BAND_NFREQ))
    assert len(R.VJP_BANDS) == 11
    for band in R.VJP_BANDS:
        _, e0, e1 = R.vjp_inputs(R.VJP_BAND_P, R.VJP_BAND_NFREQ, nf, nf, None, band=band, seed=7)
        sl = gr['identity' if band == 'identity' else f'band{band}']
        assert e1 is None
        inside = torch.zeros(nf, dtype=torch.bool)
        inside[sl] = True
        assert bool((e0[:, ~inside] == 0).all()) and bool((e0[:, inside] != 0).all())


def test_case_lists_hold_every_path():
    ec = R.embed_cases()
    assert {c[0] for c in ec} == {1, 3, 4, 5, 8193} and {c[1] for c in ec} == {-1, 0, 4, 6, 10}
    assert {c[2] for c in ec} == {3, 27, 39, 63, 64, 80, 128} and all(ldo >= R.nfeat(nf) for _, nf, ldo in ec)
    assert 8193 > 2048 * 4          # the grid is capped at 2048 blocks of 4 points: a second trip
    vc = R.vjp_cases()
    for nfreq in R.EMBED_NFREQ:
        nf = R.nfeat(nfreq)
        pairs = {(c[2], c[3]) for c in vc if c[1] == nfreq}
        assert pairs == {(a, b) for a in {nf, 64, 70} for b in {nf, 64, 70}}
        for s1 in R.VJP_S1:      # every e1 / s1 option meets every stride pair
            assert {(c[2], c[3]) for c in vc if c[1] == nfreq and c[4] == s1} == pairs
    x, _ = R.points(8193)
    sp = R.special_scalars()
    assert all(bool((x == s).any()) for s in sp) and bool(torch.signbit(x[x == 0]).any())
    for P in (1, 3, 4, 5):
        xs, _ = R.points(P)
        assert bool(torch.isin(xs, sp).any())
    z = R.softplus_sweep()
    t = z * 100.0
    assert float(t.min()) <= -120 and float(t.max()) >= 40 and float(t.sort().values.diff().max()) < 0.011
    assert bool((t > 20).any()) and bool((t == 20).any())
    c = torch.tensor(0.2)
    assert bool((z == torch.nextafter(c, torch.tensor(1.0))).any()) and bool((z == torch.nextafter(c, torch.tensor(-1.0))).any())
    assert float(R.sine_sweep().abs().max()) == 10.0
    assert len(R.RAD_CASES) == 36 and len(R.grid_cases()) == 48
    assert all(0 < c0 and c0 + nc < lda for _, lda, c0, nc, _, _ in R.scale_cols_cases()[:48])
