"""The training step's compositing kernels (csrc/nr_train.hip) call by call through the C ABI: NeuS
(wave per ray, 64-lane segments with a carried prefix product and a carried reverse suffix sum), NeuS with
the NeRF++ background, VolSDF (thread per ray; builtin background sphere and / or background samples) and
UNISURF, forward and backward each, and the two kernels that build the background net's inputs.  The
end-to-end training steps reach them at one shape with g_rgb (and g_acc) only; direct calls also pass
NULL pointers, which torch.autograd.Function never does.

Cases (tests/composite_cases.py; their conditioning is held on the CPU by tests/test_composite_ref.py):
R in {1, 63, 65, 130} for every kernel; NeuS S in {2, 64, 65, 66, 129} x s in {20, 300, 3000}; NeuS + NeRF++
(S, N_outside) in {(2, 1), (65, 3), (66, 32), (128, 32)} x s; VolSDF (S, N) in {(2, 0), (64, 0), (65, 3),
(128, 32)} x beta in {0.1, 0.01, 0.001} (use_bg = 1 with N = 0, 0 with N > 0, one case with both); UNISURF
P in {1, 2, 96, 97} x logit spread c in {1, 10, 40}; white_bkgd in {0, 1}; every upstream gradient
(g_rgb, g_depth, g_acc, g_weights / g_tau, g_sdf) random and non-zero (g_depth = 0 on rays with acc < 1e-3).

  1. against float64: tests/composite_ref.py (pinned to the oracle by tests/test_composite_ref.py) under
     autograd in fp32 and fp64 on the same fp32 inputs and upstream gradients; per element of every
     forward output and gradient |hip - f64| <= 4 E_ray + 2e-6 scale, E_ray = the fp32 reference's worst
     |fp32 - f64| over that ray's elements of the tensor, scale = the tensor's max |f64|.  d_s and d_beta
     per ray [R] and after the host's sum.  Catches: a wrong sign or factor in any term (the depth term
     gd (d / A - wd / A^2), the white_bkgd coupling ga -= sum g_rgb, g_weights, g_sdf), a carry dropped at
     a 64-lane segment boundary (S - 1 = 64, 65, 128), a block tail (R = 63, 65, 130), saturation (s = 3000:
     CDFs exactly 0 / 1, alpha = 1, the division by u = 1e-10; beta = 0.001), the VolSDF handover interval
     d_bg[0] - d_all[S-1] with the SDF sigma, the delta = 0 ReLU kink, sign(0), softplus's threshold branch.
  2. NULL upstream gradients: each pointer NULL equals a zero tensor, bit for bit.
  3. NULL optional outputs (alpha, cdf, p_i, sigma, sdf_out): every other output unchanged, bit for bit.
  4. nothing written outside: every output, gradient and the workspace (exactly *_workspace_bytes()
     long) lies between sentinels, checked after every launch of every test here; one byte less of
     workspace returns NR_ERR_WORKSPACE and writes nothing.
  5. the same launch twice is bit-identical.
  6. masking, exact zeros: VolSDF d_sdf where the background value was taken (g_sdf non-zero there), the
     rows past the composited samples; NeuS + NeRF++ d_rad at outside mid-points, d_rad_out and
     d_sigma_out at inside ones.
  7. the torch.autograd.Function wrappers of training.py give the direct calls' bits, also with
     non-contiguous views for their no-grad inputs (NeuSCompositeBG passed d_out and inside on without
     .contiguous(); fixed with this test).
  8. nr_nerf_train_input / nr_volsdf_nerf_input against float64 oracle.nets.embed with the same bar, and
     inside == (|p| <= r_obj) in fp32.

Measured on MI355X, worst (|hip - f64| - E_ray) / scale per kernel pair and tensor over all 400 cases
(MEASURED below; DESIGN.md section 3 has the same table): at most 5e-7 on every forward output, at most
1.3e-6 on every gradient but the per-ray d_s of the two NeuS kernels (1.95e-6 / 1.71e-6; 2.75e-6 /
2.32e-6 after the host's sum, whose scale is the largest single ray's).  d_s = sum_k cbar_k c_k (1 - c_k)
sdf_k: at s = 20 its terms, of both signs, add up in magnitude to 3 - 7.5 times the largest |d_s| of the
tensor (float64, on the CPU); the kernel adds them in fp64 from fp32-rounded cbar, torch in fp32, so on
one ray neither error bounds the other.  The summed d_s is the one tensor whose excess over E_ray is
above 2e-6 scale, i.e. that uses the factor on E_ray at all; none needs more than the bar.
The embedding inputs: x_emb's excess is at most 8.3e-6 of its scale; |hip - f64| is 1e-5 - 4e-5 in the
2^9 band where |x| <= 1 and up to 2.1e-4 where 1 / |p| > 1 carries the argument to 2^9 / |p| (the fp32
reference: up to 4e-3 there), 7e-8 on the identity features; v_emb 6e-8 everywhere.

Found with these tests and fixed: VolSDF's background value r_bg - |x| took |x| from __fsqrt_rn of a
plain sum of squares -- the native square root, one ulp off -- where the render kernel and torch use
sqrt(fma(z, z, fma(y, y, x x))) (norm3_ref): at beta = 0.01 one ulp of |x| = 3 moves sigma by 2.4e-5
of itself (rgb was 1e-5 of scale off on the rays whose first sample takes the background value).  A NULL
g_sdf gave d_sdf = -0.0 where a zero tensor gives +0.0.  NeuSCompositeBG.forward passed non-contiguous
d_out / inside on as they were.

A constant added to every weight adjoint (the wd / A^2 part of the depth term, g_acc, the white_bkgd
coupling) cannot show in the NeuS + NeRF++ kernel: its last distance is 1e10, acc = 1 identically and
d acc = 0.  The other three kernels have rays with acc inside (0, 1)."""
import ctypes

import pytest
import torch

import composite_cases as CC

pytestmark = pytest.mark.gpu

C_BAR = 2e-6       # the project's bar (test_gpu_tgemm.py, test_gpu_wgrad.py)
E_FACTOR = 4       # the kernels round at other points than torch (fp64 prefix products rounded per element)
SENTINEL = 0x7FC0DEAD  # a NaN payload no computation produces
GUARD = 1024       # sentinel elements before and after every buffer
NR_ERR_WORKSPACE = -4

# worst (|hip - f64| - E_ray) / scale measured on MI355X over all cases; test_vs_float64 prints the same
# table for the run at hand
MEASURED = {
    'neus': dict(rgb=1.7e-7, depth=2.1e-7, acc=1.2e-7, weights=1.4e-7, alpha=2.3e-7, cdf=3.2e-8, d_sdf=1.7e-7,
                 d_rad=1.1e-7, d_s=1.95e-6, d_s_sum=2.75e-6),
    'neus_bg': dict(rgb=2.2e-7, depth=1.6e-7, acc=1.2e-7, weights=1.6e-7, alpha=2.1e-7, cdf=3.8e-8, d_sdf=3.6e-7,
                    d_rad=2.1e-7, d_sigma_out=2.5e-7, d_rad_out=1.2e-7, d_s=1.71e-6, d_s_sum=2.32e-6),
    'volsdf': dict(rgb=3.4e-7, depth=3.2e-7, acc=5.1e-7, weights=2.1e-7, p_i=6.0e-8, sigma=3.2e-8, sdf_out=0.0,
                   d_sdf=1.23e-6, d_rad=3.1e-7, d_beta=1.09e-6, d_beta_sum=1.09e-6, d_sigma_bg=2.4e-7,
                   d_rad_bg=1.7e-7),
    'unisurf': dict(rgb=8.6e-8, depth=1.0e-7, acc=1.2e-7, weights=6.4e-8, alpha=6.4e-8, d_logits=2.4e-7, d_rad=7.3e-8),
}

STRUCT = {
    'neus': ['neus-R65-S65_s300-w1', 'neus-R65-S129_s20-w0'],
    'neus_bg': ['neus_bg-R65-S65_N3_s300-w1', 'neus_bg-R65-S66_N32_s20-w0'],
    'volsdf': ['volsdf-R65-S65_N3_beta0.01_use_bg1-w1', 'volsdf-R65-S65_N3_beta0.1_use_bg0-w0',
               'volsdf-R65-S64_N0_beta0.01_use_bg1-w1'],
    'unisurf': ['unisurf-R65-P97_c10-w1', 'unisurf-R65-P2_c1-w0'],
}
STRUCT_NAMES = [n for k in CC.KINDS for n in STRUCT[k]]


def bits_equal(a, b):
    if a.shape != b.shape:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Bufs:
    """outputs of one launch, each between GUARD sentinel elements and pre-filled with the sentinel"""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def new(self, *shape, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        if dtype == torch.uint8:
            buf = torch.full((2 * GUARD + n,), 0xA5, dtype=torch.uint8, device=self.dev)
        else:
            buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.int32, device=self.dev)
        self.all.append((buf, n))
        body = buf[GUARD:GUARD + n]
        return (body if dtype == torch.uint8 else body.view(torch.float32)).reshape(shape)

    def check(self, what):
        for i, (buf, n) in enumerate(self.all):
            fill = 0xA5 if buf.dtype == torch.uint8 else SENTINEL
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), \
                (what, f'buffer {i}', 'written outside')


def _shapes(c):
    """{name: shape} of every forward output and gradient of the case"""
    R = c.R
    if c.kind == 'neus':
        S = c.S
        return dict(rgb=(R, 3), depth=(R,), acc=(R,), weights=(R, S - 1), alpha=(R, S - 1), cdf=(R, S),
                    d_sdf=(R, S), d_rad=(R, S - 1, 3), d_s=(R,))
    if c.kind == 'neus_bg':
        S, M = c.S, c.S - 1 + c.N
        return dict(rgb=(R, 3), depth=(R,), acc=(R,), weights=(R, M), alpha=(R, M), cdf=(R, S), d_sdf=(R, S),
                    d_rad=(R, S - 1, 3), d_sigma_out=(R, M), d_rad_out=(R, M, 3), d_s=(R,))
    if c.kind == 'volsdf':
        S, N, M = c.S, c.N, c.S + c.N
        sh = dict(rgb=(R, 3), depth=(R,), acc=(R,), weights=(R, M - 1), p_i=(R, M - 1), sigma=(R, M), sdf_out=(R, S),
                  d_sdf=(R, S), d_rad=(R, S, 3), d_beta=(R,))
        if N:
            sh.update(d_sigma_bg=(R, N), d_rad_bg=(R, N, 3))
        return sh
    P = c.P
    return dict(rgb=(R, 3), depth=(R,), acc=(R,), weights=(R, P), alpha=(R, P), d_logits=(R, P), d_rad=(R, P, 3))


class Harness:
    def __init__(self):
        from neurecon_amd import _lib as L
        self.L, self.lib = L, L.lib()
        self.dev = torch.device('cuda:0')
        self.st = L.stream_of(self.dev)
        self._x = {}
        self.worst = {}

    def inputs(self, c):
        """the case's inputs and upstream gradients on the device (cached)"""
        if c.name not in self._x:
            CC.build(c)
            self._x[c.name] = ({k: v.to(self.dev).contiguous() for k, v in c.x.items()},
                               {k: v.to(self.dev).contiguous() for k, v in c.g.items()})
        return self._x[c.name]

    def run(self, c, null_up=(), null_out=(), ups=None, ws_delta=0, expect=0, legacy=False):
        """forward + backward of the case's kernel pair through the C ABI -> {name: tensor}.
        null_up / null_out: names passed as NULL; ups: replaces upstream gradients ({name: tensor});
        ws_delta: added to the workspace size passed; expect: the backward's return code; legacy:
        VolSDF's entry points without background arguments (N = 0)."""
        L, lib, p = self.L, self.lib, self.L.ptr
        x, g = self.inputs(c)
        g = dict(g, **(ups or {}))
        up = lambda k: None if k in null_up else p(g[k])
        B = Bufs(self.dev)
        sh = _shapes(c)
        o = {k: (None if k in null_out else B.new(*s)) for k, s in sh.items()}
        op = lambda k: None if o.get(k) is None else p(o[k])
        R, w, st = c.R, c.white, self.st

        def workspace(nbytes):
            ws = B.new(nbytes, dtype=torch.uint8)
            return ctypes.c_void_p(ws.data_ptr()), nbytes + ws_delta

        if c.kind == 'neus':
            S = c.S
            rc_f = lib.nr_neus_composite_fwd(p(x['sdf']), p(x['s']), p(x['rad']), p(x['dmid']), R, S, w, op('rgb'),
                                             op('depth'), op('acc'), op('weights'), op('alpha'), op('cdf'), st)
            ws, wb = workspace(lib.nr_neus_composite_bwd_workspace_bytes(R, S))
            rc_b = lib.nr_neus_composite_bwd(p(x['sdf']), p(x['s']), p(x['rad']), p(x['dmid']), R, S, w, up('g_rgb'),
                                             up('g_depth'), up('g_acc'), up('g_w'), op('d_sdf'), op('d_rad'), op('d_s'),
                                             ws, wb, st)
        elif c.kind == 'neus_bg':
            S, M = c.S, c.S - 1 + c.N
            a = (p(x['sdf']), p(x['s']), p(x['rad']), p(x['sigma_out']), p(x['rad_out']), p(x['d_out']), p(x['inside']),
                 R, S, M, w)
            rc_f = lib.nr_neus_composite_bg_fwd(*a, op('rgb'), op('depth'), op('acc'), op('weights'), op('alpha'),
                                                op('cdf'), st)
            ws, wb = workspace(lib.nr_neus_composite_bg_bwd_workspace_bytes(R, S, M))
            rc_b = lib.nr_neus_composite_bg_bwd(*a, up('g_rgb'), up('g_depth'), up('g_acc'), up('g_w'), op('d_sdf'),
                                                op('d_rad'), op('d_sigma_out'), op('d_rad_out'), op('d_s'), ws, wb, st)
        elif c.kind == 'volsdf':
            S, N = c.S, c.N
            a = (p(x['sdf']), p(x['pts']), p(x['beta']), p(x['rad']), p(x['d_all']), R, S, int(c.use_bg), CC.R_BG, w)
            bg = (p(x.get('sigma_bg')), p(x.get('rad_bg')), p(x.get('d_bg')), N)
            gr = (up('g_rgb'), up('g_depth'), up('g_acc'), up('g_w'), up('g_sdf'))
            fo = (op('rgb'), op('depth'), op('acc'), op('weights'), op('p_i'), op('sigma'), op('sdf_out'))
            if legacy:
                assert N == 0
                rc_f = lib.nr_volsdf_composite_fwd(*a, *fo, st)
                ws, wb = workspace(lib.nr_volsdf_composite_bwd_workspace_bytes(R, S))
                rc_b = lib.nr_volsdf_composite_bwd(*a, *gr, op('d_sdf'), op('d_rad'), op('d_beta'), ws, wb, st)
            else:
                rc_f = lib.nr_volsdf_composite_bg_fwd(*a, *bg, *fo, st)
                ws, wb = workspace(lib.nr_volsdf_composite_bg_bwd_workspace_bytes(R, S, N))
                rc_b = lib.nr_volsdf_composite_bg_bwd(*a, *bg, *gr, op('d_sdf'), op('d_rad'), op('d_beta'),
                                                      op('d_sigma_bg'), op('d_rad_bg'), ws, wb, st)
        else:
            P = c.P
            a = (p(x['logits']), p(x['rad']), p(x['d_all']), R, P, w)
            rc_f = lib.nr_unisurf_composite_fwd(*a, op('rgb'), op('depth'), op('acc'), op('weights'), op('alpha'), st)
            ws, wb = workspace(lib.nr_unisurf_composite_bwd_workspace_bytes(R, P))
            rc_b = lib.nr_unisurf_composite_bwd(*a, up('g_rgb'), up('g_depth'), up('g_acc'), up('g_w'), op('d_logits'),
                                                op('d_rad'), ws, wb, st)
        torch.cuda.synchronize()
        assert rc_f == 0, (c, 'forward', rc_f, lib.nr_last_error().decode())
        assert rc_b == expect, (c, 'backward', rc_b, lib.nr_last_error().decode())
        B.check(c.name)
        return {k: v.clone() for k, v in o.items() if v is not None}


@pytest.fixture(scope='module')
def h():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return Harness()


def _same(c, got, ref, what, keys=None):
    for k in (ref if keys is None else keys):
        assert k in got, (c, what, k)
        assert bits_equal(got[k], ref[k]), \
            (c, what, k, float((got[k] - ref[k]).abs().nan_to_num(float('inf')).max()) if got[k].numel() else 0.0)


def _accuracy(h, c, got, tag):
    """check 1 on one case; records the worst excess per (kind, tensor)"""
    for k, (t32, t64, E, scale) in CC.tensors(c).items():
        if k.endswith('.sum'):
            g = got[k[:-4]].sum().reshape(1)          # the wrapper's host-side sum, fp32 on the device
        else:
            g = got[k]
        g = g.cpu().double().reshape(t64.shape)
        err = (g - t64).abs()
        Eb = E.reshape(-1, *([1] * (t64.dim() - 1))).expand_as(t64) if t64.dim() else E
        ok = err <= E_FACTOR * Eb + C_BAR * scale
        if scale > 0 and t64.numel():
            excess = float(((err - Eb) / scale).nan_to_num(float('inf')).max())
            key = (c.kind, k)
            if excess > h.worst.get(key, (-1.0, ''))[0]:
                h.worst[key] = (excess, c.name)
        if not bool(ok.all()):
            i = int((err - E_FACTOR * Eb - C_BAR * scale).nan_to_num(float('inf')).reshape(-1).argmax())
            raise AssertionError(f'{tag} {c} {k}: element {i} of shape {tuple(t64.shape)}: hip {float(g.reshape(-1)[i])!r} '
                                 f'f64 {float(t64.reshape(-1)[i])!r} fp32 {float(t32.reshape(-1)[i])!r} '
                                 f'E_ray {float(Eb.reshape(-1)[i]):.3e} scale {scale:.3e}; '
                                 f'{int((~ok).sum())} of {ok.numel()} elements over the bar')


def _report(h, kind):
    rows = {k[1]: v for k, v in h.worst.items() if k[0] == kind}
    print(f'{kind}: worst (|hip - f64| - E_ray) / scale so far: ' +
          ', '.join(f'{k} {v[0]:.2e} ({v[1]})' for k, v in sorted(rows.items())))


GROUPS = [('neus', dict(S=S)) for S in CC.NEUS_S] + [('neus_bg', dict(S=S, N=N)) for S, N in CC.NEUS_BG_SN] + \
    [('volsdf', dict(S=S, N=N)) for S, N in CC.VOLSDF_SN] + [('unisurf', dict(P=P)) for P in CC.UNI_P]


@pytest.mark.parametrize('kind,match', GROUPS, ids=[f'{k}-' + '_'.join(f'{a}{b}' for a, b in m.items())
                                                    for k, m in GROUPS])
def test_vs_float64(h, kind, match):
    """check 1 over every R, scalar (s / beta / c), use_bg and white_bkgd of one shape"""
    cases = CC.cases_of(kind, **match)
    assert len(cases) in (16, 24, 32), len(cases)
    for c in cases:
        _accuracy(h, c, h.run(c), 'vs float64')
    _report(h, kind)


@pytest.mark.parametrize('name', [c.name for c in CC.cases_of('volsdf', N=0, R=65)])
def test_volsdf_entry_points_without_background_arguments(h, name):
    """nr_volsdf_composite_fwd / _bwd are the _bg_ entry points with N = 0: same bits"""
    c = CC.BY_NAME[name]
    _same(c, h.run(c, legacy=True), h.run(c), 'legacy entry points')


@pytest.mark.parametrize('name', STRUCT_NAMES)
def test_null_upstream_gradients(h, name):
    """check 2, each pointer alone and all of them together (every gradient is then 0 or, for VolSDF's
    d_rad rows and the NeuS colour gradients, the zero-g_rgb product)"""
    c = CC.BY_NAME[name]
    _, g = h.inputs(c)
    names = CC.UPSTREAM[c.kind]
    full = h.run(c)
    for sel in [(k,) for k in names] + [names]:
        zero = h.run(c, ups={k: torch.zeros_like(g[k]) for k in sel})
        null = h.run(c, null_up=sel)
        _same(c, null, zero, f'NULL {sel} vs zeros')
        if len(sel) == 1:  # and the pointer matters: a zero tensor is not the case's gradient
            assert any(not bits_equal(full[k], zero[k]) for k in CC.GRADS[c.kind] if k in full), (c, sel)


@pytest.mark.parametrize('name', STRUCT_NAMES)
def test_null_optional_outputs(h, name):
    """check 3, each optional output alone and all together"""
    c = CC.BY_NAME[name]
    full = h.run(c)
    opt = CC.OPTIONAL_OUTS[c.kind]
    for sel in [(k,) for k in opt] + [opt]:
        got = h.run(c, null_out=sel)
        assert not any(k in got for k in sel)
        _same(c, got, full, f'NULL outputs {sel}', [k for k in full if k not in sel])


@pytest.mark.parametrize('name', STRUCT_NAMES)
def test_workspace_one_byte_short(h, name):
    """check 4: NR_ERR_WORKSPACE before any launch -- the gradients keep their sentinel fill"""
    c = CC.BY_NAME[name]
    got = h.run(c, ws_delta=-1, expect=NR_ERR_WORKSPACE)
    for k in CC.GRADS[c.kind]:
        if k in got and got[k].numel():
            assert bool((got[k].contiguous().view(torch.int32) == SENTINEL).all()), (c, k)


@pytest.mark.parametrize('name', STRUCT_NAMES)
def test_repeatable(h, name):
    """check 5"""
    c = CC.BY_NAME[name]
    _same(c, h.run(c), h.run(c), 'second launch')


@pytest.mark.parametrize('name', [c.name for c in CC.cases_of('volsdf', R=65) if c.use_bg or c.N == 0])
def test_volsdf_masking(h, name):
    """check 6: no gradient reaches the network's sdf where the background value was taken -- neither
    through sigma nor the direct g_sdf term -- and the rows past the composited samples are 0"""
    c = CC.BY_NAME[name]
    x, g = h.inputs(c)
    got = h.run(c)
    S, N = c.S, c.N
    taken = got['sdf_out'] != x['sdf']
    (o32, _), _ = CC.reference(c)
    assert torch.equal(taken.cpu(), o32['sdf_out'] != c.x['sdf']), c
    if c.use_bg:
        assert 0 < int(taken.sum()) < taken.numel(), c
        assert bool((g['g_sdf'][taken] != 0).all()), c
        assert bool((got['d_sdf'][taken] == 0).all()), (c, float(got['d_sdf'][taken].abs().max()))
    else:
        assert not bool(taken.any()), c
    assert bool((got['d_sdf'][~taken] != 0).all()), c   # g_sdf alone makes them non-zero
    if N == 0:
        assert bool((got['d_rad'][:, S - 1:] == 0).all()) and bool((got['d_rad'][:, :S - 1] != 0).any()), c
    else:
        assert bool((got['d_rad_bg'][:, N - 1:] == 0).all()) and bool((got['d_sigma_bg'][:, N - 1:] == 0).all()), c
        assert bool((got['d_rad'][:, S - 1] != 0).any()), c   # the handover interval carries the last inner colour


@pytest.mark.parametrize('name', [c.name for c in CC.cases_of('neus_bg', R=65)])
def test_neus_bg_masking(h, name):
    """check 6: each mid-point's colour gradient goes to exactly one of the two nets, and the background
    sigma of an inside mid-point gets none"""
    c = CC.BY_NAME[name]
    x, _ = h.inputs(c)
    got = h.run(c)
    S1 = c.S - 1
    ins = x['inside'].bool()
    assert bool(ins[0].all()) and not bool(ins[1].any()), c
    assert bool((got['d_rad'][~ins] == 0).all()), c
    assert bool((got['d_rad_out'][:, :S1][ins] == 0).all()) and bool((got['d_sigma_out'][:, :S1][ins] == 0).all()), c
    assert bool((got['d_rad'][ins] != 0).any()) and bool((got['d_rad_out'][:, :S1][~ins] != 0).any()), c
    assert bool((got['d_sigma_out'][:, :S1][~ins] != 0).any()) and bool((got['d_rad_out'][:, S1:] != 0).any()), c


def _view(t, how):
    """t's values as a non-contiguous view"""
    if how == 'slice':      # columns 1 .. of a wider buffer
        wide = torch.full((*t.shape[:-1], t.shape[-1] + 2), 7, dtype=t.dtype, device=t.device)
        wide[..., 1:-1] = t
        v = wide[..., 1:-1]
    else:                   # the transpose of the transposed copy
        v = t.transpose(0, 1).contiguous().transpose(0, 1)
    assert torch.equal(v, t) and (not v.is_contiguous() or t.shape[0] == 1 or t.numel() == t.shape[0])
    return v


@pytest.mark.parametrize('views', [False, True], ids=['contiguous', 'views'])
@pytest.mark.parametrize('name', STRUCT_NAMES)
def test_wrapper_vs_direct_call(h, name, views):
    """check 7: training.py's autograd Functions against the direct calls, bit for bit; views: the
    no-grad inputs (d_mid, d_out, inside, pts, d_all, d_bg) as a sliced / a transposed view"""
    from neurecon_amd import training as T
    c = CC.BY_NAME[name]
    x, g = h.inputs(c)
    ref = h.run(c)
    leaf = lambda k: x[k].clone().requires_grad_(True)
    nv = (lambda t, how: _view(t, how)) if views else (lambda t, how: t)
    if c.kind == 'neus':
        ins = dict(sdf=leaf('sdf'), s=leaf('s'), rad=leaf('rad'))
        out = T.NeuSComposite.apply(ins['sdf'], ins['s'], ins['rad'], nv(x['dmid'], 'slice'), bool(c.white))
        names = ('rgb', 'depth', 'acc', 'weights', 'alpha', 'cdf')
        gmap = dict(d_sdf='sdf', d_rad='rad', d_s='s')
    elif c.kind == 'neus_bg':
        ins = dict(sdf=leaf('sdf'), s=leaf('s'), rad=leaf('rad'), sigma_out=leaf('sigma_out'), rad_out=leaf('rad_out'))
        out = T.NeuSCompositeBG.apply(ins['sdf'], ins['s'], ins['rad'], ins['sigma_out'], ins['rad_out'],
                                      nv(x['d_out'], 'slice'), nv(x['inside'], 'transpose'), bool(c.white))
        names = ('rgb', 'depth', 'acc', 'weights', 'alpha', 'cdf')
        gmap = dict(d_sdf='sdf', d_rad='rad', d_sigma_out='sigma_out', d_rad_out='rad_out', d_s='s')
    elif c.kind == 'volsdf':
        ins = dict(sdf=leaf('sdf'), beta=leaf('beta'), rad=leaf('rad'))
        bg = ()
        gmap = dict(d_sdf='sdf', d_rad='rad', d_beta='beta')
        if c.N:
            ins.update(sigma_bg=leaf('sigma_bg'), rad_bg=leaf('rad_bg'))
            bg = (ins['sigma_bg'], ins['rad_bg'], nv(x['d_bg'], 'slice'))
            gmap.update(d_sigma_bg='sigma_bg', d_rad_bg='rad_bg')
        out = T.VolSDFComposite.apply(ins['sdf'], ins['beta'], ins['rad'], nv(x['pts'], 'transpose'),
                                      nv(x['d_all'], 'slice'), bool(c.use_bg), CC.R_BG, bool(c.white), *bg)
        names = ('rgb', 'depth', 'acc', 'weights', 'sdf_out', 'p_i', 'sigma')
    else:
        ins = dict(logits=leaf('logits'), rad=leaf('rad'))
        out = T.UnisurfComposite.apply(ins['logits'], ins['rad'], nv(x['d_all'], 'slice'), bool(c.white))
        names = ('rgb', 'depth', 'acc', 'weights', 'alpha')
        gmap = dict(d_logits='logits', d_rad='rad')
    o = dict(zip(names, out))
    loss = (o['rgb'] * g['g_rgb']).sum() + (o['depth'] * g['g_depth']).sum() + (o['acc'] * g['g_acc']).sum() + \
        (o['weights'] * g['g_w']).sum()
    if c.kind == 'volsdf':
        loss = loss + (o['sdf_out'] * g['g_sdf']).sum()
    loss.backward()
    torch.cuda.synchronize()
    _same(c, {k: v.detach() for k, v in o.items()}, ref, 'wrapper forward', names)
    got = {k: ins[v].grad for k, v in gmap.items()}
    ref = dict(ref)
    for k in ('d_s', 'd_beta'):
        if k in ref:
            ref[k] = ref[k].sum().reshape(1)
    _same(c, got, ref, 'wrapper backward', list(gmap))


# ---- the background net's inputs ---------------------------------------------------------------------
def _embed_bar(name, got, r32, r64, R):
    """|hip - f64| <= 4 E_ray + 2e-6 scale per element, a ray = its M points' features"""
    g = got.cpu().double()
    err = (g - r64).abs().reshape(R, -1)
    E = (r32.double() - r64).abs().reshape(R, -1).amax(1, keepdim=True)
    scale = float(r64.abs().max())
    nf = r64.shape[-1]
    band = (err.reshape(-1, nf).amax(0) / scale)
    print(f'{name}: worst (|hip - f64| - E_ray) / scale {float(((err - E) / scale).max()):.2e}; max |hip - f64| '
          f'{float(err.max()):.2e}, max |fp32 - f64| {float(E.max()):.2e}; top band (last 8 features) '
          f'{float(band[-8:].max()):.2e}, identity features {float(band[:3].max()):.2e}')
    assert bool((err <= E_FACTOR * E + C_BAR * scale).all()), name
    return float(((err - E) / scale).max())


@pytest.mark.parametrize('R', CC.EMB_R)
@pytest.mark.parametrize('M,n_mid', CC.EMB_MN)
def test_nerf_train_input(h, R, M, n_mid):
    """check 8 for NeuS: x_emb = embed([p / |p|, 1 / |p|], 10), v_emb = embed(dir, 4), inside = |p| <= r_obj
    at the first n_mid depths.  The last band's sin / cos arguments are 2^9 x with |x| <= 1: an fp32 ulp
    of x is 3e-5 of argument, so both the kernel and the fp32 reference sit 1e-5 - 3e-5 from float64 there
    (printed per run) and 1e-7 on the identity features; the bar follows E_ray."""
    L, lib, p = h.L, h.lib, h.L.ptr
    o, d, depth = CC.embed_inputs(R, M, 100 + R + M)
    B = Bufs(h.dev)
    x_emb, v_emb = B.new(R * M, 84), B.new(R * M, 27)
    inside = B.new(R, n_mid, dtype=torch.uint8)
    og, dg, tg = o.to(h.dev), d.to(h.dev), depth.to(h.dev)
    rc = lib.nr_nerf_train_input(p(og), p(dg), p(tg), R, M, n_mid, CC.R_OBJ, p(x_emb), p(v_emb),
                                 ctypes.c_void_p(inside.data_ptr() if n_mid else B.all[-1][0].data_ptr() + GUARD),
                                 h.st)
    torch.cuda.synchronize()
    assert rc == 0, lib.nr_last_error().decode()
    B.check('nr_nerf_train_input')
    x32, v32, n32 = CC.embed_reference(o, d, depth, None, torch.float32)
    x64, v64, n64 = CC.embed_reference(o, d, depth, None, torch.float64)
    _embed_bar(f'x_emb R={R} M={M}', x_emb, x32, x64, R)
    _embed_bar(f'v_emb R={R} M={M}', v_emb, v32, v64, R)
    if n_mid:
        near = (n64[:, :n_mid] - CC.R_OBJ).abs() < 1e-6
        assert float(near.double().mean()) <= 0.01
        want = (n32[:, :n_mid] <= CC.R_OBJ)
        assert bool((inside.cpu().bool() == want)[~near].all())
        if M > 3:
            assert 0 < int(want.sum()) < want.numel()   # points on both sides of the sphere


@pytest.mark.parametrize('R', CC.EMB_R)
@pytest.mark.parametrize('N', sorted({m for m, _ in CC.EMB_MN}))
def test_volsdf_nerf_input(h, R, N):
    """check 8 for VolSDF: x_emb = embed([p / rs, 1 / rs], 10) at the given radii rs, v_emb = embed(dir, 4)"""
    lib, p = h.lib, h.L.ptr
    o, d, depth = CC.embed_inputs(R, N, 200 + R + N)
    rs = (o[:, None, :] + d[:, None, :] * depth[..., None]).norm(dim=-1).contiguous()
    B = Bufs(h.dev)
    x_emb, v_emb = B.new(R * N, 84), B.new(R * N, 27)
    og, dg, tg, rg = o.to(h.dev), d.to(h.dev), depth.to(h.dev), rs.to(h.dev)
    rc = lib.nr_volsdf_nerf_input(p(og), p(dg), p(tg), p(rg), R, N, p(x_emb), p(v_emb), h.st)
    torch.cuda.synchronize()
    assert rc == 0, lib.nr_last_error().decode()
    B.check('nr_volsdf_nerf_input')
    x32, v32, _ = CC.embed_reference(o, d, depth, rs, torch.float32)
    x64, v64, _ = CC.embed_reference(o, d, depth, rs, torch.float64)
    _embed_bar(f'x_emb R={R} N={N}', x_emb, x32, x64, R)
    _embed_bar(f'v_emb R={R} N={N}', v_emb, v32, v64, R)
