"""The training step's element-wise kernels (csrc/nr_train.hip) call by call through the C ABI: nr_embed,
nr_embed_padded, nr_embed_jvp, nr_embed_jvp_padded, nr_embed_vjp, nr_softplus100, nr_softplus_adjoint,
nr_sine30, nr_sine_adjoint, nr_scale_cols, nr_mul, nr_activation, nr_colsum and nr_radiance_input.  The
end-to-end training tests reach them at one net shape behind eight GEMMs; here each is held to its own
formula at the sizes where its code takes another path.

Cases (tests/train_ops_ref.py; their conditions are held on the CPU by tests/test_train_ops_ref.py):
embedding kernels P in {1, 3, 4, 5, 8193} (a wave per point, 4 per block, the grid capped at 2048 blocks:
8193 is the first size with a second grid-stride trip) x nfreq in {-1, 0, 4, 6, 10} x ldo in {nf, 64, 80,
128} (ldo > 64: the lane loop's second trip), points in [-3, 3] with 0.0, -0.0, +-1e-4, +-3, +-8 and the
floats nearest k pi / 2^b among them; nr_embed_vjp with ld0, ld1 in {nf, 64, 70}^2, e1 NULL or present, s1
in {1, 1/sqrt(2), -0.37}, and one case per column group with e0 zero outside it; the one-thread-per-element
kernels at n in {1, 255, 256, 257, 1000} and P in {1, 7, 130} x n in {1, 39, 256, 257} with ldh in {n, n + 3},
with and without g / zdot, s NULL and present, scale in {1, 1/sqrt(2)}, an interior column range;
nr_softplus100 on t = 100 z dense over [-120, 40] with the neighbours of 0.2f; nr_sine30 on |z| <= 10;
nr_colsum at P in {0, 1, 7, 1023, 1024, 1025, 8192, 8193, 16385} (1024 slabs of ceil(P / 1024) rows, rows
unrolled by 8) x n in {1, 63, 64, 65, 257} (64 columns per block of the final pass); nr_radiance_input with
use_view_dirs in {0, 1} x nfreq_view in {-1, 4, 10} x wfeat in {0, 5, 256} x P in {1, 130}.

  a. bit-exact: nr_mul, nr_scale_cols, the two adjoints, nr_activation modes 0, 1 and 3 equal the fp32
     replica of train_ops_ref.py (the same single IEEE operations in the kernel's order) bit for bit; the
     identity columns of nr_embed* are copies of x / v, the padding columns +0.0; every copied column of
     nr_radiance_input, and its view embedding equals nr_embed of v.  nr_softplus100 where fp32 z * 100 > 20:
     h has z's bits and s is exactly 1.0.  Catches: a wrong operand, factor or association in any term, a
     wrong column offset (col0, the strides ldh / lda / ldo), a stale value in a padding column, relu's
     and the ReLU mask's treatment of -0.0 and of the smallest normals.
  b. against float64: the sin / cos columns of nr_embed*, nr_embed_vjp, nr_softplus100 (t <= 20),
     nr_sine30, nr_activation mode 2 and nr_colsum on heavy-tailed input; |hip - f64| <= 4 E + 2e-6 scale,
     E = the fp32 CPU reference's worst |fp32 - f64| over the row's elements of the column group, scale =
     the max |f64| of the COLUMN GROUP (the three identity columns, each band's six columns; the whole
     output for vjp), so the 2^9 band of the jvp, 512 times band 0, does not hide band 0.  The heavy-tailed
     column sum: |hip - f64| <= 2e-6 sum_r |a_rc| (about 31 roundings of at most 2^-24 of the running
     magnitude: a worst-case bound).  The integer-valued column sums equal the int64 sum exactly, so a
     dropped, doubled or misplaced row shows whatever the tolerance.  Catches: a wrong factor, sign or
     band index in the embedding's Jacobian (the single-band vjp cases: a low band cannot hide behind
     the 2^9 one), a row lost at a slab edge or at the unroll's tail, a block tail, the grid-stride trip.
  c. nothing written outside: every output, and nr_colsum's workspace at exactly
     nr_colsum_workspace_bytes(n), lies between sentinels checked after every launch; one byte less of
     workspace returns NR_ERR_WORKSPACE and writes nothing; the gap columns of a strided hbar (ldh > n) and
     of e0 / e1 (ld > nf) hold NaN and must not reach the output.
  d. the same launch twice is bit-identical (nr_embed_vjp's butterfly, nr_colsum's two passes).
  e. optional pointers: e1 NULL equals e1 all zeros bit for bit (e0 holds -0.0: a lane's e0 + 0 s1 loses the
     sign, but every lane adds into +0.0); s NULL in nr_scale_cols equals s all ones bit for bit; g / zdot
     NULL in the two adjoints equals g all zeros in value, bit for bit wherever zbar != 0, and up to the
     sign of zero elsewhere: a zero g gives hbar s + (+-0.0), which is -0.0 only where hbar s = -0.0 and the
     zero term is negative (zdot < 0, or h > 0 for the sine); NULL gives +0.0 on every zero.
  f. the helpers of training.py (_embed, _softplus, _sine30, _cols, _mul, _colsum) give the direct call's
     bits on contiguous input, and on a column slice or a transpose the bits of the contiguous copy.

Found with these tests and fixed: nr_embed_vjp took any ld0 / ld1 (a stride below the feature count read
the next point's row: now NR_ERR_ARG; tests/test_capi.py); _embed, _softplus, _sine30, _cols and _mul
handed raw pointers of non-contiguous tensors on with shape[1] / numel() (now copied); the two adjoints
with g NULL gave -0.0 where hbar s = -0.0 and a zero g with zdot > 0 gives +0.0 (now hbar s + 0.0).

Measured on MI355X: MEASURED below, the worst (|hip - f64| - E) / scale per entry point and column group
(DESIGN.md section 3 has the same table); the module's teardown prints the table of the run at hand."""
import ctypes

import pytest
import torch

import train_ops_ref as R

pytestmark = pytest.mark.gpu

C_BAR = 2e-6       # the project's bar (test_gpu_composite.py, test_gpu_tgemm.py, test_gpu_wgrad.py)
E_FACTOR = 4
COLSUM_BAR = 2e-6  # of sum_r |a_rc|
SENTINEL = 0x7FC0DEAD  # a NaN payload no computation produces
GUARD = 1024       # sentinel elements before and after every buffer
NR_ERR_ARG, NR_ERR_WORKSPACE = -1, -4
F32, F64 = torch.float32, torch.float64

# worst (|hip - f64| - E) / scale measured on MI355X over all cases, per entry point and column group
# (bands: band 0 .. band nfreq-1 of the widest embedding); nr_colsum: worst |hip - f64| / sum_r |a_rc|.
# nr_embed / nr_embed_jvp are bit-identical to the padded entry points at ldo = nf.
MEASURED = {
    'nr_activation': {'sigmoid': 9.8e-09},
    'nr_colsum': {'heavy': 1.1e-07},
    'nr_embed_jvp_padded': {'band0': 6e-08, 'band1': 5.9e-08, 'band2': 6e-08, 'band3': 6e-08, 'band4': 6e-08,
                            'band5': 6e-08, 'band6': 6e-08, 'band7': 6e-08, 'band8': 6e-08, 'band9': 6e-08,
                            'identity': 0.0},
    'nr_embed_padded': {'band0': 4.6e-08, 'band1': 6e-08, 'band2': 4.8e-08, 'band3': 5.1e-08, 'band4': 5.4e-08,
                        'band5': 5e-08, 'band6': 4.7e-08, 'band7': 5.5e-08, 'band8': 4.8e-08, 'band9': 4.6e-08,
                        'identity': 0.0},
    'nr_embed_vjp': {'all': 1.9e-07},
    'nr_embed_vjp.single': {'band0': 3.8e-08, 'band1': 4.2e-08, 'band2': 3.9e-08, 'band3': 4e-08, 'band4': 3.6e-08,
                            'band5': 3.6e-08, 'band6': 3.9e-08, 'band7': 3.6e-08, 'band8': 4.5e-08, 'band9': 4.1e-08,
                            'identity': 0.0},
    'nr_radiance_input': {'view.band0': 3.4e-08, 'view.band1': 3.4e-08, 'view.band2': 4e-08, 'view.band3': 3.6e-08,
                          'view.band4': 2.9e-08, 'view.band5': 3.4e-08, 'view.band6': 4.2e-08, 'view.band7': 2.9e-08,
                          'view.band8': 3.4e-08, 'view.band9': 3.6e-08, 'view.identity': 0.0},
    'nr_sine30': {'h': 6e-08, 's': 6.4e-08},
    'nr_softplus100': {'h': 1.9e-08, 's': 4.8e-08},
}


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

    def new(self, *shape, dtype=F32):
        n = 1
        for s in shape:
            n *= s
        if dtype == torch.uint8:
            buf = torch.full((2 * GUARD + n,), 0xA5, dtype=torch.uint8, device=self.dev)
        else:
            buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.int32, device=self.dev)
        self.all.append((buf, n))
        body = buf[GUARD:GUARD + n]
        return (body if dtype == torch.uint8 else body.view(F32)).reshape(shape)

    def check(self, what):
        for i, (buf, n) in enumerate(self.all):
            fill = 0xA5 if buf.dtype == torch.uint8 else SENTINEL
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), \
                (what, f'buffer {i}', 'written outside')

    def untouched(self, t):
        return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


class Harness:
    def __init__(self):
        from neurecon_amd import _lib as L
        self.L, self.lib, self.p = L, L.lib(), L.ptr
        self.dev = torch.device('cuda:0')
        self.st = L.stream_of(self.dev)
        self.worst = {}

    def up(self, t):
        return None if t is None else t.to(self.dev).contiguous()

    def launch(self, name, what, B, *args, expect=0):
        rc = getattr(self.lib, name)(*args, self.st)
        torch.cuda.synchronize()
        assert rc == expect, (name, what, rc, self.lib.nr_last_error().decode())
        B.check((name, what))

    def twice(self, name, what, shapes, args):
        """the launch into fresh sentinel-guarded outputs, twice: args(outs) -> the argument tuple; returns
        the first launch's outputs on the CPU after checking that the second gave the same bits"""
        res = []
        for _ in range(2):
            B = Bufs(self.dev)
            outs = [B.new(*s) for s in shapes]
            self.launch(name, what, B, *args(outs))
            res.append([o.clone() for o in outs])
        for a, b in zip(*res):
            assert bits_equal(a, b), (name, what, 'not deterministic')
        return [o.cpu() for o in res[0]]

    def bar(self, entry, group, hip, r32, r64, what):
        """check b on [rows, cols] CPU tensors; records the worst excess before asserting"""
        if r64.numel() == 0:
            return
        hip, r32 = hip.double(), r32.double()
        err = (hip - r64).abs()
        E = (r32 - r64).abs().amax(1, keepdim=True)
        scale = float(r64.abs().max())
        worst = float((err - E).nan_to_num(float('inf')).max())
        excess = worst / scale if scale > 0 else (0.0 if worst <= 0 else float('inf'))
        key = (entry, group)
        self.worst[key] = max(self.worst.get(key, -1.0), excess)
        ok = err <= E_FACTOR * E + C_BAR * scale
        assert bool(ok.all()), (entry, group, what, f'excess {excess:.3e} of scale {scale:.3e}',
                                f'worst |hip - f64| {float(err.nan_to_num(float("inf")).max()):.3e}, E {float(E.max()):.3e}')


@pytest.fixture(scope='module')
def h():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    hh = Harness()
    yield hh
    table = {}   # this run's table, in MEASURED's layout
    for (e, g), v in sorted(hh.worst.items()):
        table.setdefault(e, {})[g] = float(f'{v:.2g}')
    for e, row in table.items():
        print(f"    '{e}': {row},")


def _copies(out, copies, what):
    for sl, val in copies:
        assert bits_equal(out[:, sl], val), (what, 'columns', sl.start, sl.stop, 'not the copy')


# ---- the embedding kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize('jvp', [False, True], ids=['embed', 'jvp'])
@pytest.mark.parametrize('P', R.EMBED_P)
def test_embed(h, P, jvp):
    p = h.p
    x, v = R.points(P)
    xd, vd = h.up(x), h.up(v)
    entry = 'nr_embed_jvp_padded' if jvp else 'nr_embed_padded'
    for _, nfreq, ldo in [c for c in R.embed_cases() if c[0] == P]:
        what = (P, nfreq, ldo)
        nf = R.nfeat(nfreq)
        pre = (p(xd), p(vd)) if jvp else (p(xd),)
        out, = h.twice(entry, what, [(P, ldo)], lambda o: (*pre, P, nfreq, p(o[0]), ldo))
        if ldo == nf:   # the unpadded entry points are the padded ones at ldo = nf
            dense, = h.twice(entry.replace('_padded', ''), what, [(P, nf)], lambda o: (*pre, P, nfreq, p(o[0])))
            assert bits_equal(dense, out), (what, 'unpadded entry point')
        _copies(out, R.embed_copy_replica(v if jvp else x, nfreq, ldo), what)
        ref = R.embed_jvp_ref if jvp else R.embed_ref
        a = (x, v, nfreq) if jvp else (x, nfreq)
        r32, r64 = ref(*a, F32), ref(*a, F64)
        for g, sl in R.groups(nfreq):
            h.bar(entry, g, out[:, sl], r32[:, sl], r64[:, sl], what)


def _vjp(h, x, e0, ld0, e1, ld1, s1, P, nfreq, what):
    p = h.p
    xd, e0d, e1d = h.up(x), h.up(e0), h.up(e1)
    out, = h.twice('nr_embed_vjp', what, [(P, 3)],
                   lambda o: (p(xd), p(e0d), ld0, p(e1d), ld1, 1.0 if s1 is None else s1, P, nfreq, p(o[0])))
    return out


@pytest.mark.parametrize('P', R.EMBED_P)
def test_embed_vjp(h, P):
    for i, (_, nfreq, ld0, ld1, s1) in enumerate(c for c in R.vjp_cases() if c[0] == P):
        what = (P, nfreq, ld0, ld1, s1)
        nf = R.nfeat(nfreq)
        x, e0, e1 = R.vjp_inputs(P, nfreq, ld0, ld1, s1, seed=i)
        out = _vjp(h, x, e0, ld0, e1, ld1, s1, P, nfreq, what)
        a = (x, e0[:, :nf], None if e1 is None else e1[:, :nf], s1, nfreq)
        h.bar('nr_embed_vjp', 'all', out, R.embed_vjp_ref(*a, F32), R.embed_vjp_ref(*a, F64), what)


@pytest.mark.parametrize('band', R.VJP_BANDS, ids=str)
def test_embed_vjp_single_band(h, band):
    """e0 non-zero in one column group only: the output's scale is that band's, a wrong factor in a low
    band cannot hide behind the 2^9 band"""
    P, nfreq = R.VJP_BAND_P, R.VJP_BAND_NFREQ
    nf = R.nfeat(nfreq)
    x, e0, _ = R.vjp_inputs(P, nfreq, 64, 64, None, band=band, seed=7)
    out = _vjp(h, x, e0, 64, None, 64, None, P, nfreq, ('band', band))
    a = (x, e0[:, :nf], None, None, nfreq)
    g = 'identity' if band == 'identity' else f'band{band}'
    h.bar('nr_embed_vjp.single', g, out, R.embed_vjp_ref(*a, F32), R.embed_vjp_ref(*a, F64), band)


# ---- one thread per element: flat -----------------------------------------------------------------
def _flat_z(n, seed, lo, hi):
    return (lo + (hi - lo) * torch.rand(n, generator=torch.Generator().manual_seed(seed), dtype=F64)).float()


def _softplus_check(h, z, what):
    p = h.p
    n = z.numel()
    zd = h.up(z)
    hh, ss = h.twice('nr_softplus100', what, [(n,), (n,)], lambda o: (p(zd), n, p(o[0]), p(o[1])))
    lin = z * 100.0 > 20.0   # fp32, the kernel's own product
    assert bits_equal(hh[lin], z[lin]), (what, 'h on the linear branch is not z')
    assert bits_equal(ss[lin], torch.ones(int(lin.sum()))), (what, 's on the linear branch is not 1.0')
    (h32, s32), (h64, s64) = R.softplus100_ref(z, F32), R.softplus100_ref(z, F64)
    sm = ~lin
    h.bar('nr_softplus100', 'h', hh[sm].reshape(-1, 1), h32[sm].reshape(-1, 1), h64[sm].reshape(-1, 1), what)
    h.bar('nr_softplus100', 's', ss[sm].reshape(-1, 1), s32[sm].reshape(-1, 1), s64[sm].reshape(-1, 1), what)
    return int(lin.sum())


def test_softplus100(h):
    z = R.softplus_sweep()
    nlin = _softplus_check(h, z, 'sweep')
    assert 0 < nlin < z.numel()
    for n in R.FLAT_N:
        _softplus_check(h, _flat_z(n, n, -1.2, 0.4), n)


def _sine_check(h, z, what):
    p = h.p
    n = z.numel()
    zd = h.up(z)
    hh, ss = h.twice('nr_sine30', what, [(n,), (n,)], lambda o: (p(zd), n, p(o[0]), p(o[1])))
    (h32, s32), (h64, s64) = R.sine30_ref(z, F32), R.sine30_ref(z, F64)
    h.bar('nr_sine30', 'h', hh.reshape(-1, 1), h32.reshape(-1, 1), h64.reshape(-1, 1), what)
    h.bar('nr_sine30', 's', ss.reshape(-1, 1), s32.reshape(-1, 1), s64.reshape(-1, 1), what)


def test_sine30(h):
    _sine_check(h, R.sine_sweep(), 'sweep')
    for n in R.FLAT_N:
        _sine_check(h, _flat_z(n, n, -10.0, 10.0), n)


@pytest.mark.parametrize('n', R.FLAT_N)
def test_mul(h, n):
    p = h.p
    a, b = R.mag((n,), n), R.mag((n,), n + 1)
    ad, bd = h.up(a), h.up(b)
    out, = h.twice('nr_mul', n, [(n,)], lambda o: (p(ad), p(bd), n, p(o[0])))
    assert bits_equal(out, R.mul_replica(a, b)), n


def _activation(h, y, g, mode, what):
    """nr_activation in place on copies of y / g between sentinels -> (y, g) after the launch"""
    p = h.p
    n = y.numel()
    res = []
    for _ in range(2):
        B = Bufs(h.dev)
        yb = B.new(n)
        yb.copy_(y)
        gb = None
        if g is not None:
            gb = B.new(n)
            gb.copy_(g)
        h.launch('nr_activation', what, B, p(yb), p(gb), n, mode)
        res.append((yb.cpu(), None if gb is None else gb.cpu()))
    assert bits_equal(res[0][0], res[1][0]) and (g is None or bits_equal(res[0][1], res[1][1])), (what, 'not deterministic')
    return res[0]


@pytest.mark.parametrize('n', R.FLAT_N)
def test_activation(h, n):
    y, g = R.relu_inputs(n, n)
    y0, _ = _activation(h, y, None, 0, (n, 0))
    assert bits_equal(y0, R.activation_replica(y, None, 0)), (n, 'relu')
    y1, g1 = _activation(h, y, g, 1, (n, 1))
    assert bits_equal(y1, y), (n, 'mode 1 changed y')
    assert bits_equal(g1, R.activation_replica(y, g, 1)), (n, 'relu mask')
    ys, gs = R.unit((n,), n + 5), R.mag((n,), n + 6)
    y3, g3 = _activation(h, ys, gs, 3, (n, 3))
    assert bits_equal(y3, ys), (n, 'mode 3 changed y')
    assert bits_equal(g3, R.activation_replica(ys, gs, 3)), (n, 'sigmoid backward')
    yy = torch.cat([_flat_z(n, n + 9, -100.0, 100.0), torch.linspace(-100.0, 100.0, 2001)]) if n == 1000 \
        else _flat_z(n, n + 9, -100.0, 100.0)
    y2, _ = _activation(h, yy, None, 2, (n, 2))
    h.bar('nr_activation', 'sigmoid', y2.reshape(-1, 1), R.sigmoid_ref(yy, F32).reshape(-1, 1),
          R.sigmoid_ref(yy, F64).reshape(-1, 1), n)


# ---- one thread per element: [P, n] ------------------------------------------------------------------
def _adjoint(h, sine, d, P, n, ldh, with_g, what, g_override=None):
    p = h.p
    dd = {k: h.up(v) for k, v in d.items()}
    gd = h.up(g_override) if g_override is not None else (dd['g'] if with_g else None)
    zd = dd['zdot'] if (with_g or g_override is not None) else None
    if sine:
        args = lambda o: (p(dd['hbar']), ldh, p(dd['s']), p(dd['h']), p(gd), p(zd), P, n, p(o[0]))
    else:
        args = lambda o: (p(dd['hbar']), ldh, p(dd['s']), p(gd), p(zd), P, n, p(o[0]))
    out, = h.twice('nr_sine_adjoint' if sine else 'nr_softplus_adjoint', what, [(P, n)], args)
    return out


@pytest.mark.parametrize('sine', [False, True], ids=['softplus', 'sine'])
@pytest.mark.parametrize('P', R.GRID_P)
def test_adjoints(h, P, sine):
    for _, n, ldh, with_g in [c for c in R.grid_cases() if c[0] == P]:
        what = (P, n, ldh, with_g)
        d = R.adjoint_inputs(P, n, ldh, 7 * P + n, sine)
        out = _adjoint(h, sine, d, P, n, ldh, with_g, what)
        hb = d['hbar'][:, :n].contiguous()
        g, zd = (d['g'], d['zdot']) if with_g else (None, None)
        rep = R.sine_adjoint_replica(hb, d['s'], d['h'], g, zd) if sine else R.softplus_adjoint_replica(hb, d['s'], g, zd)
        assert bits_equal(out, rep), (what, float((out - rep).abs().nan_to_num(float('inf')).max()))


@pytest.mark.parametrize('P', R.GRID_P)
def test_scale_cols(h, P):
    p = h.p
    for _, lda, col0, ncols, with_s, scale in [c for c in R.scale_cols_cases() if c[0] == P]:
        what = (P, lda, col0, ncols, with_s, scale)
        a = R.mag((P, lda), P + lda)
        s = R.mag((P, ncols), 3) if with_s else None
        ad, sd = h.up(a), h.up(s)
        out, = h.twice('nr_scale_cols', what, [(P, ncols)], lambda o: (p(ad), P, lda, col0, ncols, p(sd), scale, p(o[0])))
        assert bits_equal(out, R.scale_cols_replica(a, col0, ncols, s, scale)), what


# ---- the column sum ------------------------------------------------------------------------------------
def _colsum(h, a, P, n, what, ws_delta=0, expect=0):
    p = h.p
    ad = h.up(a) if P else torch.zeros(1, device=h.dev)
    nb = h.lib.nr_colsum_workspace_bytes(n)
    assert nb == 1024 * n * 4
    res = []
    for _ in range(2):
        B = Bufs(h.dev)
        out = B.new(n)
        ws = B.new(nb, dtype=torch.uint8)
        h.launch('nr_colsum', what, B, p(ad), P, n, p(out), ctypes.c_void_p(ws.data_ptr()), nb + ws_delta, expect=expect)
        if expect:
            assert B.untouched(out) and bool((ws == 0xA5).all()), (what, 'written despite the error')
            return None
        res.append(out.cpu())
    assert bits_equal(*res), (what, 'not deterministic')
    return res[0]


@pytest.mark.parametrize('P', R.COLSUM_P)
def test_colsum(h, P):
    for n in R.COLSUM_N:
        a = R.colsum_case('int', P, n)
        out = _colsum(h, a, P, n, ('int', P, n))
        if P == 0:
            assert bits_equal(out, torch.zeros(n)), ('P = 0', n)
        want = a.long().sum(0)
        assert torch.equal(out.double(), want.double()), (P, n, 'integer sums', int((out.double() - want.double()).abs().max()))
        a = R.colsum_case('heavy', P, n)
        out = _colsum(h, a, P, n, ('heavy', P, n))
        r64 = a.double().sum(0)
        mag = a.double().abs().sum(0)
        err = (out.double() - r64).abs()
        if P:
            key = ('nr_colsum', 'heavy')
            h.worst[key] = max(h.worst.get(key, 0.0), float((err / mag).max()))
        assert bool((err <= COLSUM_BAR * mag).all()), (P, n, float((err / mag.clamp_min(1e-300)).max()))


def test_colsum_workspace_one_byte_short(h):
    for P, n in ((1025, 65), (7, 1)):
        _colsum(h, R.colsum_case('int', P, n), P, n, ('short', P, n), ws_delta=-1, expect=NR_ERR_WORKSPACE)


# ---- the radiance net's input --------------------------------------------------------------------------
def test_radiance_input(h):
    p = h.p
    for P, uv, nfv, wf in R.RAD_CASES:
        what = (P, uv, nfv, wf)
        x, v, nrm, feat = R.radiance_inputs(P, wf)
        xd, vd, nd, fd = h.up(x), h.up(v), h.up(nrm), h.up(feat)
        copies, emb = R.radiance_input_copies(x, nrm, feat, nfv, uv, wf)
        ld = 3 + (R.nfeat(nfv) + 3 if uv else 0) + wf
        # without view directions v and nrm are unused: NULL
        out, = h.twice('nr_radiance_input', what, [(P, ld)],
                       lambda o: (p(xd), p(vd) if uv else None, p(nd) if uv else None, p(fd), P, nfv, uv, wf, p(o[0])))
        _copies(out, copies, what)
        if emb is not None:
            ve, = h.twice('nr_embed', what, [(P, R.nfeat(nfv))], lambda o: (p(vd), P, nfv, p(o[0])))
            assert bits_equal(out[:, emb], ve), (what, 'view embedding is not nr_embed of v')
        r32 = R.radiance_input_ref(x, v, nrm, feat, nfv, uv, wf, F32)
        r64 = R.radiance_input_ref(x, v, nrm, feat, nfv, uv, wf, F64)
        if emb is not None:
            for g, sl in R.groups(nfv):
                sl = slice(emb.start + sl.start, emb.start + sl.stop)
                h.bar('nr_radiance_input', 'view.' + g, out[:, sl], r32[:, sl], r64[:, sl], what)


# ---- optional pointers -------------------------------------------------------------------------------------
@pytest.mark.parametrize('s1', [1.0, -0.37])
def test_vjp_null_e1_equals_zeros(h, s1):
    P, nfreq, ld = 130, 6, 64
    nf = R.nfeat(nfreq)
    x, e0, _ = R.vjp_inputs(P, nfreq, ld, ld, None, seed=3)
    e0[::3, 1] = -0.0
    e0[1::5, 3:nf:4] = -0.0
    e0[2::7, :nf] = 0.0
    e0[4::7, :nf] = -0.0
    zeros = torch.full((P, ld), float('nan'))
    zeros[:, :nf] = 0.0
    null = _vjp(h, x, e0, ld, None, ld, None, P, nfreq, 'e1 NULL')
    zero = _vjp(h, x, e0, ld, zeros, ld, s1, P, nfreq, 'e1 zeros')
    assert bits_equal(null, zero)


@pytest.mark.parametrize('sine', [False, True], ids=['softplus', 'sine'])
def test_adjoint_null_g_equals_zeros(h, sine):
    P, n, ldh = 130, 39, 42
    d = R.adjoint_inputs(P, n, ldh, 99, sine)
    d['hbar'][::3, 0:n:2] = -0.0
    d['hbar'][1::3, 1:n:2] = 0.0
    null = _adjoint(h, sine, d, P, n, ldh, False, 'g NULL')
    zero = _adjoint(h, sine, d, P, n, ldh, False, 'g zeros', g_override=torch.zeros(P, n))
    assert torch.equal(null, zero), 'values'                  # -0.0 == +0.0 here
    nz = null != 0
    assert bits_equal(null[nz], zero[nz])
    assert bool((null == 0).any()) and not bool(torch.signbit(null[~nz]).any()), 'NULL g gives +0.0 on every zero'
    # a zero g keeps -0.0 only where hbar s = -0.0 and the zero term is negative
    hs = d['hbar'][:, :n] * d['s']
    term = (torch.zeros(P, n) * d['zdot']) * ((-900.0 * d['h']) if sine else (d['s'] * (1.0 - d['s'])) * 100.0)
    assert bits_equal(zero, hs + term)


def test_scale_cols_null_s_equals_ones(h):
    p = h.p
    P, lda, col0, ncols = 130, 44, 2, 39
    ad = h.up(R.mag((P, lda), 5))
    ones = torch.ones(P, ncols, device=h.dev)
    for scale in (1.0, R.ISQ2):
        null, = h.twice('nr_scale_cols', 'NULL', [(P, ncols)], lambda o: (p(ad), P, lda, col0, ncols, None, scale, p(o[0])))
        one, = h.twice('nr_scale_cols', 'ones', [(P, ncols)], lambda o: (p(ad), P, lda, col0, ncols, p(ones), scale, p(o[0])))
        assert bits_equal(null, one), scale


def test_embed_vjp_rejects_short_strides(h):
    """a stride below the feature count would read the next point's row: NR_ERR_ARG, nothing written"""
    p = h.p
    P, nfreq = 5, 6
    nf = R.nfeat(nfreq)
    x, e0, e1 = R.vjp_inputs(P, nfreq, nf, nf, 1.0)
    xd, e0d, e1d = h.up(x), h.up(e0), h.up(e1)
    for ld0, ld1, e1p in ((nf - 1, nf, None), (nf, nf - 1, p(e1d)), (3, nf, p(e1d))):
        B = Bufs(h.dev)
        out = B.new(P, 3)
        h.launch('nr_embed_vjp', (ld0, ld1), B, p(xd), p(e0d), ld0, e1p, ld1, 1.0, P, nfreq, p(out), expect=NR_ERR_ARG)
        assert B.untouched(out)
    B = Bufs(h.dev)
    out = B.new(P, 3)
    h.launch('nr_embed_vjp', 'ld1 unused', B, p(xd), p(e0d), nf, None, 0, 1.0, P, nfreq, p(out))   # e1 NULL: ld1 is not read


# ---- the helpers of training.py ------------------------------------------------------------------------
def _views(t):
    """the contiguous [P, n] tensor as a column slice of a wider one and as a transpose"""
    P, n = t.shape
    wide = torch.full((P, n + 4), 7.0, device=t.device)
    wide[:, 1:1 + n] = t
    return [wide[:, 1:1 + n], t.t().contiguous().t()]


def _outs(r):
    return r if isinstance(r, tuple) else (r,)


def _helper(fn, args, direct, what):
    """fn on contiguous args gives `direct`'s bits; with each tensor argument in turn (and all at once)
    replaced by a non-contiguous view it gives the same bits or raises"""
    ref = _outs(fn(*args))
    for a, b in zip(ref, direct):
        assert bits_equal(a.cpu(), b), (what, 'contiguous input')
    tens = [i for i, a in enumerate(args) if torch.is_tensor(a)]
    for kind in (0, 1):
        for sel in [[i] for i in tens] + [tens]:
            aa = list(args)
            for i in sel:
                aa[i] = _views(args[i])[kind]
                assert not aa[i].is_contiguous() or min(aa[i].shape) == 1
            try:
                got = _outs(fn(*aa))
            except (AssertionError, RuntimeError, ValueError):
                continue
            torch.cuda.synchronize()
            for a, b in zip(got, ref):
                assert bits_equal(a, b), (what, 'non-contiguous input', kind, sel)


def test_training_helpers(h):
    import neurecon_amd.training as T
    p = h.p
    P, n = 130, 39
    x, _ = R.points(P)
    xd = h.up(x)
    e, = h.twice('nr_embed', 'helper', [(P, R.nfeat(6))], lambda o: (p(xd), P, 6, p(o[0])))
    _helper(lambda t: T._embed(t, 6), [xd], [e], '_embed')
    z = h.up(_flat_z(P * n, 1, -1.2, 0.4).reshape(P, n))
    hh, ss = h.twice('nr_softplus100', 'helper', [(P, n), (P, n)], lambda o: (p(z), P * n, p(o[0]), p(o[1])))
    _helper(T._softplus, [z], [hh, ss], '_softplus')
    hh, ss = h.twice('nr_sine30', 'helper', [(P, n), (P, n)], lambda o: (p(z), P * n, p(o[0]), p(o[1])))
    _helper(T._sine30, [z], [hh, ss], '_sine30')
    a, b = h.up(R.mag((P, n), 1)), h.up(R.mag((P, n), 2))
    m, = h.twice('nr_mul', 'helper', [(P, n)], lambda o: (p(a), p(b), P * n, p(o[0])))
    _helper(T._mul, [a, b], [m], '_mul')
    s = h.up(R.mag((P, 30), 3))
    c, = h.twice('nr_scale_cols', 'helper', [(P, 30)], lambda o: (p(a), P, n, 4, 30, p(s), R.ISQ2, p(o[0])))
    _helper(lambda t, u: T._cols(t, 4, 30, u, R.ISQ2), [a, s], [c], '_cols')
    c, = h.twice('nr_scale_cols', 'helper', [(P, 30)], lambda o: (p(a), P, n, 4, 30, None, 1.0, p(o[0])))
    _helper(lambda t: T._cols(t, 4, 30), [a], [c], '_cols without s')
    big = R.colsum_case('heavy', 1025, 65)
    _helper(T._colsum, [h.up(big)], [_colsum(h, big, 1025, 65, 'helper')], '_colsum')
