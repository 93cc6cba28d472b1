"""References and cases for the training step's element-wise kernels (csrc/nr_train.hip: nr_embed*,
nr_softplus100, nr_softplus_adjoint, nr_sine30, nr_sine_adjoint, nr_scale_cols, nr_mul, nr_activation,
nr_colsum, nr_radiance_input).  No GPU code and nothing of neurecon_amd: every function is written from
the formulas in the header comment of nr_train.hip and in include/neurecon_hip.h.

  * *_ref(..., dtype): the formula on the CPU in the given dtype.  dtype=float64 on the fp32 inputs is
    the truth of tests/test_gpu_train_ops.py, dtype=float32 gives the E of its bar.  The frequency 2^b
    is a power of two, so the argument x 2^b is exact in either dtype; 30 z and 100 z round in fp32 at
    the same single multiplication the kernels use.
  * *_replica: the fp32 result of the plain-arithmetic kernels, the same single IEEE operations in
    the kernel's order (fmul / fadd / fsub are not contracted on the device), so the device's bits are
    determined.  `trace`, when given, collects every intermediate product (test_train_ops_ref.py checks
    that none is subnormal).
  * the case lists, the smallest shapes at which each kernel can still go wrong; tests/
    test_train_ops_ref.py holds their conditions on the CPU.
"""
import math

import torch

F32, F64 = torch.float32, torch.float64
ISQ2 = 1.0 / math.sqrt(2.0)


def nfeat(nfreq):
    return 3 if nfreq < 0 else 3 + 6 * nfreq


def groups(nfreq):
    """the column groups of an embedding row: the identity columns, then six columns per band"""
    return [('identity', slice(0, 3))] + [(f'band{b}', slice(3 + 6 * b, 9 + 6 * b)) for b in range(max(nfreq, 0))]


# ---- the formulas, in a given dtype -------------------------------------------------------------------
def embed_ref(x, nfreq, dtype=F64):
    """[x, sin(2^0 x), cos(2^0 x), ..., sin(2^(F-1) x), cos(2^(F-1) x)]; F < 0: x"""
    x = x.to(dtype)
    cols = [x]
    for b in range(max(nfreq, 0)):
        a = x * float(2 ** b)
        cols += [torch.sin(a), torch.cos(a)]
    return torch.cat(cols, 1)


def embed_jvp_ref(x, v, nfreq, dtype=F64):
    """J_emb(x) v = d/dt embed(x + t v): [v, 2^b v cos(2^b x), -2^b v sin(2^b x), ...]"""
    x, v = x.to(dtype), v.to(dtype)
    cols = [v]
    for b in range(max(nfreq, 0)):
        f = float(2 ** b)
        a = x * f
        cols += [v * torch.cos(a) * f, v * -torch.sin(a) * f]
    return torch.cat(cols, 1)


def embed_vjp_ref(x, e0, e1, s1, nfreq, dtype=F64):
    """J_emb(x)^T (e0 + s1 e1) -> [P, 3]; e0 / e1 [P, nf] (e1 may be None), s1 an fp32 value"""
    x = x.to(dtype)
    g = e0.to(dtype)
    if e1 is not None:
        g = g + e1.to(dtype) * torch.tensor(s1, dtype=F32).to(dtype)
    out = g[:, 0:3].clone()
    for b in range(max(nfreq, 0)):
        f = float(2 ** b)
        a = x * f
        out = out + g[:, 3 + 6 * b:6 + 6 * b] * torch.cos(a) * f + g[:, 6 + 6 * b:9 + 6 * b] * -torch.sin(a) * f
    return out


def softplus100_ref(z, dtype=F64):
    """Softplus(beta=100, threshold=20): (h, s = dh/dz); t = 100 z > 20: (z, 1)"""
    z = z.to(dtype)
    t = z * 100.0
    lin = t > 20.0
    e = torch.exp(torch.where(lin, torch.zeros_like(t), t))
    h = torch.where(lin, z, torch.log1p(e) / 100.0)
    s = torch.where(lin, torch.ones_like(z), e / (e + 1.0))
    return h, s


def sine30_ref(z, dtype=F64):
    """h = sin(30 z), s = dh/dz = 30 cos(30 z)"""
    a = 30.0 * z.to(dtype)
    return torch.sin(a), 30.0 * torch.cos(a)


def softplus_adjoint_ref(hbar, s, g, zdot, dtype=F64):
    """zbar = hbar s + g zdot 100 s (1 - s)"""
    hbar, s = hbar.to(dtype), s.to(dtype)
    v = hbar * s
    if g is not None:
        v = v + g.to(dtype) * zdot.to(dtype) * (100.0 * s * (1.0 - s))
    return v


def sine_adjoint_ref(hbar, s, h, g, zdot, dtype=F64):
    """zbar = hbar s + g zdot (-900 h)"""
    v = hbar.to(dtype) * s.to(dtype)
    if g is not None:
        v = v + g.to(dtype) * zdot.to(dtype) * (-900.0 * h.to(dtype))
    return v


def sigmoid_ref(y, dtype=F64):
    return 1.0 / (1.0 + torch.exp(-y.to(dtype)))


def radiance_input_ref(x, v, nrm, feat, nfreq_view, use_view_dirs, wfeat, dtype=F64):
    """cat([x, embed_view(v), normals, feature]), or cat([x, feature]) without view directions;
    wfeat = 0: without the feature"""
    parts = [x.to(dtype)]
    if use_view_dirs:
        parts += [embed_ref(v, nfreq_view, dtype), nrm.to(dtype)]
    if wfeat:
        parts.append(feat.to(dtype))
    return torch.cat(parts, 1)


# ---- fp32 replicas: single IEEE operations in the kernel's order ------------------------------------------
def _t(trace, *ts):
    if trace is not None:
        trace.extend(ts)


def mul_replica(a, b, trace=None):
    out = a * b
    _t(trace, out)
    return out


def scale_cols_replica(a, col0, ncols, s, scale, trace=None):
    """(a[:, col0:col0+ncols] * scale) * s; the scale skipped when 1, s when None"""
    v = a[:, col0:col0 + ncols].contiguous()
    scale = torch.tensor(scale, dtype=F32)
    if float(scale) != 1.0:
        v = v * scale
        _t(trace, v)
    if s is not None:
        v = v * s
        _t(trace, v)
    return v


def softplus_adjoint_replica(hbar, s, g, zdot, trace=None):
    """hbar * s + (g * zdot) * ((s * (1 - s)) * 100); without g: hbar * s + 0"""
    v = hbar * s
    _t(trace, v)
    if g is None:
        return v + 0.0
    p1 = s * (1.0 - s)
    d2 = p1 * 100.0
    gz = g * zdot
    t = gz * d2
    _t(trace, p1, d2, gz, t)
    return v + t


def sine_adjoint_replica(hbar, s, h, g, zdot, trace=None):
    """hbar * s + (g * zdot) * (-900 * h); without g: hbar * s + 0"""
    v = hbar * s
    _t(trace, v)
    if g is None:
        return v + 0.0
    d2 = -900.0 * h
    gz = g * zdot
    t = gz * d2
    _t(trace, d2, gz, t)
    return v + t


def activation_replica(y, g, mode, trace=None):
    """mode 0: relu(y) (+0.0 where y <= 0) -> y; 1: g where y > 0, else +0.0 -> g; 3: g * (y * (1 - y)) -> g"""
    if mode == 0:
        return torch.where(y > 0, y, torch.zeros_like(y))
    if mode == 1:
        return torch.where(y > 0, g, torch.zeros_like(g))
    assert mode == 3
    p = y * (1.0 - y)
    out = g * p
    _t(trace, p, out)
    return out


def embed_copy_replica(x, nfreq, ldo):
    """(columns, values) an embedding kernel's row holds exactly: x (or v) in the identity columns, +0.0
    in the padding columns nf..ldo"""
    nf = nfeat(nfreq)
    return [(slice(0, 3), x), (slice(nf, ldo), torch.zeros(x.shape[0], ldo - nf))]


def radiance_input_copies(x, nrm, feat, nfreq_view, use_view_dirs, wfeat):
    """[(columns, values)] of the copied columns of nr_radiance_input's row, and the columns of the view
    embedding (None without view directions)"""
    out = [(slice(0, 3), x)]
    c, emb = 3, None
    if use_view_dirs:
        nv = nfeat(nfreq_view)
        emb = slice(c, c + nv)
        c += nv
        out.append((slice(c, c + 3), nrm))
        c += 3
    if wfeat:
        out.append((slice(c, c + wfeat), feat))
    return out, emb


# ---- inputs ---------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def mag(shape, seed, lo=1e-3, hi=1e3):
    """random signs, magnitudes log-uniform in [lo, hi]: the replica inputs (no product of the replicas
    is subnormal, tests/test_train_ops_ref.py)"""
    g = _gen(seed)
    u = torch.rand(shape, generator=g, dtype=F64)
    m = torch.exp(math.log(lo) + u * (math.log(hi) - math.log(lo))).clamp(lo, hi)
    sgn = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return (m * sgn).float().clamp(-hi, hi)


def unit(shape, seed, lo=1e-3):
    """values in [lo, 1 - lo]: softplus's s, a sigmoid's output"""
    return (lo + (1.0 - 2.0 * lo) * torch.rand(shape, generator=_gen(seed), dtype=F64)).float().clamp(lo, 1.0 - lo)


def special_scalars():
    """0.0, -0.0, +-1e-4, +-3, +-8 and the floats nearest k pi / 2^b"""
    s = [0.0, -0.0, 1e-4, -1e-4, 3.0, -3.0, 8.0, -8.0]
    s += [k * math.pi / 2 ** b for b in (0, 1, 5, 9, 10) for k in (1, 2, 3, 5, 7, -1, -4)]
    return torch.tensor(s, dtype=F64).float()


P_MAX = 8193
_POOL = {}


def points(P):
    """x [P, 3] and a tangent v [P, 3]: rows of the special scalars first, then uniform in [-3, 3]; the
    small P start at different rows of the pool so that each holds special values"""
    if not _POOL:
        s = special_scalars()
        m = s.numel()
        i = torch.arange(m)
        sp = torch.stack([s[i], s[(i * 7 + 3) % m], s[(i * 11 + 5) % m]], 1)
        g = _gen(11)
        x = torch.cat([sp, torch.rand(P_MAX + 32 - m, 3, generator=g) * 6.0 - 3.0])
        v = torch.rand(P_MAX + 32, 3, generator=g) * 2.0 - 1.0
        v[3::17, 1] = 0.0
        _POOL['x'], _POOL['v'] = x, v
    r0 = {1: 2, 3: 5, 4: 11, 5: 17}.get(P, 0)
    return _POOL['x'][r0:r0 + P].clone(), _POOL['v'][r0:r0 + P].clone()


# ---- cases ----------------------------------------------------------------------------------------------
EMBED_P = (1, 3, 4, 5, 8193)     # a partial block, one block, a second block; 8193: the second grid-stride trip
EMBED_NFREQ = (-1, 0, 4, 6, 10)
EMBED_LDO = ('nf', 64, 80, 128)   # ldo > 64: the lane loop's second trip


def embed_cases():
    """(P, nfreq, ldo) of nr_embed_padded / nr_embed_jvp_padded; ldo == nf also runs nr_embed / nr_embed_jvp"""
    out = []
    for P in EMBED_P:
        for nfreq in EMBED_NFREQ:
            nf = nfeat(nfreq)
            for ldo in EMBED_LDO:
                ldo = nf if ldo == 'nf' else ldo
                if ldo >= nf:
                    out.append((P, nfreq, ldo))
    return out


VJP_S1 = (None, 1.0, ISQ2, -0.37)   # None: e1 NULL


def vjp_cases():
    """(P, nfreq, ld0, ld1, s1): every (ld0, ld1) of {nf, 64, 70}^2 at every (P, nfreq), the e1 / s1 option
    cycling so that each meets every stride pair"""
    out = []
    for i, P in enumerate(EMBED_P):
        for j, nfreq in enumerate(EMBED_NFREQ):
            nf = nfeat(nfreq)
            lds = [ld for ld in (nf, 64, 70) if ld >= nf]
            k = 0
            for ld0 in lds:
                for ld1 in lds:
                    out.append((P, nfreq, ld0, ld1, VJP_S1[(i + j + k) % 4]))
                    k += 1
    return out


def vjp_inputs(P, nfreq, ld0, ld1, s1, band=None, seed=0):
    """x, e0 [P, ld0], e1 [P, ld1] or None; the gap columns ld > nf hold NaN (they must not be read).
    band: e0 non-zero only in that group of columns ('identity' or b), e1 None."""
    nf = nfeat(nfreq)
    x, _ = points(P)
    g = _gen(1000 + seed)
    e0 = torch.full((P, ld0), float('nan'))
    e0[:, :nf] = torch.randn(P, nf, generator=g)
    e1 = None
    if band is not None:
        sl = dict(groups(nfreq))['identity' if band == 'identity' else f'band{band}']
        keep = torch.zeros(nf, dtype=torch.bool)
        keep[sl] = True
        e0[:, :nf] = torch.where(keep, e0[:, :nf], torch.zeros(()))
    elif s1 is not None:
        e1 = torch.full((P, ld1), float('nan'))
        e1[:, :nf] = torch.randn(P, nf, generator=g) * 2.0
    return x, e0, e1


VJP_BAND_NFREQ, VJP_BAND_P = 10, 130
VJP_BANDS = ['identity'] + list(range(VJP_BAND_NFREQ))

FLAT_N = (1, 255, 256, 257, 1000)                 # one-thread-per-element kernels, 256 threads per block
GRID_P, GRID_N = (1, 7, 130), (1, 39, 256, 257)


def grid_cases():
    """(P, n, ldh, with_g) of the two adjoints"""
    return [(P, n, n + pad, wg) for P in GRID_P for n in GRID_N for pad in (0, 3) for wg in (False, True)]


def scale_cols_cases():
    """(P, lda, col0, ncols, with_s, scale): an interior column range (col0 > 0, col0 + ncols < lda) at
    every shape, and the whole matrix"""
    out = [(P, n + 5, 2, n, ws, sc) for P in GRID_P for n in GRID_N for ws in (False, True) for sc in (1.0, ISQ2)]
    out += [(7, 39, 0, 39, True, ISQ2), (130, 257, 0, 257, False, 1.0)]
    return out


def adjoint_inputs(P, n, ldh, seed, sine=False):
    """hbar [P, ldh] (gap columns NaN), s, h, g, zdot [P, n] in the replicas' magnitude range"""
    hbar = torch.full((P, ldh), float('nan'))
    hbar[:, :n] = mag((P, n), seed)
    if sine:
        h = unit((P, n), seed + 1) * torch.where(mag((P, n), seed + 2) < 0, -1.0, 1.0)
        s = mag((P, n), seed + 3, lo=1e-3, hi=30.0)
    else:
        h = None
        s = unit((P, n), seed + 1)
    return dict(hbar=hbar, s=s, h=h, g=mag((P, n), seed + 4), zdot=mag((P, n), seed + 5))


def softplus_sweep():
    """z with t = 100 z dense over [-120, 40], the neighbours of 0.2f in both directions (the threshold
    t = 20) and of the t at which exp underflows / s rounds to 1"""
    z = torch.linspace(-1.2, 0.4, 16001, dtype=F64).float()
    near = [torch.tensor(0.2, dtype=F32)]
    for d in (1.0, -1.0):
        c = torch.tensor(0.2, dtype=F32)
        for _ in range(8):
            c = torch.nextafter(c, torch.tensor(d, dtype=F32))
            near.append(c)
    return torch.cat([z, torch.stack(near), torch.tensor([0.0, -0.0, 0.19999, 0.20001, -1.0397, -0.8733, 0.1664])])


def sine_sweep():
    """|z| up to 10"""
    return torch.cat([torch.linspace(-10.0, 10.0, 8001, dtype=F64).float(), torch.tensor([0.0, -0.0, 1e-4, -1e-4])])


TINY = 1.1754943508222875e-38    # the smallest normal fp32


def relu_inputs(n, seed):
    """y with +0.0, -0.0 and the smallest normals of both signs among the replicas' range; g"""
    y = mag((n,), seed)
    sp = torch.tensor([0.0, -0.0, TINY, -TINY], dtype=F32)
    k = min(n, 4)
    y[:k] = sp[(torch.arange(k) + seed) % 4]
    return y, mag((n,), seed + 1)


COLSUM_P = (0, 1, 7, 1023, 1024, 1025, 8192, 8193, 16385)   # 1024 slabs of ceil(P / 1024) rows, unrolled by 8
COLSUM_N = (1, 63, 64, 65, 257)                             # the final pass: 64 columns per block
_CS = {}


def colsum_input(kind):
    """the [16385, 257] master of a kind: 'int' integer-valued entries in [-8, 8] (every partial sum exact in
    fp32), 'heavy' a few large entries over many small ones (test_gpu_wgrad.py _mk(heavy=True)); a case is
    [:P, :n] of it, contiguous"""
    if kind not in _CS:
        P, n = max(COLSUM_P), max(COLSUM_N)
        g = _gen(5 if kind == 'int' else 6)
        if kind == 'int':
            _CS[kind] = torch.randint(-8, 9, (P, n), generator=g).float()
        else:
            _CS[kind] = torch.randn(P, n, generator=g) * torch.exp(2.0 * torch.randn(P, n, generator=g))
    return _CS[kind]


def colsum_case(kind, P, n):
    return colsum_input(kind)[:P, :n].contiguous()


RAD_CASES = [(P, uv, nfv, wf) for P in (1, 130) for uv in (0, 1) for nfv in (-1, 4, 10) for wf in (0, 5, 256)]


def radiance_inputs(P, wfeat, seed=0):
    x, _ = points(P)
    g = _gen(300 + seed)
    v = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=1)
    return x, v, mag((P, 3), 301 + seed), (mag((P, wfeat), 302 + seed) if wfeat else None)
