"""The cases of tests/test_gpu_composite.py (inputs, upstream gradients, fp32 / fp64 references) and of
the embedding-input kernels, built on the CPU with seeds fixed here, so that tests/test_composite_ref.py
can hold their conditioning caps without a GPU.

A case is one launch: kind, shape, the scalar (s, beta or the logit spread c), white_bkgd.  Inputs are
fp32; `reference(case, dtype)` runs tests/composite_ref.py under autograd on those same values in fp32
or fp64 with the case's upstream gradients and returns (outputs, gradients) named as the C ABI names
them.  s and beta enter as [R, 1] leaves, so d_s / d_beta come per ray.

g_depth is 0 on rays whose float64 acc < 1e-3: depth = sum w / (acc + 1e-10) d, so on a ray with
acc ~ 1e-8 the fp32 reference's own depth gradient is wrong by orders of magnitude and bounds nothing.
Those rays keep every other upstream gradient."""
import functools
import math
import itertools
import zlib

import torch

import composite_ref as CR

R_SET = (1, 63, 65, 130)
ACC_MIN = 1e-3            # below: g_depth = 0
LOOSE = 1e-4              # a ray is loose for a tensor when E_ray > LOOSE scale
LOOSE_SHARE = 0.02

NEUS_S = (2, 64, 65, 66, 129)
NEUS_BG_SN = ((2, 1), (65, 3), (66, 32), (128, 32))
S_SET = (20.0, 300.0, 3000.0)
VOLSDF_SN = ((2, 0), (64, 0), (65, 3), (128, 32))
BETA_SET = (0.1, 0.01, 0.001)
UNI_P = (1, 2, 96, 97)
UNI_C = (1.0, 10.0, 40.0)
R_BG = 3.0

OUTS = dict(neus=('rgb', 'depth', 'acc', 'weights', 'alpha', 'cdf'),
            neus_bg=('rgb', 'depth', 'acc', 'weights', 'alpha', 'cdf'),
            volsdf=('rgb', 'depth', 'acc', 'weights', 'p_i', 'sigma', 'sdf_out'),
            unisurf=('rgb', 'depth', 'acc', 'weights', 'alpha'))
OPTIONAL_OUTS = dict(neus=('alpha', 'cdf'), neus_bg=('alpha', 'cdf'), volsdf=('p_i', 'sigma', 'sdf_out'),
                     unisurf=('alpha',))
UPSTREAM = dict(neus=('g_rgb', 'g_depth', 'g_acc', 'g_w'), neus_bg=('g_rgb', 'g_depth', 'g_acc', 'g_w'),
                volsdf=('g_rgb', 'g_depth', 'g_acc', 'g_w', 'g_sdf'), unisurf=('g_rgb', 'g_depth', 'g_acc', 'g_w'))
GRADS = dict(neus=('d_sdf', 'd_rad', 'd_s'), neus_bg=('d_sdf', 'd_rad', 'd_sigma_out', 'd_rad_out', 'd_s'),
             volsdf=('d_sdf', 'd_rad', 'd_beta', 'd_sigma_bg', 'd_rad_bg'), unisurf=('d_logits', 'd_rad'))


class Case:
    def __init__(self, kind, R, white, **kw):
        self.kind, self.R, self.white = kind, R, int(white)
        self.__dict__.update(kw)
        dims = '_'.join(f'{k}{v:g}' for k, v in kw.items())
        self.name = f'{kind}-R{R}-{dims}-w{self.white}'
        self.seed = zlib.crc32(self.name.encode()) + RESEED.get(self.name, 0)
        self.x = None

    def __repr__(self):
        return self.name


# cases re-drawn with another seed because the first draw broke the loose-ray cap (test_composite_ref.py)
RESEED = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _depths(g, R, n, lo, hi):
    """[R, n] increasing depths in [lo, hi] with jittered spacing"""
    step = torch.rand(R, n, generator=g) + 0.25
    d = torch.cumsum(step, -1)
    d = lo + (hi - lo) * (d - d[:, :1]) / (d[:, -1:] - d[:, :1]).clamp_min(1e-6) if n > 1 else torch.full((R, 1), lo)
    return d.float().contiguous()


def _neus_inputs(c, g):
    """sdf falls from about +0.5 to between -0.1 and -0.5 with 0.02 noise (decreasing and increasing
    intervals, one surface crossing).  For S > 2 each ray is shifted by less than one step so that its
    first negative sample sits at s sdf = -u, u in [0.2, 2]: at s = 3000 the neighbouring CDFs are exactly
    1 and 0, the next alpha is exactly 1 (u = 1e-10 in the backward's division), and the ray still has one
    unsaturated CDF, so its gradient is not all rounding."""
    R, S = c.R, c.S
    end = -(0.1 + 0.4 * torch.rand(R, 1, generator=g))
    if S == 2 and R < 3:
        # the tensors' scales are this one ray's: at the far end of the range c_1 = sigmoid(-0.5 s) underflows
        # in fp32 at s = 300 and 1 - alpha_0 cancels to 1e-4 relative at s = 20
        end = torch.full((R, 1), -0.1)
    t = torch.linspace(0, 1, S)[None]
    sdf = 0.5 * (1 - t) + end * t + 0.02 * torch.randn(R, S, generator=g)
    if S > 2:
        first = (sdf < 0).float().argmax(-1).clamp_min(1)
        u = 0.2 + 1.8 * torch.rand(R, generator=g)
        sdf = sdf - (sdf[torch.arange(R), first] + u / c.s)[:, None]
    d_all = _depths(g, R, S, 0.5, 3.0)
    x = dict(sdf=sdf.contiguous(), s=torch.tensor([c.s]), rad=torch.rand(R, S - 1, 3, generator=g),
             dmid=0.5 * (d_all[:, 1:] + d_all[:, :-1]))
    if c.kind == 'neus_bg':
        N, S1 = c.N, S - 1
        M = S1 + N
        far = d_all[:, -1:] + 0.1
        d_o = far + torch.cumsum(0.05 + 0.5 * torch.rand(R, N, generator=g), -1)
        inside = (torch.rand(R, S1, generator=g) < 0.8)
        if R >= 3:  # whole rows inside / outside the bounding sphere
            inside[0] = True
            inside[1] = False
        elif S == 2:
            # one ray, one mid-point: at s = 300 the SDF alpha is 1 - 1e-13 and everything behind it is
            # the 1e-10 floor, so the lone mid-point is outside there and inside at s = 20
            inside[0, 0] = c.s < 100
        if S > 2:  # the last ray (the only one of R = 1) keeps the SDF alphas on both sides of its crossing
            inside[R - 1, first[R - 1] - 1] = True
            inside[R - 1, min(int(first[R - 1]), S1 - 1)] = True
        sig = 2.0 * torch.randn(R, M, generator=g)
        sig[R - 1, min(S1, M - 1)] = 25.0          # F.softplus's threshold branch (x > 20), a background sample
        if R >= 3:
            sig[1, 0] = 22.0                        # and at an outside mid-point
        x.update(sigma_out=sig, rad_out=torch.rand(R, M, 3, generator=g), d_out=torch.cat([x['dmid'], d_o], -1),
                 inside=inside.to(torch.uint8))
    return x


def volsdf_ray_kinds(c):
    """(empty, thin) masks [R]: the first quarter of the rays passes the sphere; the even ones of those are
    empty (acc < 1e-3), the odd ones thin; the rest hit.  The one ray of R = 1 is thin with background
    samples (they need a ray that lets light through) and hits without: every tensor's scale is then that
    ray's own, and 1 - exp(-sigma delta) of the 60 near-empty samples of a thin ray (sigma delta ~ 6e-6 at
    beta = 0.1) carries half an fp32 ulp of p ~ 1, 3e-8 each, whatever computes it -- up to 2e-6 of a
    ray whose acc is 0.1, nothing of one whose acc is 1."""
    r = torch.arange(c.R)
    past = r < c.R // 4
    thin = (past & (r % 2 == 1)) | torch.tensor(c.R == 1 and c.N > 0)
    return past & ~thin, thin


def _volsdf_inputs(c, g):
    """rays along +z through and past a unit sphere, r_bg = 3, sdf = |x| - 1 + 0.02 noise:
      hit    impact parameter b < 0.9, z in [-2.6, 2.6]: a quarter of the samples lies beyond |x| = 2, where
             r_bg - |x| is the smaller value; the sample next to the surface is an exact 0 (sign 0);
      thin   passes at b in [1.95, 2] with use_bg (|x| in [1.95, 2.06], some samples beyond 2), b = 4.5 without,
             z in [-0.5, 0.5], with one sample at sdf = +-0.3 beta (and one exact 0): optical depth of order
             1-10 at every beta, so the samples behind it -- the background's with N > 0 -- keep a gradient that
             is not rounding (a ray that hits is opaque to 1e-40 and less at beta <= 0.01);
      empty  acc < 1e-3 at every beta (negative background sigma with N > 0): |x| < 0.1 with the network's
             value 2.97 + noise there.  No ray of sdf = |x| - 1 is emptier than sigma delta ~ 6e-6 at
             beta = 0.1 under r_bg = 3 (min(|x| - 1, r_bg - |x|) <= 1), and there every weight
             1 - exp(-sigma delta) is good to 1 % in fp32, whatever computes it: the depth of such a ray is
             off by 1e-4 of the tensor's scale in the fp32 reference and in the kernel alike, on different
             rays, so E_ray bounds nothing.  At 2.9 the weights are the 1e-10 floor in fp32 and fp64.
    S = 2 has one interval: its length is 2 beta (optical depth of order 1); hit rays alternate between
    a first sample inside the sphere and one at r_bg - |x| = 0.3 beta (the background value taken)."""
    R, S, N, beta = c.R, c.S, c.N, c.beta
    empty, thin = volsdf_ray_kinds(c)
    past = empty | thin
    ar = torch.arange(R)
    b_past = 1.95 + 0.05 * torch.rand(R, generator=g) if c.use_bg else torch.full((R,), 4.5)
    b = torch.where(past, b_past, 0.9 * torch.rand(R, generator=g))
    b = torch.where(empty, torch.tensor(0.05), b)
    edge = ~past & (ar % 2 == 1) & torch.tensor(bool(c.use_bg) and S == 2)
    # on the axis |x| = |z| is exact in fp32, so r_bg - |x| = 0.3 beta carries no rounding of the norm (at
    # beta = 0.001 sigma moves by 2.4e-4 of itself per fp32 ulp of |x| = 3)
    b = torch.where(edge, torch.zeros(()), b)
    o = torch.stack([b, torch.zeros(R), -3.0 * torch.ones(R)], -1)
    dirs = torch.tensor([0.0, 0.0, 1.0]).expand(R, 3)
    if S == 2:
        z0 = torch.zeros(R)
        z0 = torch.where(edge, ((R_BG - 0.3 * beta) ** 2 - b ** 2).sqrt() + beta, z0)
        half = torch.where(empty, torch.tensor(1e-3 * beta), torch.tensor(beta))  # empty: sigma delta << 1e-10
        d_all = torch.stack([3.0 + z0 - half, 3.0 + z0 + half], -1)
    else:
        zr = torch.where(past, torch.tensor(0.5), torch.tensor(2.6))
        zr = torch.where(empty, torch.tensor(0.05), zr)
        d_all = torch.stack([_depths(g, 1, S, float(3.0 - zr[r]), float(3.0 + zr[r]))[0] for r in range(R)])
        # one pair of equal consecutive depths per ray: delta = 0, the ReLU at its kink
        j = torch.randint(1, S - 2, (R,), generator=g)
        d_all[ar, j + 1] = d_all[ar, j]
    pts = (o[:, None, :] + dirs[:, None, :] * d_all[..., None]).contiguous()
    sdf = pts.norm(dim=-1) - 1.0 + 0.02 * torch.randn(R, S, generator=g)
    sdf = torch.where(empty[:, None], sdf + 3.97 - pts.norm(dim=-1), sdf)
    sign = torch.where(ar % 4 < 2, 1.0, -1.0)
    ti = torch.nonzero(thin)[:, 0]
    if S == 2:
        sdf[ti, 0] = 0.3 * beta * sign[ti]
    else:
        near0 = (pts.norm(dim=-1) - 1.0).abs().argmin(-1)
        hi = torch.nonzero(~past)[:, 0]
        sdf[hi, near0[hi]] = 0.0
        sdf[ti, S // 3] = 0.3 * beta * sign[ti]
        sdf[ti, S // 2] = 0.0
    x = dict(sdf=sdf.contiguous(), beta=torch.tensor([beta]), rad=torch.rand(R, S, 3, generator=g), pts=pts,
             d_all=d_all.contiguous())
    if N > 0:
        sig = 2.0 * torch.randn(R, N, generator=g)
        sig = torch.where(empty[:, None], -sig.abs(), sig)   # ReLU side of sigma delta: the empty rays stay empty
        sig[:, 0] = torch.where(thin, sig[:, 0].abs() + 0.1, sig[:, 0])
        d_bg = d_all[:, -1:] + torch.cumsum(0.05 + 0.3 * torch.rand(R, N, generator=g), -1)
        x.update(sigma_bg=sig, rad_bg=torch.rand(R, N, 3, generator=g), d_bg=d_bg.contiguous())
    return x


def _unisurf_inputs(c, g):
    """logits N(0, 1) c + c / 2, |logit| < 80.  The first quarter of the rays is free space (12 + |logit|:
    every alpha < 1e-5, acc < 1e-3); the second quarter is shifted by 1 + log 2P (alpha ~ 1 / 5P at c = 1:
    acc well inside (0, 1) at P = 96 too, where d acc is not 0 and a constant added to every weight
    adjoint -- a wrong wd / A^2 -- shows); the second half starts with one logit -|N(0, 1)| (alpha in
    (1/2, 1), acc > 1/2, and at P <= 2 a gradient that is not all saturation at c = 40)."""
    R, P = c.R, c.P
    lg = torch.randn(R, P, generator=g) * c.c + c.c / 2
    empty = torch.arange(R) < R // 4
    lg = torch.where(empty[:, None], 12.0 + lg.abs(), lg)
    semi = (torch.arange(R) >= R // 4) & (torch.arange(R) < R // 2)
    lg = torch.where(semi[:, None], lg + 1.0 + math.log(2 * P), lg)
    solid = torch.arange(R) >= R // 2
    lg[:, 0] = torch.where(solid, -torch.randn(R, generator=g).abs(), lg[:, 0])
    lg = lg.clamp(-79.0, 79.0)
    return dict(logits=lg.contiguous(), rad=torch.rand(R, P, 3, generator=g), d_all=_depths(g, R, P, 0.5, 4.0))


def _forward(c, x, s_or_beta=None):
    k = c.kind
    if k in ('neus', 'neus_bg'):
        bg = (x['sigma_out'], x['rad_out'], x['d_out'], x['inside']) if k == 'neus_bg' else None
        return CR.neus(x['sdf'], x['s'] if s_or_beta is None else s_or_beta, x['rad'], x['dmid'], c.white, bg)
    if k == 'volsdf':
        bg = (x['sigma_bg'], x['rad_bg'], x['d_bg']) if c.N > 0 else None
        return CR.volsdf(x['sdf'], x['beta'] if s_or_beta is None else s_or_beta, x['rad'], x['pts'], x['d_all'],
                         c.use_bg, R_BG, c.white, bg)
    return CR.unisurf(x['logits'], x['rad'], x['d_all'], c.white)


def build(c):
    """inputs c.x and upstream gradients c.g (fp32, CPU), once"""
    if c.x is not None:
        return c
    g = _gen(c.seed)
    c.x = {'neus': _neus_inputs, 'neus_bg': _neus_inputs, 'volsdf': _volsdf_inputs, 'unisurf': _unisurf_inputs}[c.kind](c, g)
    with torch.no_grad():
        out = _forward(c, {k: (v.double() if v.is_floating_point() else v) for k, v in c.x.items()})
    c.acc64 = out['acc']
    nw = out['weights'].shape[-1]
    ups = dict(g_rgb=torch.randn(c.R, 3, generator=g), g_depth=torch.randn(c.R, generator=g),
               g_acc=torch.randn(c.R, generator=g), g_w=torch.randn(c.R, nw, generator=g))
    ups['g_depth'] = torch.where(c.acc64 < ACC_MIN, torch.zeros(()), ups['g_depth']).float()
    if c.kind == 'volsdf':
        ups['g_sdf'] = torch.randn(c.R, c.S, generator=g)
        ups['g_sdf'][ups['g_sdf'] == 0] = 1.0
    c.g = ups
    return c


DIFF_IN = dict(neus=('sdf', 'rad'), neus_bg=('sdf', 'rad', 'sigma_out', 'rad_out'),
               volsdf=('sdf', 'rad', 'sigma_bg', 'rad_bg'), unisurf=('logits', 'rad'))
GRAD_OF = dict(sdf='d_sdf', rad='d_rad', sigma_out='d_sigma_out', rad_out='d_rad_out', sigma_bg='d_sigma_bg',
               rad_bg='d_rad_bg', logits='d_logits')


def evaluate(c, dtype, ups=None):
    """composite_ref under autograd in dtype on c's fp32 inputs -> (outputs, gradients), detached"""
    build(c)
    ups = c.g if ups is None else ups
    x = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in c.x.items()}
    leaves = {}
    for k in DIFF_IN[c.kind]:
        if k in x:
            x[k] = leaves[k] = x[k].clone().requires_grad_(True)
    per_ray = None
    if c.kind != 'unisurf':
        key = 's' if c.kind.startswith('neus') else 'beta'
        per_ray = x[key].reshape(1, 1).expand(c.R, 1).clone().requires_grad_(True)
    out = _forward(c, x, per_ray)
    loss = 0
    for gk, ok in (('g_rgb', 'rgb'), ('g_depth', 'depth'), ('g_acc', 'acc'), ('g_w', 'weights'), ('g_sdf', 'sdf_out')):
        if ups.get(gk) is not None:
            loss = loss + (out[ok] * ups[gk].to(dtype)).sum()
    loss.backward()
    grads = {GRAD_OF[k]: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    if per_ray is not None:
        grads['d_s' if c.kind.startswith('neus') else 'd_beta'] = per_ray.grad.reshape(c.R)
    return {k: v.detach() for k, v in out.items()}, grads


@functools.lru_cache(maxsize=None)
def _reference(c):
    return evaluate(c, torch.float32), evaluate(c, torch.float64)


def reference(c):
    """((outs32, grads32), (outs64, grads64)), cached"""
    return _reference(c)


def per_ray_error(t32, t64):
    """E_ray [R]: the fp32 reference's worst |fp32 - f64| over each ray's elements"""
    R = t64.shape[0]
    return (t32.double() - t64).abs().reshape(R, -1).amax(1) if t64.numel() else torch.zeros(R, dtype=torch.float64)


def tensors(c):
    """{name: (t32, t64, E_ray, scale)} over every forward output and gradient of the case, plus the
    host's sums of d_s / d_beta (fp32 sum of the fp32 per-ray vector, as the wrapper forms it)"""
    (o32, g32), (o64, g64) = reference(c)
    res = {}
    for k in list(o64) + list(g64):
        a, b = (o32[k], o64[k]) if k in o64 else (g32[k], g64[k])
        if k == 'sdf_out' or not b.is_floating_point():
            a, b = a.double(), b.double()
        res[k] = (a, b, per_ray_error(a, b), float(b.abs().max()) if b.numel() else 0.0)
    for k in ('d_s', 'd_beta'):
        if k in g64:
            a, b = g32[k].sum().reshape(1), g64[k].sum().reshape(1)
            res[k + '.sum'] = (a, b, (a.double() - b).abs(), float(g64[k].abs().max()))
    return res


def _mk(kind, white_set=(0, 1), **grid):
    keys = list(grid)
    out = []
    for R in R_SET:
        for vals in itertools.product(*grid.values()):
            for w in white_set:
                out.append(Case(kind, R, w, **dict(zip(keys, vals))))
    return out


def _all_cases():
    cs = [c for c in _mk('neus', S=NEUS_S, s=S_SET) if not (c.S == 2 and c.s == 3000.0)]
    for (S, N) in NEUS_BG_SN:
        cs += [c for c in _mk('neus_bg', S=(S,), N=(N,), s=S_SET) if not (c.S == 2 and c.s == 3000.0)]
    for (S, N) in VOLSDF_SN:
        cs += _mk('volsdf', S=(S,), N=(N,), beta=BETA_SET, use_bg=(1 if N == 0 else 0,))
    cs += _mk('volsdf', S=(65,), N=(3,), beta=(0.01,), use_bg=(1,))   # the ABI allows both with N > 0
    cs += _mk('unisurf', P=UNI_P, c=UNI_C)
    return cs


CASES = _all_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
KINDS = ('neus', 'neus_bg', 'volsdf', 'unisurf')


def cases_of(kind, **match):
    return [c for c in CASES if c.kind == kind and all(getattr(c, k) == v for k, v in match.items())]


# ---- inputs of the background nets (nr_nerf_train_input, nr_volsdf_nerf_input) ---------------------------
EMB_R = (1, 65)
EMB_MN = ((1, 0), (1, 1), (3, 2), (96, 64))
R_OBJ = 1.0


def embed_inputs(R, M, seed):
    """rays from the sphere |o| = 2.5 towards the origin region, depths up to 12: points inside and outside
    the unit sphere"""
    g = _gen(seed)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 2.5
    tgt = 0.4 * torch.randn(R, 3, generator=g)
    d = torch.nn.functional.normalize(tgt - o, dim=-1)
    depth = _depths(g, R, M, 1.2, 12.0) if M > 1 else 1.2 + 2.6 * torch.rand(R, 1, generator=g)
    return o.contiguous(), d.contiguous(), depth.contiguous()


def embed_reference(o, d, depth, rs, dtype):
    """x_emb [R M, 84], v_emb [R M, 27], |p| [R, M] in dtype: embed([p / r, 1 / r], 10), embed(dir, 4) with
    r = |p| (rs None: neus.py:303-312) or the given radii (volsdf.py:456-467)"""
    from oracle.nets import embed
    o, d, depth = o.to(dtype), d.to(dtype), depth.to(dtype)
    p = o[:, None, :] + d[:, None, :] * depth[..., None]
    nrm = p.norm(dim=-1, keepdim=True)
    r = nrm if rs is None else rs.to(dtype)[..., None]
    x4 = torch.cat([p / r, 1. / r], -1)
    return (embed(x4, 10).reshape(-1, 84), embed(d[:, None, :].expand_as(p), 4).reshape(-1, 27), nrm[..., 0])
