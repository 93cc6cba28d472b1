"""The samplers in float64, checked forwards: where do the samples go, round by round.

The render kernels that place the samples (NeuS: neus_upsample, neus_direct_upsample, neus_merge,
sample_pdf_ray*; VolSDF: volsdf_first / vs_decide / vs_finalize) end in an inverse CDF whose
`denom < 1e-5` switch sits on the mass of an empty bin, so comparing emitted depths fp32 against fp32
cannot be strict.  Here a round is checked in the other direction.  Its inputs are taken as they are
(the sorted depths and the SDF values the sampler itself read), the round's CDF is rebuilt from them in
float64 with the reference's lines restated one by one (oracle/neus.py:80-93, oracle/volsdf.py:12-48,
oracle/rays.py:81-93; every constant and quirk as there), and that CDF evaluated at every emitted depth
has to return the uniform the depth was drawn for.  Either side of the switch lands within 1e-5 of u in
CDF space, so no sample is excused.

What this check cannot see (tests/test_sampler_ref.py runs the mutants):
- the lower slope clamp at -10 does not bind on the fixture nets (|d sdf / d t| <= 1 for an SDF);
- a leading previous slope equal to the first slope instead of 0 is equivalent after min and clamp
  whenever the first slope is negative or clamped, which it is on these rays;
- removing the `denom < 1e-5` switch moves a sample by less than 1e-5 in CDF space by construction; the
  switch itself stays held by the bit-for-bit sample_pdf tests (test_gpu_reintegrate.py).

The second half is an fp32 replay of the same rounds with single faults switched in (`mut`): the
stand-in for a wrong kernel that the host tests feed to the checker.
"""
import collections

import numpy as np
import torch

F64 = torch.float64

# ---------------------------------------------------------------------------------------------
# Tolerances of tests/test_gpu_sampler_rounds.py.  Each is twice what the fp32 oracle itself needs on
# the test's own rays (the device's expf and the host's differ by ulps, which at most doubles a
# weight's rounding); tests/test_sampler_ref.py measures the oracle's figures and holds these to them.
# ---------------------------------------------------------------------------------------------
K_REF = 0.4108        # NeuS: largest (residual - 1e-5) / (2**-24 L / total64) of the fp32 oracle
DELTA_REF = 4.392e-7    # VolSDF: largest relative error of the fp32 oracle's bound maximum against float64
R_REF = 5.086e-7        # VolSDF: largest forward residual of the fp32 oracle's fine samples
K_GPU, DELTA_GPU, R_GPU = 2 * K_REF, 2 * DELTA_REF, 2 * R_REF
SWITCH = 1e-5      # the width of sample_pdf's `denom < 1e-5` switch in CDF space


def _f64(x):
    if torch.is_tensor(x):
        return x.detach().cpu().to(F64)
    return torch.as_tensor(np.asarray(x), dtype=F64)


def alpha_to_w(alpha, inclusive=False):
    # neus.py:57-70: w_i = alpha_i * prod_{j<i}(1 - alpha_j + 1e-10)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1.0 - alpha + 1e-10], -1), -1)
    return alpha * (T[..., 1:] if inclusive else T[..., :-1])


def _neus_round(dv, sv, it, mut=None):
    """one 'official_solution' round (oracle/neus.py:80-93) in the dtype of its inputs"""
    s0, s1 = sv[..., :-1], sv[..., 1:]
    z0, z1 = dv[..., :-1], dv[..., 1:]
    mid = (s0 + s1) * 0.5
    slope = (s1 - s0) / (z1 - z0 + (0.0 if mut == 'slope_no_eps' else 1e-5))
    lead = slope[..., :1] if mut == 'lead_first_slope' else torch.zeros_like(slope[..., :1])
    prev = torch.cat([lead, slope[..., :-1]], -1)
    m = slope if mut == 'no_prev_slope' else torch.min(torch.stack([prev, slope], -1), -1)[0]
    if mut == 'no_upper_clamp':
        m = m.clamp_min(-10.0)
    else:
        m = m.clamp_max(0.0) if mut == 'no_lower_clamp' else m.clamp(-10.0, 0.0)
    dist = z1 - z0
    e0 = mid - m * dist * 0.5
    e1 = mid + m * dist * 0.5
    s = 64 * (2 ** {'std_next_round': it + 1, 'std_const_64': 0}.get(mut, it))
    c0 = torch.sigmoid(e0 * s)
    c1 = torch.sigmoid(e1 * s)
    a = (c0 - c1 + (0.0 if mut == 'alpha_no_eps' else 1e-5)) / (c0 + 1e-5)
    return alpha_to_w(a, inclusive=mut == 'inclusive_T')


def neus_round_weights(d, sdf, it):
    """float64 weights [n, L-1] of upsampling round `it` on the sorted depths d and their SDF [n, L]"""
    return _neus_round(_f64(d), _f64(sdf), it)


def _direct(sv, s):
    # neus.py:28-35 at s = 1 / fixed_s_recp, then alpha_to_w
    c = torch.sigmoid(sv * s)
    a = torch.clamp_min((c[..., :-1] - c[..., 1:]) / (c[..., :-1] + 1e-10), 0)
    return alpha_to_w(a)


def neus_direct_weights(sdf, s):
    """float64 weights of 'direct_use' / 'direct_more'"""
    return _direct(_f64(sdf), float(s))


def pdf_cdf(w):
    """sample_pdf's cdf (rend_util.py:255-264): (w + 1e-5) / sum, running sum with a zero in front.
    Returns cdf [n, L] and total = sum(w + 1e-5) [n]."""
    w = _f64(w) + 1e-5
    total = torch.sum(w, -1, keepdim=True)
    pdf = w / total
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    return cdf, total[..., 0]


def _sigma(sdf, alpha, beta):
    # volsdf.py:16-35
    e = 0.5 * torch.exp(-torch.abs(sdf) / beta)
    return alpha * torch.where(sdf >= 0, e, 1 - e)


def _Rt(d, sdf, alpha, beta, mut=None):
    # volsdf.py:57-61, :107-112: exclusive running sum of sigma * delta that has lost its last entry
    sigma = _sigma(sdf, alpha, beta)
    delta = d[..., 1:] - d[..., :-1]
    sd = (sigma[..., 1:] if mut == 'sigma_far_end' else sigma[..., :-1]) * delta
    Rt = torch.cat([torch.zeros_like(sd[..., :1]), torch.cumsum(sd, -1)], -1)
    return Rt, delta


def _bound(d, sdf, alpha, beta):
    # volsdf.py:38-74
    Rt, delta = _Rt(d, sdf, alpha, beta)
    a = torch.abs(sdf)
    dstar = torch.clamp_min(0.5 * (a[..., :-1] + a[..., 1:] - delta), 0.)
    err = alpha / (4 * beta) * (delta ** 2) * torch.exp(-dstar / beta)
    b = torch.exp(-Rt[..., :-1]) * (torch.exp(torch.cumsum(err, -1)) - 1.)
    b[torch.isnan(b)] = np.inf
    return b


def _ab(alpha, beta):
    """scalars, or one value per ray as a column"""
    a, b = _f64(alpha), _f64(beta)
    return (a.reshape(-1, 1) if a.ndim else a), (b.reshape(-1, 1) if b.ndim else b)


def volsdf_bound(d, sdf, alpha, beta):
    """float64 error bound per interval [n, L-1] (NaN -> inf)"""
    return _bound(_f64(d), _f64(sdf), *_ab(alpha, beta))


def _opacity_cdf(d, sdf, alpha, beta, mut=None):
    Rt, _ = _Rt(d, sdf, alpha, beta, mut)
    if mut == 'cdf_unshifted':  # the opacity at bin j itself
        return 1 - torch.exp(-Rt)
    # sample_cdf (rend_util.py:294-300) puts a zero in front of 1 - exp(-R_t[:-1]): cdf entry j is the
    # opacity at bin j - 1
    o = 1 - torch.exp(-Rt[..., :-1])
    return torch.cat([torch.zeros_like(o[..., :1]), o], -1)


def volsdf_opacity_cdf(d, sdf, alpha, beta):
    """float64 cdf [n, L] that the final sample_cdf inverts; not normalised (its last entry is < 1)"""
    return _opacity_cdf(_f64(d), _f64(sdf), *_ab(alpha, beta))


# ---------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------
def _np64(x):
    return x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, np.float64)


def forward_residual(bins, cdf, d_new, u):
    """bins, cdf [n, L]; d_new [n, m] in any order; u [n, m] or [m] in any order.  Depths and uniforms
    are matched in sorted order (an inverse CDF is monotone).  The piecewise-linear CDF at a depth is the
    interval [F_lo, F_hi] of its limits from the left and from the right: a list holds duplicate depths
    (u = 0 returns near again) and a zero-width bin carries mass.  Below the first bin F_lo = 0, at or
    above the last F_hi = 1 (an unnormalised cdf sends every u above its last entry to the last bin).
    Returns max(0, F_lo - u, u - F_hi) [n, m], in the sorted order of d_new."""
    bins, cdf, d_new, u = _np64(bins), _np64(cdf), _np64(d_new), _np64(u)
    n, L = bins.shape
    assert cdf.shape == (n, L) and d_new.shape[0] == n
    u = np.broadcast_to(u, d_new.shape)
    x, us = np.sort(d_new, -1), np.sort(u, -1)
    res = np.empty_like(x)
    for r in range(n):
        b, c, xr = bins[r], cdf[r], x[r]

        def lin(k):  # the segment k - 1 -> k at xr, for 1 <= k <= L - 1
            k = np.clip(k, 1, L - 1)
            w = b[k] - b[k - 1]
            t = np.where(w > 0, (xr - b[k - 1]) / np.where(w > 0, w, 1.0), 0.0)
            return c[k - 1] + t * (c[k] - c[k - 1])
        i = np.searchsorted(b, xr, side='left')    # bins below x
        j = np.searchsorted(b, xr, side='right')   # bins at or below x
        f_lo = np.where(i == 0, 0.0, np.where(i == L, c[L - 1], lin(i)))
        f_hi = np.where(j == L, 1.0, np.where(j == 0, 0.0, lin(j)))
        res[r] = np.maximum(0.0, np.maximum(f_lo - us[r], us[r] - f_hi))
    return res


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32).astype(np.uint64)


def multiset_split(D_after, D_before, S_after=None, S_before=None):
    """The new depths [n, m] of a round, in the order of D_after (with the SDF lists given: as (depth,
    sdf) pairs, and the new SDF values as a second result).  Asserts that every old entry is still
    there, bit for bit, as a multiset."""
    A, B = _bits(_np64(D_after)), _bits(_np64(D_before))
    if S_after is not None:
        A = (A << np.uint64(32)) | _bits(_np64(S_after))
        B = (B << np.uint64(32)) | _bits(_np64(S_before))
    n, m = A.shape[0], A.shape[1] - B.shape[1]
    assert m >= 0 and B.shape[0] == n
    idx = np.empty((n, m), np.int64)
    for r in range(n):
        left = collections.Counter(B[r].tolist())
        new = []
        for k, key in enumerate(A[r].tolist()):
            if left.get(key, 0) > 0:
                left[key] -= 1
            else:
                new.append(k)
        lost = sum(left.values())
        assert lost == 0 and len(new) == m, f'ray {r}: {lost} old entries missing, {len(new)} new instead of {m}'
        idx[r] = new
    d = np.take_along_axis(np.asarray(_np64(D_after)), idx, -1)
    if S_after is None:
        return d
    return d, np.take_along_axis(np.asarray(_np64(S_after)), idx, -1)


def neus_tol(L, total64, K):
    """per ray: the switch's width, plus the fp32 rounding of L weights of size O(1) after the division by
    the ray's total (a ray that misses the object has total ~ 1e-3: fp32 cannot define its CDF better)"""
    return SWITCH + K * 2.0 ** -24 * L / _np64(total64)


def worst(res, tol):
    """(largest residual / tol, its ray) of residuals [n, m] against a per-ray or scalar tol"""
    ratio = res / np.reshape(np.broadcast_to(np.asarray(tol, np.float64), res.shape[:1]), (-1, 1))
    r = int(np.argmax(ratio.max(-1))) if ratio.size else 0
    return (float(ratio.max()) if ratio.size else 0.0), r


def lerp32(near, far, t):
    """near (1 - t) + far t in numpy fp32, each operation rounded separately (neus.py:209-210)"""
    near, far, t = (np.asarray(a, np.float32) for a in (near, far, t))
    return (near * (np.float32(1) - t)).astype(np.float32) + (far * t).astype(np.float32)


def points32(o, d, depths):
    """o + d * depth in numpy fp32: o, d [n, 3], depths [n, L] -> [n, L, 3]"""
    o, d, depths = (np.asarray(a, np.float32) for a in (o, d, depths))
    return o[:, None, :] + (d[:, None, :] * depths[:, :, None]).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# fp32 replay with single faults: the oracle's lines in fp32 (bit-identical to oracle.neus /
# oracle.volsdf / oracle.rays without a fault; the host tests assert that), `mut` switching one in
# ---------------------------------------------------------------------------------------------
NEUS_MUTANTS = ('std_next_round', 'std_const_64', 'no_prev_slope', 'no_upper_clamp', 'slope_no_eps', 'alpha_no_eps',
                'inclusive_T', 'weights_no_eps', 'bin_shift')
VOLSDF_MUTANTS = ('cdf_unshifted', 'sigma_far_end')
NEUS_EQUIVALENT = ('no_lower_clamp', 'lead_first_slope')  # faults that change nothing on these rays (see above)


def _invert(bins, cdf, u, mut=None, eps=1e-5):
    # rend_util.py:266-292
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=False)
    lo = torch.clamp_min(inds - 1, 0)
    hi = torch.clamp_max(inds, cdf.shape[-1] - 1)
    c0, c1 = torch.gather(cdf, -1, lo), torch.gather(cdf, -1, hi)
    if mut == 'bin_shift':
        lo, hi = torch.clamp_max(lo + 1, cdf.shape[-1] - 1), torch.clamp_max(hi + 1, cdf.shape[-1] - 1)
    b0, b1 = torch.gather(bins, -1, lo), torch.gather(bins, -1, hi)
    denom = c1 - c0
    denom = torch.where(denom < eps, torch.ones_like(denom), denom)
    return b0 + (u - c0) / denom * (b1 - b0)


def replay_sample_pdf(bins, w, u, mut=None):
    w = w + (0.0 if mut == 'weights_no_eps' else 1e-5)
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    return _invert(bins, cdf, u, mut)


def replay_neus_round(dv, sv, it, u, mut=None):
    """fp32 depths [n, m] that round `it` draws from (dv, sv) [n, L] for the uniforms u [n, m]"""
    assert dv.dtype == torch.float32 and sv.dtype == torch.float32 and u.dtype == torch.float32
    return replay_sample_pdf(dv, _neus_round(dv, sv, it, mut), u, mut)


def replay_neus_direct(bins, sv, s, u):
    return replay_sample_pdf(bins, _direct(sv, float(s)), u)


def replay_volsdf_fine(dv, sv, alpha, beta, u, mut=None):
    """fp32 opacity_invert_cdf_sample (volsdf.py:104-117); alpha, beta scalars or [n, 1] fp32"""
    assert dv.dtype == torch.float32 and sv.dtype == torch.float32
    return _invert(dv, _opacity_cdf(dv, sv, alpha, beta, mut), u)


# ---------------------------------------------------------------------------------------------
# what tests/test_sampler_ref.py (the fp32 oracle as the sampler) and tests/test_gpu_sampler_rounds.py
# (the kernels as the sampler) share: cases, uniforms and the per-round checks
# ---------------------------------------------------------------------------------------------
NEUS_CAM, NEUS_SEED = 'b', 1     # reintegrate_ref.camera_rays('b'): through, grazing and past the object
N_COARSE, N_UP, N_ROUNDS = 64, 16, 4
U_SEED = 7411
# VolSDF first pass: name -> (N_samples, beta, NeRF++).  Each beta is chosen on the CPU so that both
# branches of the decision occur among the 130 rays of camera (a) and the fp32 oracle has no ray inside
# the delta band (the bound's maximum crosses eps within a few percent of beta: 0.25 / 0.30 at
# N_samples 16, 0.065 / 0.072 at 64).
VOLSDF_CAM, VOLSDF_SEED, VOLSDF_N_IMPORTANCE, VOLSDF_EPS, VOLSDF_FAR = 'a', 2, 64, 0.1, 6.0
VOLSDF_CASES = {
    'n16': (16, 0.275, False),
    'n17': (17, 0.26, False),
    'n64': (64, 0.069, False),
    'n16_nerfpp': (16, 0.255, True),
}
BAND_CAP = 0.02


def uniform_block(seed, *shape):
    """one fixed CPU-seeded block of uniforms"""
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def det_u(m):
    return torch.linspace(0.0, 1.0, steps=m)


def neus_round_check(D_prev, S_prev, D_k, S_k, it, u):
    """One ladder step.  Prefix: (D_prev, S_prev) is contained in (D_k, S_k) as a multiset of pairs, bit for
    bit, exactly N_UP depths are new, D_k is sorted and finite.  Forward: the residual [n, N_UP] of the
    new depths against the float64 CDF of round `it`, and the ray's float64 total."""
    Dk = _np64(D_k)
    assert np.isfinite(Dk).all() and (np.diff(Dk, axis=-1) >= 0).all(), 'depths not sorted and finite'
    new, _ = multiset_split(D_k, D_prev, S_k, S_prev)
    assert new.shape[-1] == N_UP, new.shape
    cdf, total = pdf_cdf(neus_round_weights(D_prev, S_prev, it))
    return forward_residual(D_prev, cdf, new, u), total.numpy()


def neus_k_ratio(res, L, total64):
    """(residual - 1e-5) / (2**-24 L / total64): the K that a residual needs"""
    return (res - SWITCH) / (2.0 ** -24 * L / np.asarray(total64, np.float64))[:, None]


def volsdf_beta_plus(far, N0, eps=VOLSDF_EPS):
    """volsdf.py:127-129 in fp32: sqrt(far^2 / (4 (N0 - 1) log(1 + eps))), far a scalar or per ray, every
    operation rounded once (numpy: IEEE square root, as the kernel's sqrtf; torch.sqrt on the host is an
    ulp off on some CPU builds)"""
    far = np.asarray(far, np.float32).reshape(-1)
    k = np.float32(4 * (N0 - 1) * np.log(1 + eps))
    return np.sqrt(((far * far).astype(np.float32) / k).astype(np.float32)).astype(np.float32)


def volsdf_first_check(d_init, sdf, alpha_net, beta_net, beta_plus, usage, beta_map, fine, u, delta, r_tol,
                       eps=VOLSDF_EPS):
    """The first sampling pass of every ray (max_upsample_steps = 0) from its inputs d_init, sdf [n, N0].
    Decision: with B64 the float64 bound's maximum, rays with B64 <= eps (1 - delta) report iter_usage 0 and
    beta_net, rays with B64 > eps (1 + delta) report -1 and their fp32 beta+ (beta_plus [n] or [1]); rays in
    between are not judged.  Samples: the fine depths [n, m] against the float64 opacity CDF at the
    (alpha, beta) of the branch the ray reported, residual <= r_tol.  Returns the figures; asserts."""
    n = d_init.shape[0]
    usage, beta_map = np.asarray(usage, np.float32).reshape(n), np.asarray(beta_map, np.float32).reshape(n)
    bplus = np.broadcast_to(np.asarray(beta_plus, np.float32).reshape(-1), (n,))
    bnet, anet = np.float32(beta_net), np.float32(alpha_net)
    B64 = volsdf_bound(d_init, sdf, float(anet), float(bnet)).max(-1).values.numpy()
    conv, nonc = B64 <= eps * (1 - delta), B64 > eps * (1 + delta)
    band = ~(conv | nonc)
    bad = (conv & ~((usage == 0) & (beta_map == bnet))) | (nonc & ~((usage == -1) & (beta_map == bplus)))
    assert not bad.any(), ('decision', np.nonzero(bad)[0].tolist(), B64[bad].tolist(), usage[bad].tolist(),
                           beta_map[bad].tolist())
    assert set(np.unique(usage).tolist()) <= {0.0, -1.0}, np.unique(usage)
    rep = usage == 0
    beta = np.where(rep, bnet, bplus).astype(np.float32)
    alpha = np.where(rep, anet, (np.float32(1) / bplus).astype(np.float32)).astype(np.float32)
    res = forward_residual(d_init, volsdf_opacity_cdf(d_init, sdf, alpha, beta), fine, u)
    w, r = worst(res, r_tol)
    assert w <= 1.0, ('samples', 'residual / tol', w, 'ray', r)
    return dict(B64=B64, n_conv=int(conv.sum()), n_nonc=int(nonc.sum()), band=float(band.mean()), res=float(res.max()),
                worst=w, ray=r)
