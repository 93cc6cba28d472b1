"""UNISURF's root finder and sample placement, held stage by stage with the SDF as a black box `f`.

The path under test: uni_prologue / rf_prologue, run_march with uni_march_scan / gather / scatter,
uni_root, uni_secant, uni_samples and rf_finish (nr_unisurf.hip), nr_root_find (nr_surface.hip).  `f` is
whatever evaluates the occupancy logit at fp32 points: the fp32 oracle on the host
(tests/test_unisurf_stages_ref.py), the model's own plain forward on the GPU
(tests/test_gpu_unisurf_stages.py).  No check needs to know how `f` is computed.

Stage 1, crossing and flags (ray_casting.py:89-131).  The march depths near (1 - t_i) + far t_i and the
march points are rebuilt in plain fp32, every operation rounded once, v_i = f_i - tau.  A ray is decided
when |v_i| > BAND for every i up to and including its first crossing pair (the whole march without a
crossing).  On a decided ray mask, mask_sign_change, the first-sample-free flag (d == 0) and the bracket
[d_idx, d_idx+1] of a hit, widened by one ulp, equal the restatement exactly.  An undecided ray has to
match the restatement as it is, or with the sign of its first in-band value reversed.  BAND covers the one
freedom the root finder has: its point arithmetic may contract into FMAs.

Stage 2, the secant ladder (ray_casting.py:11-30): N_secant_steps = k for k in RUNGS, replayed in float64
from the bracket of stage 1, every step calling `f` at the fp32-rounded point; |d - d_replay| <= D_GPU on
every decided hit.

Stage 4, the sample depths (unisurf.py:152-203): closed-form fp32 from near, far, the surface depth and
the crossing flag, replayed in numpy fp32 in the reference's order of operations and compared bit for bit.

What these checks cannot see (tests/test_unisurf_stages_ref.py runs the mutants):
- one secant step missing at k = 8: rung 7 and rung 8 differ by 7.2e-7 at most on these rays, below D_GPU;
  the step count is held at rungs 0 to 3, where a step moves the depth by 3.7e-5 to 8e-3;
- on real rays, a hit formed without the `pos2neg` test alone, or without `first_free` alone: unless a march
  value is exactly 0 the two are the same test (see FLAG_EQUIVALENT); a hit formed without both is seen on the
  IN rays, and the host test shows the checker rejecting each single fault on a synthetic march through 0;
- a bracket update that differs only when f_mid is exactly 0 (`< 0` against `<= 0`): no ray lands there;
- a crossing read from a product that underflows to 0 (|v_i v_{i+1}| < 1e-45): BAND is far above it;
- the repair pass after uni_samples' two-run merge: it only moves a sample when a run is itself out of
  order by rounding, which no configuration here provokes (the `no_final_sort` mutant drops the sort of the
  concatenated runs, the reference's line, which is seen on every ray without a crossing);
- near / far of the default geometry on rays with a crossing: only near (the first sample) and, without a
  crossing, far (the surface depth) come out of a render;
- the F.normalize windows and uni_composite, which other tests hold.

The second half is an fp32 replay of the same stages with single faults switched in (`mut`): the stand-in
for a wrong kernel that the host tests feed to the checkers.
"""
import numpy as np
import torch
import torch.nn.functional as F

from sampler_ref import lerp32, points32

# ---------------------------------------------------------------------------------------------
# Constants measured by tests/test_unisurf_stages_ref.py on the rays below and held there.
# BAND_REF: largest |p_fma - p_plain| over every march point of E, IN and T, p_fma the product and sum
# rounded once.  BAND = 4 BAND_REF: near / far may be contracted as well in the default geometry, and a
# lerp feeds a point.  D_REF: largest gap between the fp32 oracle's own secant loop and its float64 replay,
# over all rungs and ray sets.
# ---------------------------------------------------------------------------------------------
BAND_REF = 4.769e-7
D_REF = 1.671e-6
BAND = 4 * BAND_REF
D_GPU = 2 * D_REF

SEED, CAM, RADIUS = 3, 'e', 4.0
TAUS = (0.0, 0.5)
N_STEPS, N_SECANT = 256, 8
RUNGS = (0, 1, 2, 3, 8)
H_T = 0.02
T_CASES = ((64, 0), (64, 30), (64, 31), (64, 32), (64, 62), (33, 31), (2, 0))  # (N, k): first crossing in pair k
T_LADDER = (64, 31)
N_E, N_IN = 130, 32
RAYSCHUNK = 64       # 162 rays: chunks of 64, 64 and 34
DECIDED_MIN = 0.98
MIN_HITS = {0.0: 40, 0.5: 100}   # decided hits a secant check has to judge (the oracle has 50 and 119 on E)
GEOMETRIES = {
    'default': dict(radius_of_interest=RADIUS),
    'bypass': dict(near_bypass=0.5, far_bypass=4.5, too_close_threshold=0.125),       # thr = 0.5 + 4 * 0.125
    'zero': dict(near_bypass=0.0, far_bypass=4.0, too_close_threshold=0.0),           # thr = 0: d_lo2 can be 0
}
SAMPLE_COUNTS = ((64, 32), (5, 3), (1, 1))
INTERVALS = (1.0, 1e-3, 8.0)
U_SEED = 9157
EPS32 = 2.0 ** -23


# ---------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------
def rays_E():
    """the 130 pixels arange(0, 4096, 31)[:130] of camera (e): origins and unnormalised directions [130, 3]"""
    import weightgen as wg
    from oracle import rays as orays
    H, W, f, dist = wg.CAMERAS[CAM]
    ro, rd, _ = orays.get_rays(wg.look_at_c2w(dist)[None], wg.intrinsics(f, H, W)[None], H, W)
    idx = torch.arange(0, H * W, 31)[:N_E]
    return ro[0, idx].contiguous().numpy(), rd[0, idx].contiguous().numpy()


def rays_IN():
    """32 rays that start inside the surface: one RandomState(0), directions first"""
    rs = np.random.RandomState(0)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    d = unit(rs.normal(size=(N_IN, 3)))
    o = 0.3 * unit(rs.normal(size=(N_IN, 3)))
    return o.astype(np.float32), d.astype(np.float32)


def rays_all():
    (oe, de), (oi, di) = rays_E(), rays_IN()
    return np.concatenate([oe, oi]), np.concatenate([de, di])


def normalize_host(rd):
    return F.normalize(torch.from_numpy(np.asarray(rd, np.float32)), dim=-1).numpy()


def near_far32(o, d, r=RADIUS):
    """rend_util.py:167-185 in fp32 (o, d [n, 3], d normalised)"""
    from oracle import rays as orays
    near, far = orays.near_far_from_sphere(torch.from_numpy(o), torch.from_numpy(d), r=r, keepdim=False)
    return near.numpy(), far.numpy()


def near_far64(o, d, r=RADIUS):
    mid = -np.sum(o.astype(np.float64) * d.astype(np.float64), -1)
    return np.maximum(mid - r, 0.0), np.maximum(mid + r, r)


def near_far_tol(o, r=RADIUS):
    return 4 * EPS32 * (np.linalg.norm(o.astype(np.float64), axis=-1) + r)


def t_case(dstar, N, k, h=H_T):
    """per-ray near / far that put the depth d* in the middle of pair k of an N-step march of step h"""
    near = (np.asarray(dstar, np.float64) - (k + 0.5) * h).astype(np.float32)
    far = (near.astype(np.float64) + (N - 1) * h).astype(np.float32)
    return near, far


def uniform_block(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def linspace32(n):
    return torch.linspace(0.0, 1.0, steps=n).numpy()


# ---------------------------------------------------------------------------------------------
# stage 1
# ---------------------------------------------------------------------------------------------
def march(f, o, d, near, far, tau, N):
    """plain fp32: depths [n, N], points [n, N, 3], v = f - tau [n, N]"""
    n = o.shape[0]
    near = np.broadcast_to(np.asarray(near, np.float32), (n,))
    far = np.broadcast_to(np.asarray(far, np.float32), (n,))
    dp = lerp32(near[:, None], far[:, None], linspace32(N)[None])
    pts = points32(o, d, dp)
    v = (np.asarray(f(pts), np.float32) - np.float32(tau)).astype(np.float32)
    return dp, pts, v


def fma_gap(o, d, dp, pts):
    """largest |p_fma - p_plain|: the point with its product and sum rounded once, against plain fp32"""
    exact = o.astype(np.float64)[:, None, :] + d.astype(np.float64)[:, None, :] * dp.astype(np.float64)[:, :, None]
    return float(np.abs(exact.astype(np.float32).astype(np.float64) - pts.astype(np.float64)).max())


def flags(v, mut=None):
    """ray_casting.py:89-110 on v [n, N]: first_free, crossing, hit, idx (the pair (idx, idx + 1))"""
    n, N = v.shape
    first_free = v[:, 0] > 0
    sgn = np.concatenate([np.sign(v[:, :-1] * v[:, 1:]), np.ones((n, 1), np.float32)], -1)
    w = np.arange(1, N + 1) if mut == 'last_crossing' else np.arange(N, 0, -1)
    cost = sgn * w.astype(np.float32)
    idx = np.argmin(cost, -1)
    crossing = cost.min(-1) < 0
    pos2neg = v[np.arange(n), idx] > 0
    hit = crossing.copy()
    if mut not in ('no_pos2neg', 'hit_is_crossing'):
        hit &= pos2neg
    if mut not in ('no_first_free', 'hit_is_crossing'):
        hit &= first_free
    return first_free, crossing, hit, idx


def _in_band(v, idx, crossing, band):
    """[n, N]: the values that decide a ray's flags and lie in the band (a NaN counts as in it)"""
    N = v.shape[-1]
    upto = np.where(crossing, idx + 1, N - 1)
    return ~(np.abs(v) > band) & (np.arange(N)[None] <= upto[:, None])


def _expected_miss(first_free, near, far, fill):
    """d of a ray without a hit: fill 'inf' / 'far' as ray_casting.py:151-152, 'clamped' as unisurf.py:152
    on top of fill_inf=False"""
    n = first_free.shape[0]
    far = np.broadcast_to(np.asarray(far, np.float32), (n,))
    near = np.broadcast_to(np.asarray(near, np.float32), (n,))
    d = np.where(first_free, np.float32(np.inf) if fill == 'inf' else far, np.float32(0)).astype(np.float32)
    return np.maximum(np.minimum(d, far), near) if fill == 'clamped' else d


def _reading_ok(v, dp, near, far, mask, msc, d, fill):
    first_free, crossing, hit, idx = flags(v)
    n = v.shape[0]
    rows = np.arange(n)
    i1 = np.minimum(idx + 1, v.shape[1] - 1)
    lo = np.nextafter(dp[rows, idx], np.float32(-np.inf))
    hi = np.nextafter(dp[rows, i1], np.float32(np.inf))
    d_ok = np.where(hit, (d >= lo) & (d <= hi), d == _expected_miss(first_free, near, far, fill))
    ok = (mask == hit) & d_ok
    if msc is not None:
        ok &= msc == crossing
    return ok, (first_free, crossing, hit, idx)


def stage1_check(tag, v, dp, near, far, mask, msc, d, band=BAND, fill='inf'):
    """v, dp [n, N] of the plain replay; mask, msc (or None), d [n] of the code under test.  Asserts the
    flags and the bracket on every ray; returns the restatement's flags, which rays are decided, and for the
    undecided ones the crossing flag of the other reading."""
    mask, d = np.asarray(mask, bool), np.asarray(d, np.float32)
    msc = None if msc is None else np.asarray(msc, bool)
    ok, (first_free, crossing, hit, idx) = _reading_ok(v, dp, near, far, mask, msc, d, fill)
    inb = _in_band(v, idx, crossing, band)
    decided = ~inb.any(-1)
    cross_alt = crossing.copy()
    for r in np.nonzero(~decided)[0]:  # the other reading: the first in-band value with its sign reversed
        j = int(np.argmax(inb[r]))
        v2 = v[r:r + 1].copy()
        v2[0, j] = np.float32(-band if v2[0, j] >= 0 else band)
        pick = lambda a: a if a is None or np.ndim(a) == 0 else np.asarray(a)[r:r + 1]
        ok2, fl2 = _reading_ok(v2, dp[r:r + 1], pick(near), pick(far), mask[r:r + 1], pick(msc), d[r:r + 1], fill)
        ok[r] |= ok2[0]
        cross_alt[r] = fl2[1][0]
    bad = np.nonzero(~ok)[0]
    first = lambda a: a[bad].tolist()[:8]
    assert bad.size == 0, (tag, 'flags / bracket differ on rays', bad.tolist()[:8], 'decided', first(decided), 'mask',
                           first(mask), 'd', first(d), 'expected hit', first(hit), 'idx', first(idx))
    upto = np.where(crossing, idx + 1, v.shape[1] - 1)[:, None]
    min_abs_v = float(np.abs(np.where(np.arange(v.shape[1])[None] <= upto, v, np.inf)).min())
    return dict(first_free=first_free, crossing=crossing, hit=hit, idx=idx, decided=decided, cross_alt=cross_alt,
                share=float(decided.mean()), min_abs_v=min_abs_v)


# ---------------------------------------------------------------------------------------------
# stage 2
# ---------------------------------------------------------------------------------------------
def _secant(d_lo, f_lo, d_hi, f_hi):
    return -f_lo * (d_hi - d_lo) / (f_hi - f_lo) + d_lo


def secant64(f, o, d, dp, v, idx, tau, k):
    """ray_casting.py:11-30 in float64 on the rays given (hits): the bracket (idx, idx + 1) of the plain
    march, k steps, f called at the point rounded to fp32"""
    rows = np.arange(o.shape[0])
    i1 = np.minimum(idx + 1, v.shape[1] - 1)
    d_hi, f_hi = dp[rows, idx].astype(np.float64), v[rows, idx].astype(np.float64)
    d_lo, f_lo = dp[rows, i1].astype(np.float64), v[rows, i1].astype(np.float64)
    o64, d64, tau64 = o.astype(np.float64), d.astype(np.float64), float(np.float32(tau))
    dpred = _secant(d_lo, f_lo, d_hi, f_hi)
    for _ in range(k):
        p = (o64 + dpred[:, None] * d64).astype(np.float32)
        fm = np.asarray(f(p), np.float32).astype(np.float64) - tau64
        low = fm < 0
        d_lo, f_lo = np.where(low, dpred, d_lo), np.where(low, fm, f_lo)
        d_hi, f_hi = np.where(low, d_hi, dpred), np.where(low, f_hi, fm)
        dpred = _secant(d_lo, f_lo, d_hi, f_hi)
    return dpred


def stage2_check(tag, f, o, d, dp, v, s1, tau, k, d_got, tol=D_GPU):
    """|d - d_replay| on every decided hit of stage 1's result s1; returns (worst gap, its ray, hits judged)"""
    rows = np.nonzero(s1['hit'] & s1['decided'])[0]
    if rows.size == 0:
        return 0.0, -1, 0
    ref = secant64(f, o[rows], d[rows], dp[rows], v[rows], s1['idx'][rows], tau, k)
    gap = np.abs(np.asarray(d_got, np.float64)[rows] - ref)
    w = int(np.argmax(~(gap <= tol) * 1e30 + np.nan_to_num(gap)))
    assert (gap <= tol).all(), (tag, f'rung {k}', 'gap / tol', float(gap[w] / tol), 'ray', int(rows[w]))
    return float(gap.max()), int(rows[w]), int(rows.size)


def points_tol(o, depth):
    return 4 * EPS32 * (np.linalg.norm(o.astype(np.float64), axis=-1) + np.abs(depth.astype(np.float64)))


def points_check(tag, o, d, depth, pts, mask):
    """pts = o + depth dir on hits within 4 2^-23 (|o| + depth), exactly 1 elsewhere"""
    mask = np.asarray(mask, bool)
    want = o.astype(np.float64) + depth.astype(np.float64)[:, None] * d.astype(np.float64)
    with np.errstate(invalid='ignore'):
        err = np.abs(pts.astype(np.float64) - want).max(-1)
    assert (err[mask] <= points_tol(o, depth)[mask]).all(), (tag, 'points on hits', float(err[mask].max()))
    assert (pts[~mask] == 1.0).all(), (tag, 'points off hits are not 1')


# ---------------------------------------------------------------------------------------------
# stage 4
# ---------------------------------------------------------------------------------------------
def _run32(a, b, n, u, mut=None):
    """unisurf.py:158-169 / :187-198: n samples on [a, b], the linspace points or one uniform per bin"""
    if u is None:
        return lerp32(a[:, None], b[:, None], linspace32(n)[None])
    t = linspace32(n + 1)
    if mut == 'edges_linspace_n':  # the table of the unperturbed run, its last bin closed at 1
        t = np.concatenate([linspace32(n), np.ones(1, np.float32)])
    s = lerp32(a[:, None], b[:, None], t[None])
    lower, upper = s[:, :-1], s[:, 1:]
    return lower + ((upper - lower).astype(np.float32) * np.asarray(u, np.float32)).astype(np.float32)


def replay_d_all(near, far, thr, depth_surface, crossing, interval, N_query, N_freespace, u_q=None, u_f=None, mut=None):
    """unisurf.py:152-203 in numpy fp32 from the clamped surface depth [n] and the crossing flag [n]"""
    dc = np.asarray(depth_surface, np.float32)
    n = dc.shape[0]
    near, far, thr = (np.broadcast_to(np.asarray(a, np.float32), (n,)) for a in (near, far, thr))
    iv = np.float32(interval)
    d_up, d_lo = dc + iv, dc - iv
    if mut != 'no_clamps':
        d_up, d_lo = np.minimum(d_up, far), np.maximum(d_lo, near)
    if mut == 'chunk0_uniforms':  # the second ray chunk draws the first one's uniforms again
        u_q, u_f = (None if u is None else np.concatenate([u[:RAYSCHUNK], u[:RAYSCHUNK], u[2 * RAYSCHUNK:]])[:n]
                    for u in (u_q, u_f))
    d_int = _run32(d_lo, d_up, N_query, u_q, mut)
    d_lo2 = d_lo if mut == 'thr_ignored' else np.maximum(d_lo, thr)
    if mut != 'dlo2_not_reset':
        d_lo2 = np.where(np.asarray(crossing, bool), d_lo2, far)
    if mut != 'no_switch':
        d_lo2 = np.where(d_lo2 < np.float32(1e-10), far, d_lo2)
    d_free = _run32(near, d_lo2.astype(np.float32), N_freespace, u_f, mut)
    d_all = np.concatenate([d_free, d_int], -1).astype(np.float32)
    return d_all if mut == 'no_final_sort' else np.sort(d_all, -1)


def stage4_check(tag, d_all, near, far, thr, depth_surface, s1, interval, N_query, N_freespace, u_q=None, u_f=None):
    """np.array_equal on every sample of every ray; an undecided ray of stage 1 may take either crossing flag"""
    d_all = np.asarray(d_all)
    assert d_all.dtype == np.float32 and d_all.shape[-1] == N_query + N_freespace, (tag, d_all.dtype, d_all.shape)
    assert np.isfinite(d_all).all() and (np.diff(d_all, axis=-1) >= 0).all(), (tag, 'rows not sorted and finite')
    args = (interval, N_query, N_freespace, u_q, u_f)
    a = replay_d_all(near, far, thr, depth_surface, s1['crossing'], *args)
    b = replay_d_all(near, far, thr, depth_surface, s1['cross_alt'], *args)
    same = (a == d_all).all(-1) | (~s1['decided'] & (b == d_all).all(-1))
    bad = np.nonzero(~same)[0]
    if bad.size:
        r = int(bad[0])
        j = int(np.argmax(a[r] != d_all[r]))
        raise AssertionError((tag, 'd_all differs on rays', bad.tolist()[:8], f'ray {r} sample {j}: replay',
                              float(a[r, j]), 'got', float(d_all[r, j])))
    return int(d_all.shape[0])


def geometry(name, o, d):
    """near, far, thr [n] in fp32 of a geometry (unisurf.py:124-129); exact in the two bypass geometries"""
    g = GEOMETRIES[name]
    n = o.shape[0]
    if name == 'default':
        near, far = near_far32(o, d, g['radius_of_interest'])
        tc = np.float32(0.1)
    else:
        near, far = np.full(n, g['near_bypass'], np.float32), np.full(n, g['far_bypass'], np.float32)
        tc = np.float32(g['too_close_threshold'])
    thr = near + ((far - near).astype(np.float32) * tc).astype(np.float32)
    return near, far, thr.astype(np.float32)


# ---------------------------------------------------------------------------------------------
# fp32 replay with single faults: ray_casting.py:35-160 in numpy fp32 (bit-identical to
# oracle.unisurf.root_find without a fault; the host test asserts that), `mut` switching one in
# ---------------------------------------------------------------------------------------------
FLAG_MUTANTS = ('last_crossing', 'hit_is_crossing', 'bracket_idx2')
# Each alone changes nothing unless a march value is exactly 0: before the first sign change every product
# v_i v_{i+1} is positive, so v_idx has the sign of v_0 and `pos2neg` and `first_free` are one test made twice.
# Dropping both ('hit_is_crossing') turns every ray that starts inside into a hit; a synthetic march with one
# value exactly 0 (the host test's ZERO_MARCHES) separates the two.
FLAG_EQUIVALENT = ('no_pos2neg', 'no_first_free')
SECANT_MUTANTS = ('secant_no_tau', 'update_reversed', 'one_step_short')
SAMPLE_MUTANTS = ('dlo2_not_reset', 'no_switch', 'thr_ignored', 'no_clamps', 'no_final_sort')
PERTURB_MUTANTS = ('edges_linspace_n', 'chunk0_uniforms')


def replay_root_find(f, o, d, near, far, tau, N, k, fill='inf', method='secant', mut=None, marched=None):
    """-> d [n], pts [n, 3], mask [n], mask_sign_change [n]; `marched` = (dp, pts, v) spares the march"""
    n = o.shape[0]
    dp, _, v = marched if marched is not None else march(f, o, d, near, far, tau, N)
    first_free, crossing, hit, idx = flags(v, mut)
    rows = np.nonzero(hit)[0]
    ih = idx[rows]
    i1 = np.minimum(ih + (2 if mut == 'bracket_idx2' else 1), N - 1)
    d_hi, f_hi, d_lo, f_lo = dp[rows, ih], v[rows, ih], dp[rows, i1], v[rows, i1]
    om, dm = o[rows], d[rows]
    pt = lambda dpred: om + (dpred[:, None] * dm).astype(np.float32)
    if method == 'secant' and rows.size:
        steps = k - 1 if (mut == 'one_step_short' and k > 0) else k
        t32 = np.float32(0.0 if mut == 'secant_no_tau' else tau)
        with np.errstate(all='ignore'):
            dpred = _secant(d_lo, f_lo, d_hi, f_hi)
            for _ in range(steps):
                fm = (np.asarray(f(pt(dpred)), np.float32) - t32).astype(np.float32)
                low = fm > 0 if mut == 'update_reversed' else fm < 0
                d_lo, f_lo = np.where(low, dpred, d_lo), np.where(low, fm, f_lo)
                d_hi, f_hi = np.where(low, d_hi, dpred), np.where(low, f_hi, fm)
                dpred = _secant(d_lo, f_lo, d_hi, f_hi)
    else:
        dpred = np.ones(rows.size, np.float32)
    pts = np.ones((n, 3), np.float32)
    pts[rows] = pt(dpred)
    dout = _expected_miss(first_free, near, far, 'far' if fill == 'clamped' else fill)
    dout[rows] = dpred
    dout[~first_free] = 0
    if fill == 'clamped':
        dout = np.maximum(np.minimum(dout, np.broadcast_to(np.asarray(far, np.float32), (n,))),
                          np.broadcast_to(np.asarray(near, np.float32), (n,)))
    return dout.astype(np.float32), pts, hit, crossing
