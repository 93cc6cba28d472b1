"""Host: the stage checks of tests/unisurf_stages_ref.py on the fp32 oracle, and their power.

The fp32 oracle stands in for the kernels, with f = UNISURFOracle(sd).sdf_net.sdf.  (1) Its own root
finder (oracle.unisurf.root_find) and the fp32 replay without a fault go through the checkers that
test_gpu_unisurf_stages.py applies to the GPU, on the same ray sets, and pass on every ray; BAND_REF and
D_REF are measured here, printed, and the module's constants are held to the measurements.  (2) Each single
fault of the replay fails the check it is meant for, with the GPU test's tolerances.  (3) The sample depths:
the oracle's sample_depths is the replay bit for bit, and every fault changes them.
"""
import numpy as np
import pytest
import torch

import unisurf_stages_ref as us
import weightgen as wg
from oracle.unisurf import UNISURFOracle, root_find, sample_depths


@pytest.fixture(scope='module', autouse=True)
def _threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, prev)))
    yield
    torch.set_num_threads(prev)


class Host:
    """the fp32 oracle on the GPU test's ray sets, computed once and left unchanged"""

    def __init__(self):
        self.orc = UNISURFOracle(wg.unisurf_state(seed=us.SEED))
        ro, rd = us.rays_all()
        self.o, self.d = ro, us.normalize_host(rd)
        self.E, self.IN = slice(0, us.N_E), slice(us.N_E, us.N_E + us.N_IN)
        self.near, self.far = us.near_far32(self.o, self.d)
        self._march = {}
        # the default march at tau = 0.5 on E gives the depths d* that place the T rays
        d8, _, hit, _ = self.oracle_root('E', 0.5)
        self.t_rows = np.nonzero(hit)[0]
        self.dstar = d8[self.t_rows]

    def f(self, p):
        with torch.no_grad():
            return self.orc.sdf_net.sdf(torch.from_numpy(np.ascontiguousarray(p))).numpy()

    def rays(self, name):
        """o, d, near, far, N of a ray set: 'E', 'IN', 'ALL' or a (N, k) of T"""
        if isinstance(name, tuple):
            N, k = name
            near, far = us.t_case(self.dstar, N, k)
            return self.o[self.t_rows], self.d[self.t_rows], near, far, N
        s = {'E': self.E, 'IN': self.IN, 'ALL': slice(None)}[name]
        return self.o[s], self.d[s], self.near[s], self.far[s], us.N_STEPS

    def marched(self, name, tau):
        if (name, tau) not in self._march:
            o, d, near, far, N = self.rays(name)
            self._march[(name, tau)] = us.march(self.f, o, d, near, far, tau, N)
        return self._march[(name, tau)]

    def oracle_root(self, name, tau, k=us.N_SECANT, fill_inf=True, method='secant'):
        o, d, near, far, N = self.rays(name)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None]
        with torch.no_grad():
            dout, pt, hit, cr = root_find(self.orc.sdf_net.sdf, T(o), T(d), T(near), T(far), N_steps=N, logit_tau=tau,
                                          N_secant_steps=k, fill_inf=fill_inf, method=method)
        return dout[0].numpy(), pt[0].numpy(), hit[0].numpy(), cr[0].numpy()

    def replay_root(self, name, tau, k=us.N_SECANT, mut=None, **kw):
        o, d, near, far, N = self.rays(name)
        return us.replay_root_find(self.f, o, d, near, far, tau, N, k, mut=mut, marched=self.marched(name, tau), **kw)


@pytest.fixture(scope='module')
def host():
    return Host()


SETS = [('E', 0.0), ('E', 0.5), ('IN', 0.0)] + [(c, 0.5) for c in us.T_CASES]
LADDER_SETS = [('E', 0.0), ('E', 0.5), (us.T_LADDER, 0.5)]


def _stage1(h, name, tau, out, band=us.BAND):
    o, d, near, far, N = h.rays(name)
    dp, _, v = h.marched(name, tau)
    dout, _, mask, msc = out
    return us.stage1_check(f'{name} tau={tau}', v, dp, near, far, mask, msc, dout, band=band)


def test_the_ray_sets_are_what_the_issue_states(host):
    h = host
    _, _, hit0, cr0 = h.oracle_root('E', 0.0)
    _, _, hit5, cr5 = h.oracle_root('E', 0.5)
    assert (int(hit0.sum()), int(hit5.sum())) == (50, 119) and (hit0 == cr0).all() and (hit5 == cr5).all()
    dout, _, hit, cr = h.oracle_root('IN', 0.0)
    _, _, v = h.marched('IN', 0.0)
    assert (h.near[h.IN] == 0).all() and (v[:, 0] <= 0).all() and cr.all() and not hit.any() and (dout == 0).all()


def test_band_ref(host):
    """the largest gap between a march point with its product and sum rounded once and the plain fp32 point"""
    h = host
    worst = 0.0
    for name, tau in SETS:
        o, d, _, _, _ = h.rays(name)
        dp, pts, _ = h.marched(name, tau)
        worst = max(worst, us.fma_gap(o, d, dp, pts))
    print(f'BAND_REF measured {worst:.4e}, recorded {us.BAND_REF:.4e}, BAND {us.BAND:.4e}')
    assert 0.5 * us.BAND_REF <= worst <= us.BAND_REF


def test_stage1_passes_on_the_oracle_and_the_replay(host):
    """every ray set: flags and bracket; the decided share (all of every T; none undecided on E at tau = 0 even
    at a band of 1e-4); every T puts the first crossing of every ray in its pair, |v| >= 3.6e-4 up to it"""
    h = host
    for name, tau in SETS:
        for out in (h.oracle_root(name, tau), h.replay_root(name, tau)):
            s1 = _stage1(h, name, tau, out)
            assert s1['share'] >= us.DECIDED_MIN, (name, tau, s1['share'])
        print(f'stage 1 {name} tau={tau}: decided {s1["share"] * 100:.1f} %, hits {int(s1["hit"].sum())}, '
              f'smallest |v| up to the crossing {s1["min_abs_v"]:.2e}')
        if isinstance(name, tuple):
            assert s1['share'] == 1.0 and s1['hit'].all() and (s1['idx'] == name[1]).all(), (name, s1['idx'])
            if name[0] == 64:
                assert s1['min_abs_v'] >= 3.6e-4, (name, s1['min_abs_v'])
    assert _stage1(h, 'E', 0.0, h.oracle_root('E', 0.0), band=1e-4)['share'] == 1.0
    for fill_inf in (True, False):  # and the other fill
        o, d, near, far, N = h.rays('ALL')
        dp, _, v = h.marched('ALL', 0.5)
        dout, _, mask, msc = h.oracle_root('ALL', 0.5, fill_inf=fill_inf)
        us.stage1_check('ALL', v, dp, near, far, mask, msc, dout, fill='inf' if fill_inf else 'far')


def test_replay_is_the_oracle(host):
    """without a fault the numpy fp32 replay is oracle.unisurf.root_find, bit for bit, at every rung"""
    h = host
    for name, tau in LADDER_SETS + [('IN', 0.0)]:
        for k in us.RUNGS:
            a, b = h.oracle_root(name, tau, k), h.replay_root(name, tau, k)
            for x, y, what in zip(a, b, ('d', 'pts', 'mask', 'mask_sign_change')):
                assert np.array_equal(x, y), (name, tau, k, what)
    a = h.oracle_root('E', 0.5, method='bisection', fill_inf=False)
    b = h.replay_root('E', 0.5, method='bisection', fill='far')
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert (a[0][a[2]] == 1).all() and a[2].sum() == 119


def _ladder(h, name, tau, k, d_got, tol=us.D_GPU):
    o, d, near, far, N = h.rays(name)
    dp, _, v = h.marched(name, tau)
    s1 = _stage1(h, name, tau, h.oracle_root(name, tau))
    return us.stage2_check(f'{name} tau={tau}', h.f, o, d, dp, v, s1, tau, k, d_got, tol=tol)


def test_stage2_passes_on_the_oracle_and_d_ref(host):
    """the fp32 oracle's own secant loop against its float64 replay, every rung and ray set: D_REF; and
    what an early rung is worth: rung k against rung 8"""
    h = host
    d_ref = 0.0
    for name, tau in LADDER_SETS:
        d8, _, hit, _ = h.oracle_root(name, tau, 8)
        for k in us.RUNGS + (7,):
            dk, pts, mask, _ = h.oracle_root(name, tau, k)
            gap, ray, n = _ladder(h, name, tau, k, dk)
            d_ref = max(d_ref, gap if k in us.RUNGS else 0.0)
            print(f'ladder {name} tau={tau} rung {k}: oracle vs float64 replay {gap:.3e} on ray {ray} ({n} hits); '
                  f'rung {k} vs rung 8 {np.abs(dk[hit].astype(np.float64) - d8[hit]).max():.3e}')
            o, d, _, _, _ = h.rays(name)
            us.points_check(f'{name} {k}', o, d, dk, pts, mask)
    print(f'D_REF measured {d_ref:.4e}, recorded {us.D_REF:.4e}, D_GPU {us.D_GPU:.4e}')
    assert 0.5 * us.D_REF <= d_ref <= us.D_REF


def _rejected(check):
    try:
        check()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('mut', us.FLAG_MUTANTS)
def test_stage1_rejects(host, mut):
    h = host
    caught = [(name, tau) for name, tau in SETS
              if _rejected(lambda: _stage1(h, name, tau, h.replay_root(name, tau, mut=mut)))]
    print(f'{mut}: rejected on {caught}')
    assert caught, mut


# a march value of exactly 0 is what tells `pos2neg` from `first_free`: mutant -> v [1, 5]
ZERO_MARCHES = {
    'no_first_free': (0.0, 0.3, -0.2, -0.4, -0.5),   # starts on the surface: a crossing in pair (1, 2), no hit, depth 0
    'no_pos2neg': (0.4, 0.0, -0.3, 0.2, 0.5),        # through 0: the first sign change is neg to pos, in pair (2, 3)
}


@pytest.mark.parametrize('mut', us.FLAG_EQUIVALENT)
def test_pos2neg_and_first_free(host, mut):
    """No march value of the ray sets is exactly 0, so there either test alone gives the flags of both: the
    replay with one of them dropped is the oracle bit for bit (with both dropped, 'hit_is_crossing' above, the
    rays that start inside the surface become hits).  The checker itself tells them apart: on a synthetic march
    with one value exactly 0 (f is a black box) the restatement passes and each single fault is rejected,
    whichever sign the checker reads the 0 with."""
    h = host
    for name, tau in SETS:
        assert (h.marched(name, tau)[2] != 0).all()
        for x, y in zip(h.oracle_root(name, tau), h.replay_root(name, tau, mut=mut)):
            assert np.array_equal(x, y), (mut, name, tau)
    assert h.replay_root('IN', 0.0, mut='hit_is_crossing')[2].all()
    v = np.array([ZERO_MARCHES[mut]], np.float32)
    o, d = np.zeros((1, 3), np.float32), np.array([[0.0, 0.0, 1.0]], np.float32)
    near, far = np.float32(1.0), np.float32(2.0)
    dp = us.lerp32(near, far, us.linspace32(5)[None])
    for m in (None, mut):  # rung 0: the secant estimate of the bracket, no call of f
        dout, _, mask, msc = us.replay_root_find(None, o, d, near, far, 0.0, 5, 0, mut=m, marched=(dp, None, v))
        check = lambda: us.stage1_check(mut, v, dp, near, far, mask, msc, dout)
        if m is None:
            assert not check()['decided'][0] and not mask[0]
        else:
            assert mask[0] and _rejected(check), mut


@pytest.mark.parametrize('mut', us.SECANT_MUTANTS + ('bracket_idx2',))
def test_stage2_rejects(host, mut):
    """one step too few is caught at each of the rungs 1 to 3, a bracket of (idx, idx + 2) at rungs 0 and 1 (by
    rung 8 the secant has come back into pair idx on most rays); the other faults at some rung of every ladder set"""
    h = host
    for name, tau in LADDER_SETS:
        rungs = {'one_step_short': (1, 2, 3), 'bracket_idx2': (0, 1)}.get(mut, us.RUNGS)
        wrong = lambda k: h.replay_root(name, tau, k, mut=mut)[0]
        caught = [k for k in rungs if _rejected(lambda: _ladder(h, name, tau, k, wrong(k)))]
        print(f'{mut} {name} tau={tau}: rejected at rungs {caught}')
        if mut in ('one_step_short', 'bracket_idx2'):
            assert caught == list(rungs), (mut, name, tau, caught)
        elif mut == 'secant_no_tau' and tau == 0.0:
            assert not caught  # the same arithmetic
        else:
            assert caught, (mut, name, tau)
    # what the ladder cannot see: the missing step at k = 8
    assert not _rejected(lambda: _ladder(h, 'E', 0.5, 8, h.replay_root('E', 0.5, 8, mut='one_step_short')[0]))


# ---------------------------------------------------------------------------------------------
# the sample depths
# ---------------------------------------------------------------------------------------------
def _sample_cases(h):
    """(tag, near, far, thr, depth_surface, stage-1 result, interval, N_query, N_freespace, u_q, u_f) on the 162 rays"""
    n = us.N_E + us.N_IN
    for geo in us.GEOMETRIES:
        near, far, thr = us.geometry(geo, h.o, h.d)
        for tau in us.TAUS:
            dp, _, v = m = us.march(h.f, h.o, h.d, near, far, tau, us.N_STEPS)
            dc, _, mask, _ = us.replay_root_find(h.f, h.o, h.d, near, far, tau, us.N_STEPS, us.N_SECANT, fill='clamped',
                                                 marched=m)
            s1 = us.stage1_check(f'{geo} {tau}', v, dp, near, far, mask, None, dc, fill='clamped')
            for Nq, Nf in us.SAMPLE_COUNTS:
                for iv in us.INTERVALS:
                    for perturb in (False, True):
                        u_q = us.uniform_block(us.U_SEED, n, Nq).numpy() if perturb else None
                        u_f = us.uniform_block(us.U_SEED + 1, n, Nf).numpy() if perturb else None
                        tag = f'{geo} tau={tau} ({Nq}, {Nf}) interval={iv} perturb={perturb}'
                        yield tag, near, far, thr, dc, s1, iv, Nq, Nf, u_q, u_f


@pytest.fixture(scope='module')
def sample_cases(host):
    return list(_sample_cases(host))


def test_stage4_replay_is_the_oracle(host, sample_cases, golden):
    """oracle.unisurf.sample_depths (what UNISURFOracle.render places its samples with) passes the bit-for-bit
    check in every configuration, and so does the oracle's whole render in the default geometry; with the
    uniforms the reference drew, the oracle's perturbed render has the reference's recorded logits at all 96
    samples of every ray"""
    T = lambda u: None if u is None else torch.from_numpy(np.ascontiguousarray(u))
    for tag, near, far, thr, dc, s1, iv, Nq, Nf, u_q, u_f in sample_cases:
        _, d_all = sample_depths(T(near), T(far), T(thr), T(dc), T(s1['crossing']), iv, Nq, Nf, T(u_q), T(u_f))
        us.stage4_check(tag, d_all.numpy(), near, far, thr, dc, s1, iv, Nq, Nf, u_q, u_f)
    h = host
    near, far, thr = us.geometry('default', h.o, h.d)
    with torch.no_grad():
        out = h.orc.render(T(h.o)[None], T(h.d)[None], logit_tau=0.5, calc_normal=False)
    _, crossing, _, _ = us.flags(us.march(h.f, h.o, h.d, near, far, 0.5, us.N_STEPS)[2])
    s1 = dict(crossing=crossing, cross_alt=crossing, decided=np.ones(h.o.shape[0], bool))
    us.stage4_check('oracle render', out['d_all'][0].numpy(), near, far, thr, out['depth_surface'][0].numpy(), s1, 1.0,
                    64, 32)
    g = golden('unisurf_perturb')
    assert int(g['seed']) == us.SEED
    with torch.no_grad():
        out = h.orc.render(T(g['rays_o']), T(g['rays_d']), logit_tau=float(g['logit_tau']), calc_normal=False,
                           u_query=T(g['u0']), u_free=T(g['u1']))
    err = np.abs(out['implicit_surface'].numpy() - g['sdf'])
    print(f'perturbed oracle render vs the recorded logits: max abs {err.max():.3e}')
    assert (err <= 1e-4 * np.abs(g['sdf']) + 1e-6).all(), float(err.max())


@pytest.mark.parametrize('mut', us.SAMPLE_MUTANTS + us.PERTURB_MUTANTS)
def test_stage4_rejects(sample_cases, mut):
    caught = []
    for tag, near, far, thr, dc, s1, iv, Nq, Nf, u_q, u_f in sample_cases:
        if mut in us.PERTURB_MUTANTS and u_q is None:
            continue
        d_all = us.replay_d_all(near, far, thr, dc, s1['crossing'], iv, Nq, Nf, u_q, u_f, mut=mut)
        if _rejected(lambda: us.stage4_check(tag, d_all, near, far, thr, dc, s1, iv, Nq, Nf, u_q, u_f)):
            caught.append(tag)
    print(f'{mut}: rejected in {len(caught)} configurations, e.g. {caught[:3]}')
    assert caught, mut
    if mut == 'no_switch':  # the < 1e-10 switch shows only where d_lo2 can be 0: near 0 and threshold 0
        assert all(t.startswith('zero') for t in caught) and any('interval=8.0' in t for t in caught), caught
