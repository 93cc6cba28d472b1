"""GPU: UNISURF's root finder and sample placement held stage by stage (tests/unisurf_stages_ref.py).

The kernels under test are uni_prologue / rf_prologue, run_march with uni_march_scan / gather / scatter,
uni_root, uni_secant, uni_samples and rf_finish, through root_finding_surface_points (nr_root_find) and
through unisurf.volume_render.  The SDF is a black box: `f` is the model's own plain forward,
m.implicit_surface(points), the kernel the march itself launches.  No MLP runs on the host.

Rays: E (130 pixels of camera (e)), IN (32 rays that start inside the surface) and T(N, k) (the tau = 0.5
hits of E with per-ray near / far that put the GPU's own secant depth in the middle of pair k of an N-step
march: pair 0, the last pair, and pair (31, 32) across two march chunks).  E and IN together are the 162 rays
that volume_render sees whole and in chunks of 64, 64 and 34 (a non-zero ray0, a partial wave), bit-identical.

Stage 1: mask, mask_sign_change, the first-sample-free flag and the bracket against the plain fp32 march.
Stage 2: N_secant_steps = 0, 1, 2, 3, 8 against the float64 replay of the same steps, D_GPU on every hit.
Stage 3: volume_render's own root finder through the same two checks in three geometries.
Stage 4: d_all bit for bit against the numpy fp32 replay, with and without perturbation.

Printed per case: the worst residual / tolerance and its ray, the decided share, the T placement.
"""
import numpy as np
import pytest
import torch

import unisurf_stages_ref as us
import weightgen as wg
from helpers import unisurf_model
from test_gpu_sampler_rounds import Draws

pytestmark = pytest.mark.gpu
SETS = [('E', 0.0), ('E', 0.5), ('IN', 0.0)] + [(c, 0.5) for c in us.T_CASES]
LADDER_SETS = [('E', 0.0), ('E', 0.5), (us.T_LADDER, 0.5)]
N_ALL = us.N_E + us.N_IN


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()


def _np(t):
    return t.detach().cpu().numpy()


class Rig:
    """one model on the ray sets: the library's normalised directions, f, the plain marches (computed once)"""

    def __init__(self, precision):
        from neurecon_amd.ray_casting import _normalize3
        self.m = unisurf_model(wg.unisurf_state(seed=us.SEED), precision=precision)
        self.o, rd = us.rays_all()
        self.og, self.dg_raw = torch.from_numpy(self.o).cuda(), torch.from_numpy(rd).cuda()
        self.dg = _normalize3(self.dg_raw)
        self.d = _np(self.dg)
        self.E, self.IN = slice(0, us.N_E), slice(us.N_E, N_ALL)
        self.near, self.far = us.near_far32(self.o, self.d)
        self._march, self._geo = {}, {}
        # the GPU's own default march at tau = 0.5 on E places the T rays
        d8, _, mask, _ = self.root('E', 0.5)
        self.t_rows = np.nonzero(mask)[0]
        self.dstar = d8[self.t_rows]

    def f(self, p):
        with torch.no_grad():
            return _np(self.m.implicit_surface(torch.from_numpy(np.ascontiguousarray(p)).cuda()))

    def rays(self, name):
        if isinstance(name, tuple):
            near, far = us.t_case(self.dstar, *name)
            return self.t_rows, near, far, name[0]
        s = {'E': self.E, 'IN': self.IN}[name]
        return np.arange(N_ALL)[s], self.near[s], self.far[s], us.N_STEPS

    def marched(self, name, tau):
        if (name, tau) not in self._march:
            rows, near, far, N = self.rays(name)
            self._march[(name, tau)] = us.march(self.f, self.o[rows], self.d[rows], near, far, tau, N)
        return self._march[(name, tau)]

    def root(self, name, tau, k=us.N_SECANT, **kw):
        from neurecon_amd.ray_casting import root_finding_surface_points
        rows, near, far, N = self.rays(name)
        rows = torch.from_numpy(rows).cuda()
        with torch.no_grad():
            out = root_finding_surface_points(self.m.implicit_surface, self.og[rows].contiguous(),
                                              self.dg[rows].contiguous(), near=torch.from_numpy(near).cuda(),
                                              far=torch.from_numpy(far).cuda(), N_steps=N, logit_tau=tau,
                                              N_secant_steps=k, **kw)
        return tuple(_np(t) for t in out)

    def stage1(self, name, tau, out, fill='inf'):
        rows, near, far, N = self.rays(name)
        dp, _, v = self.marched(name, tau)
        dout, _, mask, msc = out
        return us.stage1_check(f'{name} tau={tau}', v, dp, near, far, mask, msc, dout, fill=fill)

    def render(self, geo, tau, monkeypatch=None, U=None, rayschunk=65536, full=False, **kw):
        """volume_render on the 162 rays -> dict of numpy arrays [162, ...]"""
        from neurecon_amd import rend_util
        from neurecon_amd.frameworks import unisurf
        if U is not None:  # per ray chunk: the interval block, then the free-space block
            blocks = []
            for r0 in range(0, N_ALL, rayschunk):
                blocks += [U[0][r0:r0 + rayschunk][None], U[1][r0:r0 + rayschunk][None]]
            monkeypatch.setattr(rend_util, 'uniform', Draws(blocks))
        with torch.no_grad():
            ex = unisurf.volume_render(self.og[None], self.dg_raw[None], self.m, batched=True, logit_tau=tau,
                                       perturb=U is not None, rayschunk=rayschunk, _sample_only=not full,
                                       **us.GEOMETRIES[geo], **kw)
        assert U is None or not rend_util.uniform.blocks, 'fewer draws than expected'
        ex = ex[2] if full else ex
        keys = ('surface_points', 'mask_surface', 'depth_surface') + (() if full else ('d_all',))
        return {k: _np(ex[k]).reshape(N_ALL, *([-1] if k in ('surface_points', 'd_all') else [])) for k in keys}

    def both(self, geo, tau, monkeypatch=None, U=None, **kw):
        """the whole render, after asserting that the render in chunks of 64, 64 and 34 rays is the same bits"""
        whole = self.render(geo, tau, monkeypatch, U, **kw)
        chunked = self.render(geo, tau, monkeypatch, U, rayschunk=us.RAYSCHUNK, **kw)
        for k in whole:
            assert np.array_equal(whole[k], chunked[k]), (geo, tau, kw, 'chunked vs whole', k)
        return whole

    def geometry(self, geo, tau):
        """stage 3 of one geometry, once: near, far, thr, the plain march, the render, its stage-1 result"""
        if (geo, tau) in self._geo:
            return self._geo[(geo, tau)]
        tag = f'{geo} tau={tau}'
        ex = self.both(geo, tau)
        near, far, thr = us.geometry(geo, self.o, self.d)
        n_far = 0
        if geo == 'default':  # near is the first sample; far is the surface depth of a ray without a crossing
            n64, f64 = us.near_far64(self.o, self.d)
            tol = us.near_far_tol(self.o)
            near = ex['d_all'][:, 0].copy()
            seen = ~ex['mask_surface'] & (ex['depth_surface'] != near)
            far = np.where(seen, ex['depth_surface'], far).astype(np.float32)
            n_far = int(seen.sum())
            en, ef = np.abs(near - n64) / tol, np.abs(far - f64) / tol
            print(f'STAGES [{tag}] near: worst error / tol {en.max():.3f} on ray {int(en.argmax())}; far ({n_far} rays '
                  f'seen): {ef.max():.3f} on ray {int(ef.argmax())}')
            assert (en <= 1).all() and (ef <= 1).all() and n_far >= 10, (tag, en.max(), ef.max(), n_far)
        m = us.march(self.f, self.o, self.d, near, far, tau, us.N_STEPS)
        dp, _, v = m
        s1 = us.stage1_check(tag, v, dp, near, far, ex['mask_surface'], None, ex['depth_surface'], fill='clamped')
        gap, ray, n = us.stage2_check(tag, self.f, self.o, self.d, dp, v, s1, tau, us.N_SECANT, ex['depth_surface'])
        us.points_check(tag, self.o, self.d, ex['depth_surface'], ex['surface_points'], ex['mask_surface'])
        for part, s in (('E', self.E), ('IN', self.IN)):
            share = float(s1['decided'][s].mean())
            print(f'STAGES [{tag}] {part}: decided {share * 100:.1f} %, hits {int(s1["hit"][s].sum())}, crossings '
                  f'{int(s1["crossing"][s].sum())}, first sample occupied {int((~s1["first_free"][s]).sum())}')
            assert share >= us.DECIDED_MIN, (tag, part, share)
        print(f'STAGES [{tag}] secant: worst gap / tol {gap / us.D_GPU:.3f} on ray {ray} ({n} hits)')
        assert n >= us.MIN_HITS[tau], (tag, 'hits judged', n)
        if near[self.IN].max() == 0:  # from near = 0 every IN ray starts inside: occupied, a crossing, no hit, depth 0
            assert not s1['first_free'][self.IN].any() and s1['crossing'][self.IN].all(), tag
            assert not s1['hit'][self.IN].any(), tag
            assert (ex['depth_surface'][self.IN] == 0).all(), tag
        self._geo[(geo, tau)] = (near, far, thr, ex, s1)
        return self._geo[(geo, tau)]


_RIGS = {}


def _rig(precision):
    if precision not in _RIGS:
        _RIGS[precision] = Rig(precision)
    return _RIGS[precision]


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_stage1_crossing_and_flags(precision):
    """every ray of E at tau 0 and 0.5, of IN and of every T, the chunked march and the full one"""
    rig = _rig(precision)
    for name, tau in SETS:
        for full in (False, True):
            s1 = rig.stage1(name, tau, rig.root(name, tau, _full_march=full))
            tag = f'STAGES [stage 1 {precision} {name} tau={tau} {"full" if full else "chunked"} march]'
            print(f'{tag}: decided {s1["share"] * 100:.1f} %, hits {int(s1["hit"].sum())} of {s1["hit"].size}, '
                  f'smallest |v| up to the crossing {s1["min_abs_v"]:.2e} (band {us.BAND:.2e})')
            assert s1['share'] >= us.DECIDED_MIN, (name, tau, full, s1['share'])
            if isinstance(name, tuple):
                placed = int((s1['hit'] & (s1['idx'] == name[1])).sum())
                print(f'{tag}: {placed} of {s1["hit"].size} rays have their first crossing in pair {name[1]}')
                assert s1['share'] == 1.0 and placed == s1['hit'].size, (name, full, s1['idx'].tolist())
    dout, _, mask, msc = rig.root('IN', 0.0)
    assert (rig.near[rig.IN] == 0).all() and msc.all() and not mask.any() and (dout == 0).all()
    assert rig.t_rows.size >= 100, rig.t_rows.size


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_stage2_secant_ladder(precision):
    """rungs 0, 1, 2, 3, 8 against the float64 replay; the points; bisection; both fills"""
    rig = _rig(precision)
    for name, tau in LADDER_SETS:
        rows, near, far, N = rig.rays(name)
        o, d = rig.o[rows], rig.d[rows]
        dp, _, v = rig.marched(name, tau)
        for k in us.RUNGS:
            dk, pts, mask, msc = out = rig.root(name, tau, k)
            s1 = rig.stage1(name, tau, out)
            gap, ray, n = us.stage2_check(f'{name} tau={tau}', rig.f, o, d, dp, v, s1, tau, k, dk)
            print(f'STAGES [ladder {precision} {name} tau={tau}] rung {k}: worst gap / tol {gap / us.D_GPU:.3f} '
                  f'(gap {gap:.3e}) on ray {ray}, {n} hits, decided {s1["share"] * 100:.1f} %')
            us.points_check(f'{name} {k}', o, d, dk, pts, mask)
            assert n >= us.MIN_HITS[tau], (name, tau, k, 'hits judged', n)
        far_out = rig.root(name, tau, fill_inf=False)
        rig.stage1(name, tau, far_out, fill='far')
        assert np.array_equal(far_out[0][mask], dk[mask]) and np.array_equal(far_out[1], pts)
        db, pb, mb, cb = rig.root(name, tau, method='bisection')
        assert np.array_equal(mb, mask) and np.array_equal(cb, msc) and (db[mask] == 1).all()
        assert np.array_equal(db[~mask], dk[~mask])
        us.points_check(f'{name} bisection', o, d, db, pb, mb)


@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_stage3_volume_render_root_finder(precision):
    """the 162 rays, whole and in chunks, three geometries at tau 0 and 0.5: flags, bracket, secant depth,
    near / far of the default geometry; the full render returns the sample pass's surface outputs"""
    rig = _rig(precision)
    for geo in us.GEOMETRIES:
        for tau in us.TAUS:
            _, _, _, ex, _ = rig.geometry(geo, tau)
            full = rig.render(geo, tau, full=True)
            for k in full:
                assert np.array_equal(full[k], ex[k]), (geo, tau, 'full render vs sample pass', k)


@pytest.mark.parametrize('perturb', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_stage4_sample_depths_bit_for_bit(precision, perturb, monkeypatch):
    """d_all of every ray in the two geometries with exact near / far: three sample counts, three intervals
    (at 8.0 both clamps bind; with near 0 and threshold 0 the < 1e-10 switch takes every crossing ray)"""
    rig = _rig(precision)
    n_cases = 0
    for geo in ('bypass', 'zero'):
        for tau in us.TAUS:
            near, far, thr, ex0, s1 = rig.geometry(geo, tau)
            for Nq, Nf in us.SAMPLE_COUNTS:
                U = None
                if perturb:
                    U = (us.uniform_block(us.U_SEED, N_ALL, Nq), us.uniform_block(us.U_SEED + 1, N_ALL, Nf))
                u_q, u_f = (None, None) if U is None else (U[0].numpy(), U[1].numpy())
                for iv in us.INTERVALS:
                    tag = f'{precision} {geo} tau={tau} ({Nq}, {Nf}) interval={iv} perturb={perturb}'
                    ex = rig.both(geo, tau, monkeypatch, U, interval=iv, N_query=Nq, N_freespace=Nf)
                    for k in ('surface_points', 'mask_surface', 'depth_surface'):  # the root finder does not see them
                        assert np.array_equal(ex[k], ex0[k]), (tag, k)
                    us.stage4_check(tag, ex['d_all'], near, far, thr, ex['depth_surface'], s1, iv, Nq, Nf, u_q, u_f)
                    n_cases += 1
            if geo == 'zero':  # rays that take the switch: d_lo2 = max(d - 8, 0) = 0 on every crossing ray
                assert s1['crossing'].sum() >= 50, (geo, tau, int(s1['crossing'].sum()))
    print(f'STAGES [stage 4 {precision} perturb={perturb}]: {n_cases} configurations x {N_ALL} rays, whole and in '
          f'chunks of {us.RAYSCHUNK}, every sample equal to the fp32 replay')
