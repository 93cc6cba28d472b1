"""Host: the forward check of tests/sampler_ref.py on the fp32 oracle, and its power.

The fp32 oracle stands in for the kernels.  (1) Its own ladder (coarse state, then four rounds of 16),
its direct rounds and its VolSDF first pass go through the checker that test_gpu_sampler_rounds.py
applies to the GPU, on the same rays, and pass on every sample; what they need -- K_ref, delta, r_ref --
is measured here, printed, and the constants the GPU test uses are held to twice these figures.  (2) Each
single fault of sampler_ref.NEUS_MUTANTS / VOLSDF_MUTANTS, switched into the fp32 replay of one round,
fails the check with the GPU test's tolerance.  (3) The checker's edges.
"""
import numpy as np
import pytest
import torch

import reintegrate_ref as rr
import sampler_ref as sr
import weightgen as wg
from oracle import rays as orays
from oracle import volsdf as ovol
from oracle.neus import NeuSOracle
from oracle.volsdf import VolSDFOracle

MODES = ('det', 'rand')


@pytest.fixture(scope='module', autouse=True)
def _threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, prev)))
    yield
    torch.set_num_threads(prev)


# ---------------------------------------------------------------------------------------------
# NeuS
# ---------------------------------------------------------------------------------------------
class NeusHost:
    """the fp32 oracle's sampler state on the GPU test's rays, computed once and left unchanged"""

    def __init__(self):
        self.orc = NeuSOracle(wg.neus_state(seed=sr.NEUS_SEED))
        ro, rd = rr.camera_rays(sr.NEUS_CAM)
        self.o, self.d = rr.prepare_rays(ro, rd)
        self.near, self.far = orays.near_far_from_sphere(self.o, self.d, r=1.0)
        self.n = self.o.shape[1]
        U = sr.uniform_block(sr.U_SEED, sr.N_ROUNDS, self.n, sr.N_UP)
        self.u = {'det': [sr.det_u(sr.N_UP).expand(1, self.n, sr.N_UP)] * sr.N_ROUNDS,
                  'rand': [U[i][None] for i in range(sr.N_ROUNDS)]}
        with torch.no_grad():
            self.states = {m: self.ladder(self.u[m]) for m in MODES}

    def lerp(self, N):
        t = torch.linspace(0, 1, N).float()
        return self.near * (1 - t) + self.far * t

    def sdf_at(self, dv):
        return self.orc.sdf_net.sdf(self.o.unsqueeze(-2) + dv.unsqueeze(-1) * self.d.unsqueeze(-2))

    def ladder(self, us):
        dv = self.lerp(sr.N_COARSE)
        sv = self.sdf_at(dv)
        states = [(dv[0], sv[0])]
        for i in range(sr.N_ROUNDS):  # oracle/neus.py:80-97
            fine = sr.replay_neus_round(dv, sv, i, us[i])
            dv = torch.cat([dv, fine], -1)
            sv = torch.cat([sv, self.sdf_at(fine)], -1)
            dv, order = torch.sort(dv, -1)
            sv = torch.gather(sv, -1, order)
            states.append((dv[0], sv[0]))
        return states


@pytest.fixture(scope='module')
def neus_host():
    return NeusHost()


def test_replay_is_the_oracle(neus_host):
    """without a fault the fp32 replay is oracle.neus.sample_depths, bit for bit"""
    h = neus_host
    with torch.no_grad():
        want = h.orc.sample_depths(h.o, h.d, h.near, h.far, sr.N_COARSE, sr.N_UP * sr.N_ROUNDS, 'official_solution',
                                   sr.N_ROUNDS)
        assert torch.equal(h.states['det'][-1][0], want[0])
        for algo, N in (('direct_use', sr.N_COARSE), ('direct_more', 256)):
            bins = h.lerp(N)
            fine = sr.replay_neus_direct(bins, h.sdf_at(bins), 64.0, sr.det_u(64).expand(1, h.n, 64))
            got = torch.sort(torch.cat([h.lerp(sr.N_COARSE), fine], -1), -1)[0]
            want = h.orc.sample_depths(h.o, h.d, h.near, h.far, sr.N_COARSE, 64, algo, N_nograd_samples=256)
            assert torch.equal(got, want), algo


def _direct_rounds(h):
    """(name, bins, sdf, new depths, u, L) of the oracle's direct rounds"""
    out = []
    with torch.no_grad():
        for name, N in (('direct_use', sr.N_COARSE), ('direct_more_256', 256), ('direct_more_2048', 2048)):
            for mode in MODES:
                u = sr.det_u(64).expand(1, h.n, 64) if mode == 'det' else sr.uniform_block(sr.U_SEED + 1, 1, h.n, 64)
                bins = h.lerp(N)
                sv = h.sdf_at(bins)
                out.append((f'{name} {mode}', bins[0], sv[0], sr.replay_neus_direct(bins, sv, 64.0, u)[0], u[0], N))
    return out


def test_neus_reference_passes_and_K_ref(neus_host):
    """every sample of every round of the oracle's ladder and direct rounds passes with K = 2 K_ref, and
    K_ref is what sampler_ref records"""
    h = neus_host
    k_ref = -np.inf
    for mode in MODES:
        st = h.states[mode]
        for k in range(1, sr.N_ROUNDS + 1):
            (Dp, Sp), (Dk, Sk) = st[k - 1], st[k]
            res, total = sr.neus_round_check(Dp, Sp, Dk, Sk, k - 1, h.u[mode][k - 1][0])
            L = Dp.shape[-1]
            kk = float(sr.neus_k_ratio(res, L, total).max())
            w, r = sr.worst(res, sr.neus_tol(L, total, sr.K_GPU))
            print(f'oracle ladder {mode} round {k}: K needed {kk:+.3f}, worst residual / tol {w:.3f} on ray {r}')
            assert w <= 1.0, (mode, k, w, r)
            k_ref = max(k_ref, kk)
    for name, bins, sv, new, u, L in _direct_rounds(h):
        cdf, total = sr.pdf_cdf(sr.neus_direct_weights(sv, 64.0))
        res = sr.forward_residual(bins, cdf, new, u)
        kk = float(sr.neus_k_ratio(res, L, total.numpy()).max())
        w, r = sr.worst(res, sr.neus_tol(L, total, sr.K_GPU))
        print(f'oracle {name}: K needed {kk:+.3f}, worst residual / tol {w:.3f} on ray {r}')
        assert w <= 1.0, (name, w, r)
        k_ref = max(k_ref, kk)
    print(f'K_ref = {k_ref!r} (recorded {sr.K_REF!r})')
    assert sr.K_GPU == 2 * sr.K_REF
    assert abs(k_ref - sr.K_REF) <= 0.01 * sr.K_REF, (k_ref, sr.K_REF)


def test_neus_ray_mix(neus_host):
    """the ray set holds rays that hit and rays that miss: sum w of the first round from its float64
    total.  (A later round's list is longer, and alpha's own 1e-5 per interval alone brings an empty
    ray's sum w to (L - 1) 1e-5: 1.1e-3 at L = 112.)"""
    Dp, Sp = neus_host.states['det'][0]
    _, total = sr.pdf_cdf(sr.neus_round_weights(Dp, Sp, 0))
    sw = total.numpy() - (Dp.shape[-1] - 1) * 1e-5
    print(f'sum w: {int((sw > 0.5).sum())} rays > 0.5, {int((sw < 1e-3).sum())} rays < 1e-3')
    assert (sw > 0.5).sum() >= 10 and (sw < 1e-3).sum() >= 10


@pytest.mark.parametrize('mut', sr.NEUS_MUTANTS)
def test_neus_mutant_fails(neus_host, mut):
    """one fault in one round, from the oracle's own state of that round: at least one sample off"""
    h = neus_host
    off = rays = 0
    for mode in MODES:
        for it in range(sr.N_ROUNDS):
            Dp, Sp = h.states[mode][it]
            u = h.u[mode][it]
            new = sr.replay_neus_round(Dp[None], Sp[None], it, u, mut)[0]
            cdf, total = sr.pdf_cdf(sr.neus_round_weights(Dp, Sp, it))
            res = sr.forward_residual(Dp, cdf, new, u[0])
            miss = ~(res <= sr.neus_tol(Dp.shape[-1], total, sr.K_GPU)[:, None])  # a NaN is a miss
            off += int(miss.sum())
            rays = max(rays, int(miss.any(-1).sum()))
    print(f'mutant {mut}: {off} samples off, up to {rays} of {h.n} rays in a round')
    assert off >= 1


@pytest.mark.parametrize('mut', sr.NEUS_EQUIVALENT)
def test_neus_equivalent_faults_are_not_seen(neus_host, mut):
    """what sampler_ref's docstring says the check cannot see on these nets: the replay with the fault
    passes like the oracle itself.  If this fails the rays have come to exercise the line: move the fault
    to NEUS_MUTANTS."""
    h = neus_host
    for mode in MODES:
        for it in range(sr.N_ROUNDS):
            Dp, Sp = h.states[mode][it]
            u = h.u[mode][it]
            new = sr.replay_neus_round(Dp[None], Sp[None], it, u, mut)[0]
            cdf, total = sr.pdf_cdf(sr.neus_round_weights(Dp, Sp, it))
            res = sr.forward_residual(Dp, cdf, new, u[0])
            assert (res <= sr.neus_tol(Dp.shape[-1], total, sr.K_GPU)[:, None]).all(), (mut, mode, it)


# ---------------------------------------------------------------------------------------------
# VolSDF, the first sampling pass
# ---------------------------------------------------------------------------------------------
class VolsdfHost:
    def __init__(self, name):
        Ns, beta, nerfpp = sr.VOLSDF_CASES[name]
        self.N0, self.nerfpp = 4 * Ns, nerfpp
        sd = wg.volsdf_state(seed=sr.VOLSDF_SEED, beta_init=beta, use_nerfplusplus=nerfpp)
        self.orc = VolSDFOracle(sd, use_nerfplusplus=nerfpp)
        ro, rd = rr.camera_rays(sr.VOLSDF_CAM)
        self.o, self.d = rr.prepare_rays(ro, rd)
        self.n = self.o.shape[1]
        if nerfpp:
            _, self.far, hit = orays.sphere_intersection(self.o, self.d, r=3.0)
            assert hit.all()
        else:
            self.far = sr.VOLSDF_FAR * torch.ones(1, self.n, 1)
        t = torch.linspace(0, 1, self.N0).float()
        self.d_init = torch.zeros(1, self.n, 1) * (1 - t) + self.far * t
        self.alpha, self.beta = self.orc.forward_ab()
        with torch.no_grad():
            self.sdf = self.orc.surface(self.o[..., None, :] + self.d[..., None, :] * self.d_init[..., :, None])
            self.fine, self.beta_map, self.usage = ovol.fine_sample(
                self.orc.surface, self.d_init, self.o, self.d, self.alpha, self.beta, self.far, eps=sr.VOLSDF_EPS,
                max_iter=0, N_final=sr.VOLSDF_N_IMPORTANCE)
        # the oracle's own line (its torch.sqrt is an ulp off IEEE on some CPU builds; the GPU test expects
        # the IEEE value of sampler_ref.volsdf_beta_plus, which the kernel's sqrtf gives)
        self.beta_plus = torch.sqrt((self.far ** 2) / (4 * (self.N0 - 1) * np.log(1 + sr.VOLSDF_EPS))).reshape(-1).numpy()
        assert np.allclose(self.beta_plus, sr.volsdf_beta_plus(self.far.numpy(), self.N0), rtol=2e-7, atol=0)

    def sample(self, u, mut=None):
        """the fp32 fine samples of every ray at the (alpha, beta) of its branch, for uniforms u"""
        conv = (self.usage == 0)[..., None]
        bp = torch.from_numpy(np.broadcast_to(self.beta_plus, (self.n,)).copy()).reshape(1, self.n, 1)
        beta = torch.where(conv, self.beta.reshape(1, 1, 1).expand_as(bp), bp)
        alpha = torch.where(conv, self.alpha.reshape(1, 1, 1).expand_as(bp), 1. / bp)
        return sr.replay_volsdf_fine(self.d_init, self.sdf, alpha, beta, u, mut)


@pytest.fixture(scope='module')
def volsdf_hosts():
    return {name: VolsdfHost(name) for name in sr.VOLSDF_CASES}


def test_volsdf_reference_passes_delta_and_r_ref(volsdf_hosts):
    delta_ref = r_ref = 0.0
    for name, h in volsdf_hosts.items():
        m = sr.VOLSDF_N_IMPORTANCE
        assert np.array_equal(h.d_init[0].numpy(), sr.lerp32(np.zeros((h.n, 1), np.float32), h.far[0].numpy(),
                                                             torch.linspace(0, 1, h.N0).numpy()[None]))
        u_det = sr.det_u(m).expand(1, h.n, m)
        assert torch.equal(h.sample(u_det), h.fine), name  # the replay is the oracle's fine_sample
        B32 = ovol.error_bound(h.d_init, h.sdf, h.alpha, h.beta).max(-1).values[0].double().numpy()
        B64 = sr.volsdf_bound(h.d_init[0], h.sdf[0], float(h.alpha), float(h.beta)).max(-1).values.numpy()
        fin = np.isfinite(B64)
        assert np.array_equal(np.isinf(B32), np.isinf(B64)), name  # infinite on both sides: agreement
        delta_ref = max(delta_ref, float((np.abs(B32[fin] - B64[fin]) / B64[fin]).max()))
        for mode in MODES:
            u = u_det if mode == 'det' else torch.sort(sr.uniform_block(sr.U_SEED + 2, 1, h.n, m), -1).values
            fine = h.fine if mode == 'det' else h.sample(u)
            info = sr.volsdf_first_check(h.d_init[0], h.sdf[0], float(h.alpha), float(h.beta), h.beta_plus,
                                         h.usage[0].numpy(), h.beta_map[0].numpy(), fine[0], u[0], sr.DELTA_GPU,
                                         sr.SWITCH + sr.R_GPU)
            print(f'oracle volsdf {name} {mode}: converged {info["n_conv"]}, not {info["n_nonc"]}, in the band '
                  f'{info["band"] * 100:.1f} %, largest residual {info["res"]:.3e}')
            assert info['band'] == 0.0 and info['n_conv'] >= 10 and info['n_nonc'] >= 10, (name, info)
            r_ref = max(r_ref, info['res'])
    print(f'delta_ref = {delta_ref!r} (recorded {sr.DELTA_REF!r}), r_ref = {r_ref!r} (recorded {sr.R_REF!r})')
    assert sr.DELTA_GPU == 2 * sr.DELTA_REF and sr.R_GPU == 2 * sr.R_REF
    assert abs(delta_ref - sr.DELTA_REF) <= 0.01 * sr.DELTA_REF, (delta_ref, sr.DELTA_REF)
    assert abs(r_ref - sr.R_REF) <= 0.01 * sr.R_REF, (r_ref, sr.R_REF)


@pytest.mark.parametrize('mut', sr.VOLSDF_MUTANTS)
def test_volsdf_mutant_fails(volsdf_hosts, mut):
    off = 0
    for name, h in volsdf_hosts.items():
        m = sr.VOLSDF_N_IMPORTANCE
        u = sr.det_u(m).expand(1, h.n, m)
        with pytest.raises(AssertionError, match='samples'):
            sr.volsdf_first_check(h.d_init[0], h.sdf[0], float(h.alpha), float(h.beta), h.beta_plus, h.usage[0].numpy(),
                                  h.beta_map[0].numpy(), h.sample(u, mut)[0], u[0], sr.DELTA_GPU, sr.SWITCH + sr.R_GPU)
        off += 1
    assert off == len(volsdf_hosts)


# ---------------------------------------------------------------------------------------------
# the checker's edges
# ---------------------------------------------------------------------------------------------
def _res(bins, cdf, d, u):
    return sr.forward_residual(np.asarray([bins], np.float64), np.asarray([cdf], np.float64),
                               np.asarray([d], np.float64), np.asarray(u, np.float64))[0]


def test_checker_duplicate_depths_are_an_interval():
    bins, cdf = [1.0, 2.0, 2.0, 3.0], [0.0, 0.25, 0.75, 1.0]   # the zero-width bin at 2 holds half the mass
    assert _res(bins, cdf, [2.0, 2.0, 2.0], [0.25, 0.5, 0.75]).max() == 0.0
    np.testing.assert_allclose(_res(bins, cdf, [2.0, 2.0], [0.2, 0.8]), [0.05, 0.05], atol=1e-15)
    np.testing.assert_allclose(_res(bins, cdf, [1.5, 2.5], [0.125, 0.875]), 0.0, atol=1e-15)
    np.testing.assert_allclose(_res(bins, cdf, [1.5], [0.5]), [0.375], atol=1e-15)


def test_checker_u0_u1_and_sorted_matching():
    bins, cdf = [1.0, 2.0, 4.0], [0.0, 0.5, 1.0]
    assert _res(bins, cdf, [1.0, 4.0], [0.0, 1.0]).max() == 0.0
    assert _res(bins, cdf, [4.0, 1.0], [0.0, 1.0]).max() == 0.0        # matched in sorted order
    assert _res(bins, cdf, [1.0, 1.0], [0.0, 0.0]).max() == 0.0        # u = 0 returns near again
    assert _res(bins, cdf, [0.5], [0.0]).max() == 0.0                   # below the first bin: F = 0
    np.testing.assert_allclose(_res(bins, cdf, [0.5], [0.1]), [0.1])
    np.testing.assert_allclose(_res(bins, cdf, [4.0], [0.7]), [0.3])   # at the last bin F_lo = its cdf ...
    for uu in (0.6, 0.9, 1.0):                                          # ... and F_hi = 1, also unnormalised
        assert _res(bins, [0.0, 0.5, 0.6], [4.0], [uu]).max() == 0.0
    np.testing.assert_allclose(_res(bins, [0.0, 0.5, 0.6], [4.0], [0.55]), [0.05])
    np.testing.assert_allclose(_res(bins, cdf, [5.0], [0.9]), [0.1])    # above it F_lo = cdf's last entry


def test_checker_two_bins_one_hot_and_zero_weights():
    cdf, total = sr.pdf_cdf(torch.tensor([[3.0]]))                      # L = 2
    assert cdf.tolist() == [[0.0, 1.0]] and abs(float(total) - 3.00001) < 1e-12
    np.testing.assert_allclose(_res([2.0, 4.0], cdf[0].numpy(), [2.0, 3.0, 4.0], [0.0, 0.5, 1.0]), 0.0, atol=1e-15)
    w = torch.zeros(1, 7)
    w[0, 3] = 1.0                                                       # one bin holds all the mass
    cdf, total = sr.pdf_cdf(w)
    bins = torch.arange(8.0)[None]
    u = sr.det_u(16)[None]
    d = sr.replay_sample_pdf(bins, w, u)
    assert sr.forward_residual(bins, cdf, d, u).max() <= sr.neus_tol(8, total, 4.0).max()
    assert ((d > 3) & (d < 4)).sum() >= 13
    cdf, total = sr.pdf_cdf(torch.zeros(1, 7))                          # all-zero weights: uniform
    np.testing.assert_allclose(cdf[0].numpy(), np.arange(8) / 7.0, atol=1e-15)
    d = sr.replay_sample_pdf(bins, torch.zeros(1, 7), u)
    assert sr.forward_residual(bins, cdf, d, u).max() <= sr.neus_tol(8, total, 4.0).max()
    np.testing.assert_allclose(d[0].numpy(), 7 * u[0].numpy(), atol=1e-5)


def test_multiset_split():
    a = np.array([[1.0, 2.0, 2.0, 3.0, 5.0]], np.float32)
    b = np.array([[1.0, 2.0, 5.0]], np.float32)
    assert sr.multiset_split(a, b).tolist() == [[2.0, 3.0]]
    sa, sb = np.array([[.1, .2, .3, .4, .5]], np.float32), np.array([[.1, .3, .5]], np.float32)
    d, s = sr.multiset_split(a, b, sa, sb)
    assert d.tolist() == [[2.0, 3.0]] and s.astype(np.float32).tolist() == [[np.float32(.2), np.float32(.4)]]
    with pytest.raises(AssertionError):                                  # an old depth moved by an ulp
        sr.multiset_split(a, np.array([[1.0, np.nextafter(np.float32(2), np.float32(3)), 5.0]], np.float32))
    with pytest.raises(AssertionError):                                  # a value paired with the wrong depth
        sr.multiset_split(a, b, sa, np.array([[.1, .4, .5]], np.float32))
