"""From sample depths to the image, in plain torch: the oracle's `integrate` of each framework run on
given sorted depths, in the dtype asked for.  Between the depths and the image no discrete decision is
left (no searchsorted, no `denom < eps`, no error-bound compare), so a render's outputs can be judged
against this on every ray, whatever the sampler did.

Every input is an fp32 value (state dict, ray origins, fp32-normalised directions, near / far, depths);
`dtype` only sets the arithmetic: fp32 runs the oracle's own lines, fp64 the same lines on the same
inputs widened.  The difference of the two is the reference's own rounding error on a ray (`E_ray`)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import rays as orays
from oracle.neus import NeuSOracle
from oracle.unisurf import UNISURFOracle
from oracle.volsdf import VolSDFOracle

# the project's north star: |x - ref| <= RT |ref| + AT on rgb / depth / mask, NORMAL_AT absolute on normals
RT, AT, NORMAL_AT = 1e-4, 1e-6, 1e-4
COND = 0.25        # a ray is well conditioned for an output when E_ray <= COND x bar
ILL_CAP = 0.02     # at most this share of a ray set may be ill conditioned for an output
ACC_MIN = 1e-3     # depth = sum w / (acc + 1e-10) d is ill-posed below this acc: not judged there


class _default_dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.prev = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.prev)


def _cast(sd, dtype):
    return {k: v.detach().cpu().to(dtype) for k, v in sd.items()}


def prepare_rays(rays_o, rays_d):
    """[B, N, 3] fp32 origins and fp32-normalised directions, as every render normalises them"""
    o = rays_o.detach().cpu().reshape(rays_o.shape[0], -1, 3).float()
    d = F.normalize(rays_d.detach().cpu().reshape(rays_d.shape[0], -1, 3).float(), dim=-1)
    return o, d


def _as(dtype, *ts):
    return [t.detach().cpu().to(dtype) for t in ts]


def neus_integrate(sd, o, d, d_all, dtype=torch.float32, obj_bounding_radius=1.0, N_outside=0, white_bkgd=False,
                   speed_factor=10.0):
    """o, d from prepare_rays; d_all [B, N, S] sorted.  NeuSOracle.integrate as it is."""
    near, far = orays.near_far_from_sphere(o, d, r=obj_bounding_radius)  # fp32, as the render computes them
    with _default_dtype(dtype), torch.no_grad():
        orc = NeuSOracle(_cast(sd, dtype), speed_factor=speed_factor, use_outside_nerf=N_outside > 0)
        o_, d_, near_, far_, da_ = _as(dtype, o, d, near, far, d_all)
        return orc.integrate(o_, d_, near_, far_, da_, d_, obj_bounding_radius, True, N_outside, white_bkgd)


def volsdf_integrate(sd, o, d, d_all, dtype=torch.float32, obj_bounding_radius=3.0, use_nerfplusplus=False,
                     N_outside=32, white_bkgd=False, speed_factor=10.0):
    with _default_dtype(dtype), torch.no_grad():
        orc = VolSDFOracle(_cast(sd, dtype), speed_factor=speed_factor, obj_bounding_radius=obj_bounding_radius,
                           use_nerfplusplus=use_nerfplusplus)
        o_, d_, da_ = _as(dtype, o, d, d_all)
        return orc.integrate(o_, d_, da_, calc_normal=True, white_bkgd=white_bkgd, N_outside=N_outside)


def unisurf_integrate(sd, o, d, d_all, dtype=torch.float32, netchunk=1048576, rayschunk=65536, white_bkgd=False):
    """the render loop's ray chunks (each one the domain of its own netchunk windows), concatenated"""
    with _default_dtype(dtype), torch.no_grad():
        orc = UNISURFOracle(_cast(sd, dtype))
        o_, d_, da_ = _as(dtype, o, d, d_all)
        parts = [orc.integrate(o_[:, i:i + rayschunk], d_[:, i:i + rayschunk], da_[:, i:i + rayschunk],
                               netchunk=netchunk, calc_normal=True, white_bkgd=white_bkgd)
                 for i in range(0, o_.shape[1], rayschunk)]
    return {k: torch.cat([p[k] for p in parts], 1) for k in parts[0]}


# ---------------------------------------------------------------------------------------------
# the ray sets and cases shared by test_reintegrate_ref.py (CPU: the inputs hold the conditioning caps on
# the oracle's own depths) and test_gpu_reintegrate.py (GPU: every ray against float64)
# ---------------------------------------------------------------------------------------------
R_FULL = 130            # with rayschunk 64: chunks of 64, 64 and 2 rays
SMALL_SETS = {1: [65], 3: [0, 65, 129]}   # rows of the R_FULL set rendered on their own


def camera_rays(cam, R=R_FULL):
    """R rays spread by linspace over the pixels of weightgen.CAMERAS[cam]: through, grazing and past
    the object.  Returns rays_o, rays_d [1, R, 3] (fp32, directions not normalised)."""
    import weightgen as wg
    H, W, f, dist = wg.CAMERAS[cam]
    ro, rd, _ = orays.get_rays(wg.look_at_c2w(dist)[None], wg.intrinsics(f, H, W)[None], H, W)
    idx = torch.linspace(0, H * W - 1, R).long()
    return ro[:, idx].contiguous(), rd[:, idx].contiguous()


def _ln(x, speed_factor=10.0):
    return torch.tensor([np.log(x) / speed_factor], dtype=torch.float32)


# name -> (camera, state kwargs, ln_s value or None, render kwargs)
NEUS_CASES = {
    'official_s20': ('b', {}, 20.0, dict(upsample_algo='official_solution', N_upsample_iters=4)),
    'official_s300': ('b', {}, 300.0, dict(upsample_algo='official_solution', N_upsample_iters=4)),
    'official_s300_white': ('b', {}, 300.0, dict(upsample_algo='official_solution', N_upsample_iters=4,
                                                 white_bkgd=True)),
    'direct_use': ('b', {}, 20.0, dict(upsample_algo='direct_use')),
    'direct_more': ('b', {}, 20.0, dict(upsample_algo='direct_more', N_nograd_samples=2048)),
    'nerfpp': ('b', dict(use_outside_nerf=True), 300.0, dict(upsample_algo='official_solution', N_upsample_iters=4,
                                                            N_outside=32)),
    'official_128_128': ('b', {}, 300.0, dict(upsample_algo='official_solution', N_upsample_iters=4, N_samples=128,
                                             N_importance=128)),
}
# name -> (camera, beta, NeRF++)
VOLSDF_CASES = {
    'beta_0.1': ('a', 0.1, False),
    'beta_1e-3': ('c', 1e-3, False),
    'beta_0.1_nerfpp': ('a', 0.1, True),
}
# config (e), 64 + 32 samples; netchunk 2048 = a third of a 64-ray chunk's 6144 points, so every full
# chunk has three normalisation windows and the windows of the chunked and the whole render coincide
UNISURF_CASES = {
    'one_window': dict(netchunk=1048576, rayschunk=65536),
    'three_windows': dict(netchunk=2048, rayschunk=64),
}


# Which ends of the opacity range a set holds: 'lo' = rays with acc < 1e-3, 'hi' = rays with acc > 0.99.
# Every set whose model can produce both holds both (NeuS at s = 300).  The others cannot, whatever the
# rays: at s = 20 the fixture's object gives acc <= 0.86 through its centre (its interior SDF is too
# shallow for sigmoid(20 sdf) to fall below 0.14); behind NeuS's NeRF++ background, inside VolSDF's
# builtin background sphere (sdf = min(sdf, R - |x|): every ray ends on it) or its NeRF++ background,
# and in UNISURF's config (e) (occupancy logits of a few units over 96 samples) every ray is opaque.
EXTREMES = {
    'neus': {'official_s20': ('lo',), 'official_s300': ('lo', 'hi'), 'official_s300_white': ('lo', 'hi'),
             'direct_use': ('lo',), 'direct_more': ('lo',), 'nerfpp': ('hi',), 'official_128_128': ('lo', 'hi')},
    'volsdf': {'beta_0.1': ('hi',), 'beta_1e-3': ('hi',), 'beta_0.1_nerfpp': ('hi',)},
    'unisurf': {'one_window': ('hi',), 'three_windows': ('hi',)},
}


def neus_case(name):
    import weightgen as wg
    cam, skw, s, kw = NEUS_CASES[name]
    sd = wg.neus_state(seed=1, **skw)
    sd['ln_s'] = _ln(s)
    kw = dict(dict(N_samples=64, N_importance=64, N_outside=0, white_bkgd=False), **kw)
    return cam, sd, kw


def volsdf_case(name):
    import weightgen as wg
    cam, beta, nerfpp = VOLSDF_CASES[name]
    seed = 5 if beta < 0.01 else 2
    sd = wg.volsdf_state(seed=seed, beta_init=beta, use_nerfplusplus=nerfpp)
    return cam, sd, beta, nerfpp


OUTPUTS = (('rgb', 'rgb'), ('depth', 'depth_volume'), ('mask', 'mask_volume'), ('normals', 'normals_volume'))


def _rows(t):
    """[B, N, ...] -> float64 numpy [B*N, k]"""
    a = t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
    return a.reshape(a.shape[0] * a.shape[1], -1)


def conditioning(ref32, ref64):
    """Per output: E_ray = max over the ray's elements of |fp32 - fp64|, the bar (per ray: its tightest
    element), the rays judged (depth: acc64 >= ACC_MIN) and the well-conditioned ones among them."""
    acc = _rows(ref64['mask_volume'])[:, 0]
    out = {}
    for name, key in OUTPUTS:
        a, b = _rows(ref32[key]), _rows(ref64[key])
        e = np.abs(a - b).max(-1)
        bar = np.full_like(e, NORMAL_AT) if name == 'normals' else (RT * np.abs(b) + AT).min(-1)
        judged = acc >= ACC_MIN if name == 'depth' else np.ones_like(e, bool)
        well = e <= COND * bar
        out[name] = dict(E=e, judged=judged, well=well,
                         ill_share=float((~well & judged).sum()) / max(int(judged.sum()), 1))
    out['acc'] = acc
    return out


def bar_excess(got, ref64, cond):
    """Per output: which judged, well-conditioned rays miss the bar against float64, and the worst
    (|got - f64| - E_ray) / max|f64| over all judged rays (a measurement)."""
    res = {}
    for name, key in OUTPUTS:
        g, b = _rows(got[key]), _rows(ref64[key])
        err = np.abs(g - b)
        tol = np.full_like(err, NORMAL_AT) if name == 'normals' else RT * np.abs(b) + AT
        c = cond[name]
        held = c['judged'] & c['well']
        miss = (err > tol).any(-1) & held
        scale = max(float(np.abs(b[c['judged']]).max()) if c['judged'].any() else 0.0, 1e-30)
        ex = (err.max(-1) - c['E'])[c['judged']]
        res[name] = dict(miss=miss, worst_err=float(err[held].max()) if held.any() else 0.0,
                         excess=float(ex.max() / scale) if ex.size else 0.0)
    return res
