"""Argument blocks for the host side of nr_neus_render / nr_volsdf_render / nr_unisurf_render: the
workspace-size cases behind render_workspace.json (gen_render_workspace.py writes it,
tests/test_render_host.py checks it) and valid base blocks for the rejected-argument tables.

Every pointer is a fake non-null address: the size entry points and the argument checks run before
any HIP call and dereference only the descriptors."""
import ctypes
import itertools

from neurecon_amd import _lib as L

FAKE = 0x10000  # fake device pointers: FAKE, 2 FAKE, ...
_KEEP = []      # descriptors referenced by the argument blocks handed out


def _fill_pointers(a, skip):
    k = 1
    for name, typ in a._fields_:
        if typ is ctypes.c_void_p and name not in skip:
            setattr(a, name, FAKE * k)
            k += 1


def descs(prec, a, nerf=False):
    sd = L.NrSdfDesc(8, 256, 4, 6, 256, prec, 0)
    rd = L.NrRadDesc(4, 256, -1, 4, 256, prec, 0, 0)
    _KEEP.extend([sd, rd])
    a.sdf, a.rad = ctypes.pointer(sd), ctypes.pointer(rd)
    if nerf:
        nd = L.NrNerfDesc(8, 256, 4, 4, 10, 4, prec)
        _KEEP.append(nd)
        a.nerf = ctypes.pointer(nd)


def neus_args(n_rays=4096, algo='official_solution', N_outside=0, nablas=False, sample_only=False,
              prec=L.PREC_F16X3, no_defer=False, max_chunk_rays=0, max_workspace_bytes=0):
    a = L.NrNeusArgs()
    # render mode without detailed outputs; no fold pack, no perturb uniforms, no workspace yet
    _fill_pointers(a, {'d_final', 'sdf_out', 'nablas_out', 'radiance_out', 'alpha_out', 'cdf_out', 'weights_out',
                       'sigma_out', 'radiance_bg_out', 'nerf_packed', 't_outside', 't_nograd', 'workspace', 'u_rand',
                       't_out_rand', 'd_all_out', 'fold_packed'})
    descs(prec, a, nerf=N_outside > 0)
    a.n_rays, a.obj_bounding_radius = n_rays, 1.0
    a.near_bypass = a.far_bypass = float('nan')
    a.N_samples, a.N_importance, a.N_upsample_iters, a.calc_normal = 64, 64, 4, 1
    a.upsample_algo, a.fixed_s = L.UPSAMPLE[algo], 64.0
    if algo == 'direct_more':
        a.N_nograd_samples, a.t_nograd = 2048, FAKE * 40
    if N_outside > 0:
        a.N_outside, a.nerf_packed, a.t_outside = N_outside, FAKE * 41, FAKE * 42
    if nablas:
        a.nablas_out = FAKE * 43
    if sample_only:
        a.sample_only, a.d_all_out = 1, FAKE * 44
    a.no_defer = int(no_defer)
    a.max_chunk_rays, a.max_workspace_bytes = max_chunk_rays, max_workspace_bytes
    return a


def volsdf_args(n_rays=16384, N_outside=0, max_upsample_steps=5):
    a = L.NrVolsdfArgs()
    _fill_pointers(a, {'d_vals', 'sdf_out', 'nablas_out', 'radiance_out', 'alpha_out', 'p_out', 'weights_out',
                       'sigma_out', 'beta_map', 'iter_usage', 'workspace', 'nerf_packed', 'rs_out', 'sigma_bg',
                       'radiance_bg', 'u_rand', 'u_out'})
    descs(L.PREC_F16X3, a, nerf=N_outside > 0)
    a.n_rays = n_rays
    a.alpha_net, a.beta_net, a.eps, a.near, a.far, a.obj_bounding_radius = 10.0, 0.1, 0.1, 0.0, 6.0, 3.0
    a.N_samples, a.N_importance, a.max_upsample_steps, a.max_bisection_steps = 128, 64, max_upsample_steps, 10
    a.calc_normal = 1
    if N_outside > 0:
        a.N_outside, a.nerf_packed, a.rs_out, a.beta_plus_k = N_outside, FAKE * 41, FAKE * 42, 190.0
    else:
        a.use_sphere_bg, a.beta_plus_init = 1, 0.4
    return a


def _no_reduce(_user):
    return 0


_REDUCE = L.WINDOW_REDUCE(_no_reduce)


def unisurf_args(n_rays=4096, layout='flat', rayschunk=65536, netchunk=1048576, sample_only=False):
    """layout: 'flat' (normal_mode 0), 'row' (normal_mode 1, one batch row), 'rows' (normal_mode 1,
    rays_per_batch = n_rays / 2 when that divides), 'shard' (the first half of batch rows twice as long)."""
    a = L.NrUnisurfArgs()
    _fill_pointers(a, {'surface_points', 'mask_surface', 'depth_surface', 'radiance_out', 'sdf_out', 'nablas_out',
                       'alpha_out', 'weights_out', 'workspace', 'u_query', 'u_free', 'window_ss', 'window_reduce',
                       'window_user', 'd_all_out'})
    descs(L.PREC_F16X3, a)
    a.n_rays = n_rays
    a.rays_per_batch = n_rays // 2 if layout == 'rows' and n_rays % 2 == 0 else n_rays
    a.radius_of_interest, a.interval, a.too_close_threshold = 4.0, 1.0, 0.1
    a.near_bypass = a.far_bypass = float('nan')
    a.N_steps, a.N_secant_steps, a.N_query, a.N_freespace = 256, 8, 64, 32
    a.normal_mode = 0 if layout == 'flat' else 1
    a.rayschunk, a.netchunk, a.calc_normal = rayschunk, netchunk, 1
    if layout == 'shard':
        a.shard_ray0, a.shard_row_rays = 0, 2 * n_rays
        a.window_ss, a.window_reduce = FAKE * 41, ctypes.cast(_REDUCE, ctypes.c_void_p)
    if sample_only:
        a.sample_only, a.d_all_out = 1, FAKE * 44
    return a


GIB = 1 << 30
P_UNISURF = 96  # N_query + N_freespace of unisurf_args


def workspace_cases():
    """{key: (entry point name, argument block)}: the smallest set that moves every workspace region"""
    out = {}

    def neus(n, **kw):
        key = 'neus/' + '/'.join(f'{k}={v}' for k, v in kw.items()) + f'/n{n}'
        out[key] = ('nr_neus_workspace_bytes', neus_args(n, **kw))
    for algo, No, n in itertools.product(L.UPSAMPLE, (0, 32), (1, 16, 37, 4096, 480000)):
        neus(n, algo=algo, N_outside=No)
    # what decides the deferred sample nablas (and the sample pass), with and without the background
    for kw in (dict(nablas=True), dict(sample_only=True), dict(prec=L.PREC_FP32), dict(no_defer=True)):
        for No, n in itertools.product((0, 32), (37, 4096)):
            neus(n, N_outside=No, **kw)
    for kw in (dict(max_chunk_rays=256), dict(max_chunk_rays=256, max_workspace_bytes=GIB),
               dict(max_workspace_bytes=GIB)):
        for No, n in itertools.product((0, 32), (16, 4096, 480000)):
            neus(n, N_outside=No, **kw)
    for No, steps, n in itertools.product((0, 32), (0, 5), (1, 37, 16384, 480000)):
        out[f'volsdf/No{No}/steps{steps}/n{n}'] = ('nr_volsdf_workspace_bytes', volsdf_args(n, No, steps))

    def unisurf(n, lay, rc, nc, so=False):
        key = f'unisurf/{lay}/rayschunk{rc}/netchunk{nc}/sample_only{int(so)}/n{n}'
        out[key] = ('nr_unisurf_workspace_bytes', unisurf_args(n, lay, rc, nc, so))
    nets = (1048576, 1024 * P_UNISURF)  # not a multiple, a multiple of P
    for lay, rc, nc, n in itertools.product(('flat', 'row', 'rows', 'shard'), (256, 65536), nets, (1, 37, 4096, 70000)):
        unisurf(n, lay, rc, nc)
    for lay, nc in itertools.product(('row', 'shard'), nets):
        # rayschunk past the 65536-ray chunk limit: whole windows per chunk when netchunk % P == 0, else rejected
        unisurf(70000, lay, 200000, nc)
    for lay, n in itertools.product(('flat', 'row', 'shard'), (37, 4096)):
        unisurf(n, lay, 65536, nets[0], True)
    return out


def workspace_totals():
    """{key: total - nr_mlp_workspace_bytes(1)} of the loaded library (the MLP scratch depends on the
    device's CU count; a rejected block's total of 0 stays 0)"""
    lib = L.lib()
    mlp = lib.nr_mlp_workspace_bytes(1)
    out = {}
    for key, (fn, a) in workspace_cases().items():
        t = getattr(lib, fn)(ctypes.byref(a))
        out[key] = t - mlp if t else 0
    return out
