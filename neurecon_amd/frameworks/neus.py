"""NeuS framework: same API as the reference's models/frameworks/neus.py, render path on HIP.

`volume_render(rays_o, rays_d, model, **kw) -> (rgb, depth, extras)` keeps the reference's
signature, argument meaning, output shapes and extras keys (neus.py:118-397); the whole ray
chunk (near/far, coarse samples, 4-round 'official_solution' upsampling, SDF + nablas, radiance,
alpha compositing) runs in libnrhip.so (`nr_neus_render`).
"""
import copy
import ctypes
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib as L
from .. import rend_util
from ..base import ImplicitSurface, NeRF, RadianceNet, check_view_dirs, wants_graph
from . import _shell
from ._shell import (HEAD, _linspace_table, alloc_outputs, bind_outputs, bypass, extras_of, f32, flat_rays, net_cfgs,
                     normals_volume, run, train_points)


class NeuS(nn.Module):
    """neus.py:72-115 (parameter tree and names identical: ln_s, implicit_surface.*, radiance_net.*,
    nerf_outside.*)."""

    def __init__(self, variance_init=0.05, speed_factor=1.0, input_ch=3, W_geo_feat=-1, use_outside_nerf=False,
                 obj_bounding_radius=1.0, surface_cfg=dict(), radiance_cfg=dict()):
        super().__init__()
        self.ln_s = nn.Parameter(data=torch.Tensor([-np.log(variance_init) / speed_factor]), requires_grad=True)
        self.speed_factor = speed_factor
        self.implicit_surface = ImplicitSurface(W_geo_feat=W_geo_feat, input_ch=input_ch,
                                                obj_bounding_size=obj_bounding_radius, **surface_cfg)
        if W_geo_feat < 0:
            W_geo_feat = self.implicit_surface.W
        self.radiance_net = RadianceNet(W_geo_feat=W_geo_feat, **radiance_cfg)
        if use_outside_nerf:
            self.nerf_outside = NeRF(input_ch=4, multires=10, multires_view=4, use_view_dirs=True)

    def forward_radiance(self, x, view_dirs):
        _, nablas, geometry_feature = self.implicit_surface.forward_with_nablas(x)
        return self.radiance_net.forward(x, view_dirs, nablas, geometry_feature)

    def forward_s(self):
        return torch.exp(self.ln_s * self.speed_factor)

    def forward(self, x, view_dirs):
        sdf, nablas, geometry_feature = self.implicit_surface.forward_with_nablas(x)
        radiances = self.radiance_net.forward(x, view_dirs, nablas, geometry_feature)
        return radiances, sdf, nablas


def _neus_uniforms(B, N, batched, rayschunk, direct, n_iters, n_up, N_importance, N_outside, dev):
    """perturb=True uniforms in the reference's draw order (neus.py:385-397 ray-chunk loop; per chunk
    sample_pdf's torch.rand(..., device) per upsampling round (rend_util.py:271) and the NeRF++
    stratification's CPU torch.rand (neus.py:310)), laid out for the library: u_rand
    [n_iters][B*N][n_up] (direct: [B*N][N_importance]), t_out [B*N][N_outside]."""
    pre = [B] if batched else []
    rd = 1 + len(pre) if not direct else len(pre)  # ray dim of the drawn blocks
    ups, outs = [], []
    for r0 in range(0, N, rayschunk):
        nc = min(rayschunk, N - r0)
        if direct:
            ups.append(rend_util.uniform([*pre, nc, N_importance], dev))
        elif n_iters > 0:
            ups.append(torch.stack([rend_util.uniform([*pre, nc, n_up], dev) for _ in range(n_iters)], 0))
        if N_outside > 0:
            outs.append(rend_util.to_device(rend_util.uniform([*pre, nc, N_outside]).float(), dev))
    u = None
    if ups:
        u = torch.cat(ups, rd)
        u = (u.reshape(B * N, N_importance) if direct else u.reshape(n_iters, B * N, n_up)).contiguous()
    t_out = torch.cat(outs, len(pre)).reshape(B * N, N_outside).contiguous() if outs else None
    return u, t_out


# a render's outputs in the order of its extras (neus.py:345-380); S samples, M = S - 1 + N_outside
OUTPUTS = HEAD + [
    ('implicit_nablas', 'nablas_out', ('S', 3), f32, ('detailed',)),
    ('implicit_surface', 'sdf_out', ('S',), f32, ('detailed',)),
    ('radiance', 'radiance_out', ('M', 3), f32, ('detailed',)),
    ('alpha', 'alpha_out', ('M',), f32, ('detailed',)),
    ('cdf', 'cdf_out', ('S',), f32, ('detailed',)),
    ('visibility_weights', 'weights_out', ('M',), f32, ('detailed',)),
    ('d_final', 'd_final', ('M',), f32, ('detailed',)),
    ('sigma_out', 'sigma_out', ('M',), f32, ('detailed', 'outside')),
    ('radiance_out', 'radiance_bg_out', ('M', 3), f32, ('detailed', 'outside')),
]


def _counts(upsample_algo, N_samples, N_importance, N_upsample_iters):
    """direct, new samples per sample_pdf (direct: one of N_importance, neus.py:215-243), total samples S"""
    if upsample_algo not in L.UPSAMPLE:
        raise NotImplementedError(upsample_algo)
    direct = upsample_algo != 'official_solution'
    n_up = N_importance if direct else (N_importance // N_upsample_iters if N_upsample_iters > 0 else 0)
    return direct, n_up, N_samples + (N_importance if direct else N_upsample_iters * n_up)


def _sampling_args(ro, rd, model, dev, rad_packed, obj_bounding_radius, rayschunk, max_workspace_gb, near_bypass,
                   far_bypass, fixed_s_recp, N_samples, N_importance, upsample_algo, N_nograd_samples,
                   N_upsample_iters, n_up):
    """the argument fields that a render and the training's sample pass fill alike"""
    sdf_desc, sdf_packed = model.implicit_surface.nr_packed(dev)
    a = L.NrNeusArgs()
    a.rays_o, a.rays_d, a.n_rays = L.ptr(ro), L.ptr(rd), ro.shape[0]
    a.sdf, a.sdf_packed = ctypes.pointer(sdf_desc), L.ptr(sdf_packed)
    a.rad, a.rad_packed = ctypes.pointer(model.radiance_net.nr_desc()), L.ptr(rad_packed)
    a.obj_bounding_radius = float(obj_bounding_radius)
    a.near_bypass, a.far_bypass = bypass(near_bypass), bypass(far_bypass)
    a.N_samples, a.N_importance, a.N_upsample_iters = N_samples, N_importance, N_upsample_iters
    a.t_coarse, a.u_fine = L.ptr(_linspace_table(N_samples, dev)), L.ptr(_linspace_table(max(n_up, 1), dev))
    a.upsample_algo = L.UPSAMPLE[upsample_algo]
    a.fixed_s = 1. / fixed_s_recp
    if upsample_algo == 'direct_more':
        a.N_nograd_samples, a.t_nograd = N_nograd_samples, L.ptr(_linspace_table(N_nograd_samples, dev))
    a.max_chunk_rays = int(rayschunk) if rayschunk else 0
    a.max_workspace_bytes = L.workspace_budget_bytes(max_workspace_gb)
    return a


def volume_render(rays_o, rays_d, model, obj_bounding_radius=1.0, batched=False, batched_info={},
                  calc_normal=False, use_view_dirs=True, rayschunk=65536, netchunk=1048576, white_bkgd=False,
                  near_bypass=None, far_bypass=None, detailed_output=True, show_progress=False, perturb=False,
                  fixed_s_recp=1 / 64., N_samples=64, N_importance=64, N_outside=0,
                  upsample_algo='official_solution', N_nograd_samples=2048, N_upsample_iters=4,
                  skip_zero_alpha=True, defer_sample_nablas=True, max_workspace_gb=None, fold_feature=True,
                  serial_order=False, **dummy_kwargs):
    """neus.py:118-397, render mode.  skip_zero_alpha (not a reference argument): mid-points whose alpha
    is exactly 0 (and, with NeRF++, the ones outside the bounding sphere) skip the SDF + radiance nets
    when the radiance output is not asked for -- their weight is an exact 0 (or their colour is the
    background's), so rgb / depth / mask / normals are bit-identical;
    False evaluates every mid-point as the reference does.  defer_sample_nablas (not a reference
    argument; with skip_zero_alpha, the f16x3 softplus net, without the per-sample nablas / radiance
    outputs; with or without NeRF++): the samples' reverse pass (their nablas feed only normals_volume,
    weighted by w_i) runs after the sampling, only on the 16-sample tiles holding a sample of non-zero
    weight -- bit-identical maps.  Memory: the library renders chunks of at most `rayschunk` rays (the
    reference's memory bound, neus.py:384-397) whose workspace fits max_workspace_gb (not a reference
    argument; None: _lib.set_workspace_budget / $NR_MAX_WORKSPACE_GB / 4 GiB) -- the maps do not depend
    on the chunking.  fold_feature (not a reference argument; f16x3 softplus SDF net and ReLU D=4 radiance
    net, else without effect): the geometry-feature layer, which has no activation, is folded into the
    radiance net's layer 0 once per weight version (RadianceNet.nr_fold_packed), so the mid-points skip one
    256x256 layer product; sampling, sdf, nablas and weights are bit-identical, radiance differs by layer
    0's rounding.  False: the feature goes through layer 0 as in the reference.  serial_order (not a
    reference argument): True keeps every launch of a chunk on the current stream with tiles at a fixed
    stride; by default the mid-point, radiance and compacted reverse-pass launches claim their tiles at run
    time and the reverse pass runs on the library's side stream beside the other two -- bit-identical maps.
    rays_o/rays_d: [(B,) N_rays, 3]; rays_d need not be normalized.
    perturb=True draws the reference's uniforms (same generators, shapes and order) and hands them
    to the kernels."""
    L.require_gpu(rays_o, 'rays_o')
    if wants_graph(model):
        return _train_render(rays_o, rays_d, model, obj_bounding_radius=obj_bounding_radius, batched=batched,
                             calc_normal=calc_normal, use_view_dirs=use_view_dirs, rayschunk=rayschunk,
                             white_bkgd=white_bkgd, near_bypass=near_bypass, far_bypass=far_bypass,
                             detailed_output=detailed_output, perturb=perturb, fixed_s_recp=fixed_s_recp,
                             N_samples=N_samples, N_importance=N_importance, N_outside=N_outside,
                             upsample_algo=upsample_algo, N_nograd_samples=N_nograd_samples,
                             N_upsample_iters=N_upsample_iters)
    direct, n_up, S = _counts(upsample_algo, N_samples, N_importance, N_upsample_iters)
    check_view_dirs(model, use_view_dirs)
    dev = rays_o.device
    ro, rd, n, B, prefix = flat_rays(rays_o, rays_d, batched)
    flags = dict(calc_normal=calc_normal, detailed=detailed_output, outside=N_outside > 0)
    rad_packed = model.radiance_net.nr_packed(dev)[1]
    s_dev = model.forward_s().detach().float().reshape(-1)[:1].contiguous()  # stays on the device
    a = _sampling_args(ro, rd, model, dev, rad_packed, obj_bounding_radius, rayschunk, max_workspace_gb, near_bypass,
                       far_bypass, fixed_s_recp, N_samples, N_importance, upsample_algo, N_nograd_samples,
                       N_upsample_iters, n_up)
    # M = samples after the NeRF++ merge (neus.py:325-343)
    out = alloc_outputs(OUTPUTS, n, dict(S=S, M=S - 1 + N_outside), flags, dev)
    bind_outputs(OUTPUTS, a, out)
    fold_packed = model.radiance_net.nr_fold_packed(model.implicit_surface, dev) if fold_feature else None
    a.fold_packed = L.ptr(fold_packed)
    a.s, a.s_dev = 0.0, L.ptr(s_dev)
    a.no_mid_skip = 0 if skip_zero_alpha else 1
    a.no_defer = 0 if defer_sample_nablas else 1
    a.serial_order = 1 if serial_order else 0
    a.calc_normal, a.white_bkgd = int(bool(calc_normal)), int(bool(white_bkgd))
    if N_outside > 0:
        if not hasattr(model, 'nerf_outside'):
            raise ValueError('N_outside > 0 needs a model built with use_outside_nerf=True')
        nerf_desc, nerf_packed = model.nerf_outside.nr_packed(dev)
        a.nerf, a.nerf_packed = ctypes.pointer(nerf_desc), L.ptr(nerf_packed)
        a.N_outside, a.t_outside = N_outside, L.ptr(_linspace_table(N_outside + 2, dev))
    if perturb:
        u_rand, t_out_rand = _neus_uniforms(B, n // B, batched, int(rayschunk), direct, N_upsample_iters, n_up,
                                            N_importance, N_outside, dev)
        a.u_rand, a.t_out_rand = L.ptr(u_rand), L.ptr(t_out_rand)
    lib = L.lib()
    run(lib.nr_neus_workspace_bytes, lib.nr_neus_render, a, dev)
    ret = extras_of(OUTPUTS, out, prefix, flags)
    return ret['rgb'], ret['depth_volume'], ret


def _sample_depths(ro, rd, model, dev, obj_bounding_radius, batched, B, rayschunk, near_bypass, far_bypass, perturb,
                   fixed_s_recp, N_samples, N_importance, upsample_algo, N_nograd_samples, N_upsample_iters,
                   N_outside=0):
    """The no-grad upsampling of a training step (neus.py:206-279): sorted sample depths [n, S] from
    the render kernels' sample pass (forward-only SDF launches, no compositing), and with perturb the
    NeRF++ strata uniforms [n, N_outside] (or None)."""
    direct, n_up, S = _counts(upsample_algo, N_samples, N_importance, N_upsample_iters)
    n = ro.shape[0]
    # the sample pass never evaluates the radiance net: no pack
    a = _sampling_args(ro, rd, model, dev, None, obj_bounding_radius, rayschunk, None, near_bypass, far_bypass,
                       fixed_s_recp, N_samples, N_importance, upsample_algo, N_nograd_samples, N_upsample_iters, n_up)
    d_all = torch.empty(n, S, device=dev)
    t_out = None
    if perturb:  # the NeRF++ strata uniforms are drawn in the same per-chunk order as the render's
        u_rand, t_out = _neus_uniforms(B, n // B, batched, int(rayschunk), direct, N_upsample_iters, n_up,
                                       N_importance, N_outside, dev)
        a.u_rand = L.ptr(u_rand)
    a.sample_only, a.d_all_out = 1, L.ptr(d_all)
    lib = L.lib()
    run(lib.nr_neus_workspace_bytes, lib.nr_neus_render, a, dev)
    return d_all, t_out


def _outside_depths(ro, rd, obj_bounding_radius, far_bypass, N_outside, t_out):
    """NeRF++ background depths (neus.py:303-311): far / flip(linspace(0,1,N+2)[1:-1]), stratified
    with t_out when perturbing; far from near_far_from_sphere on the normalised rays (neus.py:176-178)."""
    _, far = rend_util.near_far_from_sphere(ro, rd, r=obj_bounding_radius)
    if far_bypass is not None:
        far = far_bypass * torch.ones_like(far)
    t = torch.linspace(0, 1, N_outside + 2)[..., 1:-1].float().to(ro.device)
    d = far / torch.flip(t, dims=[-1])
    if t_out is not None:
        mids = .5 * (d[..., 1:] + d[..., :-1])
        upper = torch.cat([mids, d[..., -1:]], -1)
        lower = torch.cat([d[..., :1], mids], -1)
        d = lower + (upper - lower) * t_out
    return d.contiguous()


def _train_render(rays_o, rays_d, model, obj_bounding_radius=1.0, batched=False, calc_normal=False,
                  use_view_dirs=True, rayschunk=65536, white_bkgd=False, near_bypass=None, far_bypass=None,
                  detailed_output=True, perturb=False, fixed_s_recp=1 / 64., N_samples=64, N_importance=64,
                  N_outside=0, upsample_algo='official_solution', N_nograd_samples=2048, N_upsample_iters=4):
    """neus.py:118-397 with an autograd graph (training): sample depths from the no-grad sample pass,
    then SDF + nablas at the samples and mid-points (double-backward capable), the radiance net and
    the compositing as neurecon_amd.training autograd functions.  Returns the reference's
    (rgb, depth, extras) with graph-carrying rgb, depth_volume, mask_volume, implicit_nablas,
    implicit_surface, radiance, visibility_weights."""
    from .. import training as T
    check_view_dirs(model, use_view_dirs)
    dev = rays_o.device
    ro, rd_raw, n, B, prefix = flat_rays(rays_o, rays_d, batched)
    with torch.no_grad():
        d_all, t_out = _sample_depths(ro, rd_raw, model, dev, obj_bounding_radius, batched, B, rayschunk, near_bypass,
                                      far_bypass, perturb, fixed_s_recp, N_samples, N_importance, upsample_algo,
                                      N_nograd_samples, N_upsample_iters, N_outside)
    S = d_all.shape[1]
    rd, pts, mids, dmid = train_points(ro, rd_raw, d_all)  # F.normalize(rays_d, dim=-1) (neus.py:172)
    surf = model.implicit_surface
    Ws = T.effective_weights(surf)  # one weight_norm per layer, shared by both evaluations
    if T.uses_train_gemm(surf):  # samples and mid-points in one evaluation (feature for the mid-points only)
        Ps = n * S
        sdf_all, nab_all, feat_m = T.sdf_nablas(surf, torch.cat([pts.reshape(-1, 3), mids.reshape(-1, 3)]), True,
                                                Ws, feat_from=Ps)
        sdf, nablas, nab_m = sdf_all[:Ps], nab_all[:Ps], nab_all[Ps:]
    else:
        sdf, nablas, _ = T.sdf_nablas(surf, pts.reshape(-1, 3), False, Ws)    # neus.py:294
        _, nab_m, feat_m = T.sdf_nablas(surf, mids.reshape(-1, 3), True, Ws)   # neus.py:103-106, :298
    view = rd[:, None, :].expand(n, S - 1, 3).reshape(-1, 3).contiguous()
    rad = T.radiance(model.radiance_net, mids.reshape(-1, 3), view, nab_m, feat_m)
    s = model.forward_s().float().reshape(-1)[:1]
    out = {}
    if N_outside > 0:  # neus.py:303-343: the background net at cat([d_mid, outside depths])
        with torch.no_grad():
            d_out = torch.cat([dmid, _outside_depths(ro, rd, obj_bounding_radius, far_bypass, N_outside, t_out)], -1)
            d_out = d_out.contiguous()
            M = d_out.shape[1]
            x_emb = torch.empty(n * M, 84, device=dev)
            v_emb = torch.empty(n * M, 27, device=dev)
            inside = torch.empty(n, S - 1, dtype=torch.uint8, device=dev)
            L.check(L.lib().nr_nerf_train_input(L.ptr(ro), L.ptr(rd), L.ptr(d_out), n, M, S - 1,
                                                float(obj_bounding_radius), L.ptr(x_emb), L.ptr(v_emb), L.ptr(inside),
                                                L.stream_of(dev)))
        sig_o, rad_o = T.nerf(model.nerf_outside, x_emb, v_emb)
        rgb, depth, acc, w, alpha, cdf = T.NeuSCompositeBG.apply(sdf.reshape(n, S), s, rad.reshape(n, S - 1, 3),
                                                                 sig_o.reshape(n, M), rad_o.reshape(n, M, 3), d_out,
                                                                 inside, bool(white_bkgd))
        out.update(d_final=d_out, sigma_out=sig_o.reshape(n, M), radiance_out=rad_o.reshape(n, M, 3))
    else:
        rgb, depth, acc, w, alpha, cdf = T.NeuSComposite.apply(sdf.reshape(n, S), s, rad.reshape(n, S - 1, 3), dmid,
                                                              bool(white_bkgd))
        out.update(d_final=dmid)
    nablas = nablas.reshape(n, S, 3)
    # radiance: the surface net's colours at the mid-points
    out.update(rgb=rgb, depth_volume=depth, mask_volume=acc, implicit_nablas=nablas, implicit_surface=sdf.reshape(n, S),
               radiance=rad.reshape(n, S - 1, 3), alpha=alpha, cdf=cdf, visibility_weights=w)
    if calc_normal:  # neus.py:364-368
        out['normals_volume'] = normals_volume(nablas, w)
    ret = extras_of(OUTPUTS, out, prefix, dict(calc_normal=calc_normal, detailed=detailed_output,
                                               outside=N_outside > 0))
    return ret['rgb'], ret['depth_volume'], ret


class SingleRenderer(_shell.SingleRenderer):
    """neus.py:399-405"""
    render = staticmethod(volume_render)


class Trainer(_shell.Trainer):
    """neus.py:408-485: one training step's forward -- random rays of the image, the render with a
    graph (training autograd functions on libnrhip.so), L1 rgb + eikonal + BCE mask losses.  Returns
    OrderedDict(losses=..., extras=...) exactly like the reference; train.py calls backward() on
    losses['total'] (under DDP the gradient all-reduce runs over RCCL)."""
    Renderer = SingleRenderer

    def forward(self, args, indices, model_input, ground_truth, render_kwargs_train, it, device='cuda'):
        from ..config import as_cfg
        args = as_cfg(args)
        # rays [B, N_rays, 3] (neus.py:432)
        rays_o, rays_d, select_inds, target_rgb, mask_ignore = self.rays_and_targets(
            args, model_input, ground_truth, render_kwargs_train, device)
        rgb, depth_v, extras = self.renderer(rays_o, rays_d, detailed_output=True, **render_kwargs_train)
        nablas = extras['implicit_nablas']
        nablas_norm = torch.norm(nablas, dim=-1)
        mask_volume = torch.clamp(extras['mask_volume'], 1e-3, 1 - 1e-3)
        extras['mask_volume_clipped'] = mask_volume
        losses = OrderedDict()
        losses['loss_img'] = F.l1_loss(rgb, target_rgb, reduction='none')
        losses['loss_eikonal'] = args.training.w_eikonal * F.mse_loss(
            nablas_norm, nablas_norm.new_ones(nablas_norm.shape), reduction='mean')
        if args.training.with_mask:
            target_mask = rend_util.gather_rays(model_input['object_mask'].to(device), select_inds)
            losses['loss_mask'] = args.training.w_mask * F.binary_cross_entropy(mask_volume, target_mask.float(),
                                                                                reduction='mean')
            if mask_ignore is not None:
                target_mask = torch.logical_and(target_mask, mask_ignore)
            losses['loss_img'] = (losses['loss_img'] * target_mask[..., None].float()).sum() / \
                (target_mask.sum() + 1e-10)
        elif mask_ignore is not None:
            losses['loss_img'] = (losses['loss_img'] * mask_ignore[..., None].float()).sum() / (mask_ignore.sum() + 1e-10)
        else:
            losses['loss_img'] = losses['loss_img'].mean()
        self.sum_losses(losses)
        extras['implicit_nablas_norm'] = nablas_norm
        extras['scalars'] = {'1/s': 1. / self.model.forward_s().data}
        extras['select_inds'] = select_inds
        return OrderedDict([('losses', losses), ('extras', extras)])


def get_model(args):
    """neus.py:488-546 (same config keys and defaults)."""
    from ..config import as_cfg
    args = as_cfg(args)
    if not args.training.with_mask:
        assert 'N_outside' in args.model.keys() and args.model.N_outside > 0, \
            'Please specify a positive model:N_outside for neus with nerf++'
    model_config = {
        'obj_bounding_radius': args.model.obj_bounding_radius,
        'W_geo_feat': args.model.setdefault('W_geometry_feature', 256),
        'use_outside_nerf': not args.training.with_mask,
        'speed_factor': args.training.setdefault('speed_factor', 1.0),
        'variance_init': args.model.setdefault('variance_init', 0.05),
    }
    model_config['surface_cfg'], model_config['radiance_cfg'] = net_cfgs(args)
    model = NeuS(**model_config)
    render_kwargs_train = {
        'upsample_algo': args.model.setdefault('upsample_algo', 'official_solution'),
        'N_nograd_samples': args.model.setdefault('N_nograd_samples', 2048),
        'N_upsample_iters': args.model.setdefault('N_upsample_iters', 4),
        'N_outside': args.model.setdefault('N_outside', 0),
        'obj_bounding_radius': args.data.setdefault('obj_bounding_radius', 1.0),
        'batched': args.data.batch_size is not None,
        'perturb': args.model.setdefault('perturb', True),
        'white_bkgd': args.model.setdefault('white_bkgd', False),
    }
    render_kwargs_test = copy.deepcopy(render_kwargs_train)
    render_kwargs_test['rayschunk'] = args.data.val_rayschunk
    render_kwargs_test['perturb'] = False
    trainer = Trainer(model, device_ids=args.device_ids, batched=render_kwargs_train['batched'])
    return model, trainer, render_kwargs_train, render_kwargs_test, trainer.renderer
