"""What the three framework modules share around their `nr_*_render` call: ray flattening, constant
tables, output tables (allocate / bind / reshape into `extras`), the workspace-and-render sequence,
the sample points of a training render, and the renderer / trainer / config scaffolding."""
import ctypes
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib as L
from .. import rend_util

_TABLES = {}


def _linspace_table(n, device):
    """torch.linspace(0, 1, n) computed on the CPU exactly as the reference does, uploaded once."""
    key = (n, str(device))
    t = _TABLES.get(key)
    if t is None:
        t = torch.linspace(0, 1, n).float().to(device)
        _TABLES[key] = t
    return t


def flat_rays(rays_o, rays_d, batched):
    """rays [(B,) N, 3] -> ro, rd [n, 3] fp32 contiguous, n, B (1 when not batched), the extras' prefix"""
    B = rays_d.shape[0] if batched else 1
    ro = rays_o.reshape(-1, 3).float().contiguous()
    rd = rays_d.reshape(-1, 3).float().contiguous()
    return ro, rd, ro.shape[0], B, ([B, -1] if batched else [-1])


def bypass(x):
    """near_bypass / far_bypass as the library takes them: NaN = none"""
    return float('nan') if x is None else float(x)


# An output table lists a render's outputs in the order of its `extras`: rows of (extras key, args field,
# trailing shape, dtype, condition).  Shape entries are ints or names looked up in `dims`; the condition
# is None or a tuple of names that must all be true in `flags`.
def _on(cond, flags):
    return cond is None or all(flags[c] for c in cond)


f32 = torch.float32
# rgb / depth / mask (/ normals with calc_normal): the first rows of every framework's table
HEAD = [('rgb', 'rgb', (3,), f32, None), ('depth_volume', 'depth', (), f32, None),
        ('mask_volume', 'acc', (), f32, None), ('normals_volume', 'normals', (3,), f32, ('calc_normal',))]


def alloc_outputs(table, n, dims, flags, dev):
    """{extras key: tensor [n, *shape]} for the rows whose condition holds"""
    return {key: torch.empty(n, *[dims.get(s, s) for s in shape], dtype=dt, device=dev)
            for key, _, shape, dt, cond in table if _on(cond, flags)}


def bind_outputs(table, a, out):
    """the allocated outputs' pointers into the args struct (rows left out stay null)"""
    for key, field, *_ in table:
        if key in out:
            setattr(a, field, L.ptr(out[key]))


def extras_of(table, out, prefix, flags):
    """OrderedDict in table order of the [n, ...] tensors in `out`, reshaped to [*prefix, ...]"""
    ret = OrderedDict()
    for key, _, _, _, cond in table:
        if _on(cond, flags) and key in out:
            ret[key] = out[key].reshape(*prefix, *out[key].shape[1:])
    return ret


def run(ws_bytes_fn, render_fn, a, dev):
    """size the workspace for `a`, take the stream's shared buffer, render"""
    ws_bytes = ws_bytes_fn(ctypes.byref(a))
    if ws_bytes == 0:
        raise NotImplementedError('neurecon_amd: ' + L.lib().nr_last_error().decode())
    ws = L.workspace(dev, ws_bytes)
    a.workspace, a.workspace_bytes = L.ptr(ws), ws_bytes
    L.check(render_fn(ctypes.byref(a), L.stream_of(dev)))


def train_points(ro, rd_raw, d_all):
    """F.normalize(rays_d, dim=-1), then the sample points o + d * dir [n, S, 3], the mid-points
    [n, S-1, 3] and the mid depths [n, S-1] of a training render"""
    dev, (n, S) = ro.device, d_all.shape
    rd = torch.empty_like(rd_raw)
    L.check(L.lib().nr_normalize3(L.ptr(rd_raw), n, L.ptr(rd), L.stream_of(dev)))
    pts = torch.empty(n, S, 3, device=dev)
    mids = torch.empty(n, S - 1, 3, device=dev)
    dmid = torch.empty(n, S - 1, device=dev)
    L.check(L.lib().nr_neus_points(L.ptr(ro), L.ptr(rd), L.ptr(d_all), n, S, L.ptr(pts), L.ptr(mids), L.ptr(dmid),
                                   L.stream_of(dev)))
    return rd, pts, mids, dmid


def normals_volume(nablas, w):
    """sum_i w_i normalize(nabla_i) over the samples both have: nablas [n, S, 3], w [n, <= or >= S]"""
    nrm = F.normalize(nablas, dim=-1)
    k = min(w.shape[-1], nrm.shape[-2])
    return (nrm[:, :k, :] * w[:, :k, None]).sum(dim=-2)


class SingleRenderer(nn.Module):
    """an nn.Module so nn.DataParallel can scatter rays over dim 1; subclasses set `render`"""
    render = None

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, rays_o, rays_d, **kwargs):
        return type(self).render(rays_o, rays_d, self.model, **kwargs)


class Trainer(nn.Module):
    """the scaffolding of a training step's forward; subclasses set `Renderer` and write forward()"""
    Renderer = None

    def __init__(self, model, device_ids=[0], batched=True):
        super().__init__()
        self.model = model
        self.renderer = self.Renderer(model)
        if len(device_ids) > 1:
            self.renderer = nn.DataParallel(self.renderer, device_ids=device_ids, dim=1 if batched else 0)
        self.device = device_ids[0]

    @staticmethod
    def rays_and_targets(args, model_input, ground_truth, render_kwargs_train, device, mask_ignore=True):
        """random rays of the image and their targets: rays_o, rays_d [B, N_rays, 3], select_inds,
        target_rgb, mask_ignore (None when absent or not asked for)"""
        intrinsics = model_input['intrinsics'].to(device)
        c2w = model_input['c2w'].to(device)
        H, W = render_kwargs_train['H'], render_kwargs_train['W']
        rays_o, rays_d, select_inds = rend_util.get_rays(c2w, intrinsics, H, W, N_rays=args.data.N_rays)
        target_rgb = rend_util.gather_rays(ground_truth['rgb'].to(device), select_inds)
        ignore = None
        if mask_ignore and 'mask_ignore' in model_input:
            ignore = rend_util.gather_rays(model_input['mask_ignore'].to(device), select_inds)
        return rays_o, rays_d, select_inds, target_rgb, ignore

    @staticmethod
    def sum_losses(losses):
        loss = 0
        for v in losses.values():
            loss += v
        losses['total'] = loss


def net_cfgs(args):
    """surface_cfg, radiance_cfg of get_model (same config keys and defaults in the three frameworks)"""
    m = args.model
    surface_cfg = {
        'use_siren': m.surface.setdefault('use_siren', m.setdefault('use_siren', False)),
        'embed_multires': m.surface.setdefault('embed_multires', 6),
        'radius_init': m.surface.setdefault('radius_init', 1.0),
        'geometric_init': m.surface.setdefault('geometric_init', True),
        'D': m.surface.setdefault('D', 8),
        'W': m.surface.setdefault('W', 256),
        'skips': m.surface.setdefault('skips', [4]),
    }
    radiance_cfg = {
        'use_siren': m.radiance.setdefault('use_siren', m.setdefault('use_siren', False)),
        'embed_multires': m.radiance.setdefault('embed_multires', -1),
        'embed_multires_view': m.radiance.setdefault('embed_multires_view', -1),
        'use_view_dirs': m.radiance.setdefault('use_view_dirs', True),
        'D': m.radiance.setdefault('D', 4),
        'W': m.radiance.setdefault('W', 256),
        'skips': m.radiance.setdefault('skips', []),
    }
    return surface_cfg, radiance_cfg
