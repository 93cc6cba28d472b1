"""The training step's compositing -- NeuS, NeuS with the NeRF++ background, VolSDF (builtin background
sphere and / or NeRF++ background samples) and UNISURF -- as plain differentiable torch, the reference
tests/test_gpu_composite.py holds the kernels of csrc/nr_train.hip to.  The code takes its dtype from its
inputs (fp32 and fp64 run the same lines), works on any leading dimensions and is built from the oracle's
own sdf_to_alpha / alpha_to_w / sdf_to_sigma; tests/test_composite_ref.py pins it to oracle/train.py.

Every function returns a dict: the differentiable outputs rgb [.., 3], depth [..], acc [..] and the
visibility weights, then the extras the kernels can also store (alpha, cdf / p_i, sigma, sdf_out).
`s` and `beta` broadcast against sdf, so a [R, 1] leaf gives their gradient per ray (what the kernels
return; the host sums it)."""
import torch
import torch.nn.functional as F

from oracle.neus import alpha_to_w, sdf_to_alpha
from oracle.volsdf import sdf_to_sigma


def _sums(w, rad, d, white):
    rgb = torch.sum(w[..., None] * rad, -2)
    acc = torch.sum(w, -1)
    depth = torch.sum(w / (w.sum(-1, keepdim=True) + 1e-10) * d, -1)
    if white:
        rgb = rgb + (1.0 - acc[..., None])
    return rgb, depth, acc


def neus(sdf, s, rad, dmid, white, bg=None):
    """neus.py:28-70, :346-355.  sdf [.., S], rad [.., S-1, 3], dmid [.., S-1].  bg = (sigma_out [.., M],
    rad_out [.., M, 3], d_out [.., M], inside [.., S-1]) merges the NeRF++ background (neus.py:325-352):
    M = S-1 + N_outside samples at d_out, mid-point k takes the SDF alpha and colour where inside[k], the
    background's elsewhere; the last distance is 1e10."""
    cdf, alpha = sdf_to_alpha(sdf, s)
    d = dmid
    if bg is not None:
        sigma_out, rad_out, d_out, inside = bg
        dists = d_out[..., 1:] - d_out[..., :-1]
        dists = torch.cat([dists, 1e10 * torch.ones_like(dists[..., :1])], -1)
        alpha_out = 1 - torch.exp(-F.softplus(sigma_out) * dists)
        n1 = alpha.shape[-1]
        m_in = inside.to(sdf.dtype)
        m_out = (~inside.bool()).to(sdf.dtype)
        alpha = torch.cat([alpha * m_in + alpha_out[..., :n1] * m_out, alpha_out[..., n1:]], -1)
        rad = torch.cat([rad * m_in[..., None] + rad_out[..., :n1, :] * m_out[..., None], rad_out[..., n1:, :]], -2)
        d = d_out
    w = alpha_to_w(alpha)
    rgb, depth, acc = _sums(w, rad, d, white)
    return dict(rgb=rgb, depth=depth, acc=acc, weights=w, alpha=alpha, cdf=cdf)


def volsdf(sdf, beta, rad, pts, d_all, use_bg, r_bg, white, bg=None):
    """volsdf.py:16-35, :317-325, :455-506.  sdf [.., S] are the network's values at pts [.., S, 3]; with
    use_bg a sample whose r_bg - |x| is smaller takes that value; rad [.., S, 3], d_all [.., S].
    bg = (sigma_bg [.., N], rad_bg [.., N, 3], d_bg [.., N]) appends the NeRF++ background samples (their
    raw sigma); M = S + N samples, M-1 intervals."""
    sdf_out = sdf
    if use_bg:
        dbg = r_bg - pts.norm(dim=-1)
        sdf_out = torch.where(dbg < sdf, dbg, sdf)
    sigma = sdf_to_sigma(sdf_out, 1. / beta, beta)
    d = d_all
    if bg is not None:
        sigma_bg, rad_bg, d_bg = bg
        sigma = torch.cat([sigma, sigma_bg], -1)
        rad = torch.cat([rad, rad_bg], -2)
        d = torch.cat([d_all, d_bg], -1)
    delta = d[..., 1:] - d[..., :-1]
    p = torch.exp(-F.relu(sigma[..., :-1] * delta))
    tau = (1 - p + 1e-10) * torch.cumprod(torch.cat([torch.ones_like(p[..., :1]), p], -1), -1)[..., :-1]
    rgb, depth, acc = _sums(tau, rad[..., :-1, :], d[..., :-1], white)
    return dict(rgb=rgb, depth=depth, acc=acc, weights=tau, p_i=p, sigma=sigma, sdf_out=sdf_out)


def unisurf(logits, rad, d_all, white):
    """unisurf.py:53-62, :219-236.  logits [.., P], rad [.., P, 3], d_all [.., P]."""
    odds = torch.exp(-1. * logits)
    alpha = odds / (1 + odds)
    w = alpha_to_w(alpha)
    rgb, depth, acc = _sums(w, rad, d_all, white)
    return dict(rgb=rgb, depth=depth, acc=acc, weights=w, alpha=alpha)
