"""Config (b)'s SDF net with randomised biases, and its float64 evaluation on the CPU: what the call-by-call
tests of the f16x3 SDF render kernels compare against (the same model and reference as
tests/test_gpu_lean_stream.py, with the geometry feature added)."""
import math

import numpy as np
import torch

import weightgen as wg


def randomised_state(seed):
    """wg.neus_state with every SDF-net bias redrawn (sigma 0.03: three times weightgen's, distinct per row)
    and the sdf row of the last layer scaled element-wise by U(0.5, 1.5): a bias, scale or aux entry read from
    the wrong chunk or op changes the result"""
    sd = wg.neus_state(seed=seed)
    rs = np.random.RandomState(1000 + seed)
    for l in range(9):
        k = f'implicit_surface.surface_fc_layers.{l}.bias'
        b = rs.normal(0.0, 0.03, size=tuple(sd[k].shape))
        if l == 8:
            b[0] = -0.5 + rs.normal(0.0, 0.05)
        sd[k] = torch.tensor(b, dtype=torch.float32)
    k = 'implicit_surface.surface_fc_layers.8.weight_v'
    v = sd[k].clone()
    v[0] *= torch.tensor(rs.uniform(0.5, 1.5, size=(v.shape[1],)), dtype=torch.float32)
    sd[k] = v
    return sd


def float64_sdf_nabla_feature(m, x):
    """points -> sdf, d sdf / d x and the geometry feature in float64 on the CPU (base.py:243-282), from the
    model's effective fp32 weights"""
    from oracle.nets import embed, softplus100
    sl = [(l.effective_weight().detach().cpu().double(), l.bias.detach().cpu().double())
          for l in m.implicit_surface.surface_fc_layers]
    x = x.detach().cpu().double().requires_grad_(True)
    xe = embed(x, 6)
    h = xe
    for i in range(8):
        if i == 4:
            h = torch.cat([h, xe], -1) / math.sqrt(2)
        h = softplus100(h @ sl[i][0].T + sl[i][1])
    out = h @ sl[8][0].T + sl[8][1]
    nab, = torch.autograd.grad(out[:, 0].sum(), x)
    return out[:, 0].detach().numpy(), nab.numpy(), out[:, 1:].detach().numpy()
