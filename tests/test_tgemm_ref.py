"""Pins tests/tgemm_ref.py (the float64 reference tests/test_gpu_tgemm.py holds nr_train_gemm to) to
the operator itself, on the CPU: the per-call references composed in SdfNablaTG's order (primal, nabla
chain, tangent, adjoint; neurecon_amd/training.py) and in RadianceTG's backward order reproduce float64
autograd of the oracle's nets (oracle.nets.SDFNet through oracle.train.nablas_graph, oracle.nets.RadianceNet)
under random upstream gradients, each quantity at 1e-10 of its largest entry: sdf, nablas, feature, the
data adjoints zbar_l (autograd's bias gradient of one point's loss) and dW_l = zbar_l^T h_in + delta_l^T
hdot_in.  So a factor, a transposition or a row restriction read wrongly from the packs' conventions
fails here, without a GPU."""
import pytest
import torch

import weightgen as wg
from tgemm_ref import ISQ2, TG_MUL, TG_NONE, TG_RELUMASK, TG_SOFTPLUS, TG_SPADJ, radiance_ops, sdf_ops, tgemm_ref

REL = 1e-10
P = 8


def _close(name, got, ref):
    sc = float(ref.abs().max())
    e = float((got - ref).abs().max())
    print(f'{name}: max |composed - autograd| {e / sc:.2e} of {sc:.3e}')
    assert e <= REL * sc, name


def _per_point_bias_grads(losses, biases):
    """[P, n_l] per layer: the gradient of point p's loss with respect to b_l = that point's zbar_l"""
    rows = [torch.autograd.grad(lp, biases, retain_graph=True) for lp in losses]
    return [torch.stack([r[l] for r in rows]) for l in range(len(biases))]


def test_sdf_chain_of_references_vs_float64_autograd():
    from oracle.nets import SDFNet, embed
    from oracle.train import nablas_graph
    sd = {k: v.double() for k, v in wg.neus_state(seed=11).items() if k.startswith('implicit_surface.')
          and not k.endswith('obj_bounding_size')}
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    net = SDFNet(sd)
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x = r(P, 3) * 0.7
    gs, gn, gf = r(P), r(P, 3), r(P, 256) * 0.01
    s, n, h = nablas_graph(net, x)
    per_point = (s * gs) + (n * gn).sum(-1) + (h * gf).sum(-1)
    Wt = [w for w, _ in net.layers]
    bt = [b for _, b in net.layers]
    zbar_ref = _per_point_bias_grads(per_point, bt)
    dW_ref = torch.autograd.grad(per_point.sum(), Wt)

    # ---- the same from per-call references, in SdfNablaTG's order ----
    W = [w.detach() for w in Wt]
    b = [v.detach() for v in bt]
    ops = sdf_ops(W, b)
    nv = [256, 256, 256, 217, 256, 256, 256, 256]

    def call(i, mode, x1, n1, **kw):
        M, bias, rv = ops[i]
        return tgemm_ref(M, bias, mode, x1, n1, rowvec=rv, **kw)

    xg = x.clone().requires_grad_(True)
    h0g = embed(xg, 6)
    h0 = h0g.detach()
    H, S, delta = [None] * 8, [None] * 8, [None] * 8
    for l in range(8):                                                     # primal F0..F7
        if l == 0:
            o = call(l, TG_SOFTPLUS, h0, 39)
        elif l == 4:
            o = call(l, TG_SOFTPLUS, H[3], 217, x2=h0, n2=39)
        else:
            o = call(l, TG_SOFTPLUS, H[l - 1], nv[l - 1])
        H[l], S[l] = o['y'], o['y2']
    delta[7], sdf = o['y3'], o['dot'] + b[8][0]
    feat = call(8, TG_NONE, H[7], 256)['y']
    for l in range(7, 0, -1):                                              # nabla chain B7..B1
        o = call(16 - l, TG_MUL, delta[l], nv[l], ny=nv[l - 1], a=S[l - 1])
        delta[l - 1] = o['y2']
        if l == 4:
            e_skip = o['yb']
    e_first = call(16, TG_NONE, delta[0], 256)['y']
    nab = torch.autograd.grad(h0g, xg, e_first + e_skip, retain_graph=True)[0]
    _close('sdf', sdf, s.detach())
    _close('nablas', nab, n.detach())
    _close('feature', feat, h.detach())
    hd0 = torch.autograd.functional.jvp(lambda t: embed(t, 6), x, gn)[1]    # tangent seed J_emb g_nab
    ZD, HD = [None] * 8, [None] * 8
    for l in range(8):                                                     # tangent F0..F7 (no bias)
        if l == 0:
            o = call(l, TG_MUL, hd0, 39, bias=False, a=S[l])
        elif l == 4:
            o = call(l, TG_MUL, HD[3], 217, x2=hd0, n2=39, bias=False, a=S[l])
        else:
            o = call(l, TG_MUL, HD[l - 1], nv[l - 1], bias=False, a=S[l])
        ZD[l], HD[l] = o['y'], o['y2']
    Z = [None] * 8                                                         # adjoint B8, B7..B1
    Z[7] = call(17, TG_SPADJ, gf, 256, x2=gs[:, None], n2=1, a=S[7], zd=ZD[7], g_row=True)['y']
    for l in range(7, 0, -1):
        Z[l - 1] = call(16 - l, TG_SPADJ, Z[l], nv[l], ny=nv[l - 1], a=S[l - 1], g=delta[l - 1], g_scaled=True,
                        zd=ZD[l - 1])['y']
    for l in range(8):
        _close(f'zbar_{l}', Z[l], zbar_ref[l])
        if l == 0:
            hin, hdin = h0, hd0
        elif l == 4:
            hin, hdin = torch.cat([H[3], h0], 1) * ISQ2, torch.cat([HD[3], hd0], 1) * ISQ2
        else:
            hin, hdin = H[l - 1], HD[l - 1]
        _close(f'dW_{l}', Z[l].t() @ hin + delta[l].t() @ hdin, dW_ref[l])
    ob = torch.cat([gs[:, None], gf], 1)
    _close('zbar_8', ob, zbar_ref[8])
    dW8 = ob.t() @ H[7]
    dW8[0] += HD[7].sum(0)
    _close('dW_8', dW8, dW_ref[8])


@pytest.mark.parametrize('view', [True, False])
def test_radiance_backward_chain_of_references_vs_float64_autograd(view):
    from oracle.nets import RadianceNet, embed
    sd = {k: v.double().clone().requires_grad_(True) for k, v in wg.neus_state(seed=11, use_view_dirs=view).items()
          if k.startswith('radiance_net.')}
    net = RadianceNet(sd, multires_view=4, use_view_dirs=view)
    gen = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, v = r(P, 3), torch.nn.functional.normalize(r(P, 3), dim=-1)
    nrm, feat = r(P, 3).requires_grad_(True), r(P, 256).requires_grad_(True)
    gy = r(P, 3)
    zs = []
    y = net.forward(x, v, nrm, feat, z_out=zs)
    assert min(float(z.abs().min()) for z in zs) > 1e-9  # no unit on its ReLU kink
    per_point = (y * gy).sum(-1)
    Wt = [w for w, _ in net.layers]
    bt = [b for _, b in net.layers]
    zbar_ref = _per_point_bias_grads(per_point, bt)
    dW_ref = torch.autograd.grad(per_point.sum(), Wt, retain_graph=True)
    d_in = torch.autograd.grad(per_point.sum(), [feat] + ([nrm] if view else []))

    # ---- RadianceTG.backward's order over the training pack's ops ----
    W = [w.detach() for w in Wt]
    nvw = 27 if view else 0
    ns = 3 + nvw + (3 if view else 0)
    ops = radiance_ops(W, ns)
    inp = torch.cat([x, embed(v, 4), nrm.detach(), feat.detach()] if view else [x, feat.detach()], 1)
    Hs = [torch.relu(z) for z in zs]                                      # the forward's saved activations
    yd = y.detach()
    g = gy * yd * (1 - yd)                                                # sigmoid'
    _close('zbar_4', g, zbar_ref[4])
    _close('dW_4', g.t() @ Hs[3], dW_ref[4])
    gz = tgemm_ref(ops[0][0], None, TG_RELUMASK, g, 3, bias=False, a=Hs[3])['y']
    for l in range(3, 0, -1):
        _close(f'zbar_{l}', gz, zbar_ref[l])
        _close(f'dW_{l}', gz.t() @ Hs[l - 1], dW_ref[l])
        gz = tgemm_ref(ops[4 - l][0], None, TG_RELUMASK, gz, 256, bias=False, a=Hs[l - 1])['y']
    _close('zbar_0', gz, zbar_ref[0])
    _close('dW_0', gz.t() @ inp, dW_ref[0])
    o = tgemm_ref(ops[4][0], None, TG_NONE, gz, 256, ny=256, bias=False)
    _close('d feature', o['y'], d_in[0])
    if view:
        _close('d normals', o['yb'][:, 3 + nvw:3 + nvw + 3], d_in[1])
