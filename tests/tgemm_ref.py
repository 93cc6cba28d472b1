"""Float64 reference of one training layer GEMM call (nr_train_gemm, include/neurecon_hip.h "Training
layer GEMMs"), in plain torch: no GPU and no library needed.

  z = [x1[:, :n1] ; x2[:, :n2]] M^T (+ b)              M, b: the op's effective matrix / bias, float64
  NR_TG_NONE      y = z yscale
  NR_TG_SOFTPLUS  y = softplus(z; beta 100, threshold 20), y2 = softplus'(z), y3 = y2 rowvec,
                  dot = y . rowvec + dot_bias
  NR_TG_MUL       y = z yscale, y2 = a y
  NR_TG_SPADJ     y = z yscale s + [g zdot 100 s (1 - s)],  s = a;  the bracket with g = the g tensor,
                  g = rowvec (g_row), or with g_scaled (g holds s g): g zdot 100 (1 - s)
  NR_TG_RELUMASK  y = z where a > 0, else 0
The output columns are [y (the op's first output segment) ; yb (its second)]; the epilogue tensors
(a, g, zdot) cover the first segment only, so yb is specified for NONE and MUL (yb = z yscale).

sdf_ops / radiance_ops give (M, b, rowvec) per op from a net's effective weights W_l [out, in], read
the way neurecon_amd/training.py uses the packs (nr_sdf_pack / nr_sdf_train_pack / nr_radiance_train_pack
in csrc/nr_capi.hip): the skip layer's input is cat([h3, embed(x)]) / sqrt(2), so F4 and B4 carry
W4 / sqrt(2); B_l = W_l^T restricted to the stored rows; B8 = W8^T over the inputs [d feature ; d sdf]
with W8[0, :] as its row vector (which also rides F7); the radiance pack's ops are W4^T (head), W3^T,
W2^T, W1^T and W0^T with its outputs ordered [d feature ; d small inputs].
tests/test_tgemm_ref.py pins the composition of these per-call references to float64 autograd of the
oracle's nets."""
import math

import torch
import torch.nn.functional as F

TG_NONE, TG_SOFTPLUS, TG_MUL, TG_SPADJ, TG_RELUMASK = 0, 1, 3, 4, 5
ISQ2 = 1.0 / math.sqrt(2.0)


def tgemm_ref(M, b, mode, x1, n1, x2=None, n2=0, ny=None, bias=True, yscale=1.0, a=None, g=None, zd=None,
              g_row=False, g_scaled=False, rowvec=None, dot_bias=0.0, dtype=torch.float64):
    """expected outputs of one call as a dict: z (the product before the epilogue, all valid output
    columns), y / yb (the first ny valid columns / the rest), y2, y3, dot (None where the mode has none).
    M [n_out, n1 + n2], b [n_out] or None, rowvec [ny] or None; everything is converted to dtype
    (float32: the same formula as the fp32 matrix product plus elementwise code the kernel replaced)."""
    d = lambda t: None if t is None else t.to(dtype)
    M, b, rowvec = d(M), d(b), d(rowvec)
    X = d(x1)[:, :n1]
    if n2:
        X = torch.cat([X, d(x2)[:, :n2]], 1)
    z = X @ M.t()
    if bias and b is not None:
        z = z + b
    ny = z.shape[1] if ny is None else ny
    zy = z[:, :ny]
    out = dict(z=z, y=None, yb=None, y2=None, y3=None, dot=None)
    cut = lambda t: d(t)[:, :ny]
    if mode == TG_NONE:
        out['y'] = zy * yscale
    elif mode == TG_SOFTPLUS:
        out['y'] = F.softplus(zy, beta=100, threshold=20)
        out['y2'] = torch.where(zy * 100 > 20, torch.ones_like(zy), torch.sigmoid(100 * zy))
        if rowvec is not None:
            out['y3'] = out['y2'] * rowvec
            out['dot'] = out['y'] @ rowvec + dot_bias
    elif mode == TG_MUL:
        out['y'] = zy * yscale
        out['y2'] = cut(a) * out['y']
    elif mode == TG_SPADJ:
        s = cut(a)
        y = zy * yscale * s
        if g_row:
            y = y + rowvec * cut(zd) * (100 * s * (1 - s))
        elif g is not None:
            y = y + cut(g) * cut(zd) * (100 * (1 - s) if g_scaled else 100 * s * (1 - s))
        out['y'] = y
    elif mode == TG_RELUMASK:
        out['y'] = torch.where(cut(a) > 0, zy, torch.zeros_like(zy))
    else:
        raise ValueError(mode)
    if z.shape[1] > ny and mode in (TG_NONE, TG_MUL):
        out['yb'] = z[:, ny:] * yscale
    return out


def sdf_ops(Ws, bs):
    """op index (nr_sdf_op_info: 0..8 = F0..F8, 9..16 = B7..B0, 17 = B8) -> (M, b, rowvec) of the D = 8,
    skip-4 SDF net with effective weights Ws[l] [out, in] and biases bs[l] (b None: a transposed op)"""
    W = [w.double() for w in Ws]
    b = [v.double() for v in bs]
    ops = {}
    for l in range(8):
        ops[l] = (W[l] * ISQ2 if l == 4 else W[l], b[l], W[8][0] if l == 7 else None)
    ops[8] = (W[8][1:], b[8][1:], None)
    for l in range(7, -1, -1):
        ops[16 - l] = ((W[l] * ISQ2 if l == 4 else W[l]).t(), None, None)
    ops[17] = (torch.cat([W[8][1:], W[8][:1]], 0).t(), None, W[8][0])
    return ops


def radiance_ops(Ws, ns):
    """training-pack op index (0 = head^T, 1..3 = W3^T..W1^T, 4 = W0^T) -> (M, None, None) of the D = 4
    radiance net; W0's columns are [small inputs (ns) | feature (256)], op 4's outputs [d feature ; d small]"""
    W = [w.double() for w in Ws]
    ops = {0: (W[4].t(), None, None)}
    for i in (1, 2, 3):
        ops[i] = (W[4 - i].t(), None, None)
    ops[4] = (torch.cat([W[0][:, ns:], W[0][:, :ns]], 1).t(), None, None)
    return ops
