"""CPU-side checks of the C-ABI boundary: the library loads (no GPU needed) and exports every
function include/neurecon_hip.h declares; struct layouts agree with the ctypes mirror."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, 'include', 'neurecon_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(nr_[a-z0-9_]+)\s*\(', src)))


@pytest.fixture(scope='module')
def lib():
    from neurecon_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def test_exports_every_declared_symbol(lib):
    names = _declared()
    assert len(names) >= 12
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_ctypes_mirror_covers_header(lib):
    from neurecon_amd import _lib
    assert sorted(_lib.EXPORTED) == _declared()


def test_version_and_error_text(lib):
    assert lib.nr_version() >= 1
    assert isinstance(lib.nr_last_error(), bytes)


def test_descriptor_validation_without_gpu(lib):
    from neurecon_amd import _lib
    bad = _lib.NrSdfDesc(8, 128, 4, 6, 256, 0)
    assert lib.nr_sdf_packed_bytes(ctypes.byref(bad)) == 0
    assert b'W=256' in lib.nr_last_error()
    good = _lib.NrSdfDesc(8, 256, 4, 6, 256, 0)
    assert lib.nr_sdf_packed_bytes(ctypes.byref(good)) > 4 * 1024 * 1024
    rad = _lib.NrRadDesc(4, 256, -1, 4, 256, 0)
    assert lib.nr_radiance_packed_bytes(ctypes.byref(rad)) > 0


def test_struct_sizes(lib):
    from neurecon_amd import _lib
    assert ctypes.sizeof(_lib.NrSdfDesc) == 28
    assert ctypes.sizeof(_lib.NrRadDesc) == 32
    assert ctypes.sizeof(_lib.NrNerfDesc) == 28


def test_cpu_tensors_are_rejected():
    import torch
    from neurecon_amd.frameworks.neus import volume_render
    import weightgen as wg
    from helpers import neus_model
    from neurecon_amd.frameworks.neus import NeuS
    with pytest.raises(RuntimeError, match='GPU'):
        volume_render(torch.zeros(1, 4, 3), torch.ones(1, 4, 3), None)


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """Every ctypes mirror struct has the size and field offsets gcc computes from the header."""
    import subprocess
    from neurecon_amd import _lib
    structs = [getattr(_lib, n) for n in dir(_lib) if n.startswith('Nr') and isinstance(getattr(_lib, n), type)
               and issubclass(getattr(_lib, n), ctypes.Structure)]
    assert len(structs) >= 7  # 3 descriptors, 3 render-argument blocks, kernel stats
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "neurecon_hip.h"', 'int main(void) {']
    for S in structs:
        lines.append(f'printf("{S.__name__} %zu\\n", sizeof({S.__name__}));')
        for f, _ in S._fields_:
            lines.append(f'printf("{S.__name__}.{f} %zu\\n", offsetof({S.__name__}, {f}));')
    lines.append('return 0; }')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for S in structs:
        assert int(got[S.__name__]) == ctypes.sizeof(S), S.__name__
        for f, _ in S._fields_:
            assert int(got[f'{S.__name__}.{f}']) == getattr(S, f).offset, (S.__name__, f)


def _wgrad_args(P=1000, m=256, n=256, npairs=1, ld=None):
    from neurecon_amd import _lib
    w = _lib.NrWgrad()
    w.P, w.npairs, w.m, w.n, w.scale = P, npairs, m, n, 1.0
    for q in range(2):  # fake non-null device pointers: argument checks run before any HIP call
        w.a[q], w.b[q] = 0x1000, 0x2000
        w.lda[q], w.ldb[q] = ld or m, ld or n
    w.c, w.ldc = 0x3000, n
    w.workspace = 0x4000
    w.workspace_bytes = 1 << 40
    return w


@pytest.mark.parametrize('case, code, text', [
    ('npairs', -1, 'npairs'),
    ('lda', -1, 'leading dimension'),
    ('null_out', -1, 'null output'),
    ('vec_without_avec', -1, 'avec'),
    ('operand_2gib', -1, '2 GiB'),
    ('workspace', -4, 'workspace'),
])
def test_wgrad_rejects_bad_arguments(lib, case, code, text):
    """nr_wgrad's argument checks (include/neurecon_hip.h NrWgrad) fail loudly before touching the GPU"""
    w = _wgrad_args()
    if case == 'npairs':
        w.npairs = 3
    elif case == 'lda':
        w.lda[0] = 100
    elif case == 'null_out':
        w.c = 0
    elif case == 'vec_without_avec':
        w.vec = 0x5000
    elif case == 'operand_2gib':
        w = _wgrad_args(P=1 << 22, m=256, n=256)  # 4 M rows x 256 x 4 B = 4 GiB
    elif case == 'workspace':
        w.workspace_bytes = 16
    rc = lib.nr_wgrad(ctypes.byref(w), None)
    assert rc == code, (rc, lib.nr_last_error())
    assert text in lib.nr_last_error().decode()


def test_wgrad_workspace_sizes(lib):
    """partials [S][n tiles x 128][m tiles x 256] + column-sum / vector partials, S ~ 256 / tiles"""
    one = lib.nr_wgrad_workspace_bytes(65536, 256, 256, 1)
    assert one >= 256 * 256 * 4 * 8
    assert lib.nr_wgrad_workspace_bytes(65536, 3, 256, 1) <= one
    assert lib.nr_wgrad_workspace_bytes(33, 17, 5, 1) > 0


def test_r05_training_entries_reject_bad_arguments(lib):
    """nr_weight_norm_*, nr_nerf_train_* and nr_radiance_train_fwd32 check their arguments before any HIP
    call (fake device pointers: nothing is dereferenced on the error paths)"""
    from neurecon_amd import _lib
    P = ctypes.c_void_p
    # weight norm: layer count, shapes, outputs
    assert lib.nr_weight_norm_fwd(None, 0, None) == -1 and 'NR_WN_MAX' in lib.nr_last_error().decode()
    arr = (_lib.NrWnLayer * 17)()
    assert lib.nr_weight_norm_fwd(arr, 17, None) == -1
    one = (_lib.NrWnLayer * 1)()
    one[0].v, one[0].g, one[0].norm, one[0].w, one[0].rows, one[0].cols = 0x1000, 0x2000, 0x3000, 0x4000, 0, 8
    assert lib.nr_weight_norm_fwd(one, 1, None) == -1 and 'bad layer' in lib.nr_last_error().decode()
    one[0].rows = 4
    assert lib.nr_weight_norm_bwd(one, 1, None) == -1 and 'null output' in lib.nr_last_error().decode()
    # NeRF++ training: the forward needs the fp32 pack and an aligned embedding; the backward every pointer
    nd = _lib.NrNerfDesc(8, 256, 4, 4, 10, 4, _lib.PREC_F16X3)
    assert lib.nr_nerf_train_packed_bytes(ctypes.byref(nd)) > 8 * 8 * 33 * 1024  # 8 ops of 8 x 33 KB chunks + views^T
    h8 = (P * 8)(*([0x10000] * 8))
    rc = lib.nr_nerf_train_fwd32(ctypes.byref(nd), 0x1000, 0x2000, 0x3000, 64, h8, 0x4000, 0x5000, 0x6000, 0x7000, None)
    assert rc == -1 and 'NR_PREC_FP32' in lib.nr_last_error().decode()
    nd.precision = _lib.PREC_FP32
    rc = lib.nr_nerf_train_fwd32(ctypes.byref(nd), 0x1000, 0x2004, 0x3000, 64, h8, 0x4000, 0x5000, 0x6000, 0x7000, None)
    assert rc == -1 and '16-byte' in lib.nr_last_error().decode()
    gz = (P * 8)(*([0x20000] * 7 + [0]))
    rc = lib.nr_nerf_train_bwd32(ctypes.byref(nd), 0x1000, 0x2000, 0x3000, h8, None, None, 64, 0x4000, 0x5000, 0x6000,
                                 gz, None)
    assert rc == -1 and 'null layer pointer' in lib.nr_last_error().decode()
    # the radiance training forward: the small-input stride covers the small inputs
    rd = _lib.NrRadDesc(4, 256, -1, 4, 256, _lib.PREC_FP32)
    rc = lib.nr_radiance_train_fwd32(ctypes.byref(rd), 0x1000, 0x2000, 0x3000, 8, 64, 0x4000, 0x5000, 0x6000, 0x7000,
                                     0x8000, None)
    assert rc == -1 and 'ld_small' in lib.nr_last_error().decode()


def test_train_gemm_rejects_bad_arguments(lib):
    """nr_train_gemm checks its arguments before any HIP call (fake device pointers: nothing is
    dereferenced on the error paths), among them the 32-bit offsets of its inputs: B0 (16 input blocks of
    a 256-wide tensor, 4 output blocks of a 64-wide one) on 5 M points would wrap the byte offset of x1"""
    from neurecon_amd import _lib

    def args(**kw):
        t = _lib.NrTrainGemm()
        t.op, t.P, t.x1, t.ld1, t.n1, t.y, t.ldy = 0x1000, 1024, 0x10000, 256, 256, 0x20000, 256
        t.mode, t.yscale = _lib.TG_NONE, 1.0
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def call(t, shape=(16, 0, 16, 0)):
        return lib.nr_train_gemm(None if t is None else ctypes.byref(t), *shape, None), lib.nr_last_error().decode()
    rc, msg = call(None)
    assert rc == -1 and 'null argument' in msg
    rc, msg = call(args(y=None))
    assert rc == -1 and 'no output' in msg
    rc, msg = call(args(mode=_lib.TG_SOFTPLUS), (18, 4, 16, 0))             # F4 without its second segment
    assert rc == -1 and 'missing input segment' in msg
    rc, msg = call(args(), (16, 0, 12, 0))
    assert rc == -2 and 'unsupported' in msg
    rc, msg = call(args(mode=_lib.TG_SPADJ, a=0x30000, lda=256), (4, 0, 16, 0))   # a shape of another mode
    assert rc == -2 and 'unsupported' in msg
    rc, msg = call(args(P=1000, blocked=_lib.BLK_X1))
    assert rc == -1 and 'multiples of 16' in msg
    rc, msg = call(args(blocked=_lib.BLK_Y, ldy=250))
    assert rc == -1 and 'multiples of 16' in msg
    # 32-bit byte offsets: P ld 4 of every tensor, the inputs included
    rc, msg = call(args(P=5_000_000, ld1=256, ldy=64), (16, 0, 4, 0))
    assert rc == -1 and '2 GB' in msg
    rc, msg = call(args(P=5_000_000, ld1=256, ldy=64, blocked=_lib.BLK_X1), (16, 0, 4, 0))  # the blocked extent
    assert rc == -1 and '2 GB' in msg
    rc, msg = call(args(P=5_000_000, mode=_lib.TG_SOFTPLUS, ld1=64, n1=39, x2=0x40000, ld2=256, n2=39, ldy=64),
                   (18, 4, 16, 0))                                                             # ... of x2
    assert rc == -1 and '2 GB' in msg
    rc, msg = call(args(P=5_000_000, ld1=64, ldy=256), (16, 0, 4, 0))                        # as before: an output
    assert rc == -1 and '2 GB' in msg
    assert call(args(P=0))[0] == 0                                                             # empty: no launch


def test_r06_entries_reject_bad_arguments(lib):
    """nr_gemm32 checks its sizes and leading dimensions before any HIP call (fake device pointers);
    the library no longer exports the removed nr_sdf5_enable switch"""
    A, B, C = 0x1000, 0x2000, 0x3000
    assert lib.nr_gemm32(None, 8, B, 8, 0, None, C, 8, 16, 8, 8, 0, None) == -1
    assert 'null argument' in lib.nr_last_error().decode()
    assert lib.nr_gemm32(A, 4, B, 8, 0, None, C, 8, 16, 8, 8, 0, None) == -1      # lda < K
    assert 'leading dimension' in lib.nr_last_error().decode()
    assert lib.nr_gemm32(A, 8, B, 4, 1, None, C, 8, 16, 8, 8, 0, None) == -1      # transposed B: ldb < K
    assert lib.nr_gemm32(A, 8, B, 8, 0, None, C, 4, 16, 8, 8, 0, None) == -1      # ldc < N
    assert lib.nr_gemm32(A, 0, B, 8, 0, None, C, 8, 16, 8, 0, 0, None) == -1      # K = 0
    assert 'K must be positive' in lib.nr_last_error().decode()
    assert lib.nr_gemm32(A, 8, B, 8, 0, None, C, 8, 128 * 65536, 8, 8, 0, None) == -1
    assert 'row tiles' in lib.nr_last_error().decode()
    assert lib.nr_gemm32(A, 8, B, 8, 0, None, C, 8, 0, 8, 8, 0, None) == 0        # empty: no launch
    assert not hasattr(lib, 'nr_sdf5_enable')


def test_adam_step_rejects_bad_arguments(lib):
    """nr_adam_step checks its table and hyper-parameters before any HIP call"""
    from neurecon_amd import _lib
    assert lib.nr_adam_step(None, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert 'NR_ADAM_MAX' in lib.nr_last_error().decode()
    arr = (_lib.NrAdamTensor * 1)()
    arr[0].param, arr[0].grad, arr[0].exp_avg, arr[0].exp_avg_sq, arr[0].n = 0x1000, 0x2000, 0x3000, 0x4000, 0
    assert lib.nr_adam_step(arr, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert 'bad tensor' in lib.nr_last_error().decode()
    arr[0].n = 10
    assert lib.nr_adam_step(arr, 1, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == -1      # step counts from 1
    assert lib.nr_adam_step(arr, 1, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, None) == -1      # beta1 < 1
    assert 'hyper-parameter' in lib.nr_last_error().decode()
    assert lib.nr_adam_step(arr, _lib.ADAM_MAX + 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == -1


def test_adam_optimizer_rejects_cpu_parameters():
    """neurecon_amd.optim.Adam has no CPU path: a CPU parameter raises instead of falling back"""
    import torch
    from neurecon_amd.optim import Adam
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match='GPU'):
        Adam([p]).step()


def test_train_elementwise_entries_reject_bad_arguments(lib):
    """the element-wise training kernels (nr_train.hip) check their arguments before any HIP call: NULL
    pointers, negative sizes, nfreq > 10, strides below the row (ldo / ld0 / ld1 < nf, ldh < n, col0 +
    ncols > lda), a bad mode; fake device pointers, only argument sets that return before a launch"""
    X, V, O, A, B, S, G, Z, H = (0x1000 * k for k in range(1, 10))
    bad = lambda rc: rc == -1 and 'bad argument' in lib.nr_last_error().decode()
    # nr_embed / nr_embed_padded / nr_embed_jvp / nr_embed_jvp_padded
    assert bad(lib.nr_embed(None, 4, 6, O, None)) and bad(lib.nr_embed(X, 4, 6, None, None))
    assert bad(lib.nr_embed(X, -1, 6, O, None)) and bad(lib.nr_embed(X, 4, 11, O, None))
    assert bad(lib.nr_embed_padded(X, 4, 6, O, 38, None)) and bad(lib.nr_embed_padded(X, 4, -1, O, 2, None))
    assert bad(lib.nr_embed_padded(X, 4, 0, O, 2, None)) and bad(lib.nr_embed_padded(None, 4, 6, O, 64, None))
    assert bad(lib.nr_embed_jvp(None, V, 4, 6, O, None)) and bad(lib.nr_embed_jvp(X, None, 4, 6, O, None))
    assert bad(lib.nr_embed_jvp(X, V, 4, 6, None, None)) and bad(lib.nr_embed_jvp(X, V, -1, 6, O, None))
    assert bad(lib.nr_embed_jvp(X, V, 4, 11, O, None)) and bad(lib.nr_embed_jvp_padded(X, V, 4, 10, O, 62, None))
    # nr_embed_vjp, with the stride checks: ld0 >= nf, and ld1 >= nf when e1 is given
    vjp = lambda x=X, e0=A, ld0=39, e1=B, ld1=39, P=4, nfreq=6, out=O: \
        lib.nr_embed_vjp(x, e0, ld0, e1, ld1, 1.0, P, nfreq, out, None)
    assert bad(vjp(x=None)) and bad(vjp(e0=None)) and bad(vjp(out=None)) and bad(vjp(P=-1)) and bad(vjp(nfreq=11))
    for kw in (dict(ld0=38), dict(ld1=38), dict(ld0=3), dict(nfreq=-1, ld0=2), dict(nfreq=10, ld0=64, ld1=62)):
        assert vjp(**kw) == -1 and 'ld0 / ld1' in lib.nr_last_error().decode(), kw
    assert vjp(P=0) == 0 and vjp(P=0, e1=None, ld1=0) == 0        # e1 NULL: ld1 is not read
    assert vjp(P=0, ld0=38) == -1                                 # checked before the empty return
    # nr_softplus100 / nr_sine30 / nr_mul
    for f in (lib.nr_softplus100, lib.nr_sine30):
        assert bad(f(None, 8, H, S, None)) and bad(f(Z, 8, None, S, None)) and bad(f(Z, 8, H, None, None))
        assert bad(f(Z, -1, H, S, None)) and f(Z, 0, H, S, None) == 0
    assert bad(lib.nr_mul(None, B, 8, O, None)) and bad(lib.nr_mul(A, None, 8, O, None))
    assert bad(lib.nr_mul(A, B, 8, None, None)) and bad(lib.nr_mul(A, B, -1, O, None))
    assert lib.nr_mul(A, B, 0, O, None) == 0
    # nr_scale_cols: the column range lies inside the row
    sc = lambda a=A, P=4, lda=10, col0=2, ncols=6, out=O: lib.nr_scale_cols(a, P, lda, col0, ncols, None, 1.0, out, None)
    assert bad(sc(a=None)) and bad(sc(out=None)) and bad(sc(P=-1)) and bad(sc(col0=-1)) and bad(sc(ncols=-1))
    assert bad(sc(col0=5)) and bad(sc(lda=7))
    assert sc(P=0) == 0 and sc(ncols=0) == 0
    # the two adjoints: ldh >= n; g and zdot come together
    sp = lambda hbar=H, ldh=8, s=S, g=G, zdot=Z, P=4, n=8, out=O: lib.nr_softplus_adjoint(hbar, ldh, s, g, zdot, P, n, out, None)
    assert bad(sp(hbar=None)) and bad(sp(s=None)) and bad(sp(out=None)) and bad(sp(P=-1)) and bad(sp(n=-1))
    assert bad(sp(ldh=7)) and bad(sp(g=None)) and bad(sp(zdot=None))
    assert sp(P=0) == 0 and sp(n=0, ldh=0) == 0 and sp(P=0, g=None, zdot=None) == 0
    si = lambda hbar=H, ldh=8, s=S, h=A, g=G, zdot=Z, P=4, n=8, out=O: lib.nr_sine_adjoint(hbar, ldh, s, h, g, zdot, P, n, out, None)
    assert bad(si(hbar=None)) and bad(si(s=None)) and bad(si(h=None)) and bad(si(out=None)) and bad(si(P=-1))
    assert bad(si(n=-1)) and bad(si(ldh=7)) and bad(si(zdot=None))
    assert si(P=0) == 0 and si(P=0, g=None, zdot=None) == 0
    # nr_activation: mode 0..3, g for the two backward modes
    assert bad(lib.nr_activation(None, G, 8, 0, None)) and bad(lib.nr_activation(A, G, -1, 0, None))
    assert bad(lib.nr_activation(A, G, 8, 4, None)) and bad(lib.nr_activation(A, G, 8, -1, None))
    assert bad(lib.nr_activation(A, None, 8, 1, None)) and bad(lib.nr_activation(A, None, 8, 3, None))
    assert all(lib.nr_activation(A, G, 0, m, None) == 0 for m in range(4)) and lib.nr_activation(A, None, 0, 2, None) == 0
    # nr_colsum launches even with P = 0: rejecting calls only
    assert lib.nr_colsum_workspace_bytes(65) == 1024 * 65 * 4
    cs = lambda a=A, P=8, n=65, out=O, ws=B, nb=1024 * 65 * 4: lib.nr_colsum(a, P, n, out, ws, nb, None)
    assert bad(cs(a=None)) and bad(cs(out=None)) and bad(cs(P=-1)) and bad(cs(n=0)) and bad(cs(n=-1))
    assert cs(ws=None) == -4 and 'workspace' in lib.nr_last_error().decode()
    assert cs(nb=1024 * 65 * 4 - 1) == -4 and cs(n=66) == -4
    # nr_radiance_input: v and normals with view directions, the feature unless wfeat = 0
    ri = lambda x=X, v=V, nrm=A, feat=B, P=4, nfv=4, uv=1, wf=256, out=O: \
        lib.nr_radiance_input(x, v, nrm, feat, P, nfv, uv, wf, out, None)
    assert bad(ri(x=None)) and bad(ri(out=None)) and bad(ri(v=None)) and bad(ri(nrm=None)) and bad(ri(feat=None))
    assert bad(ri(P=-1)) and bad(ri(nfv=11)) and bad(ri(wf=-1))
    assert ri(P=0) == 0 and ri(P=0, uv=0, v=None, nrm=None) == 0 and ri(P=0, wf=0, feat=None) == 0
