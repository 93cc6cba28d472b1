"""The training layer GEMM (nr_train_gemm, tgemm_kernel in csrc/nr_mlp.hip) call by call: every layer
product of the f16x3 training step, with its hand-issued loads and stores, counted waits, next-tile
prefetch, cold scalar load path, ragged last tile, two-segment inputs and outputs, NULL outputs, three
g conventions and two tensor layouts.

The cases are the kernel's own calls: training._tg is recorded during one forward + backward of
sdf_nablas and of the radiance net with and without view dirs (f16x3 nets, P = (2 CU + 1) 128 + 48
points), so the operands are the step's real tensors; the set of (KB, KB2, NBO, NB2, mode) recorded
must equal NR_TG_SHAPES.  Every call is then re-issued on its recorded operands (rows are independent,
so any row range is a valid case) at P_multi = (2 CU + 1) 128 + 37 -- two workgroups run three tiles, the
others two, the prefetch and the weight-stream wrap execute, the last tile has 37 rows -- and at
P = 1, 37, 128, 130; outputs always sit between 256 sentinel rows in buffers 16 columns wider than their
blocks, and every launch checks the sentinels.

  1. against float64 (tests/tgemm_ref.py, pinned to autograd by tests/test_tgemm_ref.py), per element:
     |hip - f64| <= |fp32 - f64| + 2e-6 scale (tests/test_gpu_wgrad.py's bar), fp32 = the same formula
     in fp32 torch, scale = the launch's max |z64| times the epilogue's largest slope (1 for y, the ReLU
     mask and SPADJ's hbar s; |yscale| max|a| for MUL's y2; 25 for softplus', times max|rowvec| for y3;
     for SPADJ the larger of max |z64| and max |g zdot s'|, the second term being elementwise fp32
     arithmetic whose rounding follows its own size; max |dot64| for dot).  Valid columns only.
  2. tile-position invariance, bit for bit: the P_multi launch equals the same rows issued in launches of
     at most 128 CU rows (one tile per workgroup, cold path only).
  3. blocked layout against row-major, bit for bit, with the blocked mask the step passes.
  4. NaN in the dead input columns [n, 16 blocks) and in the row padding changes no output bit.
  5. x1 as an unaligned strided view (prefetch off, scalar path) equals the contiguous copy bit for bit.
  6. nothing outside the outputs is written (the sentinels, at P_multi and P = 1).
  7. NULL outputs: the step's form and every single-output form equal the all-outputs form.
  8. the same launch twice is bit-identical.

Measured worst (|hip - f64| - |fp32 - f64|) / scale per mode on MI355X, over all calls and sizes:
SOFTPLUS 3.9e-7, NONE 4.2e-7, MUL 4.7e-7, SPADJ 2.8e-7, RELUMASK 3.5e-7: no mode needs more
than the 2e-6."""
import inspect
import os
import re

import pytest
import torch

import weightgen as wg
from helpers import neus_model
from tgemm_ref import TG_MUL, TG_NONE, TG_RELUMASK, TG_SOFTPLUS, TG_SPADJ, radiance_ops, sdf_ops, tgemm_ref

pytestmark = pytest.mark.gpu

C_BAR = 2e-6
P_SMALL = (1, 37, 128, 130)
MODE_NAME = {TG_NONE: 'NONE', TG_SOFTPLUS: 'SOFTPLUS', TG_MUL: 'MUL', TG_SPADJ: 'SPADJ', TG_RELUMASK: 'RELUMASK'}
BITS = dict(x1=1, x2=2, y=4, yb=8, y2=16, y3=32, a=64, g=128, zd=256)            # NR_BLK_*
IN_LD = dict(x1='ld1', x2='ld2', a='lda', g='ldg', zd='ldzd')
OUT_LD = dict(y='ldy', yb='ldyb', y2='ldy2', y3='ldy3')
SENTINEL = 0x7FC0DEAD  # a NaN payload no computation produces

# the calls of the three recorded runs, in issue order (SdfNablaTG.forward / .backward, RadianceTG.backward),
# with the op index of nr_sdf_op_info / the radiance training pack
SDF_CALLS = ([(f'F{l}', l) for l in range(8)] + [('F8', 8)] + [(f'nabla.B{l}', 16 - l) for l in range(7, 0, -1)] +
             [('B0', 16)] + [(f'tangent.F{l}', l) for l in range(8)] + [('B8', 17)] +
             [(f'adjoint.B{l}', 16 - l) for l in range(7, 0, -1)])
RAD_CALLS = [('headT', 0), ('W3T', 1), ('W2T', 2), ('W1T', 3), ('W0T', 4)]
NAMES = ['sdf.' + n for n, _ in SDF_CALLS] + [f'{p}.{n}' for p in ('rad_view', 'rad_noview') for n, _ in RAD_CALLS]
TWO_SEGMENT = ('sdf.F4', 'sdf.tangent.F4', 'sdf.B8')  # KB2 > 0: no next-tile prefetch to switch off (check 5)


def to_blocked(t):
    """row-major [P, C] -> the same shape with its memory in the 16 x 16 blocked order (NR_BLK_*:
    element (p, c) at ((p / 16) (C / 16) + c / 16) 256 + (p % 16) 16 + c % 16)"""
    P, C = t.shape
    return t.reshape(P // 16, 16, C // 16, 16).permute(0, 2, 1, 3).contiguous().reshape(P, C)


def from_blocked(t):
    P, C = t.shape
    return t.reshape(P // 16, C // 16, 16, 16).permute(0, 2, 1, 3).contiguous().reshape(P, C)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Case:
    pass


class Harness:
    def __init__(self):
        from neurecon_amd import _lib as L
        from neurecon_amd import training as T
        self.L, self.T = L, T
        self.tg = T._tg
        self.sig = inspect.signature(T._tg)
        self.CU = torch.cuda.get_device_properties(0).multi_processor_count
        self.P_blk = (2 * self.CU + 1) * 128 + 48
        self.P_multi = (2 * self.CU + 1) * 128 + 37
        self.cases = {}
        self.keep = []
        self.worst = {}
        self._record()

    # ---- recording -------------------------------------------------------------------------
    def _run_recorded(self, fn):
        calls = []

        def recorder(*args, **kw):
            ba = self.sig.bind(*args, **kw)
            ba.apply_defaults()
            calls.append(dict(ba.arguments))
            return self.tg(*args, **kw)
        mp = pytest.MonkeyPatch()
        mp.setattr(self.T, '_tg', recorder)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            mp.undo()
        return calls

    def _record(self):
        T, P = self.T, self.P_blk
        gen = torch.Generator().manual_seed(17)
        r = lambda *s: torch.randn(*s, generator=gen).cuda()
        m = neus_model(wg.neus_state(seed=11), precision='f16x3')
        m.train()
        surf = m.implicit_surface
        assert T.uses_train_gemm(surf) and T.uses_train_gemm(m.radiance_net)
        x = r(P, 3) * 0.7
        gs, gn, gf = r(P), r(P, 3), r(P, 256) * 0.01
        out = {}

        def sdf_step():
            Ws = T.effective_weights(surf)
            s, n, f = T.sdf_nablas(surf, x, True, Ws)
            ((s * gs).sum() + (n * gn).sum() + (f * gf).sum()).backward()
            out.update(Ws=[w.detach() for w in Ws], nab=n.detach(), feat=f.detach())
        calls = self._run_recorded(sdf_step)
        assert len(calls) == len(SDF_CALLS), len(calls)
        desc, packed = surf.nr_packed(x.device)
        info = T._op_info('sdf', desc, 18)
        ops = sdf_ops([w.double() for w in out['Ws']], [l.bias.detach().double() for l in surf.surface_fc_layers])
        for (name, i), a in zip(SDF_CALLS, calls):
            base = surf._nr_train_cache[1].data_ptr() if i == 17 else packed.data_ptr()
            assert a['op'] == base + info[i][0], name
            self._add('sdf.' + name, a, ops[i], calls, ny=217 if i == 12 else None)  # B4: [g_3 ; e_skip]
        self.keep += [m, packed]
        v = torch.nn.functional.normalize(r(P, 3), dim=-1)
        gy = r(P, 3)
        for prefix, view in (('rad_view', True), ('rad_noview', False)):
            mm = m if view else neus_model(wg.neus_state(seed=11, use_view_dirs=False), precision='f16x3',
                                           use_view_dirs=False)
            mm.train()
            net = mm.radiance_net
            assert T.uses_train_gemm(net)
            nrm = out['nab'].clone().requires_grad_(True) if view else None
            feat = out['feat'].clone().requires_grad_(True)
            calls = self._run_recorded(lambda: (T.radiance(net, x, v, nrm, feat) * gy).sum().backward())
            assert len(calls) == len(RAD_CALLS), len(calls)
            info = T._op_info('rad', net.nr_desc(), 10)
            Ws = [w.detach() for w in T.weight_norm_all(net.layers)]
            ns = Ws[0].shape[1] - 256
            ops = radiance_ops(Ws, ns)
            for (name, i), a in zip(RAD_CALLS, calls):
                assert a['op'] == net._nr_train_cache[1].data_ptr() + info[5 + i][0], name
                self._add(f'{prefix}.{name}', a, ops[i], calls, ny=256 if i == 4 else None)  # [d feature ; d small]
            self.keep.append(mm)

    def _add(self, name, a, op, calls, ny=None):
        c = Case()
        c.name, c.args = name, a
        KB, KB2, NBO, NB2 = a['shape']
        c.key = (KB, KB2, NBO, NB2, a['mode'])
        c.M, c.b, c.rv = (None if t is None else t.cuda() for t in op)
        c.wy, c.wyb = 16 * (NBO - NB2), 16 * NB2
        assert (ny is not None) == (NB2 > 0), name
        c.ny = c.M.shape[0] if ny is None else ny
        c.nyb = c.M.shape[0] - c.ny
        assert c.ny <= c.wy and c.nyb <= c.wyb and c.M.shape[1] == a['n1'] + a['n2'], name
        assert a['P'] == self.P_blk and a['head'] is None, name
        # inputs as row-major [P, ld] tensors (a raw address is a tensor an earlier call wrote)
        by_ptr = {t.data_ptr(): t for q in calls for t in q.values() if isinstance(t, torch.Tensor)}
        c.inp = {}
        for role, ldk in IN_LD.items():
            t = a[role]
            if t is None:
                continue
            if isinstance(t, int):
                t = by_ptr[t]
            t = t.detach().reshape(self.P_blk, -1)
            assert t.shape[1] == a[ldk], (name, role)
            c.inp[role] = from_blocked(t) if a['blocked'] & BITS[role] else t.contiguous()
        for role, ldk in OUT_LD.items():
            assert a[role] is None or a[ldk] == (c.wyb if role == 'yb' else c.wy), (name, role)
        c.step_outs = tuple(k for k in ('y', 'yb', 'y2', 'y3', 'dot') if a[k] is not None)
        mode = a['mode']
        c.all_outs = ('y',) + ('yb',) * (NB2 > 0 and mode in (TG_NONE, TG_MUL)) + \
            ('y2',) * (mode in (TG_SOFTPLUS, TG_MUL)) + ('y3', 'dot') * (mode == TG_SOFTPLUS and c.rv is not None)
        assert set(c.step_outs) <= set(c.all_outs), name
        self.cases[name] = c

    # ---- one launch ------------------------------------------------------------------------
    def launch(self, c, P, row0=0, blocked=0, outs=None, fill=None, strided=False):
        """c's call on rows [row0, row0 + P) of its operands -> {role: [P, width] row-major copy}.
        blocked: NR_BLK_* mask; outs: the outputs passed (the rest NULL); fill: value written to the dead
        columns of x1 / x2, widened to whole blocks; strided: x1 as wide[:, 1:].  Every output lies
        between 256 sentinel rows, 16 columns wider than its blocks: the sentinels are checked here."""
        a = c.args
        outs = c.all_outs if outs is None else outs
        dev = c.M.device
        kw = dict(bias=a['bias'], yscale=a['yscale'], g_row=a['g_row'], g_scaled=a['g_scaled'], dot_bias=a['dot_bias'],
                  n2=a['n2'], stream=self.L.stream_of(dev), blocked=blocked)
        for role, ldk in IN_LD.items():
            t = c.inp.get(role)
            if t is None:
                continue
            t = t[row0:row0 + P]
            if fill is not None and role in ('x1', 'x2'):
                n = a['n1'] if role == 'x1' else a['n2']
                nblk = a['shape'][1] if role == 'x2' else a['shape'][0] - a['shape'][1]
                w = torch.full((P, max(t.shape[1], 16 * nblk)), fill, device=dev)
                w[:, :n] = t[:, :n]
                t = w
            if strided and role == 'x1':
                wide = torch.full((P, t.shape[1] + 1), float('nan'), device=dev)
                wide[:, 1:] = t
                t = wide[:, 1:]
                assert not t.is_contiguous() or P == 1
            elif blocked & BITS[role]:
                t = to_blocked(t)
            else:
                t = t.contiguous()
            kw[role], kw[ldk] = t, t.stride(0)
        x1, ld1 = kw.pop('x1'), kw.pop('ld1')
        bufs = {}
        for role in outs:
            if role == 'dot':
                buf = torch.full((512 + P,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
                kw['dot'] = buf[256:]
            else:
                w = c.wyb if role == 'yb' else c.wy
                buf = torch.full((512 + P, w + 16), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
                kw[role], kw[OUT_LD[role]] = buf[256:], w + 16
            bufs[role] = buf
        y, ldy = kw.pop('y', None), kw.pop('ldy', 0)
        self.tg(a['op'], P, a['shape'], a['mode'], x1, ld1, a['n1'], y, ldy, **kw)
        res = {}
        intact = lambda t: bool((t.contiguous().view(torch.int32) == SENTINEL).all())
        for role, buf in bufs.items():
            body = buf[256:256 + P]
            assert intact(buf[:256]) and intact(buf[256 + P:]), (c.name, role, P, 'guard rows overwritten')
            if role == 'dot':
                res[role] = body.clone()
                continue
            if blocked & BITS[role]:
                body = from_blocked(body)
            w = body.shape[1] - 16
            assert intact(body[:, w:]), (c.name, role, P, 'row padding overwritten')
            res[role] = body[:, :w].clone()
        return res

    def refs(self, c, dtype):
        a = c.args
        return tgemm_ref(c.M, c.b, a['mode'], c.inp['x1'], a['n1'], x2=c.inp.get('x2'), n2=a['n2'], ny=c.ny,
                         bias=a['bias'], yscale=a['yscale'], a=c.inp.get('a'), g=c.inp.get('g'), zd=c.inp.get('zd'),
                         g_row=a['g_row'], g_scaled=a['g_scaled'], rowvec=c.rv, dot_bias=a['dot_bias'], dtype=dtype)


@pytest.fixture(scope='module')
def h():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return Harness()


def _same(c, got, ref, what, roles=None):
    for role in (ref if roles is None else roles):
        assert bits_equal(got[role], ref[role]), \
            (c.name, what, role, float((got[role] - ref[role]).abs().nan_to_num(float('inf')).max()))


def test_every_kernel_instance_is_recorded(h):
    """the recorded (KB, KB2, NBO, NB2, mode) set is NR_TG_SHAPES: an instance no call of the three runs
    reaches (or a new one) fails here -- find the call that uses it, or delete the instance"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neurecon_amd', 'csrc',
                            'nr_mlp.hip')).read()
    body = src[src.index('#define NR_TG_SHAPES(X)'):src.index('int launch_tgemm')]
    modes = dict(TG_NONE=TG_NONE, TG_SOFTPLUS=TG_SOFTPLUS, TG_MUL=TG_MUL, TG_SPADJ=TG_SPADJ, TG_RELUMASK=TG_RELUMASK)
    shapes = [(int(m[0]), int(m[1]), int(m[2]), int(m[3]), modes[m[4]])
              for m in re.findall(r'X\((\d+), (\d+), (\d+), (\d+), (TG_\w+)\)', body)]
    assert len(shapes) == 20 and len(set(shapes)) == 20
    assert list(h.cases) == NAMES
    assert {c.key for c in h.cases.values()} == set(shapes)
    assert {n for n, c in h.cases.items() if c.key[1] > 0} == set(TWO_SEGMENT)


@pytest.mark.parametrize('name', NAMES)
def test_vs_float64(h, name):
    """check 1 at P_multi and P = 1, 37, 128, 130 (all outputs the mode defines, valid columns)"""
    c = h.cases[name]
    a = c.args
    r64, r32 = h.refs(c, torch.float64), h.refs(c, torch.float32)
    zmax = float(r64['z'].abs().max())
    amax = float(c.inp['a'][:, :c.ny].abs().max()) if 'a' in c.inp else 0.0
    rvmax = float(c.rv.abs().max()) if c.rv is not None else 0.0
    scale = dict(y=zmax * abs(a['yscale']), yb=zmax * abs(a['yscale']))
    if a['mode'] == TG_MUL:
        scale['y2'] = zmax * abs(a['yscale']) * amax
    elif a['mode'] == TG_SOFTPLUS:
        scale.update(y=zmax, y2=25 * zmax, y3=25 * zmax * rvmax)
        if r64['dot'] is not None:
            scale['dot'] = float(r64['dot'].abs().max())
    elif a['mode'] == TG_SPADJ:
        gterm = r64['y'] - r64['z'][:, :c.ny] * a['yscale'] * c.inp['a'][:, :c.ny].double()
        scale['y'] = max(zmax * abs(a['yscale']), float(gterm.abs().max()))
    elif a['mode'] == TG_RELUMASK:
        scale['y'] = zmax
    nvalid = dict(y=c.ny, y2=c.ny, y3=c.ny, yb=c.nyb)
    worst = -1.0
    for P in (h.P_multi,) + P_SMALL:
        out = h.launch(c, P)
        for role in c.all_outs:
            got = out[role].double()
            if role == 'dot':
                e_hip, e_32 = (got - r64[role][:P]).abs(), (r32[role][:P].double() - r64[role][:P]).abs()
            else:
                n = nvalid[role]
                ref = r64[role][:P, :n]
                e_hip, e_32 = (got[:, :n] - ref).abs(), (r32[role][:P, :n].double() - ref).abs()
            ratio = float(((e_hip - e_32) / scale[role]).max())
            worst = max(worst, ratio)
            print(f'{name} [{MODE_NAME[a["mode"]]}] P={P} {role}: max |hip - f64| {float(e_hip.max()) / scale[role]:.2e}, '
                  f'max |fp32 - f64| {float(e_32.max()) / scale[role]:.2e}, worst excess {ratio:.2e} (of {scale[role]:.3e})')
            assert bool((e_hip <= e_32 + C_BAR * scale[role]).all()), (name, P, role, ratio)
    m = MODE_NAME[a['mode']]
    h.worst[m] = max(h.worst.get(m, -1.0), worst)
    print(f'{name}: worst (|hip - f64| - |fp32 - f64|) / scale {worst:.2e}; per mode so far {h.worst}')


@pytest.mark.parametrize('name', NAMES)
def test_tile_position_invariance(h, name):
    """check 2: the P_multi launch (2-3 tiles per workgroup: prefetched inputs, the weight stream wrapping
    to the next tile, the double-buffered epilogue operands) against the same rows in launches of at most
    128 CU rows, where every workgroup runs one tile from the cold path -- bit for bit"""
    c = h.cases[name]
    full = h.launch(c, h.P_multi)
    step = 128 * h.CU
    parts = [h.launch(c, min(step, h.P_multi - r0), row0=r0) for r0 in range(0, h.P_multi, step)]
    assert len(parts) == 3
    _same(c, {k: torch.cat([p[k] for p in parts]) for k in full}, full, 'one tile per workgroup vs 2-3 tiles')


@pytest.mark.parametrize('name', NAMES)
def test_blocked_vs_row_major(h, name):
    """check 3: the blocked mask the step passes for this call, at (2 CU + 1) 128 + 48 points"""
    c = h.cases[name]
    mask = c.args['blocked']
    assert mask != 0, name  # every call of the step has a blocked tensor when P % 16 == 0
    row = h.launch(c, h.P_blk)
    blk = h.launch(c, h.P_blk, blocked=mask)
    _same(c, blk, row, f'blocked {mask:#x} vs row-major')
    if set(c.step_outs) != set(c.all_outs):  # and in the step's own output form
        _same(c, h.launch(c, h.P_blk, blocked=mask, outs=c.step_outs), row, 'blocked, step outputs', c.step_outs)


@pytest.mark.parametrize('name', NAMES)
def test_dead_input_columns(h, name):
    """check 4: columns [n, 16 blocks) of x1 / x2 and their row padding hold NaN (the 217-of-224 layer,
    the 39-of-64 embedding, the 3-of-32 colour gradient, the 1-of-32 sdf column): bit-identical to zeros
    there, on the cold path (small P, first tiles) and the prefetched one (P_multi)"""
    c = h.cases[name]
    for P in (h.P_multi,) + P_SMALL:
        zero = h.launch(c, P, fill=0.0)
        _same(c, h.launch(c, P, fill=float('nan')), zero, f'NaN in dead columns, P={P}')
        if P == h.P_multi:  # widening the inputs to whole blocks changes nothing either
            _same(c, zero, h.launch(c, P), 'whole-block inputs vs the step\'s leading dimensions')


@pytest.mark.parametrize('name', [n for n in NAMES if n not in TWO_SEGMENT])
def test_unaligned_strided_x1(h, name):
    """check 5: x1 = wide[:, 1:] (row stride ld + 1, base 4 bytes off 16: no prefetch, scalar loads)"""
    c = h.cases[name]
    assert c.key[1] == 0
    for P in (h.P_multi,) + P_SMALL:
        _same(c, h.launch(c, P, strided=True), h.launch(c, P), f'strided x1, P={P}')


@pytest.mark.parametrize('name', NAMES)
def test_nothing_outside_the_outputs_is_written(h, name):
    """check 6: launch() asserts the 256 sentinel rows before and after every output and the 16 sentinel
    columns of every row; here for the ragged P_multi (clamped lanes rewrite the last row, nothing else)
    and P = 1 in the all-outputs form, the step's form and the blocked layout"""
    c = h.cases[name]
    for P in (h.P_multi, 1):
        h.launch(c, P)
        h.launch(c, P, outs=c.step_outs)
    h.launch(c, h.P_blk, blocked=c.args['blocked'], outs=c.step_outs)


@pytest.mark.parametrize('name', NAMES)
def test_null_outputs(h, name):
    """check 7: the step's own output form (MUL with y NULL, B4 with y NULL and yb, SPADJ B4 with yb NULL,
    W0^T with y and yb, ...) and every single-output form give the values of the all-outputs launch"""
    c = h.cases[name]
    for P in (h.P_multi, 130):
        ref = h.launch(c, P)
        forms = {c.step_outs} | {(r,) for r in c.all_outs}
        for outs in sorted(forms):
            if set(outs) == set(c.all_outs):
                continue
            _same(c, h.launch(c, P, outs=outs), ref, f'outputs {outs}, P={P}', outs)
        if c.key[3] > 0 and 'yb' not in c.all_outs:
            # the adjoint B4 leaves yb NULL (its epilogue tensors cover y only, so yb's values are
            # unspecified): storing it into a guarded dummy changes nothing else
            _same(c, h.launch(c, P, outs=c.all_outs + ('yb',)), ref, f'with a dummy yb, P={P}', c.all_outs)


@pytest.mark.parametrize('name', NAMES)
def test_repeatable(h, name):
    """check 8"""
    c = h.cases[name]
    for P in (h.P_multi, 37):
        _same(c, h.launch(c, P), h.launch(c, P), f'second launch, P={P}')
