"""The colour kernels behind nr_radiance_forward, nr_neus_fold_forward and nr_nerf_forward, call by call, against
the float64 references of tests/mlp_ref.py (which tests/test_mlp_ref.py proves fit: condition A and the deliberate
errors).

launch_radiance dispatches on (precision, small-input blocks KBS, activation, depth, fold): rad4_kernel<KBS, FOLD>
for the f16x3 ReLU D = 4 nets, radiance_kernel<prec, KBS, ACT, D> for the rest; launch_nerf on the precision
(nerf_kernel<fp32>, nerf4_kernel).  The grid of mlp_ref.RAD_CONFIGS x precisions, the folded pairs and NeRF reach
every instance that can be dispatched (test_grid_reaches_every_instance): 4 + 14 + 2 = 20.  The library compiles 22:
radiance_kernel<f16x3, 2 | 4, ReLU, 4> exist as code but rad4_kernel takes their place in the dispatch, so no call
can reach them.

Bars, the ones these kernels already answer to (mlp_ref.bar, BAR_NERF): ReLU radiance rtol 1e-5 / atol 1e-6, SIREN
radiance 1e-4 / 1e-6, NeRF fp32 1e-5 / 1e-6, NeRF f16x3 1e-4 / 1e-5.  Every assertion prints worst
err / (atol + rtol |ref|) first."""
import ctypes

import pytest
import torch

import mlp_ref as R
from helpers import SURF
from sdf_ref import float64_sdf_nabla_feature, randomised_state

pytestmark = pytest.mark.gpu

GRID = [(c, p) for c in R.RAD_CONFIGS for p in R.PRECISIONS]
GRID_IDS = [f'{R.cfg_id(c)}-{p}' for c, p in GRID]
FOLD_CONFIGS = [c for c in R.RAD_CONFIGS if not c.siren and c.D == 4]  # with the f16x3 softplus SDF net
FOLD_IDS = [R.cfg_id(c) for c in FOLD_CONFIGS]
CAPS = (1, 3)  # workgroups: at 300 points one then runs three 128-point tiles, the last one ragged
PAD = 128      # rows past P in the buffers of the C ABI tests
SENTINEL = 0x7FC0BEEF  # the bits of a quiet NaN that no kernel produces


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()  # must load: no fallback exists


class _Nets:
    """models on the GPU, float64 layers and inputs, each built once"""

    def __init__(self):
        self.rad, self.layers, self.inputs, self.ref = {}, {}, {}, {}
        self.nerf, self.surface, self.fold_ref = {}, None, {}

    def radiance(self, c, precision):
        if (c, precision) not in self.rad:
            self.rad[c, precision] = R.radiance_module(c, precision).cuda()
        return self.rad[c, precision]

    def rad_layers(self, c):
        if c not in self.layers:
            self.layers[c] = R.radiance_layers(R.radiance_module(c, 'fp32'))
        return self.layers[c]

    def cls(self, name, c):
        """(CPU tensors, GPU tensors) of input class `name` for configuration c"""
        key = (name, c.mv if (name == 'view_edges' and c.view) else None, c.siren if name == 'mixed_scale' else None)
        if key not in self.inputs:
            t = {'unit': R.unit, 'zeros': R.zeros, 'mixed_scale': lambda: R.mixed_scale(R.MIXED_GAIN[c.siren]),
                 'view_edges': lambda: R.view_edges(c.mv if c.view else -1), 'nerf_unit': R.nerf_unit,
                 'nerf_edges': R.nerf_edges}[name]()
            self.inputs[key] = t, tuple(a.cuda() for a in t)
        return self.inputs[key]

    def rad_ref(self, name, c):
        if (name, c) not in self.ref:
            self.ref[name, c] = R.float64_rgb(self.rad_layers(c), c, *self.cls(name, c)[0])
        return self.ref[name, c]

    def nerf_net(self, precision):
        if precision not in self.nerf:
            self.nerf[precision] = R.nerf_module(precision).cuda()
        return self.nerf[precision]

    def nerf_ref(self, name):
        if name not in self.ref:
            self.ref[name] = R.float64_nerf(R.nerf_layers(R.nerf_module('fp32')), *self.cls(name, None)[0])
        return self.ref[name]

    def sdf(self):
        """config (b)'s f16x3 SDF net with randomised biases (sdf_ref), the folded pairs' first half"""
        if self.surface is None:
            from neurecon_amd.base import ImplicitSurface
            s = ImplicitSurface(W_geo_feat=256, radius_init=0.5, obj_bounding_size=1.0, precision='f16x3', **SURF)
            pre = 'implicit_surface.'
            s.load_state_dict({k[len(pre):]: v for k, v in randomised_state(seed=11).items() if k.startswith(pre)})
            self.surface = s.cuda().eval()
        return self.surface

    def folded_ref(self, name, c):
        """points -> float64 SDF net -> its geometry feature -> float64 radiance net"""
        if (name, c) not in self.fold_ref:
            x, v, n, _ = self.cls(name, c)[0]

            class M:
                implicit_surface = self.sdf()
            f = torch.from_numpy(float64_sdf_nabla_feature(M, x)[2])
            self.fold_ref[name, c] = R.float64_rgb(self.rad_layers(c), c, x, v, n, f)
        return self.fold_ref[name, c]


@pytest.fixture(scope='module')
def nets():
    return _Nets()


def _rows(t, P):
    return tuple(a[:P].contiguous() for a in t)


def _forward(m, x, v, n, f):
    with torch.no_grad():
        return m.forward(x, v, n, f)


def _folded(surface, m, x, v, n, vdiv=1):
    """nr_neus_fold_forward: sdf4_kernel with F8' in F8's place, then rad4_kernel<KBS, true>"""
    from neurecon_amd import _lib as L
    dev = x.device
    with torch.no_grad():
        sdesc, spk = surface.nr_packed(dev)
        rdesc, rpk = m.nr_packed(dev)
        fpk = m.nr_fold_packed(surface, dev)
    assert fpk is not None
    P = x.shape[0]
    u, sdf, rgb = torch.empty(P, 256, device=dev), torch.empty(P, device=dev), torch.empty(P, 3, device=dev)
    L.check(L.lib().nr_neus_fold_forward(ctypes.byref(sdesc), L.ptr(spk), ctypes.byref(rdesc), L.ptr(rpk), L.ptr(fpk),
                                         L.ptr(x), L.ptr(v if m.use_view_dirs else None), vdiv,
                                         L.ptr(n if m.use_view_dirs else None), P, L.ptr(u), L.ptr(sdf), L.ptr(rgb),
                                         L.stream_of(dev)))
    return rgb


def _nerf(m, x4, v):
    with torch.no_grad():
        sigma, rgb = m.forward(x4, v)
    return sigma, rgb


def _check(tag, got, ref, bar, failed):
    w = R.worst(got, ref, *bar)
    print(f'{tag}: worst err / (atol + rtol |ref|) = {w:.4f}')
    if not w <= 1.0:
        failed.append(f'{tag}: {w:.4f}')


# -- which kernel a call runs -----------------------------------------------------------------------------------
def _instance(desc, fold=False):
    """the kernel instance launch_radiance picks for this descriptor: rad_layout's rule (small-input columns: x,
    then with view dirs the view embedding and the normals; KBS = 2 up to 32 columns, else 4), then the dispatch"""
    from neurecon_amd import _lib as L
    ns = 3 if desc.no_view_dirs else 3 + (3 if desc.multires_view < 0 else 3 + 6 * desc.multires_view) + 3
    kbs = 2 if ns <= 32 else 4
    prec = 'f16x3' if desc.precision == L.PREC_F16X3 else 'fp32'
    if prec == 'f16x3' and not desc.siren and desc.D == 4:
        return f'rad4_kernel<{kbs}, {"true" if fold else "false"}>'
    assert not fold
    return f'radiance_kernel<{prec}, {kbs}, {"sine" if desc.siren else "ReLU"}, {desc.D}>'


def test_grid_reaches_every_instance(nets):
    from neurecon_amd import _lib as L
    compiled = {f'rad4_kernel<{k}, {f}>' for k in (2, 4) for f in ('false', 'true')} | \
        {f'radiance_kernel<{p}, {k}, {a}, {d}>' for p in R.PRECISIONS for k in (2, 4) for a in ('ReLU', 'sine')
         for d in (4, 5)} | {'nerf_kernel<fp32>', 'nerf4_kernel'}
    replaced = {'radiance_kernel<f16x3, 2, ReLU, 4>', 'radiance_kernel<f16x3, 4, ReLU, 4>'}  # by rad4_kernel
    assert len(compiled) == 22 and replaced < compiled
    reached = {_instance(R.radiance_module(c, p).nr_desc()) for c, p in GRID}
    reached |= {_instance(R.radiance_module(c, 'f16x3').nr_desc(), fold=True) for c in FOLD_CONFIGS}
    reached |= {'nerf4_kernel' if R.nerf_module(p).nr_desc().precision == L.PREC_F16X3 else 'nerf_kernel<fp32>'
                for p in R.PRECISIONS}
    for name in sorted(reached):
        print('reached:', name)
    missed = sorted(compiled - replaced - reached)
    assert not missed, f'instances the grid misses: {missed}'
    assert not reached & replaced and len(reached) == 20
    # the library's own layout follows the same rule: per layer 8 chunks of (2 K + 1) KiB, K = 16 input blocks plus
    # KBS in layer 0, then less than 4 KiB of scales, bounds and head; a KBS of 4 in place of 2 adds 32 KiB
    lib = L.lib()
    for c, p in GRID:
        d = R.radiance_module(c, p).nr_desc()
        kbs = 2 if R.n_small(c) <= 32 else 4
        ops = sum(8 * (2 * ((16 + kbs) if i == 0 else 16) + 1) * 1024 for i in range(c.D))
        assert 0 <= lib.nr_radiance_packed_bytes(ctypes.byref(d)) - ops < 4096, (c, p)


# -- every instance against float64 -----------------------------------------------------------------------------
@pytest.mark.parametrize('c,precision', GRID, ids=GRID_IDS)
def test_radiance_unit_vs_float64(nets, c, precision):
    """P = one lane, one column, a column + 1, one tile, a tile + 1, a ragged third tile"""
    m, ref, failed = nets.radiance(c, precision), nets.rad_ref('unit', c), []
    print(_instance(m.nr_desc()))
    for P in R.SIZES:
        _check(f'{R.cfg_id(c)} {precision} unit P={P}', _forward(m, *_rows(nets.cls('unit', c)[1], P)), ref[:P],
               R.bar(c), failed)
    assert not failed, failed


@pytest.mark.parametrize('c,precision', GRID, ids=GRID_IDS)
def test_radiance_classes_vs_float64(nets, c, precision):
    m, failed = nets.radiance(c, precision), []
    for name in ('mixed_scale', 'zeros', 'view_edges'):
        _check(f'{R.cfg_id(c)} {precision} {name}', _forward(m, *nets.cls(name, c)[1]), nets.rad_ref(name, c),
               R.bar(c), failed)
    assert not failed, failed


@pytest.mark.parametrize('c', FOLD_CONFIGS, ids=FOLD_IDS)
def test_folded_pair_vs_float64(nets, c):
    """rad4_kernel<2 | 4, true> behind the SDF net's F8'"""
    m, failed = nets.radiance(c, 'f16x3'), []
    print(_instance(m.nr_desc(), fold=True))
    for name, sizes in (('unit', R.SIZES), ('view_edges', (R.N_POINTS,))):
        ref = nets.folded_ref(name, c)
        for P in sizes:
            x, v, n, _ = _rows(nets.cls(name, c)[1], P)
            _check(f'{R.cfg_id(c)} folded {name} P={P}', _folded(nets.sdf(), m, x, v, n), ref[:P], R.bar(c), failed)
    assert not failed, failed


@pytest.mark.parametrize('precision', R.PRECISIONS)
def test_nerf_vs_float64(nets, precision):
    m, failed = nets.nerf_net(precision), []
    for name, sizes in (('nerf_unit', R.SIZES), ('nerf_edges', (R.N_POINTS,))):
        sigma64, rgb64 = nets.nerf_ref(name)
        for P in sizes:
            sigma, rgb = _nerf(m, *_rows(nets.cls(name, None)[1], P))
            _check(f'nerf {precision} {name} P={P} sigma', sigma, sigma64[:P], R.BAR_NERF[precision], failed)
            _check(f'nerf {precision} {name} P={P} rgb', rgb, rgb64[:P], R.BAR_NERF[precision], failed)
    assert not failed, failed


# -- more tiles than workgroups ---------------------------------------------------------------------------------
def _capped(run):
    """run() without a cap, then under each cap: the outputs"""
    from neurecon_amd import _lib as L
    outs = [run()]
    try:
        for cap in CAPS:
            L.set_workgroup_cap(cap)
            outs.append(run())
        torch.cuda.synchronize()
    finally:
        L.set_workgroup_cap(0)
    return outs


def _same_under_caps(tag, run):
    plain, *capped = _capped(run)
    for cap, out in zip(CAPS, capped):
        for a, b in zip(plain, out):
            assert torch.equal(a, b), (tag, cap, float((a - b).abs().max()))


@pytest.mark.parametrize('c,precision', GRID, ids=GRID_IDS)
def test_radiance_second_and_third_tile(nets, c, precision):
    """1 and 3 workgroups for 300 points: a workgroup restarts its weight stream for a second and a third tile
    (has_next); bit for bit the uncapped run's values, which test_radiance_*_vs_float64 hold to the bar"""
    m = nets.radiance(c, precision)
    for name in ('unit', 'mixed_scale'):
        t = nets.cls(name, c)[1]
        _same_under_caps(f'{R.cfg_id(c)} {precision} {name}', lambda: (_forward(m, *t),))


@pytest.mark.parametrize('c', FOLD_CONFIGS, ids=FOLD_IDS)
def test_folded_pair_second_and_third_tile(nets, c):
    m = nets.radiance(c, 'f16x3')
    x, v, n, _ = nets.cls('unit', c)[1]
    _same_under_caps(f'{R.cfg_id(c)} folded', lambda: (_folded(nets.sdf(), m, x, v, n),))


@pytest.mark.parametrize('precision', R.PRECISIONS)
def test_nerf_second_and_third_tile(nets, precision):
    m = nets.nerf_net(precision)
    for name in ('nerf_unit', 'nerf_edges'):
        t = nets.cls(name, None)[1]
        _same_under_caps(f'nerf {precision} {name}', lambda: _nerf(m, *t))


# -- rows past P, and vdir_div, straight on the C ABI -----------------------------------------------------------
def _padded(t, rows=None):
    """t's rows (or its first `rows`) at the head of a buffer whose remaining PAD rows are NaN"""
    t = t if rows is None else t[:rows]
    return torch.cat([t, torch.full((PAD,) + tuple(t.shape[1:]), float('nan'), device=t.device)]).contiguous()


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda')


def _untouched(buf, P):
    return bool((buf[P:] == SENTINEL).all())


def _radiance_abi(m, x, v, n, f, P, vdiv, rgb):
    from neurecon_amd import _lib as L
    dev = x.device
    with torch.no_grad():
        desc, packed = m.nr_packed(dev)
    L.check(L.lib().nr_radiance_forward(ctypes.byref(desc), L.ptr(packed), L.ptr(x), L.ptr(v), vdiv, L.ptr(n), L.ptr(f),
                                        P, L.ptr(rgb), L.stream_of(dev)))
    torch.cuda.synchronize()


def _nerf_abi(m, x4, v, P, vdiv, sigma, rgb):
    from neurecon_amd import _lib as L
    dev = x4.device
    with torch.no_grad():
        desc, packed = m.nr_packed(dev)
    L.check(L.lib().nr_nerf_forward(ctypes.byref(desc), L.ptr(packed), L.ptr(x4), L.ptr(v), vdiv, P, L.ptr(sigma),
                                    L.ptr(rgb), L.stream_of(dev)))
    torch.cuda.synchronize()


def _per_ray(v, div):
    """the first ceil(P / div) directions, one per ray, and their expansion to one per point"""
    P = len(v)
    rays = v[:(P + div - 1) // div].contiguous()
    return rays, rays.repeat_interleave(div, 0)[:P].contiguous()


ABI_RADIANCE = {'rad4_kernel': (R.RadCfg(4, True, 4, False), 'f16x3'),
                'radiance_kernel fp32': (R.RadCfg(3, True, 4, False), 'fp32'),
                'radiance_kernel sine': (R.RadCfg(4, True, 5, True), 'f16x3')}


@pytest.mark.parametrize('family', list(ABI_RADIANCE))
def test_radiance_abi_rows_past_P_and_vdir_div(nets, family):
    """nr_radiance_forward at P = 300 on buffers of 428 rows, the last 128 NaN (inputs) or a sentinel (rgb): rows
    below P equal the plain call's bit for bit, rows from P on keep the sentinel; then vdir_div = 7 on 43 ray
    directions followed by NaN rows (the last ray has 6 points) against vdir_div = 1 on the expanded directions"""
    c, precision = ABI_RADIANCE[family]
    m, P = nets.radiance(c, precision), R.N_POINTS
    x, v, n, f = nets.cls('unit', c)[1]
    plain = _forward(m, x, v, n, f)
    rgb = _sentinel(P + PAD, 3)
    _radiance_abi(m, _padded(x), _padded(v), _padded(n), _padded(f), P, 1, rgb.view(torch.float32))
    assert torch.equal(rgb[:P].view(torch.float32), plain), family
    assert _untouched(rgb, P), family
    rays, expanded = _per_ray(v, 7)
    assert len(rays) == 43 and P - 42 * 7 == 6
    want = _forward(m, x, expanded, n, f)
    assert not torch.equal(want, plain)  # the directions matter
    rgb = _sentinel(P + PAD, 3)
    _radiance_abi(m, _padded(x), _padded(rays), _padded(n), _padded(f), P, 7, rgb.view(torch.float32))
    assert torch.equal(rgb[:P].view(torch.float32), want), family
    assert _untouched(rgb, P), family


@pytest.mark.parametrize('precision', R.PRECISIONS)
def test_nerf_abi_rows_past_P_and_vdir_div(nets, precision):
    """the same on nr_nerf_forward: nerf_kernel<fp32> and nerf4_kernel"""
    m, P = nets.nerf_net(precision), R.N_POINTS
    x4, v = nets.cls('nerf_unit', None)[1]
    plain = _nerf(m, x4, v)
    rays, expanded = _per_ray(v, 7)
    want = _nerf(m, x4, expanded)
    assert not torch.equal(want[1], plain[1])
    for vbuf, div, ref in ((_padded(v), 1, plain), (_padded(rays), 7, want)):
        sigma, rgb = _sentinel(P + PAD), _sentinel(P + PAD, 3)
        _nerf_abi(m, _padded(x4), vbuf, P, div, sigma.view(torch.float32), rgb.view(torch.float32))
        assert torch.equal(sigma[:P].view(torch.float32), ref[0]), (precision, div)
        assert torch.equal(rgb[:P].view(torch.float32), ref[1]), (precision, div)
        assert _untouched(sigma, P) and _untouched(rgb, P), (precision, div)
