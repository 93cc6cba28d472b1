"""Claimed tiles and the two-branch chunk of the NeuS render against the serial, fixed-stride order.

By default the mid-point launch, the radiance launch and the compacted reverse pass take their 128-point tiles
with one atomic per tile (nr_mlp.h), and the reverse pass runs on the library's side stream beside the other
two (nr_neus.hip neus_chunk).  Which workgroup runs a tile changes no point's arithmetic, so every map and
every detailed output must equal the `serial_order=True` render of the same rays bit for bit.

Config (b)'s architecture with weightgen weights; 48 and 80 rays taken evenly from the 64 x 64 config-(b)
camera (3072 and 5120 coarse points).  Workgroup caps 1, 3 and none: with cap 3 each of the three launches
runs several rounds with a ragged last one, with cap 1 one workgroup claims every tile, without a cap most
workgroups run one tile and some claim and find nothing.  Each case first asserts, from the library's
profile census, that the three launches had more tiles than the cap."""
import os

import numpy as np
import pytest
import torch

import weightgen as wg
from helpers import neus_model
from neurecon_amd import _lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAPS = ('rgb', 'depth', 'mask_volume', 'normals_volume')
DETAILED = ('implicit_surface', 'implicit_nablas', 'radiance', 'visibility_weights')
CLAIMED = ('sdf_nabla_feat', 'radiance', 'sdf_nabla_bwd')  # mid-point, radiance, compacted reverse launch


@pytest.fixture(scope='module')
def model():
    return neus_model(wg.neus_state(seed=1), precision='f16x3')


def _rays(n):
    g = np.load(os.path.join(HERE, 'golden', 'neus_b.npz'))
    idx = np.round(np.linspace(0, g['rays_o'].shape[1] - 1, n)).astype(np.int64)
    return torch.from_numpy(g['rays_o'][:, idx]).cuda(), torch.from_numpy(g['rays_d'][:, idx]).cuda()


def _render(m, ro, rd, detailed, census=False, **kw):
    """(outputs by name, per-launch census or None)"""
    from neurecon_amd.frameworks.neus import volume_render
    if census:
        L.profile_read()
        L.profile_enable(True)
    try:
        with torch.no_grad():
            rgb, depth, ex = volume_render(ro, rd, m, batched=True, calc_normal=True, N_samples=64, N_importance=64,
                                           detailed_output=detailed, **kw)
        torch.cuda.synchronize()
    finally:
        if census:
            L.profile_enable(False)
    out = dict(ex, rgb=rgb, depth=depth)
    return {k: out[k] for k in (DETAILED + MAPS if detailed else MAPS)}, (L.profile_read() if census else None)


def _same(got, want, what):
    for k, w in want.items():
        assert torch.equal(got[k], w), (what, k, float((got[k] - w).abs().max()))


@pytest.fixture(scope='module')
def serial(model):
    """the serial, fixed-stride renders of both ray sets: computed once, compared against by every case"""
    ref = {}
    for n in (48, 80):
        ro, rd = _rays(n)
        ref[n] = (ro, rd, _render(model, ro, rd, False, serial_order=True)[0],
                  _render(model, ro, rd, True, serial_order=True)[0])
        assert float(ref[n][2]['normals_volume'].abs().max()) > 0.0
    return ref


@pytest.mark.parametrize('cap', [1, 3, 0])
@pytest.mark.parametrize('n', [48, 80])
def test_claimed_tiles_match_the_serial_order(model, serial, n, cap):
    ro, rd, maps, detailed = serial[n]
    try:
        L.set_workgroup_cap(cap)
        got, census = _render(model, ro, rd, False, census=True)
        # the inputs exercise the claims: each claimed launch ran once, on more tiles than workgroups
        for name in CLAIMED:
            launches, _, units = census[name]
            print(f'{n} rays, cap {cap}: {name} {units:.0f} points = {units / 128:.1f} tiles')
            assert launches == 1 and units / 128 > cap, (name, launches, units)
        _same(got, maps, f'{n} rays, cap {cap}')
        # detailed outputs: every mid-point through the claimed mid-point and radiance launches
        got, census = _render(model, ro, rd, True, census=True)
        for name in CLAIMED[:2]:
            assert census[name][2] / 128 > cap, (name, census[name])
        _same(got, detailed, f'{n} rays, cap {cap}, detailed')
    finally:
        L.set_workgroup_cap(0)


def test_three_calls_in_a_row(model, serial):
    """the counters are zeroed by every call and the side stream serves every call"""
    ro, rd, maps, _ = serial[80]
    try:
        L.set_workgroup_cap(3)
        for i in range(3):
            _same(_render(model, ro, rd, False)[0], maps, f'call {i}')
    finally:
        L.set_workgroup_cap(0)


def test_two_chunks_match_one(model, serial):
    """a workspace budget below the 80 rays' one-chunk workspace: two chunks, each joined before its compositing"""
    ro, rd, maps, _ = serial[80]
    key = (str(ro.device), torch.cuda.current_stream(ro.device).cuda_stream)
    L._WS.pop(key, None)  # the next render sizes the stream's buffer to exactly its own need
    _, census = _render(model, ro, rd, False, census=True)
    assert census['neus_prologue'][0] == 1
    one_chunk = L._WS[key].numel()
    # one ray's workspace is about 1 MB (0.8 MB of it reverse-pass slabs): 8 MiB less holds 64 to 79 rays
    budget_gb = (one_chunk - (8 << 20)) / float(1 << 30)
    try:
        L.set_workgroup_cap(3)
        got, census = _render(model, ro, rd, False, census=True, max_workspace_gb=budget_gb)
        assert census['neus_prologue'][0] == 2, census['neus_prologue']
        assert census['sdf_nabla_bwd'][0] == 2
        _same(got, maps, 'two chunks')
    finally:
        L.set_workgroup_cap(0)
