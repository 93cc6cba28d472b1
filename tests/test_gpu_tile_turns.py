"""Tile turns of the f16x3 SDF render kernels: what sdf4_kernel does at the start and the end of a 128-point tile
(the positional encoding and the chain rule through it) against values recorded from the commit before the
encoding changed.

The render launches evaluate each of a point's 18 encoding arguments once, sin and cos together, on one of the
point's four lanes and hand the values to the lanes whose operand rows they are; the fused nabla launch without
the feature (<true, false, 0>) keeps one call per row.  tests/golden/tile_turns.npz holds sdf, nablas and geometry
feature of the four `_run` instances (forward only, forward + feature, fused nabla, nabla + feature) as the parent
commit computed them; the instances agreed bit for bit there, so one copy of each serves all four.  Every instance
must still give exactly these values (torch.equal).

Points: 300 inside the unit sphere, then the encoding's edge cases -- coordinates at +0, -0, +-1e-30, +-1 and +-4
(UNISURF's radius of interest), and coordinates within 2 ulp of k pi / 2^(band + 1), k = 1..4, for every band,
where sin or cos of 2^band x crosses a zero or an extremum and the argument reduction changes quadrant.  One more
set of 128 CUs + 300 points makes some workgroups run a second tile; for it the fixture keeps the rows of the
first three and the last four tiles (the feature: of the last two).

Config (b)'s architecture with randomised biases, as tests/test_gpu_lean_stream.py.  The float64 bars are
tests/test_gpu_fold.py's: rtol 1e-5, atol 1e-6.

Regenerate (only from a commit whose values are the reference): python tests/test_gpu_tile_turns.py"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == '__main__':
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(HERE, 'golden'), HERE]

from helpers import neus_model  # noqa: E402
from sdf_ref import float64_sdf_nabla_feature, randomised_state  # noqa: E402

pytestmark = pytest.mark.gpu

RT, AT = 1e-5, 1e-6
SIZES = (1, 16, 17, 128, 129, 300)
FIXTURE = os.path.join(HERE, 'golden', 'tile_turns.npz')
SEED = 11


def _sphere_points(n, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, 3)
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * rs.uniform(0.05, 0.98, (n, 1)) ** (1 / 3)
    return x.astype(np.float32)


def _edge_points():
    """the encoding's edge cases, one special coordinate per point (its axis cycling), the other two drawn inside
    the unit ball; then a few points with all three coordinates special"""
    special = [0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 4.0, -4.0]
    for band in range(6):
        for k in range(1, 5):
            c = np.float32(k * math.pi / 2 ** (band + 1))
            for ulp in (-2, -1, 0, 1, 2):
                v = c
                for _ in range(abs(ulp)):
                    v = np.nextafter(v, np.float32(np.inf if ulp > 0 else -np.inf), dtype=np.float32)
                special.append(float(v))
    rs = np.random.RandomState(21)
    pts = rs.uniform(-0.5, 0.5, (len(special), 3)).astype(np.float32)
    for i, v in enumerate(special):
        pts[i, i % 3] = np.float32(v)
    corners = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [1e-30, -1e-30, 0.0], [1.0, -1.0, 1.0], [4.0, -4.0, 4.0],
                        [-4.0, 4.0, -0.0], [math.pi / 2, math.pi / 4, math.pi / 64]], dtype=np.float32)
    return np.concatenate([pts, corners])


def _small_points():
    return np.concatenate([_sphere_points(300, 5), _edge_points()])


def _big_rows(P):
    """rows of the P-point set that the fixture keeps: the first three tiles (the workgroups that run a second
    tile run these first) and the last four (the last three are second tiles); feature rows: the last two tiles"""
    rows = np.concatenate([np.arange(0, 384), np.arange((P - 1) // 128 * 128 - 384, P)])
    frows = np.arange((P - 1) // 128 * 128 - 128, P)
    return rows, frows


def _model():
    return neus_model(randomised_state(seed=SEED), precision='f16x3')


def _paths(m, xs):
    """(sdf, nablas, feature) of the four launch_sdf instances"""
    s = m.implicit_surface
    with torch.no_grad():
        out = dict(fwd=s._run(xs, nabla=False, feature=False), feat=s._run(xs, nabla=False, feature=True),
                   nabla=s._run(xs, nabla=True, feature=False), nabla_feat=s._run(xs, nabla=True, feature=True))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from neurecon_amd import _lib
    _lib.lib()  # must load: no fallback exists


@pytest.fixture(scope='module')
def fx():
    g = dict(np.load(FIXTURE))
    m = _model()
    x = torch.from_numpy(g['x']).cuda()
    return m, g, x, float64_sdf_nabla_feature(m, x)


def _worst(a, ref):
    return float((np.abs(a.cpu().numpy().astype(np.float64) - ref) / (AT + RT * np.abs(ref))).max())


def _same(name, got, want):
    want = torch.from_numpy(want).to(got.device)
    assert torch.equal(got, want), (name, float((got - want).abs().max()))


def test_fixture_points_are_the_documented_ones(fx):
    """the fixture's inputs are rebuilt here, so its edge cases cannot drift from the docstring's"""
    _, g, _, _ = fx
    assert np.array_equal(g['x'].view(np.uint32), _small_points().view(np.uint32))  # bit patterns: -0 is not +0


@pytest.mark.parametrize('P', SIZES)
def test_prefixes_match_parent(fx, P):
    """P = one lane, one wave, a wave boundary, one tile, a tile boundary, a ragged third tile"""
    m, g, x, _ = fx
    out = _paths(m, x[:P].contiguous())
    for k, (sdf, nab, feat) in out.items():
        _same(k + ' sdf', sdf, g['sdf'][:P])
        if nab is not None:
            _same(k + ' nablas', nab, g['nabla'][:P])
        if feat is not None:
            _same(k + ' feature', feat, g['feature'][:P])


def test_all_points_match_parent_and_float64(fx):
    """the 300 points and every edge case in one launch per instance: the parent's values bit for bit, and sdf,
    nablas and feature of every instance within the float64 bars"""
    m, g, x, ref64 = fx
    out = _paths(m, x)
    for k, got in out.items():
        for what, v, want, r64 in zip(('sdf', 'nablas', 'feature'), got, (g['sdf'], g['nabla'], g['feature']), ref64):
            if v is None:
                continue
            _same(f'{k} {what}', v, want)
            w = _worst(v, r64)
            print(f'{k}: {what} worst err / (atol + rtol |ref|) = {w:.4f}')
            assert w <= 1.0, (k, what)


def test_second_tile_matches_parent(fx):
    """128 points per CU and 300 more: some workgroups run a second tile, so whatever a tile hands to the next one
    (prefetched weights and tables, registers kept across the turn) is exercised"""
    m, g, _, _ = fx
    P = int(g['big_P'])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 128 * cus < P, f'{cus} CUs: no workgroup runs a second tile at {P} points'
    xs = torch.from_numpy(_sphere_points(P, 9)).cuda()
    rows, frows = _big_rows(P)
    r, fr = torch.from_numpy(rows).cuda(), torch.from_numpy(frows).cuda()
    out = _paths(m, xs)
    for k, (sdf, nab, feat) in out.items():
        _same(k + ' sdf', sdf[r], g['big_sdf'])
        if nab is not None:
            _same(k + ' nablas', nab[r], g['big_nabla'])
        if feat is not None:
            _same(k + ' feature', feat[fr], g['big_feature'])
    # the rows the fixture does not keep: equal across the instances
    assert torch.equal(out['nabla_feat'][1], out['nabla'][1])
    assert torch.equal(out['nabla_feat'][2], out['feat'][2])
    for k in ('feat', 'nabla', 'nabla_feat'):
        assert torch.equal(out[k][0], out['fwd'][0]), k
    # float64 on every row the fixture keeps, every instance (the feature: the rows of the last two tiles)
    sdf64, nab64, feat64 = float64_sdf_nabla_feature(m, xs[r])
    assert np.array_equal(rows[-len(frows):], frows)  # the feature rows are the kept rows' tail
    for k, (sdf, nab, feat) in out.items():
        w = [_worst(sdf[r], sdf64), _worst(nab[r], nab64) if nab is not None else 0.0,
             _worst(feat[fr], feat64[-len(frows):]) if feat is not None else 0.0]
        print(f'second tile, {k}: sdf {w[0]:.4f}, nablas {w[1]:.4f}, feature {w[2]:.4f} of the float64 bar')
        assert max(w) <= 1.0, k


def test_compacted_reverse_launch_matches_fused():
    """64 rays of config (b): the deferred sample nablas (forward launches, then the compacted reverse-only
    launch) against the fused launch, map by map"""
    from neurecon_amd.frameworks.neus import volume_render
    g = np.load(os.path.join(HERE, 'golden', 'neus_b.npz'))
    ro, rd = torch.from_numpy(g['rays_o'][:, :64]).cuda(), torch.from_numpy(g['rays_d'][:, :64]).cuda()
    m = neus_model(randomised_state(seed=1), precision='f16x3')
    outs = []
    for defer in (True, False):
        with torch.no_grad():
            rgb, depth, ex = volume_render(ro, rd, m, batched=True, calc_normal=True, N_samples=64, N_importance=64,
                                           detailed_output=False, defer_sample_nablas=defer)
        outs.append((rgb, depth, ex['mask_volume'], ex['normals_volume']))
    for name, a, b in zip(('rgb', 'depth', 'mask', 'normals'), *outs):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert float(outs[0][3].abs().max()) > 0.0


def _generate():
    """write the fixture from the library this tree builds (run on the commit whose values are the reference)"""
    m = _model()
    x = torch.from_numpy(_small_points()).cuda()
    out = _paths(m, x)
    for k in ('feat', 'nabla', 'nabla_feat'):
        assert torch.equal(out[k][0], out['fwd'][0]), k
    assert torch.equal(out['nabla'][1], out['nabla_feat'][1]) and torch.equal(out['feat'][2], out['nabla_feat'][2])
    sdf64, nab64, feat64 = float64_sdf_nabla_feature(m, x)
    print(f'{len(x)} points: sdf {_worst(out["fwd"][0], sdf64):.4f}, nablas {_worst(out["nabla"][1], nab64):.4f}, '
          f'feature {_worst(out["feat"][2], feat64):.4f} of the float64 bar')
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P = 128 * cus + 300
    rows, frows = _big_rows(P)
    big = _paths(m, torch.from_numpy(_sphere_points(P, 9)).cuda())
    for k in ('feat', 'nabla', 'nabla_feat'):
        assert torch.equal(big[k][0], big['fwd'][0]), k
    assert torch.equal(big['nabla'][1], big['nabla_feat'][1]) and torch.equal(big['feat'][2], big['nabla_feat'][2])
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, x=x.cpu().numpy(),
                        sdf=out['fwd'][0].cpu().numpy(), nabla=out['nabla'][1].cpu().numpy(),
                        feature=out['feat'][2].cpu().numpy(), big_P=np.int64(P),
                        big_sdf=big['fwd'][0].cpu().numpy()[rows], big_nabla=big['nabla'][1].cpu().numpy()[rows],
                        big_feature=big['feat'][2].cpu().numpy()[frows])
    print('wrote fixture:', P, 'points in the large set,', cus, 'CUs')


if __name__ == '__main__':
    _generate()
