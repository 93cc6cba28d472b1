"""Host side of the three render entry points, without a GPU: workspace totals against the table
recorded before the host path was restructured (tests/golden/render_workspace.json, written by
tests/golden/gen_render_workspace.py), the return code and message of every argument clause that is
checked before the first HIP call, and the workspace-too-small error."""
import ctypes
import json
import os

import pytest

import render_host_cases as C
from neurecon_amd import _lib as L

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'render_workspace.json')


def test_workspace_totals_match_the_recorded_table():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = C.workspace_totals()
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f'{len(bad)} of {len(want)} totals differ, e.g. {list(bad.items())[:5]}'
    assert sum(1 for v in want.values() if v > 0) >= 140  # the table is about sizes, not rejections


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _desc(which, **kw):
    def f(a):
        d = getattr(a, which).contents
        for k, v in kw.items():
            setattr(d, k, v)
    return f


def _null_desc(which, typ):
    return lambda a: setattr(a, which, ctypes.POINTER(typ)())


def _siren(a):  # a SIREN SDF net must be D=5, skip=-1, multires=-1
    a.sdf.contents.siren = 1


# clauses shared by the three renders: (id, mutation, code, message substring); {fn} is the entry point's name
COMMON = [
    ('null_sdf', _null_desc('sdf', L.NrSdfDesc), ARG, 'null NrSdfDesc'),
    ('sdf_shape', _desc('sdf', D=7), UNSUPPORTED, 'SDF net: only D=8, W=256, skips=[4]'),
    ('sdf_prec', _desc('sdf', precision=5), UNSUPPORTED, 'SDF net: unknown precision mode'),
    ('siren_shape', _siren, UNSUPPORTED, 'SIREN SDF net: only D=5, W=256'),
    ('null_rad', _null_desc('rad', L.NrRadDesc), ARG, 'null NrRadDesc'),
    ('rad_shape', _desc('rad', W=128), UNSUPPORTED, 'radiance net: only D=4 or 5, W=256'),
    ('rad_prec', _desc('rad', precision=-1), UNSUPPORTED, 'radiance net: unknown precision mode'),
    ('null_rays_o', _set(rays_o=None), ARG, '{fn}: null ray or output pointer'),
    ('null_rays_d', _set(rays_d=None), ARG, '{fn}: null ray or output pointer'),
    ('null_rgb', _set(rgb=None), ARG, '{fn}: null ray or output pointer'),
    ('null_depth', _set(depth=None), ARG, '{fn}: null ray or output pointer'),
    ('null_acc', _set(acc=None), ARG, '{fn}: null ray or output pointer'),
    ('null_sdf_packed', _set(sdf_packed=None), ARG, '{fn}: null argument'),
    ('null_t_coarse', _set(t_coarse=None), ARG, '{fn}: null argument'),
    ('no_normals', _set(normals=None), ARG, '{fn}: calc_normal needs normals output'),
]
NERF = [
    ('nerf_shape', _desc('nerf', D=4), UNSUPPORTED, 'NeRF net: only the NeRF++ background configuration'),
    ('nerf_prec', _desc('nerf', precision=7), UNSUPPORTED, 'NeRF net: unknown precision mode'),
]

NEUS = [(i, m, c, s, {}) for i, m, c, s in COMMON] + [
    ('sample_only_no_out', _set(sample_only=1), ARG, '{fn}: null ray or output pointer', {}),
    ('null_rad_packed', _set(rad_packed=None), ARG, '{fn}: null argument', {}),
    ('fold_fp32', _set(fold_packed=C.FAKE), ARG, '{fn}: a fold pack needs the f16x3 softplus SDF net', dict(prec=L.PREC_FP32)),
    ('one_sample', _set(N_samples=1), ARG, '{fn}: N_samples must be >= 2', {}),
    ('negative_outside', _set(N_outside=-1), ARG, '{fn}: N_outside must be >= 0', {}),
    ('null_nerf', _null_desc('nerf', L.NrNerfDesc), ARG, 'null NrNerfDesc', dict(N_outside=32)),
    ('null_nerf_packed', _set(nerf_packed=None), ARG, '{fn}: N_outside > 0 needs the NeRF++ net', dict(N_outside=32)),
    ('null_t_outside', _set(t_outside=None), ARG, '{fn}: N_outside > 0 needs the NeRF++ net', dict(N_outside=32)),
    ('algo_high', _set(upsample_algo=3), ARG, '{fn}: unknown upsample_algo', {}),
    ('algo_low', _set(upsample_algo=-1), ARG, '{fn}: unknown upsample_algo', {}),
    ('direct_no_u', _set(u_fine=None), ARG, '{fn}: direct upsampling needs N_importance >= 1', dict(algo='direct_use')),
    ('direct_no_imp', _set(N_importance=0), ARG, '{fn}: direct upsampling needs N_importance >= 1', dict(algo='direct_use')),
    ('direct_no_s', _set(fixed_s=0.0), ARG, '{fn}: direct upsampling needs N_importance >= 1', dict(algo='direct_use')),
    ('more_few', _set(N_nograd_samples=1), ARG, '{fn}: direct_more needs N_nograd_samples >= 2', dict(algo='direct_more')),
    ('more_no_t', _set(t_nograd=None), ARG, '{fn}: direct_more needs N_nograd_samples >= 2', dict(algo='direct_more')),
    ('round_too_big', _set(N_importance=4 * 33), UNSUPPORTED, '{fn}: N_importance/N_upsample_iters must be in [1, 32]', {}),
    ('round_empty', _set(N_importance=3), UNSUPPORTED, '{fn}: N_importance/N_upsample_iters must be in [1, 32]', {}),
    ('official_no_u', _set(u_fine=None), UNSUPPORTED, '{fn}: N_importance/N_upsample_iters must be in [1, 32]', {}),
] + [(i, m, c, s, dict(N_outside=32)) for i, m, c, s in NERF]

VOLSDF = [(i, m, c, s, {}) for i, m, c, s in COMMON] + [
    ('null_rad_packed', _set(rad_packed=None), ARG, '{fn}: null argument', {}),
    ('null_t_init', _set(t_init=None), ARG, '{fn}: null argument', {}),
    ('null_u_up', _set(u_up=None), ARG, '{fn}: null argument', {}),
    ('null_u_fine', _set(u_fine=None), ARG, '{fn}: null argument', {}),
    ('no_samples', _set(N_samples=0), ARG, '{fn}: bad sample counts', {}),
    ('no_importance', _set(N_importance=0), ARG, '{fn}: bad sample counts', {}),
    ('negative_steps', _set(max_upsample_steps=-1), ARG, '{fn}: bad sample counts', {}),
    ('negative_bisect', _set(max_bisection_steps=-1), ARG, '{fn}: bad sample counts', {}),
    ('many_samples', _set(N_samples=257), UNSUPPORTED, '{fn}: 4*N_samples and N_importance must be <= 1024', {}),
    ('many_importance', _set(N_importance=1025), UNSUPPORTED, '{fn}: 4*N_samples and N_importance must be <= 1024', {}),
    ('beta_zero', _set(beta_net=0.0), ARG, '{fn}: beta must be positive', {}),
    ('beta_plus_zero', _set(beta_plus_init=0.0), ARG, '{fn}: beta must be positive', {}),
    ('sphere_and_nerf', _set(use_sphere_bg=1), ARG, '{fn}: NeRF++ background excludes the builtin sphere', dict(N_outside=32)),
    ('null_nerf', _null_desc('nerf', L.NrNerfDesc), ARG, '{fn}: N_outside > 0 needs nerf, nerf_packed', dict(N_outside=32)),
    ('null_nerf_packed', _set(nerf_packed=None), ARG, '{fn}: N_outside > 0 needs nerf, nerf_packed', dict(N_outside=32)),
    ('null_rs_out', _set(rs_out=None), ARG, '{fn}: N_outside > 0 needs nerf, nerf_packed', dict(N_outside=32)),
    ('beta_k_zero', _set(beta_plus_k=0.0), ARG, '{fn}: N_outside > 0 needs nerf, nerf_packed', dict(N_outside=32)),
] + [(i, m, c, s, dict(N_outside=32)) for i, m, c, s in NERF]

UNISURF = [(i, m, c, s, {}) for i, m, c, s in COMMON if i != 'null_t_coarse'] + [
    ('sample_only_no_out', _set(sample_only=1), ARG, '{fn}: null ray or output pointer', {}),
    ('sample_only_sharded', lambda a: None, ARG, '{fn}: sample_only is not a sharded render',
     dict(layout='shard', sample_only=True)),
    ('null_rad_packed', _set(rad_packed=None), ARG, '{fn}: null argument', {}),
    ('null_t_march', _set(t_march=None), ARG, '{fn}: null argument', {}),
    ('null_t_query', _set(t_query=None), ARG, '{fn}: null argument', {}),
    ('null_t_free', _set(t_free=None), ARG, '{fn}: null argument', {}),
    ('one_step', _set(N_steps=1), ARG, '{fn}: bad sample counts', {}),
    ('negative_secant', _set(N_secant_steps=-1), ARG, '{fn}: bad sample counts', {}),
    ('no_query', _set(N_query=0), ARG, '{fn}: bad sample counts', {}),
    ('no_free', _set(N_freespace=0), ARG, '{fn}: bad sample counts', {}),
    ('normal_mode', _set(normal_mode=2), ARG, '{fn}: normal_mode must be 0|1', {}),
    ('u_query_alone', _set(u_query=C.FAKE), ARG, '{fn}: u_query and u_free go together', {}),
    ('u_free_alone', _set(u_free=C.FAKE), ARG, '{fn}: u_query and u_free go together', {}),
    ('no_rayschunk', _set(rayschunk=0), ARG, '{fn}: rayschunk/netchunk must be positive', dict(layout='row')),
    ('no_netchunk', _set(netchunk=0), ARG, '{fn}: rayschunk/netchunk must be positive', dict(layout='row')),
    ('ragged_batch', _set(rays_per_batch=1000), ARG, '{fn}: n_rays % rays_per_batch != 0', {}),
    ('window_straddle', lambda a: None, UNSUPPORTED, '{fn}: rayschunk too large for windowed normalisation',
     dict(layout='row', n_rays=70000, rayschunk=200000)),
    ('shard_too_big', lambda a: None, UNSUPPORTED, '{fn}: rayschunk too large for windowed normalisation',
     dict(layout='shard', n_rays=70000)),
    ('shard_flat', _set(normal_mode=0), ARG, '{fn}: a sharded render needs normal_mode 1', dict(layout='shard')),
    ('shard_no_ss', _set(window_ss=None), ARG, '{fn}: a sharded render needs normal_mode 1', dict(layout='shard')),
    ('shard_no_reduce', _set(window_reduce=None), ARG, '{fn}: a sharded render needs normal_mode 1', dict(layout='shard')),
    ('shard_before_row', _set(shard_ray0=-1), ARG, '{fn}: shard outside its batch row', dict(layout='shard')),
    ('shard_past_row', _set(shard_ray0=4097), ARG, '{fn}: shard outside its batch row', dict(layout='shard')),
]

RENDERS = {'neus': ('nr_neus_render', C.neus_args, NEUS), 'volsdf': ('nr_volsdf_render', C.volsdf_args, VOLSDF),
           'unisurf': ('nr_unisurf_render', C.unisurf_args, UNISURF)}
ROWS = [pytest.param(fw, row, id=f'{fw}-{row[0]}') for fw, (_, _, rows) in RENDERS.items() for row in rows]


@pytest.mark.parametrize('fw,row', ROWS)
def test_rejected_arguments(fw, row):
    """one mutation of a valid block: the clause that rejects it, by return code and message (all of them
    are checked before any HIP call; the fake pointers are never dereferenced)"""
    fn, make, _ = RENDERS[fw]
    _, mutate, code, msg, base = row
    lib = L.lib()
    a = make(**base)
    a.workspace, a.workspace_bytes = None, 0  # a block that passed every clause would stop here, before any launch
    mutate(a)
    assert getattr(lib, fn)(ctypes.byref(a), None) == code
    assert msg.format(fn=fn) in lib.nr_last_error().decode()


@pytest.mark.parametrize('fw', RENDERS)
def test_null_args_and_empty_call(fw):
    fn, make, _ = RENDERS[fw]
    lib = L.lib()
    assert getattr(lib, fn)(None, None) == ARG
    assert f'{fn}: null args' in lib.nr_last_error().decode()
    assert getattr(lib, fn.replace('_render', '_workspace_bytes'))(None) == 0
    a = make(n_rays=0)  # an empty shard: nothing to render, null ray / output pointers allowed
    a.rays_o = a.rays_d = a.rgb = a.depth = a.acc = a.normals = None
    assert getattr(lib, fn)(ctypes.byref(a), None) == 0


@pytest.mark.parametrize('fw', RENDERS)
def test_workspace_too_small(fw):
    fn, make, _ = RENDERS[fw]
    lib = L.lib()
    a = make()
    need = getattr(lib, fn.replace('_render', '_workspace_bytes'))(ctypes.byref(a))
    assert need > 0
    for ws, nbytes in [(C.FAKE * 50, need - 1), (C.FAKE * 50, 0), (None, need)]:
        a.workspace, a.workspace_bytes = ws, nbytes
        assert getattr(lib, fn)(ctypes.byref(a), None) == WORKSPACE
        assert f'{fn}: workspace too small' in lib.nr_last_error().decode()
