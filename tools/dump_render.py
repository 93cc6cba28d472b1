"""Render fixed scenes with the three frameworks (render mode: every `extras` tensor; training: one
forward + backward, the losses and every parameter's gradient), run every case of tests/composite_cases.py
through the training compositing kernels (forward and backward, every output and gradient) and save or
compare all of it bit for bit:

    dump_render.py save PATH            writes them
    dump_render.py check PATH [PATH2]   compares this tree's with PATH's; exit status 1 on a difference

With PATH2 (a second save of the same tree as PATH) the training tensors that differ between PATH and
PATH2 are run-to-run noise of that tree (atomics in the weight gradients): they are listed and left
out.  Render-mode and compositing-case tensors are never left out.  Used to A/B a change that must not
alter any output bit."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')]


def _extras(ret):
    rgb, depth, ex = ret
    assert ex['rgb'] is rgb and ex['depth_volume'] is depth
    return {k: v for k, v in ex.items() if isinstance(v, torch.Tensor)}


def renders():
    import bench
    import weightgen as wg
    from helpers import neus_model, unisurf_model, volsdf_model
    from neurecon_amd import rend_util
    from neurecon_amd.frameworks import neus, unisurf, volsdf
    dev = torch.device('cuda', 0)
    out = {}
    with torch.no_grad():
        model = bench.make_model(dev, 'f16x3')
        c2w, K = bench.camera(dev)
        ro, rd, _ = rend_util.get_rays(c2w, K, 64, 64)
        for tag, kw in [('b', dict(bench.render_kwargs())), ('b_perturb', dict(bench.render_kwargs(), perturb=True)),
                        ('b_detailed', dict(bench.render_kwargs(), detailed_output=True))]:
            torch.manual_seed(5)
            n = 1024 if kw['detailed_output'] else ro.shape[1]  # the per-sample tensors of 1024 rays are enough
            out['neus_' + tag] = _extras(neus.volume_render(ro[:, :n], rd[:, :n], model, **kw))
        mn = neus_model(wg.neus_state(seed=4, use_outside_nerf=True), use_outside_nerf=True, precision='f16x3')
        for tag, kw in [('nerfpp', {}), ('nerfpp_detailed', dict(detailed_output=True))]:
            kw = dict(bench.render_kwargs(), N_outside=32, **kw)
            out['neus_' + tag] = _extras(neus.volume_render(ro[:, :1024], rd[:, :1024], mn, **kw))
        # the compositing variants that only large sample counts reach (the dispatch at the end of neus_chunk,
        # LDS bytes per ray against 65536), 8 rays, detailed.  N_samples = 64, the rest in N_importance; a round
        # of the official upsampling takes at most 32 new samples, so N_upsample_iters is N_importance / 32
        # rounded up to a divisor (the entries above use 4 rounds of 16):
        #   neus_composite<1>            9 S 16 > 65536:        S = 512              (448 = 14 x 32)
        #   neus_composite_outside_w<1>  (6 M + 4 S) 16 > 65536: S = 400, N_outside 32 (336 = 12 x 28)
        #   neus_composite_outside       (6 M + 4 S) 4 > 65536:  S = 1600, N_outside 80 (1536 = 48 x 32)
        for tag, m, S, iters, n_out in [('rpw1', model, 512, 14, 0), ('outside_rpw1', mn, 400, 12, 32),
                                        ('outside_per_ray', mn, 1600, 48, 80)]:
            kw = dict(bench.render_kwargs(), detailed_output=True, N_importance=S - 64, N_upsample_iters=iters,
                      N_outside=n_out)
            out['neus_' + tag] = _extras(neus.volume_render(ro[:, :8], rd[:, :8], m, **kw))
            assert out['neus_' + tag]['cdf'].shape[-1] == S, (tag, out['neus_' + tag]['cdf'].shape)

        ro, rd = bench.camera_for(dev, 16, 32, 80.0, 2.7)
        vkw = dict(near=0.0, far=6.0, obj_bounding_radius=3.0, batched=True, calc_normal=True, detailed_output=True,
                   N_samples=64, N_importance=64, max_upsample_steps=6)
        mv = volsdf_model(wg.volsdf_state(seed=3, beta_init=0.1), 0.1, precision='f16x3')
        mvo = volsdf_model(wg.volsdf_state(seed=3, beta_init=0.1, use_nerfplusplus=True), 0.1, precision='f16x3',
                           use_nerfplusplus=True)
        for tag, m, kw in [('builtin', mv, {}), ('builtin_perturb', mv, dict(perturb=True)),
                           ('nerfpp', mvo, dict(use_nerfplusplus=True, N_outside=32)),
                           ('nerfpp_perturb', mvo, dict(use_nerfplusplus=True, N_outside=32, perturb=True))]:
            torch.manual_seed(6)
            out['volsdf_' + tag] = _extras(volsdf.volume_render(ro, rd, m, **dict(vkw, **kw)))

        ro, rd = bench.camera_for(dev, 32, 32, 80.0, 3.0)
        ukw = dict(calc_normal=True, detailed_output=True, logit_tau=0.0, radius_of_interest=4.0, N_query=64,
                   N_freespace=32)
        mu = unisurf_model(wg.unisurf_state(seed=3), precision='f16x3')
        ro2, rd2 = ro.reshape(2, -1, 3), rd.reshape(2, -1, 3)  # two batch rows of 512 rays
        for tag, o, d, kw in [('windows', ro2, rd2, dict(batched=True, rayschunk=200, netchunk=5000)),
                              ('unbatched', ro[0], rd[0], dict(batched=False)),
                              ('perturb', ro2, rd2, dict(batched=True, perturb=True))]:
            torch.manual_seed(7)
            out['unisurf_' + tag] = _extras(unisurf.volume_render(o, d, mu, **dict(ukw, **kw)))
    torch.cuda.synchronize()
    return {k: {n: t.cpu() for n, t in v.items()} for k, v in out.items()}


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def train_steps():
    """one Trainer forward + backward per framework on its 8x8 training fixture"""
    import weightgen as wg
    from helpers import neus_model, unisurf_model, volsdf_model
    from neurecon_amd.frameworks import neus, unisurf, volsdf
    gold = lambda name: dict(np.load(os.path.join(ROOT, 'tests', 'golden', name)))
    g = gold('unisurf_train.npz')
    cases = [
        ('neus', neus.Trainer, neus_model(wg.neus_state(seed=1), precision='f16x3'), gold('neus_train.npz'),
         _ns(data=_ns(N_rays=-1), training=_ns(w_eikonal=0.1, w_mask=1.0, with_mask=True)),
         dict(H=8, W=8, upsample_algo='official_solution', N_nograd_samples=2048, N_upsample_iters=4, N_outside=0,
              obj_bounding_radius=1.0, batched=True, perturb=True, white_bkgd=False)),
        ('volsdf', volsdf.Trainer, volsdf_model(wg.volsdf_state(seed=3, beta_init=0.1), 0.1, precision='f16x3'),
         gold('volsdf_train.npz'),
         _ns(data=_ns(N_rays=-1), model=_ns(obj_bounding_radius=3.0), training=_ns(w_eikonal=0.1)),
         dict(H=8, W=8, near=0.0, far=6.0, obj_bounding_radius=3.0, batched=True, perturb=True, white_bkgd=False,
              max_upsample_steps=6, use_nerfplusplus=False, N_samples=64, N_importance=64)),
        ('unisurf', unisurf.Trainer, unisurf_model(wg.unisurf_state(seed=3), precision='f16x3'), g,
         _ns(data=_ns(N_rays=-1), training=_ns(w_reg=0.01, perturb_surface_pts=0.01, delta_max=1.0, delta_min=0.05,
                                               delta_beta=1.5e-5)),
         dict(H=8, W=8, batched=True, perturb=True, white_bkgd=False, logit_tau=float(g['logit_tau']),
              radius_of_interest=4.0, N_query=64, N_freespace=32)),
    ]
    T = lambda a: torch.from_numpy(np.asarray(a)).cuda()
    out = {}
    for fw, Trainer, m, g, args, kw in cases:
        m.train()
        mi = {'intrinsics': T(g['K']), 'c2w': T(g['c2w'])}
        if 'target_mask' in g:
            mi['object_mask'] = T(g['target_mask'])
        torch.manual_seed(100)  # the ray perturbation, eikonal points and surface perturbation of the step
        ret = Trainer(m, device_ids=[0])(args, None, mi, {'rgb': T(g['target_rgb'])}, kw, 0, device='cuda')
        ret['losses']['total'].mean().backward()
        d = {'loss/' + k: v.detach() for k, v in ret['losses'].items()}
        d.update({'grad/' + k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None})
        d.update({'extras/' + k: v.detach() for k, v in ret['extras'].items() if isinstance(v, torch.Tensor)})
        out['train_' + fw] = {k: v.cpu() for k, v in d.items()}
    torch.cuda.synchronize()
    return out


def composites():
    """every case of tests/composite_cases.py through the training compositing kernels' C entry points,
    forward and backward (the harness of tests/test_gpu_composite.py): all outputs and gradients"""
    import composite_cases as CC
    from test_gpu_composite import Harness
    h = Harness()
    return {'composite_' + c.name: {k: v.cpu() for k, v in h.run(c).items()} for c in CC.CASES}


def _differing(a, b):
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    bad = []
    for tag in a:
        assert list(a[tag]) == list(b[tag]), f'{tag}: keys or key order differ: {list(a[tag])} vs {list(b[tag])}'
        for name in a[tag]:
            x, y = a[tag][name], b[tag][name]
            raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8)  # bit for bit: NaNs and -0 count too
            same = x.shape == y.shape and x.dtype == y.dtype and torch.equal(raw(x), raw(y))
            if not same:
                bad.append((tag, name))
    return bad


def main():
    mode, path = sys.argv[1], sys.argv[2]
    out = dict(renders(), **train_steps(), **composites())
    n = sum(len(v) for v in out.values())
    if mode == 'save':
        torch.save(out, path)
        print(f'saved {n} tensors of {len(out)} runs to {path}')
        return
    ref = torch.load(path, weights_only=True)
    noise = _differing(ref, torch.load(sys.argv[3], weights_only=True)) if len(sys.argv) > 3 else []
    for tag, name in noise:
        print('NOISE (differs between the two reference saves, left out):', tag, name)
    if any(not tag.startswith('train_') for tag, _ in noise):
        print('a render-mode tensor differs between the two reference saves')
        sys.exit(1)
    bad = [tn for tn in _differing(ref, out) if tn not in noise]
    for tag, name in bad:
        print('DIFF', tag, name)
    print(f'{n - len(noise)} tensors compared, {len(noise)} left out: ' +
          ('bit-identical' if not bad else f'{len(bad)} differ'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
