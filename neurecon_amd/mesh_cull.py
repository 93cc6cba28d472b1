"""Cull an extracted mesh by what the training cameras constrain, on the device.

Every published DTU Chamfer distance of NeuS, VolSDF and UNISURF is computed on a culled mesh: each vertex is
projected into every training camera, and a vertex that lands outside a dilated object mask in a view that
sees it is removed, so that the table, the background shell and whatever the net invented where no camera
looked do not enter the accuracy side of the distance.  This module is that step, between `mesh_util.filter_mesh`
and `mesh_metrics.evaluate_mesh`:

* `dilate_masks`: binary dilation of a mask stack by a square of side 2 r + 1 (libnrhip `nr_mask_dilate`).
* `vertex_views`: per vertex, in how many views it falls inside the image, inside the mask, and in front of the
  mesh's own depth (libnrhip `nr_mesh_view_test`, on depth frames of `nr_mesh_render`).
* `cull_mesh`: the hull rule (n_in_mask == n_in_image) and the visibility rule (n_visible >= min_visible)
  chained into `filter_mesh`.
* `load_cameras_npz`: the cameras of a DTU `cameras.npz`, as dataio/DTU.py reads them.

    python -m neurecon_amd.mesh_cull in.ply out.ply --cameras cameras.npz --H H --W W [--masks masks.npy | DIR]
        [--dilate R] [--depth-tol T] [--min-visible K] [--keep largest] [--min-faces K] [--to-world]

prints one JSON line.  With --to-world the output is in the space the DTU clouds live in and feeds
`python -m neurecon_amd.mesh_metrics` directly.

Both kernels' results are pure functions of their inputs (integers: two runs are bit-identical); the rules
are stated in the header comment of neurecon_amd/csrc/nr_meshcull.hip and restated in numpy in
tests/mesh_cull_ref.py.

Out of scope: reading DTU's `.mat` ObsMask files, bilinear mask sampling, near-plane clipping (a vertex closer
than `near` is in no image, and the depth frames drop a face with such a vertex whole: the renderer's limit),
sharding the views across ranks.
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

from . import _lib as L
from .mesh_util import _LARGE_THRESHOLD, _mesh_faces, filter_mesh, read_ply, write_ply
from .rend_util import load_K_Rt_from_P

_MAX_FRAME_BYTES = 256 << 20  # depth_z + face_id frames held at a time by vertex_views
IN_IMAGE, IN_MASK, VISIBLE = 1, 2, 4  # the bits of `flags`


def _device_of(*xs):
    dev = next((t.device for t in xs if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError('neurecon_amd: mesh_cull needs a GPU (ROCm) device; the path is HIP-only')
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def _mask_stack(masks, name):
    """-> (tensor [B, H, W] of bool or uint8 on its own device, the input's rank)"""
    t = _tensor(masks)
    if t.dim() not in (2, 3) or t.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'{name}: masks must be bool or uint8 [H, W] or [B, H, W], got {t.dtype} {tuple(t.shape)}')
    rank = t.dim()
    t = t.reshape(-1, *t.shape[-2:])
    if t.shape[1] == 0 or t.shape[2] == 0 or t.shape[1] * t.shape[2] >= 2 ** 31:
        raise ValueError(f'{name}: needs H, W > 0 and H * W < 2^31, got {t.shape[1]} x {t.shape[2]}')
    return t, rank


def _radius(radius, name):
    r = int(radius)
    if r != radius or not 0 <= r < 2 ** 15:
        raise ValueError(f'{name} must be an integer in [0, 2^15), got {radius!r}')
    return r


def _dilate(m8, r, dev):
    """m8 uint8 [B, H, W] on dev, contiguous -> uint8 [B, H, W]"""
    B, H, W = m8.shape
    lib = L.lib()
    out = torch.empty_like(m8)
    with torch.cuda.device(dev):
        ws_bytes = lib.nr_mask_dilate_workspace_bytes(B, H, W)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        L.check(lib.nr_mask_dilate(L.ptr(m8), L.ptr(out), B, H, W, r, L.ptr(ws), ws_bytes, L.stream_of(dev)))
    return out


def dilate_masks(masks, radius):
    """Binary dilation on the device (libnrhip `nr_mask_dilate`): masks [H, W] or [B, H, W], bool or uint8 (non-zero
    is set), tensor or array -> a device bool tensor of the same rank.  A pixel is set iff a set pixel lies within
    `radius` of it in both row and column: a square structuring element of side 2 radius + 1, pixels outside
    the image count as unset -- `cv2.dilate(mask, np.ones((k, k)))`, `scipy.ndimage.binary_dilation` with a
    structure of ones.  radius 0 returns masks != 0; a radius beyond the image is legal; radius < 2^15."""
    r = _radius(radius, 'dilate_masks: radius')
    t, rank = _mask_stack(masks, 'dilate_masks')
    dev = _device_of(t)
    m8 = t.detach().to(dev).contiguous().view(torch.uint8) if t.dtype == torch.bool else t.detach().to(dev).contiguous()
    out = _dilate(m8, r, dev).view(torch.bool)
    return out if rank == 3 else out[0]


def _host64(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


def _cameras(c2w, intrinsics, near, who):
    """the cameras in float64 exactly as render_mesh takes them -> (poses [B, 4, 4], Ks [B, n, n], cams [B, 18])"""
    if c2w is None or intrinsics is None:
        raise ValueError(f'{who} needs c2w and intrinsics')
    poses, Ks = _host64(c2w), _host64(intrinsics)
    if poses.shape[-2:] != (4, 4) or poses.ndim not in (2, 3):
        raise ValueError(f'{who}: c2w must be [4, 4] or [B, 4, 4], got {poses.shape}')
    poses = poses.reshape(-1, 4, 4)
    if Ks.ndim not in (2, 3) or Ks.shape[-2:] not in ((4, 4), (3, 3)):
        raise ValueError(f'{who}: intrinsics must be [4, 4] or [3, 3] (or one per camera), got {Ks.shape}')
    Ks = Ks.reshape(-1, *Ks.shape[-2:])
    if Ks.shape[0] not in (1, poses.shape[0]):
        raise ValueError(f'{who}: {Ks.shape[0]} intrinsics for {poses.shape[0]} cameras')
    Ks = np.broadcast_to(Ks, (poses.shape[0], *Ks.shape[-2:]))
    near = float(near)
    if not (0.0 < near < math.inf):
        raise ValueError(f'{who}: near must be finite and > 0, got {near}')
    cams = np.empty((poses.shape[0], 18), np.float64)
    for b, (pose, K) in enumerate(zip(poses, Ks)):
        cams[b, :12] = np.linalg.inv(pose)[:3].reshape(-1)
        cams[b, 12:] = (K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1], near)
    if not np.isfinite(cams).all() or (cams[:, 12] == 0).any() or (cams[:, 13] == 0).any():
        raise ValueError(f'{who}: the cameras must be finite with non-zero fx and fy')
    return poses, Ks, cams


def _render_depth(v, f, pose, cam, H, W, zbuf, fbuf, ws, ws_bytes, st):
    """depth_z and face_id of one camera through nr_mesh_render, every other output null"""
    a = L.NrMeshRenderArgs()
    V, F = v.shape[0], f.shape[0]
    a.verts, a.faces = v.data_ptr() if V else None, f.data_ptr() if F else None
    a.V, a.F, a.H, a.W = V, F, H, W
    a.w2c[:] = cam[:12].tolist()
    a.m[:] = pose[:3, :3].reshape(-1).tolist()
    a.fx, a.fy, a.cx, a.cy, a.skew, a.near = (float(x) for x in cam[12:18])
    a.large_threshold = _LARGE_THRESHOLD
    a.zdepth, a.face_id = zbuf.data_ptr(), fbuf.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    L.check(L.lib().nr_mesh_render(ctypes.byref(a), st))


def vertex_views(verts, faces=None, c2w=None, intrinsics=None, H=None, W=None, masks=None, dilate=0, depth_tol=None,
                 near=1e-4, return_flags=False, max_frame_bytes=None):
    """Per vertex, the number of cameras that see it: in the image, inside the mask, in front of the mesh
    (libnrhip `nr_mesh_view_test`, neurecon_amd/csrc/nr_meshcull.hip) -> dict(n_in_image int32 [V], n_in_mask
    int32 [V] or None without masks, n_visible int32 [V] or None without depth_tol, n_views: int, and with
    `return_flags` flags uint8 [B, V]: bit 1 in_image, 2 in_mask, 4 visible), device tensors.

    verts [V, 3], faces [F, 3] (tensors or arrays; faces may be None without depth_tol).  c2w [4, 4] or
    [B, 4, 4], intrinsics [4, 4] / [3, 3] (or one per camera): taken in float64 exactly as `render_mesh` takes
    them, and the vertex is projected operation for operation as the renderer projects it.
      in_image  the projection (u, v) is finite, camera-space z >= near, 0 <= u <= W - 1, 0 <= v <= H - 1
      in_mask   in_image and the mask's nearest pixel (round half to even) is set.  masks [B, H, W] (or [H, W]
                for one camera), bool or uint8; dilated once by `dilate` pixels (`dilate_masks`) first.
      visible   in_image and z <= zmax + depth_tol, zmax the largest depth_z of the 2 x 2 pixels around (u, v) in
                the mesh's own depth frame (`nr_mesh_render`), +inf where one of them is a miss: conservative
                at a silhouette.  The frames are rendered in chunks of views that fit max_frame_bytes
                (default 256 MiB, at least one view); the result does not depend on the chunking."""
    who = 'vertex_views'
    if H is None or W is None:
        raise ValueError(f'{who} needs H and W')
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError(f'{who}: needs H, W > 0 and H * W < 2^31, got {H} x {W}')
    poses, _, cams = _cameras(c2w, intrinsics, near, who)
    B = poses.shape[0]
    r = _radius(dilate, f'{who}: dilate')
    if depth_tol is not None:
        depth_tol = float(depth_tol)
        if not (0.0 <= depth_tol < math.inf):
            raise ValueError(f'{who}: depth_tol must be finite and >= 0, got {depth_tol}')
        if faces is None:
            raise ValueError(f'{who}: depth_tol needs the faces (the mesh is rendered for its depth)')
    mt = None
    if masks is not None:
        mt, _ = _mask_stack(masks, who)
        if tuple(mt.shape) != (B, H, W):
            raise ValueError(f'{who}: masks must be [{B}, {H}, {W}] like the cameras, got {tuple(mt.shape)}')
    vt = _tensor(verts)
    if vt.dim() != 2 or vt.shape[1] != 3 or vt.shape[0] >= 2 ** 31:
        raise ValueError(f'{who}: verts must be [V, 3] with V < 2^31, got {tuple(vt.shape)}')
    frame_bytes = _MAX_FRAME_BYTES if max_frame_bytes is None else int(max_frame_bytes)
    if frame_bytes < 0:
        raise ValueError(f'{who}: max_frame_bytes must be >= 0, got {max_frame_bytes}')

    dev = _device_of(verts, faces, masks)
    v = vt.detach().to(device=dev, dtype=torch.float32).contiguous()
    V = v.shape[0]
    f = None
    if depth_tol is not None:
        ft = _tensor(faces)
        f, _ = _mesh_faces(ft.reshape(-1, 3).to(dev) if ft.numel() == 0 else ft.to(dev), V)
        if f.shape[0] >= 2 ** 31 - 1:
            raise ValueError(f'{who}: {f.shape[0]} faces do not fit the 31-bit face index')
    m8 = None
    if mt is not None:
        m8 = mt.detach().to(dev).contiguous()
        m8 = m8.view(torch.uint8) if m8.dtype == torch.bool else m8
        if r > 0:
            m8 = _dilate(m8, r, dev)
    lib = L.lib()
    with torch.cuda.device(dev):
        st = L.stream_of(dev)
        cams_d = torch.from_numpy(cams).to(dev)
        counts = torch.zeros((V, 3), dtype=torch.int32, device=dev)
        flags = torch.zeros((B, V), dtype=torch.uint8, device=dev) if return_flags else None
        a = L.NrMeshViewArgs()
        a.verts, a.V, a.H, a.W = (v.data_ptr() if V else None), V, H, W
        a.depth_tol = 0.0 if depth_tol is None else depth_tol
        a.counts = counts.data_ptr() if V else None

        def test(b0, n, zbuf, fbuf, accumulate):
            a.n_views, a.cams = n, cams_d.data_ptr() + 18 * 8 * b0
            a.masks = None if m8 is None else m8.data_ptr() + b0 * H * W
            a.zdepth = None if zbuf is None else zbuf.data_ptr()
            a.face_id = None if fbuf is None else fbuf.data_ptr()
            a.flags = None if flags is None or V == 0 else flags.data_ptr() + b0 * V
            a.accumulate = accumulate
            L.check(lib.nr_mesh_view_test(ctypes.byref(a), st))
        if depth_tol is None:
            if B:
                test(0, B, None, None, 0)
        elif B:
            per = max(1, min(B, frame_bytes // (8 * H * W)))
            zbuf = torch.empty((per, H, W), dtype=torch.float32, device=dev)
            fbuf = torch.empty((per, H, W), dtype=torch.int32, device=dev)
            ws_bytes = lib.nr_mesh_render_workspace_bytes(V, f.shape[0], H, W)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            for b0 in range(0, B, per):
                n = min(per, B - b0)
                for k in range(n):
                    _render_depth(v, f, poses[b0 + k], cams[b0 + k], H, W, zbuf[k], fbuf[k], ws, ws_bytes, st)
                test(b0, n, zbuf, fbuf, 1 if b0 else 0)
    out = dict(n_in_image=counts[:, 0].contiguous(), n_in_mask=counts[:, 1].contiguous() if m8 is not None else None,
               n_visible=counts[:, 2].contiguous() if depth_tol is not None else None, n_views=B)
    if return_flags:
        out['flags'] = flags
    return out


def cull_mesh(verts, faces=None, c2w=None, intrinsics=None, H=None, W=None, masks=None, dilate=0, depth_tol=None,
              min_visible=1, min_in_image=0, keep='all', min_faces=0, normals=None, colors=None, near=1e-4,
              max_frame_bytes=None):
    """Remove the vertices the cameras do not constrain, then filter components -> dict(verts, faces, index,
    normals, colors, kept bool [V], n_in_image, n_in_mask, n_visible, n_views), device tensors (normals / colors
    None when not given).  `verts` may be the dict `read_ply` returns.

    With the counts of `vertex_views`, a vertex is kept iff
      n_in_mask == n_in_image          when masks are given: the visual-hull rule of the DTU scripts -- every view
                                       that has the vertex in its image has it inside its (dilated) mask; a view
                                       that does not see it does not vote;
      n_in_image >= min_in_image;
      n_visible >= min_visible         when depth_tol is given.
    The kept vertices go through `filter_mesh(vertex_mask=kept, keep=keep, min_faces=min_faces)`: a face stays
    iff its three vertices stay, order is kept, `index` [V'] maps new -> old vertex and the attributes follow
    with index_select.  Raises ValueError when nothing stays."""
    if isinstance(verts, dict):
        mesh = verts
        verts = mesh['verts']
        faces = mesh['faces'] if faces is None else faces
        normals = mesh.get('normals') if normals is None else normals
        colors = mesh.get('colors') if colors is None else colors
    if faces is None:
        raise ValueError('cull_mesh needs verts and faces')
    if keep not in ('all', 'largest'):
        raise ValueError(f"cull_mesh: keep must be 'all' or 'largest', got {keep!r}")
    if int(min_faces) < 0 or int(min_visible) < 0 or int(min_in_image) < 0:
        raise ValueError('cull_mesh: min_faces, min_visible and min_in_image must be >= 0')
    V = _tensor(verts).shape[0]
    for name, attr in (('normals', normals), ('colors', colors)):
        if attr is not None and (_tensor(attr).dim() != 2 or _tensor(attr).shape[0] != V):
            raise ValueError(f'cull_mesh: {name} must have one row per vertex ({V}), got {tuple(_tensor(attr).shape)}')
    vv = vertex_views(verts, faces, c2w, intrinsics, H, W, masks=masks, dilate=dilate, depth_tol=depth_tol, near=near,
                      max_frame_bytes=max_frame_bytes)
    kept = vv['n_in_image'] >= int(min_in_image)
    if vv['n_in_mask'] is not None:
        kept &= vv['n_in_mask'] == vv['n_in_image']
    if vv['n_visible'] is not None:
        kept &= vv['n_visible'] >= int(min_visible)
    dev = kept.device
    v = _tensor(verts).detach().to(device=dev, dtype=torch.float32).contiguous()
    ft = _tensor(faces)
    f = (ft.reshape(-1, 3) if ft.numel() == 0 else ft).to(dev)
    v2, f2, index = filter_mesh(v, f, keep=keep, min_faces=int(min_faces), vertex_mask=kept)
    out = dict(verts=v2, faces=f2, index=index, normals=None, colors=None, kept=kept, n_views=vv['n_views'],
               n_in_image=vv['n_in_image'], n_in_mask=vv['n_in_mask'], n_visible=vv['n_visible'])
    for name, attr in (('normals', normals), ('colors', colors)):
        if attr is not None:
            out[name] = _tensor(attr).detach().to(dev).index_select(0, index)
    return out


def load_cameras_npz(path, n_views=None):
    """The cameras of a DTU `cameras.npz` as dataio/DTU.py:42-52 reads them -> (c2w [B, 4, 4] float32, intrinsics
    [B, 4, 4] float64, scale_mat_0 [4, 4] float64): per view P = (world_mat_i @ scale_mat_i)[:3] of the matrices
    cast to float32, split by `rend_util.load_K_Rt_from_P`.  No downscaling and no rescaling of the camera
    radius.  n_views: read the first n; default every consecutive world_mat_i from 0.  scale_mat_0 (as stored)
    takes the normalised space the mesh lives in to the world the DTU clouds live in."""
    with np.load(path) as cam:
        if n_views is None:
            n_views = 0
            while f'world_mat_{n_views}' in cam.files:
                n_views += 1
        n_views = int(n_views)
        if n_views <= 0:
            raise ValueError(f'load_cameras_npz: {path} holds no world_mat_0')
        missing = [k for i in range(n_views) for k in (f'world_mat_{i}', f'scale_mat_{i}') if k not in cam.files]
        if missing:
            raise ValueError(f'load_cameras_npz: {path} lacks {missing[:4]}')
        worlds = [cam[f'world_mat_{i}'].astype(np.float32) for i in range(n_views)]
        scales = [cam[f'scale_mat_{i}'].astype(np.float32) for i in range(n_views)]
        scale0 = np.asarray(cam['scale_mat_0'], dtype=np.float64)
    Ks, poses = [], []
    for world, scale in zip(worlds, scales):
        K, pose = load_K_Rt_from_P((world @ scale)[:3, :4])
        Ks.append(K)
        poses.append(pose)
    return np.stack(poses), np.stack(Ks), scale0


def _load_masks(path):
    """a .npy / .npz stack [B, H, W], or a directory of images (sorted by name, set where > 127.5)"""
    if os.path.isdir(path):
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError('mesh_cull: reading a directory of mask images needs PIL (pillow); save the stack '
                               'as a .npy file instead') from e
        names = sorted(n for n in os.listdir(path) if not n.startswith('.'))
        if not names:
            raise ValueError(f'mesh_cull: {path} holds no mask image')
        return np.stack([np.asarray(Image.open(os.path.join(path, n)).convert('L'), dtype=np.float32) > 127.5
                         for n in names])
    data = np.load(path)
    if isinstance(data, np.lib.npyio.NpzFile):
        with data:
            if len(data.files) != 1:
                raise ValueError(f'mesh_cull: {path} must hold one array, got {data.files}')
            data = data[data.files[0]]
    return np.ascontiguousarray(data != 0)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m neurecon_amd.mesh_cull',
                                 description='Cull a mesh (PLY) by the masks and the visibility of the cameras of a '
                                             'DTU cameras.npz, on the device; prints one JSON line.')
    ap.add_argument('input', help='the extracted mesh (a PLY with vertex and face elements)')
    ap.add_argument('output', help='the culled mesh (PLY)')
    ap.add_argument('--cameras', required=True, help='cameras.npz with world_mat_i and scale_mat_i')
    ap.add_argument('--H', type=int, required=True)
    ap.add_argument('--W', type=int, required=True)
    ap.add_argument('--masks', default=None, help='a .npy / .npz stack [B, H, W], or a directory of mask images')
    ap.add_argument('--dilate', type=int, default=0, help='radius in pixels the masks are dilated by')
    ap.add_argument('--depth-tol', type=float, default=None, help='keep only vertices some camera sees, to this depth')
    ap.add_argument('--min-visible', type=int, default=1)
    ap.add_argument('--keep', choices=('all', 'largest'), default='all')
    ap.add_argument('--min-faces', type=int, default=0)
    ap.add_argument('--to-world', action='store_true', help='write the vertices through scale_mat_0')
    a = ap.parse_args(argv)
    mesh = read_ply(a.input)
    masks = None if a.masks is None else _load_masks(a.masks)
    c2w, K, scale0 = load_cameras_npz(a.cameras, None if masks is None else len(masks))
    out = cull_mesh(mesh, None, c2w, K, a.H, a.W, masks=masks, dilate=a.dilate, depth_tol=a.depth_tol,
                    min_visible=a.min_visible, keep=a.keep, min_faces=a.min_faces)
    verts = out['verts'].cpu().numpy()
    normals = None if out['normals'] is None else out['normals'].cpu().numpy()
    if a.to_world:
        A = scale0[:3, :3]
        verts = (verts.astype(np.float64) @ A.T + scale0[:3, 3]).astype(np.float32)
        if normals is not None:  # normals go through the inverse transpose
            n = normals.astype(np.float64) @ np.linalg.inv(A)
            normals = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)).astype(np.float32)
    write_ply(a.output, verts, out['faces'], normals=normals, colors=out['colors'])
    print(json.dumps(dict(input=a.input, output=a.output, views=out['n_views'], verts_in=int(len(mesh['verts'])),
                          faces_in=int(len(mesh['faces'])), verts_out=int(len(verts)),
                          faces_out=int(out['faces'].shape[0]), dilate=a.dilate, depth_tol=a.depth_tol,
                          to_world=bool(a.to_world))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
