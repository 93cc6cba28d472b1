"""Mesh extraction: drop-in for utils/mesh_util.py:82-112.

The hot part — the N^3 SDF grid query (134 M forward SDF evaluations at N=512) — runs in
libnrhip (`nr_sdf_grid`: voxel coordinates generated on the device with the reference's float64
formula, then the forward SDF kernel), with no host point array and no per-chunk host copies.

Marching cubes and PLY writing need nothing but this package: `marching_cubes` runs on the device
over the SDF volume (libnrhip `nr_mc_count` + `nr_mc_emit`, neurecon_amd/csrc/nr_mcubes.hip) and
returns a welded indexed mesh as device tensors; `write_ply` writes the binary PLY layout plyfile
writes for the reference.  `marching='native'` selects that path, `'skimage'` the reference's
(scikit-image + plyfile on the host), `'auto'` (the default) the reference's when both packages
import and the native one otherwise.  On the native path of `extract_mesh` the volume never leaves
the device.

How the native mesh differs from skimage's (Lewiner) one: the vertices are the same grid-edge
crossings (skimage interpolates them in fp32, here in float64 rounded once), one per sign-changing
edge.  The triangulation can differ inside cells that have an ambiguous face or interior: skimage
picks among Lewiner's sub-cases from the corner values, the native table resolves an ambiguous face
by one fixed rule on its four corner classes (each inside corner is cut off on its own) and never
looks at the interior.  Both are watertight.  The vertex and face orders differ: native vertices
are ordered by the owning grid point's flat index, then axis; faces by cell, then table order.

Note: the reference computes the voxel y / x indices with true division (`(i / N) % N`,
`((i / N) / N) % N`, mesh_util.py:92-93), i.e. with fractional parts z/N and y/N + z/N^2 of a
voxel; the grid reproduces that bit for bit (tests/test_gpu_surface.py), it does not "fix" it.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L

_GRID_CHUNK = 1 << 22  # points per native launch (48 MB of coordinates in the workspace)


def sdf_grid_range(implicit_surface, volume_size, N, start, count, chunk=None, device=None):
    """SDF at flat voxel indices [start, start+count) of extract_mesh's N^3 grid -> device tensor [count].
    Inference only, like the reference (`.data`, mesh_util.py:104): no graph, also under grad mode."""
    N, start, count = int(N), int(start), int(count)
    if start < 0 or count < 0 or start + count > N ** 3:
        raise ValueError(f'voxel range [{start}, {start + count}) outside the {N}^3 grid')
    dev = torch.device(device) if device is not None else next(implicit_surface.parameters()).device
    if dev.type != 'cuda':
        raise RuntimeError('neurecon_amd: sdf_grid needs the model on a GPU (ROCm) device; the path is HIP-only')
    with torch.no_grad():
        return _grid_range(implicit_surface, volume_size, N, start, count, chunk, dev)


def _grid_range(implicit_surface, volume_size, N, start, count, chunk, dev):
    out = torch.empty(count, device=dev)
    if count == 0:
        return out
    chunk = min(int(chunk or _GRID_CHUNK), count)
    desc, packed = implicit_surface.nr_packed(dev)
    lib = L.lib()
    ws_bytes = lib.nr_sdf_grid_workspace_bytes(chunk)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = L.stream_of(dev)
    for j in range(0, count, chunk):
        n = min(chunk, count - j)
        L.check(lib.nr_sdf_grid(ctypes.byref(desc), L.ptr(packed), ctypes.c_double(float(volume_size)), N,
                                start + j, n, ctypes.c_void_p(out.data_ptr() + 4 * j), L.ptr(ws), ws_bytes, st))
    return out


def sdf_grid(implicit_surface, volume_size=2.0, N=512, chunk=None, device=None):
    """SDF of extract_mesh's N^3 grid (mesh_util.py:82-108) as a device tensor [N, N, N]."""
    N = int(N)
    return sdf_grid_range(implicit_surface, volume_size, N, 0, N ** 3, chunk, device).reshape(N, N, N)


def _vec3(x, name):
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    if v.size == 1:
        v = np.repeat(v, 3)
    if v.size != 3:
        raise ValueError(f'{name} must be a scalar or have 3 elements')
    return (ctypes.c_double * 3)(*v.tolist())


def marching_cubes(volume, level=0.0, spacing=(1., 1., 1.), origin=(0., 0., 0.), scale=None, offset=None):
    """Marching cubes of a device volume [n0, n1, n2] (every dim >= 2) at `level` -> (verts [V, 3] fp32,
    faces [F, 3] int32) device tensors: a welded indexed mesh, one vertex per grid edge with exactly one
    end below the level (`level` is compared as fp32), normals toward larger values.  A vertex at
    index-space coordinates idx lies at ((idx * spacing + origin) / scale) - offset, evaluated in float64
    (skimage's `spacing`, then the reference's transform, mesh_util.py:37-48).  Orders, the table and the
    exact definitions: neurecon_amd/csrc/nr_mcubes.hip.  Raises ValueError when nothing crosses the level."""
    L.require_gpu(volume, 'volume')
    if volume.dim() != 3 or min(volume.shape) < 2:
        raise ValueError(f'marching_cubes needs a 3-D volume with every dim >= 2, got {tuple(volume.shape)}')
    vol = volume.detach().to(torch.float32).contiguous()
    dev = vol.device
    n0, n1, n2 = (int(x) for x in vol.shape)
    sp, org = _vec3(spacing, 'spacing'), _vec3(origin, 'origin')
    off = _vec3(0.0 if offset is None else offset, 'offset')
    sc = ctypes.c_double(1.0 if scale is None else float(scale))
    lib = L.lib()
    lv = ctypes.c_float(float(level))
    with torch.cuda.device(dev):
        ws_bytes = lib.nr_mc_workspace_bytes(n0, n1, n2)
        if ws_bytes == 0:
            raise ValueError(f'marching_cubes: volume {tuple(vol.shape)} is too large')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        st = L.stream_of(dev)
        L.check(lib.nr_mc_count(L.ptr(vol), n0, n1, n2, lv, L.ptr(ws), ws_bytes, L.ptr(totals), st))
        V, F = (int(x) for x in totals.cpu())  # the one host read: 16 bytes
        if V == 0:
            raise ValueError('Surface level must be within volume data range.')
        if max(V, F) >= 2 ** 31:
            raise ValueError(f'marching_cubes: {V} vertices / {F} faces do not fit the int32 indices of a PLY')
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        L.check(lib.nr_mc_emit(L.ptr(vol), n0, n1, n2, lv, sp, org, sc, off, L.ptr(ws), ws_bytes, V, F,
                               L.ptr(verts), V, L.ptr(faces), F, st))
    return verts, faces


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(dtype, copy=False)


def write_ply(path, verts, faces):
    """Binary little-endian PLY of an indexed triangle mesh, the elements plyfile writes for the reference
    (mesh_util.py:59-74): vertex x/y/z as float, face vertex_indices as `list uchar int`.  verts [V, 3],
    faces [F, 3]: numpy arrays or tensors (device tensors are copied to the host)."""
    v, f = _host(verts, '<f4'), _host(faces, '<i4')
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f'write_ply needs verts [V, 3] and faces [F, 3], got {v.shape} and {f.shape}')
    header = (f'ply\nformat binary_little_endian 1.0\nelement vertex {v.shape[0]}\n'
              'property float x\nproperty float y\nproperty float z\n'
              f'element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n')
    rec = np.empty(f.shape[0], dtype=np.dtype([('n', 'u1'), ('vertex_indices', '<i4', (3,))]))  # packed: 13 bytes
    rec['n'] = 3
    rec['vertex_indices'] = f
    with open(path, 'wb') as out:
        out.write(header.encode('ascii'))
        np.ascontiguousarray(v).tofile(out)
        rec.tofile(out)


def _have_skimage_and_plyfile():
    try:
        import skimage.measure  # noqa: F401
        import plyfile  # noqa: F401
    except ImportError:
        return False
    return True


def _marching_mode(marching):
    if marching not in ('auto', 'native', 'skimage'):
        raise ValueError(f"marching must be 'auto', 'native' or 'skimage', got {marching!r}")
    if marching == 'auto':
        return 'skimage' if _have_skimage_and_plyfile() else 'native'
    return marching


def convert_sigma_samples_to_ply(input_3d_sigma_array, voxel_grid_origin, volume_size, ply_filename_out, level=5.0,
                                 offset=None, scale=None, marching='auto'):
    """mesh_util.py:13-79: marching cubes at `level` with spacing `volume_size`, + origin, / scale, - offset,
    written as a PLY.  marching='skimage': scikit-image + plyfile on a host array, as the reference;
    'native': `marching_cubes` + `write_ply` on a device tensor (a numpy array is uploaded to the current
    device); 'auto': skimage when both packages import, else native."""
    if _marching_mode(marching) == 'native':
        vol = input_3d_sigma_array
        if not isinstance(vol, torch.Tensor):
            if not torch.cuda.is_available():
                raise RuntimeError('neurecon_amd: native marching cubes needs a GPU (ROCm) device; the path is HIP-only')
            vol = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).cuda()
        verts, faces = marching_cubes(vol, level=level, spacing=volume_size, origin=voxel_grid_origin, scale=scale,
                                      offset=offset)
        write_ply(ply_filename_out, verts, faces)
        return
    try:
        import skimage.measure
        import plyfile
    except ImportError as e:
        raise ImportError("neurecon_amd.mesh_util: marching='skimage' needs scikit-image and plyfile; "
                          "marching='native' needs neither") from e
    if isinstance(input_3d_sigma_array, torch.Tensor):
        input_3d_sigma_array = input_3d_sigma_array.detach().cpu().numpy()
    verts, faces, _, _ = skimage.measure.marching_cubes(input_3d_sigma_array, level=level, spacing=volume_size)
    pts = np.asarray(verts, dtype=np.float64) + np.asarray(voxel_grid_origin, dtype=np.float64)[None]
    if scale is not None:
        pts = pts / scale
    if offset is not None:
        pts = pts - offset
    v = np.zeros((pts.shape[0],), dtype=[('x', 'f4'), ('y', 'f4'), ('z', 'f4')])
    v['x'], v['y'], v['z'] = pts[:, 0], pts[:, 1], pts[:, 2]
    f = np.zeros((faces.shape[0],), dtype=[('vertex_indices', 'i4', (3,))])
    f['vertex_indices'] = faces
    plyfile.PlyData([plyfile.PlyElement.describe(v, 'vertex'),
                     plyfile.PlyElement.describe(f, 'face')]).write(ply_filename_out)


def extract_mesh(implicit_surface, volume_size=2.0, level=0.0, N=512, filepath='./surface.ply', show_progress=True,
                 chunk=16 * 1024, marching='auto'):
    """mesh_util.py:82-112, its quirks included: the grid is sampled with step s / (N - 1) but handed to
    marching cubes with spacing s / N and origin -s / 2 (:84, :112).  Writes `filepath`, returns None.
    `chunk` is accepted for API compatibility (the device grid uses larger launches).  On the native
    marching path the volume stays on the device."""
    s = volume_size
    out = sdf_grid(implicit_surface, s, N)
    if _marching_mode(marching) != 'native':
        out = out.cpu().numpy()
    convert_sigma_samples_to_ply(out, [-s / 2., -s / 2., -s / 2.], [float(s) / N] * 3, filepath, level=level,
                                 marching=marching)

