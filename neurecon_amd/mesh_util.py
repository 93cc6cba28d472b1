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

Mesh finishing, all on the device and off by default: `mesh_components` / `filter_mesh` label connected
components and drop the small ones, keeping the order of what stays (libnrhip `nr_mesh_components`,
`nr_mesh_filter_count` + `nr_mesh_filter_emit`, neurecon_amd/csrc/nr_meshops.hip); `grid_sample_positions`
maps a marching-cubes vertex back to the point of space the sheared grid above sampled;
`vertex_attributes` evaluates normals (the SDF gradient) and colours (the radiance net, seen head-on) there
with the render path's net kernels; `write_ply` carries both.  `extract_mesh`'s keywords keep / min_faces /
vertex_normals / vertex_colors / coords chain them; `simplify` / `simplify_position` put
`neurecon_amd.mesh_simplify.simplify_mesh` (vertex clustering, neurecon_amd/csrc/nr_meshsimplify.hip) between
the filter and the attributes.

Looking at the result, also on the device: `read_ply` reads the PLY back (the layouts `write_ply` writes, and
the same elements as ASCII), `render_mesh` turns a mesh into a shaded frame, a depth map comparable with
`volume_render`'s depth, normals, barycentrics and a face-id map (libnrhip `nr_mesh_render`,
neurecon_amd/csrc/nr_meshrender.hip), standing in for the Open3D pass of tools/render_view.py:438-486.  It
samples exactly the pixels `rend_util.get_rays` shoots through, with the real principal point, so a mesh frame
overlays the volume-rendered frame of the same camera pixel for pixel.  A visibility-buffer rasteriser:
exact integer coverage on vertices snapped to 1/256 pixel, the nearest face by a 64-bit atomic minimum of
(depth bits, face index); every output is a pure function of the inputs.

Measuring the result is `neurecon_amd.mesh_metrics`: `evaluate_mesh` samples the mesh's surface, searches the
exact nearest neighbour against a ground-truth point cloud in both directions and returns accuracy,
completeness, Chamfer distance and precision / recall / F-score, on the device (libnrhip `nr_mesh_face_cdf`,
`nr_mesh_sample`, `nr_nn_build`, `nr_nn_query`); `read_ply_points` there reads the clouds `read_ply` refuses
for having no faces.
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


def _mesh_faces(faces, n_verts):
    L.require_gpu(faces, 'faces')
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'faces must be an integer tensor [F, 3], got {faces.dtype} {tuple(faces.shape)}')
    V = int(n_verts)
    if not 0 <= V < 2 ** 31 or faces.shape[0] >= 2 ** 31:
        raise ValueError(f'{V} vertices / {faces.shape[0]} faces do not fit int32 indices')
    if faces.dtype == torch.int64:  # an index beyond int32 must stay out of range after the cast
        faces = faces.clamp(-1, 2 ** 31 - 1)
    return faces.detach().to(torch.int32).contiguous(), V


def _components(faces, V):
    """-> labels [V], face_count [V] (int32, device), totals: host ints (components, largest label, its faces)"""
    dev = faces.device
    F = faces.shape[0]
    lib = L.lib()
    with torch.cuda.device(dev):
        ws_bytes = lib.nr_mesh_workspace_bytes(V, F)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        labels = torch.empty(V, dtype=torch.int32, device=dev)
        face_count = torch.empty(V, dtype=torch.int32, device=dev)
        totals = torch.empty(4, dtype=torch.int64, device=dev)
        L.check(lib.nr_mesh_components(L.ptr(faces), F, V, L.ptr(labels), L.ptr(face_count), L.ptr(totals), L.ptr(ws),
                                       ws_bytes, L.stream_of(dev)))
        n, largest, largest_faces, status = (int(x) for x in totals.cpu())  # the one host read: 32 bytes
    if status & 1:
        raise ValueError(f'faces name a vertex outside [0, {V})')
    if status:
        raise L.NrError(f'nr_mesh_components: status {status} (an iteration cap was reached)')
    return labels, face_count, (n, largest, largest_faces)


def mesh_components(faces, n_verts, return_largest=False):
    """Connected components of an indexed triangle mesh on the device (libnrhip `nr_mesh_components`):
    faces [F, 3] integer device tensor over vertices 0 .. n_verts-1 -> (labels [V] int32: the smallest vertex
    index of the vertex's component; face_count [V] int32: the component's faces, stored at its label, 0
    elsewhere; n_components: int).  A vertex no face names is a component with 0 faces.  With
    `return_largest` also (label, faces) of the component with most faces (a tie: the smaller label).
    Fully defined, so two runs are bit-identical; definitions: neurecon_amd/csrc/nr_meshops.hip.
    Raises ValueError when a face names a vertex outside [0, n_verts)."""
    faces, V = _mesh_faces(faces, n_verts)
    labels, face_count, (n, largest, largest_faces) = _components(faces, V)
    if return_largest:
        return labels, face_count, n, (largest, largest_faces)
    return labels, face_count, n


def filter_mesh(verts, faces, keep='all', min_faces=0, vertex_mask=None):
    """Drop parts of an indexed mesh on the device, keeping the order of what stays -> (verts', faces', index).
    keep='largest': only the connected component with most faces (a tie: the one with the smaller label);
    min_faces=k: only components with at least k faces; vertex_mask [V] bool: only these vertices (the three
    combine with `and`).  A face stays iff its three vertices stay.  `index` [V'] int64 maps new -> old vertex,
    ascending: verts' = verts[index], and any other per-vertex attribute follows with index_select.  With
    keep='all', min_faces=0 and no mask the inputs are returned untouched (index = arange).  Raises ValueError
    when nothing stays."""
    if keep not in ('all', 'largest'):
        raise ValueError(f"keep must be 'all' or 'largest', got {keep!r}")
    min_faces = int(min_faces)
    if min_faces < 0:
        raise ValueError(f'min_faces must be >= 0, got {min_faces}')
    L.require_gpu(verts, 'verts')
    if verts.dim() != 2:
        raise ValueError(f'verts must be [V, C], got {tuple(verts.shape)}')
    dev = verts.device
    if keep == 'all' and min_faces == 0 and vertex_mask is None:
        return verts, faces, torch.arange(verts.shape[0], device=dev)
    f32, V = _mesh_faces(faces, verts.shape[0])
    F = f32.shape[0]
    mask = None
    if keep == 'largest' or min_faces > 0:
        labels, face_count, (_, largest, _) = _components(f32, V)
        if keep == 'largest':
            mask = labels == largest
        if min_faces > 0:
            big = face_count.index_select(0, labels.long()) >= min_faces
            mask = big if mask is None else mask & big
    if vertex_mask is not None:
        vm = torch.as_tensor(vertex_mask, device=dev).reshape(-1) != 0
        if vm.shape[0] != V:
            raise ValueError(f'vertex_mask must have one entry per vertex ({V}), got {vm.shape[0]}')
        mask = vm if mask is None else mask & vm
    mask = mask.contiguous()
    lib = L.lib()
    with torch.cuda.device(dev):
        ws_bytes = lib.nr_mesh_workspace_bytes(V, F)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        st = L.stream_of(dev)
        L.check(lib.nr_mesh_filter_count(L.ptr(f32), F, V, L.ptr(mask), L.ptr(ws), ws_bytes, L.ptr(totals), st))
        Vk, Fk = (int(x) for x in totals.cpu())  # the one host read: 16 bytes
        if Vk == 0:
            raise ValueError('filter_mesh: no vertex is left')
        vsrc = torch.empty(Vk, dtype=torch.int32, device=dev)
        faces_out = torch.empty((Fk, 3), dtype=torch.int32, device=dev)
        L.check(lib.nr_mesh_filter_emit(L.ptr(f32), F, V, L.ptr(mask), L.ptr(ws), ws_bytes, Vk, Fk, L.ptr(vsrc), Vk,
                                        L.ptr(faces_out), Fk, st))
    index = vsrc.long()
    return verts.index_select(0, index), faces_out.to(faces.dtype), index


def grid_sample_positions(idx, volume_size, N):
    """Index-space coordinates (a, b, c) of extract_mesh's N^3 grid [..., 3] -> the point of space the grid
    sampled there, fp32 [..., 3]: ((a + b/N + c/N^2) step - s/2, (b + c/N) step - s/2, c step - s/2) with
    step = s / (N - 1), i.e. the reference's sheared lattice (mesh_util.py:92-100), not the s / N lattice its
    writer assumes (:112).  At integer indices the float64 value is the reference's own, operation for
    operation (flat index i = (a N + b) N + c; i % N, (i / N) % N, ((i / N) / N) % N; * step + origin); between
    them the map is affine, so it is evaluated as the multilinear blend of the eight surrounding lattice
    points in float64 (weights 0 and 1 at integer indices: exact) and rounded to fp32 once.  A marching-cubes
    vertex at parameter t on a grid edge thus lands at parameter t between the two sampled points.  Index-space
    vertices come from `marching_cubes(vol, level)` with unit spacing and zero origin.  Plain torch."""
    N = int(N)
    if N < 2:
        raise ValueError(f'grid_sample_positions needs N >= 2, got {N}')
    idx = torch.as_tensor(idx)
    if idx.shape[-1] != 3:
        raise ValueError(f'idx must be [..., 3], got {tuple(idx.shape)}')
    s = volume_size
    step, origin = s / (N - 1), -s / 2.
    p = idx.to(torch.float64)
    lo = p.floor().clamp(0, N - 2)
    t = p - lo

    n = torch.full_like(p[..., 0], N)  # a tensor: a device division by a scalar multiplies by its reciprocal

    def lattice(a, b, c):  # mesh_util.py:87-100 at integer a, b, c
        i = (a * N + b) * N + c
        x2 = torch.fmod(i, n)
        x1 = torch.fmod(i / n, n)
        x0 = torch.fmod((i / n) / n, n)
        return torch.stack([x0 * step + origin, x1 * step + origin, x2 * step + origin], -1)

    out = torch.zeros_like(p)
    for corner in range(8):
        d = [(corner >> 2) & 1, (corner >> 1) & 1, corner & 1]
        w = torch.ones_like(p[..., 0])
        for q in range(3):
            w = w * (t[..., q] if d[q] else 1.0 - t[..., q])
        out = out + w[..., None] * lattice(lo[..., 0] + d[0], lo[..., 1] + d[1], lo[..., 2] + d[2])
    return out.to(torch.float32)


_ATTR_CHUNK = 1 << 20  # points per net launch of vertex_attributes


def vertex_attributes(model, positions, normals=True, colors=False, chunk=None):
    """Per-vertex normals and colours of a surface at `positions` [V, 3] (device) -> (normals or None, colors or
    None), fp32 [V, 3].  `model`: a NeuS / VolSDF / UNISURF model, or an ImplicitSurface (normals only).
    Normals: F.normalize(nablas, dim=-1) of implicit_surface.forward_with_nablas: the SDF gradient, toward
    larger values like the face orientation.  Colours: model.forward(positions, view_dirs=-normals)[0]: the
    surface seen head-on.  Runs on the render path's net kernels under no_grad, in chunks; nothing else is
    computed here."""
    L.require_gpu(positions, 'positions')
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f'positions must be [V, 3], got {tuple(positions.shape)}')
    surface = getattr(model, 'implicit_surface', model)
    if colors and surface is model:
        raise ValueError('vertex_attributes: colors need a model with a radiance net, not an ImplicitSurface')
    if not (normals or colors):
        return None, None
    chunk = int(chunk or _ATTR_CHUNK)
    pos = positions.detach().float().contiguous()
    ns, cs = [], []
    with torch.no_grad():
        for j in range(0, pos.shape[0], chunk):
            x = pos[j:j + chunk]
            n = torch.nn.functional.normalize(surface.forward_with_nablas(x)[1], dim=-1)
            ns.append(n)
            if colors:
                cs.append(model.forward(x, view_dirs=-n)[0])
    empty = pos.new_zeros((0, 3))
    n_all = torch.cat(ns) if ns else empty
    c_all = (torch.cat(cs) if cs else empty) if colors else None
    return (n_all if normals else None), c_all


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(dtype, copy=False)


def _host_colors(colors):
    """uint8 as given; float: floor(clamp(c, 0, 1) * 255 + 0.5), evaluated in float64 (NaN -> 0)"""
    if isinstance(colors, torch.Tensor):
        colors = colors.detach().cpu().numpy()
    c = np.asarray(colors)
    if c.dtype == np.uint8:
        return c
    if not np.issubdtype(c.dtype, np.floating):
        raise ValueError(f'write_ply: colors must be uint8 or float, got {c.dtype}')
    c = np.nan_to_num(c.astype(np.float64), nan=0.0)
    return np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY of an indexed triangle mesh, the elements plyfile writes for the reference
    (mesh_util.py:59-74): vertex x/y/z as float, face vertex_indices as `list uchar int`.  verts [V, 3],
    faces [F, 3]: numpy arrays or tensors (device tensors are copied to the host).  normals [V, 3] add
    `property float nx/ny/nz` after x y z, colors [V, 3] then `property uchar red/green/blue` (uint8 as given,
    float quantised as floor(clamp(c, 0, 1) * 255 + 0.5)); with neither, the layout above, byte for byte."""
    v, f = _host(verts, '<f4'), _host(faces, '<i4')
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f'write_ply needs verts [V, 3] and faces [F, 3], got {v.shape} and {f.shape}')
    fields, props = [('xyz', '<f4', (3,))], 'property float x\nproperty float y\nproperty float z\n'
    n = c = None
    if normals is not None:
        n = _host(normals, '<f4')
        fields.append(('n', '<f4', (3,)))
        props += 'property float nx\nproperty float ny\nproperty float nz\n'
    if colors is not None:
        c = _host_colors(colors)
        fields.append(('rgb', 'u1', (3,)))
        props += 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    for name, a in (('normals', n), ('colors', c)):
        if a is not None and a.shape != v.shape:
            raise ValueError(f'write_ply needs {name} {v.shape} like verts, got {a.shape}')
    header = (f'ply\nformat binary_little_endian 1.0\nelement vertex {v.shape[0]}\n' + props +
              f'element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n')
    rec = np.empty(f.shape[0], dtype=np.dtype([('n', 'u1'), ('vertex_indices', '<i4', (3,))]))  # packed: 13 bytes
    rec['n'] = 3
    rec['vertex_indices'] = f
    with open(path, 'wb') as out:
        out.write(header.encode('ascii'))
        if n is None and c is None:
            np.ascontiguousarray(v).tofile(out)
        else:
            vrec = np.empty(v.shape[0], dtype=np.dtype(fields))  # packed: 12 / 24 / 15 / 27 bytes
            vrec['xyz'] = v
            if n is not None:
                vrec['n'] = n
            if c is not None:
                vrec['rgb'] = c
            vrec.tofile(out)
        rec.tofile(out)


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}


def _ply_header(data, path):
    """-> (format, [(element, count, [property tuples])], offset of the body)"""
    if not data.startswith(b'ply'):
        raise ValueError(f'read_ply: {path} is not a PLY file')
    end = data.find(b'end_header')
    nl = data.find(b'\n', end)
    if end < 0 or nl < 0:
        raise ValueError(f'read_ply: {path} has no end_header line')
    fmt, elements = None, []
    for line in data[:end].decode('ascii', 'replace').splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format' and len(tok) >= 2:
            fmt = tok[1]
        elif tok[0] == 'element' and len(tok) == 3:
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == 'property' and elements and len(tok) in (3, 5):
            if any(t not in _PLY_TYPES for t in tok[1:-1] if t != 'list') or (len(tok) == 5) != (tok[1] == 'list'):
                raise ValueError(f'read_ply: {path}: unknown property type in {line!r}')
            elements[-1][2].append(tuple(tok[1:]))
        else:
            raise ValueError(f'read_ply: {path}: cannot parse header line {line!r}')
    if fmt == 'binary_big_endian':
        raise ValueError(f'read_ply: {path} is big-endian; only binary_little_endian and ascii are read')
    if fmt not in ('binary_little_endian', 'ascii'):
        raise ValueError(f'read_ply: {path}: unknown format {fmt!r}')
    return fmt, elements, nl + 1


def read_ply(path):
    """Read an indexed triangle mesh from a PLY file -> dict(verts [V, 3] float32, faces [F, 3] int32,
    normals [V, 3] float32 or None, colors [V, 3] uint8 or None), numpy arrays.  Reads what `write_ply` writes
    (binary little-endian; 12, 24, 15 or 27 bytes per vertex) and the same elements as ASCII PLY: an element
    `vertex` with scalar properties, of which x y z, nx ny nz (all three, else None) and red green blue (all
    three, else None) are kept and every other one is skipped by its declared size, then an element `face`
    with one list property of vertex indices.  Raises ValueError for a face list that is not all triangles,
    a big-endian file, a truncated file and anything else it cannot parse."""
    with open(path, 'rb') as f:
        data = f.read()
    fmt, elements, pos = _ply_header(data, path)
    if [e[0] for e in elements] != ['vertex', 'face']:
        raise ValueError(f'read_ply: {path}: needs the elements vertex and face, in that order, got '
                         f'{[e[0] for e in elements]}')
    (_, V, vprops), (_, F, fprops) = elements
    if any(p[0] == 'list' for p in vprops) or len(fprops) != 1 or fprops[0][0] != 'list':
        raise ValueError(f'read_ply: {path}: needs scalar vertex properties and one list property per face')
    names = [p[1] for p in vprops]
    if len(set(names)) != len(names) or not all(k in names for k in 'xyz'):
        raise ValueError(f'read_ply: {path}: vertex properties {names} must be distinct and hold x, y, z')
    _, count_t, index_t, _ = fprops[0]
    if fmt == 'ascii':
        tok = data[pos:].split()
        nv = V * len(names)
        if len(tok) < nv + 4 * F:
            if len(tok) > nv and F > 0 and tok[nv] != b'3':
                raise ValueError(f'read_ply: {path}: only triangle faces are read')
            raise ValueError(f'read_ply: {path} is truncated')
        try:
            vtab = np.array(tok[:nv], dtype=np.float64).reshape(V, len(names))
            ftab = np.array(tok[nv:nv + 4 * F], dtype=np.int64).reshape(F, 4)
        except ValueError as e:
            raise ValueError(f'read_ply: {path}: bad number in the body') from e
        if (ftab[:, 0] != 3).any():
            raise ValueError(f'read_ply: {path}: only triangle faces are read')
        if len(tok) != nv + 4 * F:
            raise ValueError(f'read_ply: {path}: {len(tok) - nv - 4 * F} extra values after the faces')
        col = {n: vtab[:, k].astype(_PLY_TYPES[vprops[k][0]]) for k, n in enumerate(names)}
        idx = ftab[:, 1:]
    else:
        vdt = np.dtype([(n, '<' + _PLY_TYPES[p[0]]) for n, p in zip(names, vprops)])
        fdt = np.dtype([('n', '<' + _PLY_TYPES[count_t]), ('v', '<' + _PLY_TYPES[index_t], (3,))])
        body = len(data) - pos - V * vdt.itemsize
        if body < 0:
            raise ValueError(f'read_ply: {path} is truncated')
        if F > 0 and body >= fdt['n'].itemsize and int(np.frombuffer(data, fdt['n'], 1, pos + V * vdt.itemsize)[0]) != 3:
            raise ValueError(f'read_ply: {path}: only triangle faces are read')
        if body < F * fdt.itemsize:
            raise ValueError(f'read_ply: {path} is truncated')
        vrec = np.frombuffer(data, vdt, V, pos)
        frec = np.frombuffer(data, fdt, F, pos + V * vdt.itemsize)
        if (frec['n'] != 3).any():
            raise ValueError(f'read_ply: {path}: only triangle faces are read')
        if body != F * fdt.itemsize:
            raise ValueError(f'read_ply: {path}: {body - F * fdt.itemsize} extra bytes after the faces')
        col = {n: vrec[n] for n in names}
        idx = frec['v']

    def cols(keys, dtype):
        return np.stack([col[k] for k in keys], 1).astype(dtype) if all(k in col for k in keys) else None
    rgb = ('red', 'green', 'blue')
    colors = cols(rgb, np.uint8) if all(k in col and col[k].dtype == np.uint8 for k in rgb) else cols(rgb, np.float32)
    if idx.size and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
        raise ValueError(f'read_ply: {path}: a vertex index does not fit int32')
    return dict(verts=cols('xyz', np.float32), faces=np.ascontiguousarray(idx).astype(np.int32),
                normals=cols(('nx', 'ny', 'nz'), np.float32), colors=colors)


_LARGE_THRESHOLD = 64  # pixel samples in a face's box above which a workgroup rasterises it


def _dev_array(a, dtype, dev, name, V=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[1] != 3 or (V is not None and t.shape[0] != V):
        raise ValueError(f'render_mesh: {name} must be [{"V" if V is None else V}, 3], got {tuple(t.shape)}')
    return t.detach().to(device=dev, dtype=dtype).contiguous()


def render_mesh(verts, faces=None, c2w=None, intrinsics=None, H=None, W=None, normals=None, colors=None, near=1e-4,
                ambient=0.3, base_color=(0.7, 0.7, 0.7), background=1.0, large_threshold=None):
    """Render an indexed triangle mesh on the device (libnrhip `nr_mesh_render`, neurecon_amd/csrc/
    nr_meshrender.hip) through the pixels `rend_util.get_rays(c2w, intrinsics, H, W)` shoots its rays through:
    integer pixel coordinates and the real principal point, so the frame overlays the volume-rendered frame
    of the same camera pixel for pixel.  Stands in for the Open3D pass of tools/render_view.py:438-486.

    verts [V, 3], faces [F, 3], normals / colors [V, 3] or None: tensors or arrays -- or `verts` is the dict
    `read_ply` returns (its normals and colours are used unless given here).  colors: uint8, or float in
    [0, 1].  c2w [4, 4] or [B, 4, 4] (a loop over the cameras; outputs are stacked), intrinsics [4, 4] / [3, 3]
    (or one per camera).  The camera is taken in float64 as given; world -> camera is np.linalg.inv of the
    float64 c2w, on the host.  get_rays works on the fp32 camera: hand both the same fp32 values.

    -> dict of device tensors: rgb [H, W, 3] = base (ambient + (1 - ambient) |n . d|), `background` at a miss;
    depth [H, W]: distance along the normalised ray (volume_render's depth), 0 at a miss; depth_z [H, W]:
    camera-space z; normal [H, W, 3]: world space, unit (the blend of the vertex normals, else the face
    normal); mask [H, W] bool; face_id [H, W] int32, -1 at a miss; bary [H, W, 3]: perspective-correct weights
    of the face's three vertices; n_clipped: int64 scalar tensor, faces dropped whole because a vertex lies
    closer than `near`, is not finite or projects beyond 2^20 pixels (there is no polygon clipping);
    n_degenerate: faces skipped for zero snapped area or an index outside [0, V); n_large: faces that took the
    workgroup-per-face path (both int64 scalar tensors).
    Faces are two-sided; the nearest wins, a depth tie goes to the smaller face index; every output is a
    pure function of the inputs.  large_threshold: box size (pixel samples) above which a face takes the
    workgroup-per-face path; the result does not depend on it."""
    if isinstance(verts, dict):
        mesh = verts
        verts = mesh['verts']
        faces = mesh['faces'] if faces is None else faces
        normals = mesh.get('normals') if normals is None else normals
        colors = mesh.get('colors') if colors is None else colors
    if faces is None or c2w is None or intrinsics is None or H is None or W is None:
        raise ValueError('render_mesh needs verts, faces, c2w, intrinsics, H and W')
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError(f'render_mesh: needs H, W > 0 and H * W < 2^31, got {H} x {W}')
    dev = next((t.device for t in (verts, faces, c2w) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError('neurecon_amd: render_mesh needs a GPU (ROCm) device; the path is HIP-only')
        dev = torch.device('cuda', torch.cuda.current_device())
    v = _dev_array(verts, torch.float32, dev, 'verts')
    V = v.shape[0]
    ft = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
    f, _ = _mesh_faces(ft.reshape(-1, 3).to(dev) if ft.numel() == 0 else ft.to(dev), V)  # no face: any shape
    F = f.shape[0]
    if F >= 2 ** 31 - 1:
        raise ValueError(f'render_mesh: {F} faces do not fit the 31-bit face index')
    n = None if normals is None else _dev_array(normals, torch.float32, dev, 'normals', V)
    c = None
    if colors is not None:
        ct = colors if isinstance(colors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(colors))
        c = _dev_array(ct, torch.float32, dev, 'colors', V)
        if ct.dtype == torch.uint8:
            c = c / torch.full_like(c, 255.0)  # a true division (by a scalar it would multiply by 1 / 255)

    def host64(x):
        return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)
    poses, Ks = host64(c2w), host64(intrinsics)
    batched = poses.ndim == 3
    if poses.shape[-2:] != (4, 4) or poses.ndim not in (2, 3):
        raise ValueError(f'render_mesh: c2w must be [4, 4] or [B, 4, 4], got {poses.shape}')
    poses = poses.reshape(-1, 4, 4)
    if Ks.ndim not in (2, 3) or Ks.shape[-2:] not in ((4, 4), (3, 3)):
        raise ValueError(f'render_mesh: intrinsics must be [4, 4] or [3, 3] (or one per camera), got {Ks.shape}')
    Ks = np.broadcast_to(Ks.reshape(-1, *Ks.shape[-2:]), (poses.shape[0], *Ks.shape[-2:]))
    lt = _LARGE_THRESHOLD if large_threshold is None else int(large_threshold)
    if lt < 0:
        raise ValueError(f'render_mesh: large_threshold must be >= 0, got {lt}')
    base, bg = _vec3(base_color, 'base_color'), _vec3(background, 'background')
    lib = L.lib()
    frames = []
    with torch.cuda.device(dev):
        ws_bytes = lib.nr_mesh_render_workspace_bytes(V, F, H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = L.stream_of(dev)
        for pose, K in zip(poses, Ks):
            w2c = np.linalg.inv(pose)
            out = dict(rgb=torch.empty((H, W, 3), device=dev), depth=torch.empty((H, W), device=dev),
                       normal=torch.empty((H, W, 3), device=dev),
                       mask=torch.empty((H, W), dtype=torch.uint8, device=dev),
                       face_id=torch.empty((H, W), dtype=torch.int32, device=dev),
                       bary=torch.empty((H, W, 3), device=dev), depth_z=torch.empty((H, W), device=dev))
            counters = torch.empty(3, dtype=torch.int64, device=dev)
            a = L.NrMeshRenderArgs()
            a.verts, a.faces = v.data_ptr() if V else None, f.data_ptr() if F else None
            a.normals = None if n is None or V == 0 else n.data_ptr()
            a.colors = None if c is None or V == 0 else c.data_ptr()
            a.V, a.F, a.H, a.W = V, F, H, W
            a.w2c[:] = w2c[:3].reshape(-1).tolist()
            a.m[:] = pose[:3, :3].reshape(-1).tolist()
            a.fx, a.fy, a.cx, a.cy, a.skew = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                                              float(K[0, 1]))
            a.near, a.large_threshold, a.ambient = float(near), lt, float(ambient)
            a.base[:], a.background[:] = list(base), list(bg)
            a.rgb, a.depth, a.normal = out['rgb'].data_ptr(), out['depth'].data_ptr(), out['normal'].data_ptr()
            a.mask, a.face_id, a.bary = out['mask'].data_ptr(), out['face_id'].data_ptr(), out['bary'].data_ptr()
            a.zdepth, a.counters = out['depth_z'].data_ptr(), counters.data_ptr()
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
            L.check(lib.nr_mesh_render(ctypes.byref(a), st))
            out['mask'] = out['mask'].view(torch.bool)
            out['n_clipped'], out['n_degenerate'], out['n_large'] = counters[0], counters[1], counters[2]
            frames.append(out)
    if not batched:
        return frames[0]
    return {k: torch.stack([fr[k] for fr in frames]) for k in frames[0]}


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
                 chunk=16 * 1024, marching='auto', keep='all', min_faces=0, vertex_normals=False,
                 vertex_colors=False, model=None, coords='reference', simplify=None, simplify_position='average'):
    """mesh_util.py:82-112, its quirks included: the grid is sampled with step s / (N - 1) but handed to
    marching cubes with spacing s / N and origin -s / 2 (:84, :112).  Writes `filepath`, returns None.
    `chunk` is accepted for API compatibility (the device grid uses larger launches).  On the native
    marching path the volume stays on the device.

    Mesh finishing (native marching only; with all of these at their defaults the call is the one above):
    keep='largest' / min_faces=k drop connected components (`filter_mesh`); vertex_normals / vertex_colors
    add per-vertex nx ny nz / red green blue (`vertex_attributes`; colours need `model`, the NeuS / VolSDF /
    UNISURF model that owns `implicit_surface`); coords='sampled' writes each vertex at the point of space
    the grid sampled (`grid_sample_positions`: the un-sheared, correctly scaled mesh) instead of the
    reference's s / N lattice.  Attributes are always evaluated at the sampled positions, whichever
    coordinates are written.  Order: marching cubes, filter, attributes on the surviving vertices.

    simplify=h (a cell size in world units, native marching only) runs `mesh_simplify.simplify_mesh` on the
    written vertices after the component filter and before the attributes; simplify_position 'average' (the
    cell's mean) or 'nearest' (the input vertex nearest to it).  With coords='sampled' the vertices live in
    the model's space: given `model=` and 'average' they are first put back on the model's zero set by
    `mesh_simplify.snap_to_surface`, and the attributes are evaluated at the written vertices.  With
    coords='reference' (the sheared lattice) the attributes are evaluated at the sampled position of each
    vertex's source vertex (`simplify_mesh`'s index), which lies on the iso-surface."""
    s = volume_size
    mode = _marching_mode(marching)
    if coords not in ('reference', 'sampled'):
        raise ValueError(f"coords must be 'reference' or 'sampled', got {coords!r}")
    options = dict(keep=keep != 'all', min_faces=min_faces != 0, vertex_normals=bool(vertex_normals),
                   vertex_colors=bool(vertex_colors), coords=coords != 'reference', simplify=simplify is not None)
    used = [k for k, v in options.items() if v]
    if not used:
        out = sdf_grid(implicit_surface, s, N)
        if mode != 'native':
            out = out.cpu().numpy()
        convert_sigma_samples_to_ply(out, [-s / 2., -s / 2., -s / 2.], [float(s) / N] * 3, filepath, level=level,
                                     marching=marching)
        return
    if mode != 'native':
        raise ValueError(f"extract_mesh: {used[0]} needs marching='native' (marching={marching!r} resolved to the "
                         'scikit-image path, which has no mesh finishing)')
    if vertex_colors and model is None:
        raise ValueError('extract_mesh: vertex_colors=True needs model= (the model whose radiance net gives the colours)')
    vol = sdf_grid(implicit_surface, s, N)
    idx, faces = marching_cubes(vol, level=level)  # index space: unit spacing, zero origin
    if coords == 'reference':  # the vertices of the default call, bit for bit
        verts, _ = marching_cubes(vol, level=level, spacing=[float(s) / N] * 3, origin=[-s / 2., -s / 2., -s / 2.])
    else:
        verts = grid_sample_positions(idx, s, N)
    del vol
    verts, faces, index = filter_mesh(verts, faces, keep=keep, min_faces=min_faces)
    if simplify is not None:
        from .mesh_simplify import simplify_mesh, snap_to_surface
        verts, faces, src = simplify_mesh(verts, faces, simplify, position=simplify_position)
        index = index.index_select(0, src)  # new vertex -> its source vertex among marching cubes'
        if coords == 'sampled' and simplify_position == 'average' and model is not None:
            verts = snap_to_surface(implicit_surface, verts)
    normals = colors = None
    if vertex_normals or vertex_colors:
        pos = verts if coords == 'sampled' else grid_sample_positions(idx.index_select(0, index), s, N)
        normals, colors = vertex_attributes(model if vertex_colors else implicit_surface, pos,
                                            normals=vertex_normals, colors=vertex_colors)
    write_ply(filepath, verts, faces, normals=normals, colors=colors)

