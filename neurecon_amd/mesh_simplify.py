"""Making an extracted mesh smaller on the device: vertex clustering (libnrhip `nr_mesh_simplify_count` +
`nr_mesh_simplify_emit`, neurecon_amd/csrc/nr_meshsimplify.hip), the step users of `extract_mesh`'s PLY run in
MeshLab (clustering decimation) or Open3D (`simplify_vertex_clustering`) before they ship, view or evaluate it.

`simplify_mesh` merges all vertices in one cell of a uniform grid into one vertex and drops the faces that
collapse or repeat; every result is a pure function of the inputs (two runs are bit-identical; the rule in
full: the header comment of the kernel file, restated in tests/mesh_simplify_ref.py).  `snap_to_surface` puts
averaged vertices, which sit slightly inside a convex surface, back on the model's own zero set.

    python -m neurecon_amd.mesh_simplify in.ply out.ply --cell H [--position nearest]

reads a PLY, simplifies it, carries normals and colours across and prints one JSON line.
"""
import argparse
import ctypes
import json
import sys

import numpy as np
import torch

from . import _lib as L
from .mesh_util import _ATTR_CHUNK, _mesh_faces, read_ply, write_ply

MAX_CELLS = 1 << 27
_POSITIONS = {'average': 0, 'nearest': 1}


def _grid(verts, cell):
    """lo [3] float64 and dim [3] ints of the clustering grid: lo / hi the exact per-axis min / max of the
    vertices (the first host read: 24 bytes), dim = floor((hi - lo) / cell) + 1 in float64."""
    lohi = torch.stack([verts.amin(0), verts.amax(0)]).cpu().numpy().astype(np.float64)
    if not np.isfinite(lohi).all():
        raise ValueError('simplify_mesh: a vertex coordinate is not finite')
    lo, hi = lohi
    n = np.floor((hi - lo) / np.float64(cell)) + 1.0
    if not (n <= MAX_CELLS).all() or float(n[0]) * float(n[1]) * float(n[2]) > MAX_CELLS:
        raise ValueError(f'simplify_mesh: cell={cell} gives {n[0]:.0f} x {n[1]:.0f} x {n[2]:.0f} cells, more than '
                         f'2^27; use a larger cell')
    return lo, [int(x) for x in n]


def simplify_mesh(verts, faces=None, cell=None, position='average', return_clusters=False):
    """Vertex clustering on the device -> (verts' [K, 3] fp32, faces' [F', 3], index [K] int64), device tensors.
    verts [V, 3], faces [F, 3]: device tensors, or `verts` is the dict `read_ply` returns (uploaded to the current
    device).  cell: the cell size, in the units of the vertices.

    The grid starts at the per-axis minimum of the vertices.  Every occupied cell becomes one vertex, in
    ascending cell order (x fastest): position='average' puts it at the mean of the cell's vertices (in-cell
    fractions quantised to 2^-20 of a cell and summed as integers, so the mean does not depend on any order),
    position='nearest' at the input vertex nearest to that mean (a tie: the smaller index), unchanged, so it
    still lies on the iso-surface.  `index` names that input vertex in both modes: any per-vertex attribute
    follows with index_select, the `filter_mesh` contract.  A face stays iff its vertices fall into three
    different cells and no earlier face has the same three (in either orientation); the order of what stays is
    kept, F' = 0 is a valid result.  Vertices no face names any more stay: `filter_mesh(min_faces=1)` drops them.
    With `return_clusters` also vertex_cluster [V] int32 (the output vertex of each input vertex) and
    cluster_size [K] int32.
    Raises ValueError for a non-finite coordinate, a face naming a vertex outside [0, V), and a cell so small
    that the grid would have more than 2^27 cells."""
    if isinstance(verts, dict):
        mesh = verts
        verts, faces = mesh['verts'], (mesh['faces'] if faces is None else faces)
    if faces is None or cell is None:
        raise ValueError('simplify_mesh needs verts, faces and cell')
    if position not in _POSITIONS:
        raise ValueError(f"position must be 'average' or 'nearest', got {position!r}")
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise ValueError(f'simplify_mesh: cell must be finite and > 0, got {cell}')
    if not isinstance(verts, torch.Tensor):
        if not torch.cuda.is_available():
            raise RuntimeError('neurecon_amd: simplify_mesh needs a GPU (ROCm) device; the path is HIP-only')
        verts = torch.from_numpy(np.ascontiguousarray(verts)).cuda()
    L.require_gpu(verts, 'verts')
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f'verts must be [V, 3], got {tuple(verts.shape)}')
    dev = verts.device
    if not isinstance(faces, torch.Tensor):
        faces = torch.from_numpy(np.ascontiguousarray(faces))
    if faces.numel() == 0:
        faces = faces.reshape(-1, 3)
    faces = faces.to(dev)
    v = verts.detach().to(torch.float32).contiguous()
    f32, V = _mesh_faces(faces, v.shape[0])
    F = f32.shape[0]
    if F > 2 ** 30:
        raise ValueError(f'simplify_mesh: {F} faces are more than 2^30')
    if V == 0:
        if F:
            raise ValueError('faces name a vertex outside [0, 0)')
        e32 = torch.empty(0, dtype=torch.int32, device=dev)
        out = (v, faces.reshape(0, 3), torch.empty(0, dtype=torch.int64, device=dev))
        return out + (e32, e32.clone()) if return_clusters else out
    lib = L.lib()
    with torch.cuda.device(dev):
        lo, dim = _grid(v, cell)
        cells = dim[0] * dim[1] * dim[2]
        ws_bytes = lib.nr_mesh_simplify_workspace_bytes(V, F, cells)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        totals = torch.empty(3, dtype=torch.int64, device=dev)
        st = L.stream_of(dev)
        L.check(lib.nr_mesh_simplify_count(L.ptr(v), V, L.ptr(f32), F, cell, (ctypes.c_double * 3)(*lo.tolist()),
                                           (ctypes.c_int64 * 3)(*dim), L.ptr(ws), ws_bytes, L.ptr(totals), st))
        K, Fk, status = (int(x) for x in totals.cpu())  # the second host read: 24 bytes
        if status & 1:
            raise ValueError(f'faces name a vertex outside [0, {V})')
        if status & 4:
            raise ValueError('simplify_mesh: a vertex coordinate is not finite')
        if status:
            raise L.NrError(f'nr_mesh_simplify_count: status {status} (the probe cap of the duplicate table was reached)')
        verts_out = torch.empty((K, 3), dtype=torch.float32, device=dev)
        index = torch.empty(K, dtype=torch.int32, device=dev)
        size = torch.empty(K, dtype=torch.int32, device=dev)
        faces_out = torch.empty((Fk, 3), dtype=torch.int32, device=dev)
        vclu = torch.empty(V, dtype=torch.int32, device=dev)
        L.check(lib.nr_mesh_simplify_emit(L.ptr(v), V, L.ptr(f32), F, cells, _POSITIONS[position], L.ptr(ws), ws_bytes,
                                          K, Fk, L.ptr(verts_out), L.ptr(index), L.ptr(size), K, L.ptr(faces_out), Fk,
                                          L.ptr(vclu), st))
    out = (verts_out, faces_out.to(faces.dtype), index.long())
    return out + (vclu, size) if return_clusters else out


def snap_to_surface(implicit_surface, positions, iters=2, chunk=None):
    """`iters` Newton steps of `positions` [V, 3] (device) towards the zero set of `implicit_surface` (an
    ImplicitSurface, or a model that owns one): p <- p - sdf * nablas / max(|nablas|^2, 1e-12), with sdf and
    nablas from `forward_with_nablas` (the render path's net kernels, under no_grad, in chunks), every step in
    fp32: exactly
        sdf, nablas = surface.forward_with_nablas(p)[:2]
        p = p - sdf[:, None] * nablas / (nablas * nablas).sum(-1, keepdim=True).clamp_min(1e-12)
    An averaged vertex of `simplify_mesh` sits slightly inside a convex surface; this puts it back."""
    L.require_gpu(positions, 'positions')
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f'positions must be [V, 3], got {tuple(positions.shape)}')
    iters = int(iters)
    if iters < 0:
        raise ValueError(f'iters must be >= 0, got {iters}')
    surface = getattr(implicit_surface, 'implicit_surface', implicit_surface)
    chunk = int(chunk or _ATTR_CHUNK)
    p = positions.detach().float().contiguous()
    with torch.no_grad():
        for _ in range(iters):
            parts = []
            for j in range(0, p.shape[0], chunk):
                x = p[j:j + chunk]
                sdf, nablas = surface.forward_with_nablas(x)[:2]
                g2 = (nablas * nablas).sum(-1, keepdim=True).clamp_min(1e-12)
                parts.append(x - sdf.reshape(-1, 1) * nablas / g2)
            p = torch.cat(parts) if parts else p
    return p


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m neurecon_amd.mesh_simplify',
                                 description='Simplify a mesh (PLY) by vertex clustering on the device; normals and '
                                             'colours follow their vertices; prints one JSON line.')
    ap.add_argument('input', help='the extracted mesh (a PLY with vertex and face elements)')
    ap.add_argument('output', help='the simplified mesh (PLY)')
    ap.add_argument('--cell', type=float, required=True, help='cell size, in the units of the vertices')
    ap.add_argument('--position', choices=tuple(_POSITIONS), default='average')
    a = ap.parse_args(argv)
    mesh = read_ply(a.input)
    verts, faces, index = simplify_mesh(mesh, None, a.cell, position=a.position)
    idx = index.cpu().numpy()
    normals = None if mesh['normals'] is None else mesh['normals'][idx]
    colors = None if mesh['colors'] is None else mesh['colors'][idx]
    write_ply(a.output, verts, faces, normals=normals, colors=colors)
    print(json.dumps(dict(input=a.input, output=a.output, cell=a.cell, position=a.position,
                          verts_in=int(len(mesh['verts'])), faces_in=int(len(mesh['faces'])),
                          verts_out=int(verts.shape[0]), faces_out=int(faces.shape[0]))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
