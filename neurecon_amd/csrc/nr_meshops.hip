// neurecon_amd — mesh finishing on the device: connected components of an indexed triangle mesh
// and order-preserving filtering (what users of the reference do to extract_mesh's PLY in a separate
// mesh tool: "keep the largest component", "drop components under k faces").
// Input: faces int32 [F, 3] over vertices 0 .. V-1 (device).  Everything is integer: no result
// depends on the schedule, two runs are bit-identical.
//
// Definitions
//   * Two vertices are in one COMPONENT iff a chain of faces connects them (consecutive faces share
//     a vertex).  A vertex no face names is a component of its own with 0 faces.
//   * labels[v] = the smallest vertex index in v's component.  A component's label is that index.
//   * face_count[l] = number of faces of the component with label l; 0 at every v that is no label.
//     A face belongs to the component of its vertices (all three are in one, by definition).
//   * totals = {components, label of the largest, its face count, status}.  Largest = most faces, a
//     tie goes to the smaller label.  V == 0: {0, -1, 0, status}.
//   * Degenerate faces (a repeated vertex) and repeated faces are allowed and counted.
//   * A face with an index outside [0, V) is INVALID: never dereferenced, skipped (it joins nothing
//     and is counted nowhere), and status bit 0 is set.  Status bit 1: a loop reached its iteration
//     cap (cannot happen, see below); the labels are then not to be used.
//   * Filter.  A vertex is KEPT iff vkeep[v] != 0.  A face is kept iff its three indices are valid and
//     name kept vertices.  Kept vertices and kept faces keep their relative order; vsrc[new] = old
//     vertex index (ascending); faces_out holds the kept faces with new indices.
//
// Labelling: a lock-free union-find in `parent` (one int32 per vertex, parent[v] <= v, roots have
// parent[v] == v).
//   init      parent[v] = v, face_count[v] = 0, the header words = 0.
//   hook      one thread per face: unite(a, b), unite(b, c).  unite finds both roots, then hooks the
//             HIGHER root under the lower: atomicCAS(&parent[hi], hi, lo) (device scope).  A failed
//             CAS returns the parent some other thread gave hi meanwhile; the find continues from
//             that returned value.  While finding, a path is halved with atomicMin(&parent[x],
//             grandparent): a parent only ever decreases, and only to a vertex of the same component.
//   flatten   (next launch: the kernel boundary makes every hook visible) labels[v] = root of v.
//             All unions are done, so every component is one tree and its root, having the smallest
//             index of the tree, is the component's smallest vertex.
//   count     one thread per face: face_count[labels[a]] += 1, integer atomicAdd, one add per distinct
//             label of a wave.
//   reduce    one thread per vertex: roots counted (one 64-bit atomicAdd per wave); the largest by a
//             64-bit atomicMax of (face_count << 32) | ~label, one per wave.
//   finish    one thread decodes the header into totals.
// Why hook cannot hang.  gfx950 has 8 XCDs with private L2s, so a load of parent[] may return an old
// value while other workgroups hook.  That is harmless: an old parent is still a vertex of the same
// component with a smaller index, so following it stays inside the component and moves strictly
// down.  No decision is taken on a loaded value alone: a root is only hooked by the CAS, which is
// executed at memory, and when it fails the loop goes on from the value the CAS returned (< hi),
// never from a re-read.  Both walkers of a unite therefore only ever move to strictly smaller
// indices, whatever any other workgroup does or whenever its stores become visible: a unite ends
// after at most 2 V steps, and no loop waits for another workgroup.  The cap of 2 V + 64 steps is
// there so that a mistake in this argument ends as status bit 1, never as a hang.
//
// Filter passes (the two-phase shape of nr_mc_count / nr_mc_emit)
//   count     per-workgroup (256 items) sums of kept vertices and of kept faces from wave ballots;
//   scan      exclusive scan of both arrays in place, one workgroup each (independent, no hand-off);
//             totals {V', F'}.  The workspace then carries what nr_mesh_filter_emit needs.
//   (host)    the caller reads the totals (16 bytes) and allocates vsrc / faces_out.
//   emit      verts: rank = workgroup base + earlier waves + earlier lanes -> vsrc, and new[v] (-1 for a
//             dropped vertex); faces (next launch): the same rank for faces, indices through new[].
// Workspace: 256 header bytes + 4 bytes per vertex (parent, reused as new[]) + 4 bytes per 256
// vertices + 4 bytes per 256 faces, each array rounded up to 256 bytes.
#include "nr_meshcommon.h"

namespace nr {

constexpr int kMoWG = 256;       // items per workgroup (4 waves)
constexpr int kMoScanWG = 1024;  // threads of a scan workgroup

enum { kMoBadIndex = 1, kMoCapReached = 2 };

struct MoHeader {  // the first 256 bytes of the workspace
  unsigned long long n_components, best;
  unsigned status;
};

__device__ __forceinline__ int mo_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x as far as this thread can see (a stale root is caught by the caller's CAS); halves the path.
// Every step moves to a strictly smaller index.
__device__ __forceinline__ bool mo_find(int* __restrict__ parent, int& x, int64_t& steps, int64_t cap) {
  for (;;) {
    const int p = mo_load(parent + x);
    if (p == x) return true;
    const int g = mo_load(parent + p);
    if (g != p) atomicMin(parent + x, g);
    x = g;
    if (++steps > cap) return false;
  }
}

__device__ __forceinline__ bool mo_unite(int* __restrict__ parent, int u, int v, int64_t cap) {
  int64_t steps = 0;
  for (;;) {
    if (!mo_find(parent, u, steps, cap) || !mo_find(parent, v, steps, cap)) return false;
    if (u == v) return true;
    const int hi = u > v ? u : v, lo = u > v ? v : u;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return true;
    u = old;  // hi has a parent already: old < hi, fresh from memory
    v = lo;
    if (++steps > cap) return false;
  }
}

__global__ __launch_bounds__(kMoWG) void mo_init(int* __restrict__ parent, int* __restrict__ face_count, int64_t V,
                                                 MoHeader* __restrict__ hdr) {
  const int64_t v = (int64_t)blockIdx.x * kMoWG + threadIdx.x;
  if (v < V) {
    parent[v] = (int)v;
    face_count[v] = 0;
  }
  if (v == 0) {
    hdr->n_components = 0;
    hdr->best = 0;
    hdr->status = 0;
  }
}

__global__ __launch_bounds__(kMoWG) void mo_hook(const int* __restrict__ faces, int64_t F, int64_t V,
                                                 int* __restrict__ parent, MoHeader* __restrict__ hdr, int64_t cap) {
  const int64_t f = (int64_t)blockIdx.x * kMoWG + threadIdx.x;
  if (f >= F) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (!face_valid(a, b, c, V)) {
    atomicOr(&hdr->status, (unsigned)kMoBadIndex);
    return;
  }
  if (!mo_unite(parent, a, b, cap) || !mo_unite(parent, b, c, cap)) atomicOr(&hdr->status, (unsigned)kMoCapReached);
}

__global__ __launch_bounds__(kMoWG) void mo_flatten(const int* __restrict__ parent, int* __restrict__ labels,
                                                    int64_t V, MoHeader* __restrict__ hdr) {
  const int64_t v = (int64_t)blockIdx.x * kMoWG + threadIdx.x;
  if (v >= V) return;
  int x = (int)v;
  int64_t steps = 0;
  for (int p = parent[x]; p != x; p = parent[x]) {  // p < x: at most V steps
    x = p;
    if (++steps > V) {
      atomicOr(&hdr->status, (unsigned)kMoCapReached);
      break;
    }
  }
  labels[v] = x;
}

__global__ __launch_bounds__(kMoWG) void mo_count(const int* __restrict__ faces, int64_t F, int64_t V,
                                                  const int* __restrict__ labels, int* __restrict__ face_count) {
  const int64_t f = (int64_t)blockIdx.x * kMoWG + threadIdx.x;
  int label = -1;
  if (f < F) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (face_valid(a, b, c, V)) label = labels[a];
  }
  // one add per distinct label of the wave (at most 64 rounds, all inside the wave)
  const int lane = threadIdx.x & 63;
  bool todo = label >= 0;
  for (;;) {
    const unsigned long long m = __ballot(todo);
    if (!m) break;
    const int leader = __ffsll(m) - 1;
    const int l = __shfl(label, leader);
    const bool mine = todo && label == l;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) atomicAdd(face_count + l, __popcll(same));
    if (mine) todo = false;
  }
}

__global__ __launch_bounds__(kMoWG) void mo_reduce(const int* __restrict__ labels, const int* __restrict__ face_count,
                                                   int64_t V, MoHeader* __restrict__ hdr) {
  const int64_t v = (int64_t)blockIdx.x * kMoWG + threadIdx.x;
  const bool root = v < V && labels[v] == (int)v;
  unsigned long long key = 0;
  if (root) key = ((unsigned long long)(unsigned)face_count[v] << 32) | (unsigned)~(unsigned)v;
  const unsigned long long m = __ballot(root);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(key >> 32), off), lo = __shfl_xor((unsigned)key, off);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && m) {
    atomicAdd(&hdr->n_components, (unsigned long long)__popcll(m));
    atomicMax(&hdr->best, key);
  }
}

__global__ void mo_finish(const MoHeader* __restrict__ hdr, int64_t* __restrict__ totals) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long best = hdr->best;  // 0 only when there is no vertex: ~label has bit 31 set
  totals[0] = (int64_t)hdr->n_components;
  totals[1] = best ? (int64_t)(int)~(unsigned)best : -1;
  totals[2] = (int64_t)(best >> 32);
  totals[3] = (int64_t)hdr->status;
}

__device__ __forceinline__ bool mo_face_kept(const int* __restrict__ faces, int64_t f, int64_t F, int64_t V,
                                             const uint8_t* __restrict__ vkeep, int& a, int& b, int& c) {
  if (f >= F) return false;
  a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  return face_valid(a, b, c, V) && vkeep[a] && vkeep[b] && vkeep[c];
}

// workgroups [0, nbv): vertices; [nbv, nbv + nbf): faces
__global__ __launch_bounds__(kMoWG) void mo_filter_count(const int* __restrict__ faces, int64_t F, int64_t V,
                                                         const uint8_t* __restrict__ vkeep, int64_t nbv,
                                                         int* __restrict__ wv, int* __restrict__ wf) {
  __shared__ int lds[kMoWG / 64];
  const bool is_face = blockIdx.x >= nbv;
  const int64_t blk = is_face ? blockIdx.x - nbv : blockIdx.x;
  const int64_t i = blk * kMoWG + threadIdx.x;
  bool keep;
  if (is_face) {
    int a, b, c;
    keep = mo_face_kept(faces, i, F, V, vkeep, a, b, c);
  } else {
    keep = i < V && vkeep[i];
  }
  int all;
  wave_prefix<kMoWG>(__popcll(__ballot(keep)), lds, all);
  if (threadIdx.x == 0) (is_face ? wf : wv)[blk] = all;
}

// in place: w[b] = items kept before workgroup b; *total = all of them.  Workgroup 0 scans wv into
// totals[0], workgroup 1 scans wf into totals[1]; thread t owns a contiguous strip.
__global__ __launch_bounds__(kMoScanWG) void mo_scan(int* __restrict__ wv, int64_t nbv, int* __restrict__ wf,
                                                     int64_t nbf, int64_t* __restrict__ totals) {
  __shared__ int64_t s[kMoScanWG];
  int* __restrict__ w = blockIdx.x == 0 ? wv : wf;
  const int64_t nb = blockIdx.x == 0 ? nbv : nbf;
  const int64_t all = strip_scan<kMoScanWG>(nb, s, [&](int64_t q) { return (int64_t)w[q]; },
                                            [&](int64_t q, int64_t e) { w[q] = (int)e; });
  if (threadIdx.x == kMoScanWG - 1) totals[blockIdx.x] = all;
}

__global__ __launch_bounds__(kMoWG) void mo_emit_verts(const uint8_t* __restrict__ vkeep, int64_t V,
                                                       const int* __restrict__ wv, int* __restrict__ vnew,
                                                       int* __restrict__ vsrc, int64_t Vk) {
  __shared__ int lds[kMoWG / 64];
  const int64_t v = (int64_t)blockIdx.x * kMoWG + threadIdx.x;
  const bool keep = v < V && vkeep[v];
  const unsigned long long m = __ballot(keep);
  const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
  int all;
  const int64_t slot = (int64_t)wv[blockIdx.x] + wave_prefix<kMoWG>(__popcll(m), lds, all) + __popcll(m & lt);
  if (v >= V) return;
  const bool store = keep && slot < Vk;
  vnew[v] = store ? (int)slot : -1;
  if (store) vsrc[slot] = (int)v;
}

__global__ __launch_bounds__(kMoWG) void mo_emit_faces(const int* __restrict__ faces, int64_t F, int64_t V,
                                                       const uint8_t* __restrict__ vkeep, const int* __restrict__ wf,
                                                       const int* __restrict__ vnew, int* __restrict__ faces_out,
                                                       int64_t Fk) {
  __shared__ int lds[kMoWG / 64];
  const int64_t f = (int64_t)blockIdx.x * kMoWG + threadIdx.x;
  int a = 0, b = 0, c = 0;
  const bool keep = mo_face_kept(faces, f, F, V, vkeep, a, b, c);
  const unsigned long long m = __ballot(keep);
  const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
  int all;
  const int64_t slot = (int64_t)wf[blockIdx.x] + wave_prefix<kMoWG>(__popcll(m), lds, all) + __popcll(m & lt);
  if (!keep || slot >= Fk) return;
  faces_out[3 * slot] = vnew[a];
  faces_out[3 * slot + 1] = vnew[b];
  faces_out[3 * slot + 2] = vnew[c];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct MoPlan {
  int64_t nbv, nbf;
  size_t o_idx, o_wv, o_wf, total;
};

static bool mo_plan(int64_t V, int64_t F, MoPlan& p) {
  if (V < 0 || F < 0 || V > INT32_MAX || F > INT32_MAX) return false;
  p.nbv = (V + kMoWG - 1) / kMoWG;
  p.nbf = (F + kMoWG - 1) / kMoWG;
  size_t o = 256;  // MoHeader
  p.o_idx = o; o += a256((size_t)V * 4);
  p.o_wv = o; o += a256((size_t)p.nbv * 4);
  p.o_wf = o; o += a256((size_t)p.nbf * 4);
  p.total = o;
  return true;
}

}  // namespace nr

using namespace nr;

extern "C" {

size_t nr_mesh_workspace_bytes(int64_t V, int64_t F) {
  MoPlan pl;
  return mo_plan(V, F, pl) ? pl.total : 0;
}

int nr_mesh_components(const int32_t* faces, int64_t F, int64_t V, int32_t* labels, int32_t* face_count,
                       int64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  MoPlan pl;
  NR_REQUIRE(mo_plan(V, F, pl), NR_ERR_ARG, "nr_mesh_components: vertex and face counts must be in [0, INT32_MAX]");
  NR_REQUIRE((faces || F == 0) && ((labels && face_count) || V == 0) && totals, NR_ERR_ARG,
             "nr_mesh_components: null argument");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_mesh_components: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  MoHeader* hdr = (MoHeader*)ws;
  int* parent = (int*)(ws + pl.o_idx);
  const unsigned gv = (unsigned)(pl.nbv > 0 ? pl.nbv : 1), gf = (unsigned)pl.nbf;
  NR_LAUNCH("mesh_init", (double)V, mo_init, dim3(gv), dim3(kMoWG), st, parent, face_count, V, hdr);
  if (F > 0) NR_LAUNCH("mesh_hook", (double)F, mo_hook, dim3(gf), dim3(kMoWG), st, faces, F, V, parent, hdr, 2 * V + 64);
  if (V > 0) NR_LAUNCH("mesh_flatten", (double)V, mo_flatten, dim3(gv), dim3(kMoWG), st, parent, labels, V, hdr);
  if (F > 0 && V > 0)
    NR_LAUNCH("mesh_count", (double)F, mo_count, dim3(gf), dim3(kMoWG), st, faces, F, V, labels, face_count);
  if (V > 0) NR_LAUNCH("mesh_reduce", (double)V, mo_reduce, dim3(gv), dim3(kMoWG), st, labels, face_count, V, hdr);
  hipLaunchKernelGGL(mo_finish, dim3(1), dim3(64), 0, st, hdr, totals);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int nr_mesh_filter_count(const int32_t* faces, int64_t F, int64_t V, const uint8_t* vkeep, void* workspace,
                         size_t workspace_bytes, int64_t* totals, void* stream) {
  MoPlan pl;
  NR_REQUIRE(mo_plan(V, F, pl), NR_ERR_ARG, "nr_mesh_filter_count: vertex and face counts must be in [0, INT32_MAX]");
  NR_REQUIRE((faces || F == 0) && (vkeep || V == 0) && totals, NR_ERR_ARG, "nr_mesh_filter_count: null argument");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_mesh_filter_count: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int *wv = (int*)(ws + pl.o_wv), *wf = (int*)(ws + pl.o_wf);
  if (pl.nbv + pl.nbf > 0)
    NR_LAUNCH("mesh_filter_count", (double)(V + F), mo_filter_count, dim3((unsigned)(pl.nbv + pl.nbf)), dim3(kMoWG), st,
              faces, F, V, vkeep, pl.nbv, wv, wf);
  NR_LAUNCH("mesh_scan", (double)(pl.nbv + pl.nbf), mo_scan, dim3(2), dim3(kMoScanWG), st, wv, pl.nbv, wf, pl.nbf, totals);
  return NR_OK;
}

int nr_mesh_filter_emit(const int32_t* faces, int64_t F, int64_t V, const uint8_t* vkeep, void* workspace,
                        size_t workspace_bytes, int64_t Vk, int64_t Fk, int32_t* vsrc, int64_t vsrc_cap,
                        int32_t* faces_out, int64_t faces_cap, void* stream) {
  MoPlan pl;
  NR_REQUIRE(mo_plan(V, F, pl), NR_ERR_ARG, "nr_mesh_filter_emit: vertex and face counts must be in [0, INT32_MAX]");
  NR_REQUIRE((faces || F == 0) && (vkeep || V == 0), NR_ERR_ARG, "nr_mesh_filter_emit: null argument");
  NR_REQUIRE(Vk >= 0 && Fk >= 0 && Vk <= V && Fk <= F, NR_ERR_ARG,
             "nr_mesh_filter_emit: kept counts must be in [0, V] and [0, F]");
  NR_REQUIRE(vsrc_cap >= Vk && faces_cap >= Fk, NR_ERR_ARG,
             "nr_mesh_filter_emit: output capacity below the kept vertex / face count");
  NR_REQUIRE((vsrc || Vk == 0) && (faces_out || Fk == 0), NR_ERR_ARG, "nr_mesh_filter_emit: null output");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_mesh_filter_emit: workspace too small");
  if (Vk == 0 && Fk == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* vnew = (int*)(ws + pl.o_idx);
  const int *wv = (const int*)(ws + pl.o_wv), *wf = (const int*)(ws + pl.o_wf);
  if (V > 0)
    NR_LAUNCH("mesh_emit_verts", (double)V, mo_emit_verts, dim3((unsigned)pl.nbv), dim3(kMoWG), st, vkeep, V, wv, vnew,
              vsrc, Vk);
  if (Fk > 0)
    NR_LAUNCH("mesh_emit_faces", (double)F, mo_emit_faces, dim3((unsigned)pl.nbf), dim3(kMoWG), st, faces, F, V, vkeep,
              wf, vnew, faces_out, Fk);
  return NR_OK;
}

}  // extern "C"
