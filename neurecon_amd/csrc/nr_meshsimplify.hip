// neurecon_amd — simplifying an indexed triangle mesh on the device by vertex clustering: the step users of
// extract_mesh's PLY run in a separate tool (MeshLab's clustering decimation, Open3D's
// simplify_vertex_clustering) before they ship, view or evaluate the mesh.  All vertices of one cell of a
// uniform grid become one vertex; faces that collapse or repeat are dropped.
//
// Every output is a pure function of the inputs: integers, and float64 arithmetic with each operation rounded
// on its own (dsub / ddiv / dmul / dadd of nr_common.h and the contract(off) pragma below).  Two runs are
// bit-identical; tests/mesh_simplify_ref.py restates the rule in numpy, operation for operation, and the
// device is compared to it by equality.
//
// Inputs.  verts fp32 [V, 3], faces int32 [F, 3], h > 0 the cell size, lo[3] the grid origin (float64), dim[3]
// the cells per axis (>= 1 each, dim_x dim_y dim_z <= 2^27).  The Python wrapper takes lo / hi as the exact
// per-axis minimum / maximum of the vertices and dim_a = floor((hi_a - lo_a) / h) + 1 in float64.
//
// The rule
//   Cell.     per axis a, with x_a widened:  t_a = (x_a - lo_a) / h,  c_a = clamp(floor(t_a), 0, dim_a - 1),
//             cell = (c_z dim_y + c_y) dim_x + c_x.
//   Cluster.  A cluster is an occupied cell; its id is the rank of its cell among the occupied cells in
//             ascending `cell`.  Output vertex k is cluster k, whether a face names it or not.
//   Mean.     f_a = clamp(t_a - c_a, 0, 1),  q_a = min(floor(f_a 2^20), 2^20 - 1) as an integer;  S_a = sum of q_a
//             and n = the count over the cluster's vertices (integer atomics: n < 2^31, S < 2^51, the sums do
//             not depend on their order);  m_a = lo_a + (c_a + S_a / (n 2^20)) h, evaluated in this order:
//             n 2^20 (exact), the quotient, + c_a, x h, + lo_a.
//   Representative.  d2 = ((dx dx) + (dy dy)) + (dz dz), dx = x - m_x (widened x).  The source vertex of a
//             cluster is its member with the smallest (d2, index): a 64-bit atomicMin on the bits of the
//             non-negative double (they order like the values), then, in the next launch, an atomicMin on the
//             index among the members whose d2 has exactly those bits (the same device function computes d2
//             in both launches).
//   Position. position 0 ('average'): vertex k = (float) m.  position 1 ('nearest'): vertex k = verts[index[k]],
//             unchanged.  index [K] is written in both modes: per-vertex attributes follow with index_select.
//   Faces.    (A, B, C) = the clusters of a face's vertices.  Face f SURVIVES iff A, B, C are pairwise distinct
//             and no face g < f with pairwise distinct clusters has the same unordered set {A, B, C} (the
//             opposite orientation counts as the same).  Survivors are written in ascending f as (A, B, C) in
//             the original order.  F' = 0 is a valid result.
//   A face naming a vertex outside [0, V) is never dereferenced: it does not survive and status bit 0 is
//   set.  A vertex with a non-finite coordinate sets status bit 2 (NaN clamps to cell 0 / f = 0: nothing is
//   read or written out of range, the outputs are not to be used).
//
// Passes (nr_mesh_simplify_count), each a launch of its own: no workgroup waits for another anywhere.
//   bin        one thread per vertex: its cell -> vclu[v]; cellid[cell] = 1 (every writer stores the same value).
//   cell scan  the three-launch form: per-workgroup (256 cells) counts of occupied cells from wave ballots,
//              one workgroup strip_scans them (total = K), then cellid[cell] = rank (-1 if empty) and
//              clcell[rank] = cell.
//   accumulate one thread per vertex: k = cellid[cell] -> vclu[v]; n[k] += 1, S_a[k] += q_a (integer atomics).
//   mean       one thread per cluster: m[k].
//   dist, pick one thread per vertex each: the two atomicMin rounds above.
//   face hash  duplicate removal, expected linear in F whatever the mesh: an open-addressing table of T slots,
//              T = the power of two >= max(2 F, 64), a slot holding a face index (-1: empty).  A face with
//              pairwise distinct clusters starts at the slot its sorted key hashes to and walks on (linear
//              probing): an empty slot is claimed by atomicCAS; a slot holding a face of the same key gets an
//              atomicMin with f; a slot of another key is passed.  Slots are never released and a slot's key
//              never changes (only faces of its key lower it), and all faces of a key walk the same slots and
//              stop at the first that is empty or theirs, so a key lives in exactly one slot, which ends
//              holding the smallest face index of the key.  Which slot that is depends on the schedule; the
//              kept set does not.  fslot[f] remembers the slot.
//   face count per-workgroup counts of the faces f with table[fslot[f]] == f; the same scan gives F'.
//   finish     totals = {K, F', status}: the one host read.
// Why the probe loop ends.  At most F keys are inserted into T >= 2 F slots, so every walk meets an empty slot
// or its own key within T steps; the loop is bounded by T and a walk that exhausts it sets status bit 1 (cannot
// happen), as does a slot value outside [0, F).  A mistake in this argument ends as NrError, never as a hang.
// Emit (nr_mesh_simplify_emit): verts' / index / cluster_size per cluster, vertex_cluster per vertex, and the
// surviving faces compacted in order (rank = workgroup base + earlier waves + earlier lanes).
//
// Workspace, every array rounded up to 256 bytes, Kmax = min(V, cells), T as above:
//   256 (header) + 4 cells (cellid) + 4 ceil(cells / 256) + 4 V (vclu) + Kmax (4 clcell + 4 n + 24 S + 8 best
//   + 4 index + 24 mean) + 4 T (table) + 4 F (fslot) + 4 ceil(F / 256).
// Limits: 0 <= V <= INT32_MAX, 0 <= F <= 2^30, 1 <= cells <= 2^27.
#include "nr_meshcommon.h"

#pragma clang fp contract(off)  // no a * b + c -> fma anywhere in this file (header comment)

namespace nr {

constexpr int kMsWG = 256;       // items per workgroup (4 waves)
constexpr int kMsScanWG = 1024;  // threads of the scan workgroup
constexpr int64_t kMsMaxCells = (int64_t)1 << 27;
constexpr int64_t kMsMaxFaces = (int64_t)1 << 30;
constexpr double kMsQ = 1048576.0;  // 2^20 steps per cell and axis
constexpr unsigned kMsNoSlot = 0xFFFFFFFFu;

enum { kMsBadIndex = 1, kMsCapReached = 2, kMsNonFinite = 4 };

struct MsHeader {  // the first 256 bytes of the workspace
  long long K, Fp;
  unsigned status;
};

struct MsGrid {
  double h, lo[3];
  int dim[3];
};

// NaN -> a
__device__ __forceinline__ double ms_clamp(double x, double a, double b) { return x >= a ? (x <= b ? x : b) : a; }

// the cell coordinates and the quantised in-cell fractions of one vertex
__device__ __forceinline__ void ms_locate(const float* __restrict__ p, const MsGrid& g, int c[3], long long q[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t = ddiv(dsub((double)p[a], g.lo[a]), g.h);
    const double cf = ms_clamp(floor(t), 0.0, (double)(g.dim[a] - 1));
    const double f = ms_clamp(dsub(t, cf), 0.0, 1.0);
    const double qf = floor(dmul(f, kMsQ));
    c[a] = (int)cf;
    q[a] = qf < kMsQ - 1.0 ? (long long)qf : (long long)kMsQ - 1;
  }
}

__device__ __forceinline__ unsigned long long ms_d2_bits(const float* __restrict__ p, const double* __restrict__ m) {
  const double dx = dsub((double)p[0], m[0]), dy = dsub((double)p[1], m[1]), dz = dsub((double)p[2], m[2]);
  const double d2 = dadd(dadd(dmul(dx, dx), dmul(dy, dy)), dmul(dz, dz));
  return (unsigned long long)__double_as_longlong(d2);
}

__global__ __launch_bounds__(kMsWG) void ms_init(MsHeader* __restrict__ hdr, int64_t kmax, int* __restrict__ cnt,
                                                 unsigned long long* __restrict__ sum,
                                                 unsigned long long* __restrict__ best, int* __restrict__ bidx) {
  const int64_t k = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (k == 0) {
    hdr->K = 0;
    hdr->Fp = 0;
    hdr->status = 0;
  }
  if (k >= kmax) return;
  cnt[k] = 0;
  sum[3 * k] = sum[3 * k + 1] = sum[3 * k + 2] = 0;
  best[k] = ~0ull;
  bidx[k] = INT32_MAX;
}

__global__ __launch_bounds__(kMsWG) void ms_bin(const float* __restrict__ verts, int64_t V, MsGrid g,
                                                int* __restrict__ vclu, int* __restrict__ cellid,
                                                MsHeader* __restrict__ hdr) {
  const int64_t v = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (v >= V) return;
  const float* p = verts + 3 * v;
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) atomicOr(&hdr->status, (unsigned)kMsNonFinite);
  int c[3];
  long long q[3];
  ms_locate(p, g, c, q);
  const int cell = (c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0];  // < 2^27
  vclu[v] = cell;
  cellid[cell] = 1;
}

__global__ __launch_bounds__(kMsWG) void ms_cell_count(const int* __restrict__ cellid, int64_t cells,
                                                       int* __restrict__ wc) {
  __shared__ int lds[kMsWG / 64];
  const int64_t i = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  const bool occ = i < cells && cellid[i] != 0;
  int all;
  wave_prefix<kMsWG>(__popcll(__ballot(occ)), lds, all);
  if (threadIdx.x == 0) wc[blockIdx.x] = all;
}

// in place: w[b] = items counted before workgroup b; *total = all of them.  One workgroup.
__global__ __launch_bounds__(kMsScanWG) void ms_scan(int* __restrict__ w, int64_t nb, long long* __restrict__ total) {
  __shared__ int64_t s[kMsScanWG];
  const int64_t all = strip_scan<kMsScanWG>(nb, s, [&](int64_t q) { return (int64_t)w[q]; },
                                            [&](int64_t q, int64_t e) { w[q] = (int)e; });
  if (threadIdx.x == kMsScanWG - 1) *total = all;
}

__global__ __launch_bounds__(kMsWG) void ms_cell_apply(int* __restrict__ cellid, int64_t cells,
                                                       const int* __restrict__ wc, int* __restrict__ clcell,
                                                       int64_t kmax) {
  __shared__ int lds[kMsWG / 64];
  const int64_t i = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  const bool occ = i < cells && cellid[i] != 0;
  const unsigned long long m = __ballot(occ);
  const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
  int all;
  const int64_t rank = (int64_t)wc[blockIdx.x] + wave_prefix<kMsWG>(__popcll(m), lds, all) + __popcll(m & lt);
  if (i >= cells) return;
  const bool store = occ && rank < kmax;  // rank < K <= kmax: always
  cellid[i] = store ? (int)rank : -1;
  if (store) clcell[rank] = (int)i;
}

__global__ __launch_bounds__(kMsWG) void ms_accum(const float* __restrict__ verts, int64_t V, MsGrid g,
                                                  int* __restrict__ vclu, const int* __restrict__ cellid,
                                                  int* __restrict__ cnt, unsigned long long* __restrict__ sum) {
  const int64_t v = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (v >= V) return;
  int c[3];
  long long q[3];
  ms_locate(verts + 3 * v, g, c, q);
  const int k = cellid[vclu[v]];  // >= 0: ms_bin marked this cell
  vclu[v] = k;
  if (k < 0) return;  // cannot happen
  atomicAdd(cnt + k, 1);
#pragma unroll
  for (int a = 0; a < 3; ++a) atomicAdd(sum + 3 * (int64_t)k + a, (unsigned long long)q[a]);
}

__global__ __launch_bounds__(kMsWG) void ms_mean(const MsHeader* __restrict__ hdr, MsGrid g,
                                                 const int* __restrict__ clcell, const int* __restrict__ cnt,
                                                 const unsigned long long* __restrict__ sum, double* __restrict__ mean) {
  const int64_t k = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (k >= hdr->K) return;
  const int cell = clcell[k];
  const int c[3] = {cell % g.dim[0], (cell / g.dim[0]) % g.dim[1], cell / (g.dim[0] * g.dim[1])};
  const double den = dmul((double)cnt[k], kMsQ);
#pragma unroll
  for (int a = 0; a < 3; ++a)
    mean[3 * k + a] = dadd(g.lo[a], dmul(dadd((double)c[a], ddiv((double)sum[3 * k + a], den)), g.h));
}

__global__ __launch_bounds__(kMsWG) void ms_dist(const float* __restrict__ verts, int64_t V,
                                                 const int* __restrict__ vclu, const double* __restrict__ mean,
                                                 unsigned long long* __restrict__ best) {
  const int64_t v = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (v >= V) return;
  const int k = vclu[v];
  if (k < 0) return;
  const unsigned long long bits = ms_d2_bits(verts + 3 * v, mean + 3 * (int64_t)k);
  if (bits < __hip_atomic_load(best + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(best + k, bits);
}

__global__ __launch_bounds__(kMsWG) void ms_pick(const float* __restrict__ verts, int64_t V,
                                                 const int* __restrict__ vclu, const double* __restrict__ mean,
                                                 const unsigned long long* __restrict__ best, int* __restrict__ bidx) {
  const int64_t v = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (v >= V) return;
  const int k = vclu[v];
  if (k < 0) return;
  if (ms_d2_bits(verts + 3 * v, mean + 3 * (int64_t)k) == best[k]) atomicMin(bidx + k, (int)v);
}

// the sorted clusters of face f; false unless its indices are valid and the clusters pairwise distinct
__device__ __forceinline__ bool ms_face_key(const int* __restrict__ faces, int64_t f, int64_t V,
                                            const int* __restrict__ vclu, int key[3], bool& valid) {
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  valid = face_valid(a, b, c, V);
  if (!valid) return false;
  const int A = vclu[a], B = vclu[b], C = vclu[c];
  const int lo = min(A, min(B, C)), hi = max(A, max(B, C));
  key[0] = lo, key[1] = A ^ B ^ C ^ lo ^ hi, key[2] = hi;
  return key[0] != key[1] && key[1] != key[2];
}

__global__ __launch_bounds__(kMsWG) void ms_face_hash(const int* __restrict__ faces, int64_t F, int64_t V,
                                                      const int* __restrict__ vclu, int* __restrict__ table, int64_t T,
                                                      unsigned* __restrict__ fslot, MsHeader* __restrict__ hdr) {
  const int64_t f = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (f >= F) return;
  int key[3];
  bool valid;
  fslot[f] = kMsNoSlot;
  if (!ms_face_key(faces, f, V, vclu, key, valid)) {
    if (!valid) atomicOr(&hdr->status, (unsigned)kMsBadIndex);
    return;
  }
  unsigned long long x = ((unsigned long long)(unsigned)key[0] << 32 | (unsigned)key[1]) * 0x9E3779B97F4A7C15ull;
  x ^= (unsigned long long)(unsigned)key[2] * 0xC2B2AE3D27D4EB4Full;
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  int64_t s = (int64_t)(x & (unsigned long long)(T - 1));
  for (int64_t probe = 0; probe < T; ++probe, s = (s + 1) & (T - 1)) {
    const int cur = atomicCAS(table + s, -1, (int)f);
    if (cur == -1) {  // claimed
      fslot[f] = (unsigned)s;
      return;
    }
    if (cur < 0 || cur >= F) break;  // cannot happen: slots hold -1 or an inserted face
    int other[3] = {-1, -1, -1};
    bool ov;
    ms_face_key(faces, cur, V, vclu, other, ov);  // an inserted face: valid and distinct
    if (other[0] == key[0] && other[1] == key[1] && other[2] == key[2]) {
      if (f < cur) atomicMin(table + s, (int)f);  // the slot only ever decreases: nothing to do when cur < f
      fslot[f] = (unsigned)s;
      return;
    }
  }
  atomicOr(&hdr->status, (unsigned)kMsCapReached);
}

__device__ __forceinline__ bool ms_face_kept(const unsigned* __restrict__ fslot, const int* __restrict__ table,
                                             int64_t f, int64_t F, int64_t T) {
  if (f >= F) return false;
  const unsigned s = fslot[f];
  return s != kMsNoSlot && (int64_t)s < T && table[s] == (int)f;
}

__global__ __launch_bounds__(kMsWG) void ms_face_count(const unsigned* __restrict__ fslot, const int* __restrict__ table,
                                                       int64_t F, int64_t T, int* __restrict__ wf) {
  __shared__ int lds[kMsWG / 64];
  const int64_t f = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  int all;
  wave_prefix<kMsWG>(__popcll(__ballot(ms_face_kept(fslot, table, f, F, T))), lds, all);
  if (threadIdx.x == 0) wf[blockIdx.x] = all;
}

__global__ void ms_finish(const MsHeader* __restrict__ hdr, int64_t* __restrict__ totals) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  totals[0] = (int64_t)hdr->K;
  totals[1] = (int64_t)hdr->Fp;
  totals[2] = (int64_t)hdr->status;
}

__global__ __launch_bounds__(kMsWG) void ms_emit_verts(const MsHeader* __restrict__ hdr, const float* __restrict__ verts,
                                                       int64_t V, int64_t K, int position,
                                                       const double* __restrict__ mean, const int* __restrict__ cnt,
                                                       const int* __restrict__ bidx, float* __restrict__ verts_out,
                                                       int* __restrict__ index, int* __restrict__ cluster_size) {
  const int64_t k = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (k >= K || k >= hdr->K) return;
  const int src = bidx[k];
  const bool ok = src >= 0 && src < V;  // always: a cluster has a member
  index[k] = ok ? src : -1;
  cluster_size[k] = cnt[k];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    verts_out[3 * k + a] = position == 1 ? (ok ? verts[3 * (int64_t)src + a] : 0.0f) : (float)mean[3 * k + a];
}

__global__ __launch_bounds__(kMsWG) void ms_emit_clusters(const int* __restrict__ vclu, int64_t V,
                                                          int* __restrict__ vertex_cluster) {
  const int64_t v = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (v < V) vertex_cluster[v] = vclu[v];
}

__global__ __launch_bounds__(kMsWG) void ms_emit_faces(const int* __restrict__ faces, int64_t F, int64_t V,
                                                       const int* __restrict__ vclu, const unsigned* __restrict__ fslot,
                                                       const int* __restrict__ table, int64_t T,
                                                       const int* __restrict__ wf, int* __restrict__ faces_out,
                                                       int64_t Fk) {
  __shared__ int lds[kMsWG / 64];
  const int64_t f = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  const bool keep = ms_face_kept(fslot, table, f, F, T);
  const unsigned long long m = __ballot(keep);
  const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
  int all;
  const int64_t slot = (int64_t)wf[blockIdx.x] + wave_prefix<kMsWG>(__popcll(m), lds, all) + __popcll(m & lt);
  if (!keep || slot >= Fk) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (!face_valid(a, b, c, V)) return;  // cannot happen: only valid faces are given a slot
  faces_out[3 * slot] = vclu[a];
  faces_out[3 * slot + 1] = vclu[b];
  faces_out[3 * slot + 2] = vclu[c];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct MsPlan {
  int64_t nbv, nbf, nbc, nbk, kmax, T;
  size_t o_cellid, o_wc, o_vclu, o_clcell, o_cnt, o_sum, o_best, o_bidx, o_mean, o_table, o_fslot, o_wf, total;
};

static bool ms_plan(int64_t V, int64_t F, int64_t cells, MsPlan& p) {
  if (V < 0 || F < 0 || V > INT32_MAX || F > kMsMaxFaces || cells < 1 || cells > kMsMaxCells) return false;
  p.nbv = (V + kMsWG - 1) / kMsWG;
  p.nbf = (F + kMsWG - 1) / kMsWG;
  p.nbc = (cells + kMsWG - 1) / kMsWG;
  p.kmax = V < cells ? V : cells;
  p.nbk = (p.kmax + kMsWG - 1) / kMsWG;
  p.T = 64;
  while (p.T < 2 * F) p.T <<= 1;
  const size_t k = (size_t)p.kmax;
  size_t o = 256;  // MsHeader
  p.o_cellid = o; o += a256((size_t)cells * 4);
  p.o_wc = o; o += a256((size_t)p.nbc * 4);
  p.o_vclu = o; o += a256((size_t)V * 4);
  p.o_clcell = o; o += a256(k * 4);
  p.o_cnt = o; o += a256(k * 4);
  p.o_sum = o; o += a256(k * 24);
  p.o_best = o; o += a256(k * 8);
  p.o_bidx = o; o += a256(k * 4);
  p.o_mean = o; o += a256(k * 24);
  p.o_table = o; o += a256((size_t)p.T * 4);
  p.o_fslot = o; o += a256((size_t)F * 4);
  p.o_wf = o; o += a256((size_t)p.nbf * 4);
  p.total = o;
  return true;
}

}  // namespace nr

using namespace nr;

extern "C" {

size_t nr_mesh_simplify_workspace_bytes(int64_t V, int64_t F, int64_t cells) {
  MsPlan pl;
  return ms_plan(V, F, cells, pl) ? pl.total : 0;
}

int nr_mesh_simplify_count(const float* verts, int64_t V, const int32_t* faces, int64_t F, double h, const double* lo,
                           const int64_t* dim, void* workspace, size_t workspace_bytes, int64_t* totals, void* stream) {
  NR_REQUIRE(h > 0.0 && h - h == 0.0, NR_ERR_ARG, "nr_mesh_simplify_count: the cell size h must be finite and > 0");
  NR_REQUIRE(lo && dim && totals, NR_ERR_ARG, "nr_mesh_simplify_count: null argument");
  NR_REQUIRE(lo[0] - lo[0] == 0.0 && lo[1] - lo[1] == 0.0 && lo[2] - lo[2] == 0.0, NR_ERR_ARG,
             "nr_mesh_simplify_count: the grid origin must be finite");
  NR_REQUIRE(dim[0] >= 1 && dim[1] >= 1 && dim[2] >= 1, NR_ERR_ARG, "nr_mesh_simplify_count: every dim must be >= 1");
  NR_REQUIRE(dim[0] <= kMsMaxCells && dim[1] <= kMsMaxCells && dim[2] <= kMsMaxCells &&
                 dim[0] * dim[1] <= kMsMaxCells && dim[0] * dim[1] * dim[2] <= kMsMaxCells,
             NR_ERR_ARG, "nr_mesh_simplify_count: more than 2^27 cells; use a larger cell");
  const int64_t cells = dim[0] * dim[1] * dim[2];
  MsPlan pl;
  NR_REQUIRE(ms_plan(V, F, cells, pl), NR_ERR_ARG, "nr_mesh_simplify_count: needs 0 <= V <= INT32_MAX and 0 <= F <= 2^30");
  NR_REQUIRE((verts || V == 0) && (faces || F == 0), NR_ERR_ARG, "nr_mesh_simplify_count: null verts or faces");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_mesh_simplify_count: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  MsHeader* hdr = (MsHeader*)ws;
  int *cellid = (int*)(ws + pl.o_cellid), *wc = (int*)(ws + pl.o_wc), *vclu = (int*)(ws + pl.o_vclu);
  int *clcell = (int*)(ws + pl.o_clcell), *cnt = (int*)(ws + pl.o_cnt), *bidx = (int*)(ws + pl.o_bidx);
  unsigned long long *sum = (unsigned long long*)(ws + pl.o_sum), *best = (unsigned long long*)(ws + pl.o_best);
  double* mean = (double*)(ws + pl.o_mean);
  int *table = (int*)(ws + pl.o_table), *wf = (int*)(ws + pl.o_wf);
  unsigned* fslot = (unsigned*)(ws + pl.o_fslot);
  MsGrid g;
  g.h = h;
  for (int a = 0; a < 3; ++a) g.lo[a] = lo[a], g.dim[a] = (int)dim[a];
  const unsigned gv = (unsigned)pl.nbv, gf = (unsigned)pl.nbf, gc = (unsigned)pl.nbc, gk = (unsigned)pl.nbk;
  NR_HIP_CHECK(hipMemsetAsync(cellid, 0, (size_t)cells * 4, st));
  NR_HIP_CHECK(hipMemsetAsync(table, 0xFF, (size_t)pl.T * 4, st));  // every slot -1
  NR_LAUNCH("simplify_init", (double)pl.kmax, ms_init, dim3(gk > 0 ? gk : 1), dim3(kMsWG), st, hdr, pl.kmax, cnt, sum,
            best, bidx);
  if (V > 0) NR_LAUNCH("simplify_bin", (double)V, ms_bin, dim3(gv), dim3(kMsWG), st, verts, V, g, vclu, cellid, hdr);
  NR_LAUNCH("simplify_cell_count", (double)cells, ms_cell_count, dim3(gc), dim3(kMsWG), st, cellid, cells, wc);
  NR_LAUNCH("simplify_scan", (double)pl.nbc, ms_scan, dim3(1), dim3(kMsScanWG), st, wc, pl.nbc, &hdr->K);
  NR_LAUNCH("simplify_cell_apply", (double)cells, ms_cell_apply, dim3(gc), dim3(kMsWG), st, cellid, cells, wc, clcell,
            pl.kmax);
  if (V > 0) {
    NR_LAUNCH("simplify_accum", (double)V, ms_accum, dim3(gv), dim3(kMsWG), st, verts, V, g, vclu, cellid, cnt, sum);
    NR_LAUNCH("simplify_mean", (double)pl.kmax, ms_mean, dim3(gk), dim3(kMsWG), st, hdr, g, clcell, cnt, sum, mean);
    NR_LAUNCH("simplify_dist", (double)V, ms_dist, dim3(gv), dim3(kMsWG), st, verts, V, vclu, mean, best);
    NR_LAUNCH("simplify_pick", (double)V, ms_pick, dim3(gv), dim3(kMsWG), st, verts, V, vclu, mean, best, bidx);
  }
  if (F > 0) {
    NR_LAUNCH("simplify_face_hash", (double)F, ms_face_hash, dim3(gf), dim3(kMsWG), st, faces, F, V, vclu, table, pl.T,
              fslot, hdr);
    NR_LAUNCH("simplify_face_count", (double)F, ms_face_count, dim3(gf), dim3(kMsWG), st, fslot, table, F, pl.T, wf);
    NR_LAUNCH("simplify_scan", (double)pl.nbf, ms_scan, dim3(1), dim3(kMsScanWG), st, wf, pl.nbf, &hdr->Fp);
  }
  hipLaunchKernelGGL(ms_finish, dim3(1), dim3(64), 0, st, hdr, totals);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int nr_mesh_simplify_emit(const float* verts, int64_t V, const int32_t* faces, int64_t F, int64_t cells, int position,
                          void* workspace, size_t workspace_bytes, int64_t K, int64_t Fk, float* verts_out,
                          int32_t* index, int32_t* cluster_size, int64_t verts_cap, int32_t* faces_out,
                          int64_t faces_cap, int32_t* vertex_cluster, void* stream) {
  MsPlan pl;
  NR_REQUIRE(ms_plan(V, F, cells, pl), NR_ERR_ARG,
             "nr_mesh_simplify_emit: needs 0 <= V <= INT32_MAX, 0 <= F <= 2^30 and 1 <= cells <= 2^27");
  NR_REQUIRE(position == 0 || position == 1, NR_ERR_ARG, "nr_mesh_simplify_emit: position must be 0 (average) or 1 (nearest)");
  NR_REQUIRE(K >= 0 && Fk >= 0 && K <= pl.kmax && Fk <= F, NR_ERR_ARG,
             "nr_mesh_simplify_emit: the counts must be in [0, min(V, cells)] and [0, F]");
  NR_REQUIRE(verts_cap >= K && faces_cap >= Fk, NR_ERR_ARG,
             "nr_mesh_simplify_emit: output capacity below the cluster / face count");
  NR_REQUIRE((verts || V == 0) && (faces || F == 0), NR_ERR_ARG, "nr_mesh_simplify_emit: null verts or faces");
  NR_REQUIRE(((verts_out && index && cluster_size) || K == 0) && (faces_out || Fk == 0) && (vertex_cluster || V == 0),
             NR_ERR_ARG, "nr_mesh_simplify_emit: null output");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_mesh_simplify_emit: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const MsHeader* hdr = (const MsHeader*)ws;
  const int *vclu = (const int*)(ws + pl.o_vclu), *cnt = (const int*)(ws + pl.o_cnt);
  const int *bidx = (const int*)(ws + pl.o_bidx), *table = (const int*)(ws + pl.o_table);
  const int* wf = (const int*)(ws + pl.o_wf);
  const double* mean = (const double*)(ws + pl.o_mean);
  const unsigned* fslot = (const unsigned*)(ws + pl.o_fslot);
  if (K > 0)
    NR_LAUNCH("simplify_emit_verts", (double)K, ms_emit_verts, dim3((unsigned)((K + kMsWG - 1) / kMsWG)), dim3(kMsWG), st,
              hdr, verts, V, K, position, mean, cnt, bidx, verts_out, index, cluster_size);
  if (V > 0)
    NR_LAUNCH("simplify_emit_clusters", (double)V, ms_emit_clusters, dim3((unsigned)pl.nbv), dim3(kMsWG), st, vclu, V,
              vertex_cluster);
  if (Fk > 0)
    NR_LAUNCH("simplify_emit_faces", (double)F, ms_emit_faces, dim3((unsigned)pl.nbf), dim3(kMsWG), st, faces, F, V, vclu,
              fslot, table, pl.T, wf, faces_out, Fk);
  return NR_OK;
}

}  // extern "C"
