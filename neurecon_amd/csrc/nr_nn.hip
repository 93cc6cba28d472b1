// neurecon_amd — exact nearest neighbour of M queries in N points on a uniform grid: the search behind the
// mesh metrics (accuracy / completeness / Chamfer distance, precision / recall / F-score of an extracted mesh
// against a ground-truth point cloud; neurecon_amd/mesh_metrics.py), run once in each direction.  The
// sampler that feeds it is nr_meshsample.hip.
//
// THE RULE (tests/mesh_metrics_ref.py restates it as a dense brute force; the results are the same bits)
//   points fp32 [N, 3], queries fp32 [M, 3].  Per pair, float64, every operation rounded on its own
//   (`#pragma clang fp contract(off)` below the includes, plain operators under it; nr_common.h on why
//   not __dmul_rn):
//       dx = (double) q.x - (double) p.x,  dy, dz alike;   d2 = ((dx dx) + (dy dy)) + (dz dz)
//   The neighbour of q is the point with the smallest (d2, index), compared lexicographically: a tie in d2
//   goes to the smaller index.  With max_dist (>= 0, +inf = none) the result is kept iff d2 <= max_dist max_dist
//   (the product in float64), else index -1 and d2 = +inf.  A point with a non-finite coordinate is never a
//   neighbour (status bit 0).  A query with a non-finite coordinate gets -1 / +inf.  N == 0, or no finite
//   point: every query gets -1 / +inf.  Finite fp32 coordinates give a finite d2 (< 2^260).
//   Nothing below changes a result: the grid only decides which pairs are looked at, and the order inside a
//   cell, which varies from run to run, only the order in which a minimum is taken.
//
// BUILD (nr_nn_build)
//   box      lo, hi = the exact minimum / maximum of the finite points per axis: fp32 values mapped to
//            order-preserving unsigned keys, reduced per workgroup, then integer atomicMin / atomicMax.  Order-free.
//   grid     cell size h > 0 from the caller.  dim_a = floor((hi_a - lo_a) / h) + 1 (1 on a degenerate axis);
//            while a dim or dim_x dim_y dim_z exceeds CAP = max(1, min(4 N, 2^26)), h is doubled and the dims
//            are taken again (one thread, at most 2200 doublings, then dims = 1: always valid).  The h that
//            is left is THE h of everything below.  No finite point: lo = 0, dims = 1.
//   cell     c_a(x) = clamp(floor(((double) x - lo_a) / h), 0, dim_a - 1), the clamp applied in float64 before
//            the conversion; cell = (c_z dim_y + c_y) dim_x + c_x.  The same function bins points and queries.
//   sort     counting sort by cell: histogram (integer atomicAdd), exclusive scan in place (per-workgroup
//            sums, one workgroup over the sums, fix-up: three launches, no hand-off between workgroups),
//            scatter (slot = atomicAdd(&start[cell], 1)) of 16-byte records (x, y, z, original index).
//            After the scatter start[c] is the END of cell c, so cell c is the run [start[c - 1], start[c])
//            (0 for c == 0) and the cells x0 .. x1 of one grid row are ONE contiguous run.
// QUERY (nr_nn_query; one lane per query, no atomics in the search, no loop waits for another workgroup)
//   The queries are binned by their own (clamped) cell with the same kernels and processed in that order,
//   so the lanes of a wave64 walk neighbouring cells; results are written at the original query index.
//   Rings r = 0, 1, 2, ... around the query's cell C: ring r = the grid cells at Chebyshev distance exactly r
//   from C.  After ring r every cell within Chebyshev distance r has been searched.  With
//   L_r = r h (1 - 2^-20) the search stops after ring r when
//       (a) best_d2 <= L_r L_r,  or  (b) L_r >= max_dist,  or  (c) ring r + 1 lies wholly outside the grid,
//           i.e. r + 1 > max_a max(C_a, dim_a - 1 - C_a).
//   (c) bounds the loop by max(dims) rings whatever the data; a counter capped at max(dims) + 1 is wired to
//   status bit 1 so that a mistake in this argument ends as an error, never as a hang.
//
// WHY STOPPING IS EXACT
//   Claim 1: a finite point p NOT searched after ring r has |p_a - q_a| > r h (1 - 2^-25) on some axis a.
//     p's cell differs from C by >= r + 1 on some axis a; write P, Q for the clamped cell coordinates there.
//     Exact arithmetic first, v(x) = (x - lo) / h, c(x) = clamp(floor(v(x)), 0, dim - 1).  Points lie inside
//     the box, so floor(v(p)) >= 0 and, unless P = dim - 1, floor(v(p)) = P.
//       P >= Q + r + 1:  Q < dim - 1, so q was not clamped from above: v(q) < Q + 1 (also when q lies below
//         the box and was clamped up to 0: v(q) < 0 < 1).  v(p) >= P.  So p - q > (P - Q - 1) h >= r h.
//       P <= Q - r - 1:  P < dim - 1, so v(p) < P + 1.  Q >= 1, so q was not clamped from below: v(q) >= Q (also
//         when q lies above the box and was clamped down).  So q - p > (Q - P - 1) h >= r h.
//     A query outside the box is thus covered: the clamp moves its cell toward the points, never past one.
//     Rounding: the computed v' = fl(fl(x - lo) / h) = v (1 + e), |e| <= 2^-52, and floor(v') <= v' < floor(v') + 1
//     give v >= P (1 - 2^-52) and v < (Q + 1)(1 + 2^-52) in place of the exact bounds; cell coordinates are
//     below CAP <= 2^26, so each bound moves by at most 2^26 2^-52 h = 2^-26 h and the gap is
//     > (r - 2^-25) h >= r h (1 - 2^-25) for r >= 1 (for r = 0 the claim is empty).
//   Claim 2: (a) and (b) lose nothing.  A computed d2 is within (1 + 2^-50) of the true squared distance and
//     L_r carries two more roundings; 2^-20 covers all of it with room: by claim 1 an unsearched point has
//     computed d2 > (r h)^2 (1 - 2^-24) > L_r^2 (1 + 2^-20).  Under (a) that is > best_d2 strictly, so an
//     unsearched point can neither win nor tie.  Under (b) it is > max_dist^2 (1 + 2^-20) > fl(max_dist^2):
//     it would be dropped.  For r = 0, (a) reads best_d2 <= 0: a point with d2 == 0 has the query's
//     coordinates, hence the query's cell, and every such point (so the smallest index) is in ring 0.
//   Claim 3: ties are decided by (d2, index) over all searched points, whatever their order.
//
// Workspace (nr_nn_workspace_bytes(N, M)), C = CAP(N):  256 header bytes + 2 x 4 (C + 1) (cell tables of the
// points and of the queries) + 4 ceil((C + 1) / 1024) (scan sums) + 16 N (records) + 4 M (query order), each
// array rounded up to 256 bytes.  nr_nn_build needs the part up to the records: nr_nn_workspace_bytes(N, 0).
#include "nr_meshcommon.h"

#pragma clang fp contract(off)  // no a * b + c -> fma anywhere in this file (header comment)

namespace nr {

constexpr int kNnWG = 256;
constexpr int kNnScanItems = 1024;  // items per workgroup of the scan passes (4 per thread)
constexpr int kNnScanWG = 1024;     // threads of the one workgroup that scans the sums
constexpr int kNnBoundsGrid = 1024; // workgroups of nn_bounds at most
constexpr unsigned kNnMagic = 0x4e4e4731u;
constexpr int64_t kNnMaxCells = (int64_t)1 << 26;

enum { kNnNonFinitePoint = 1, kNnCapReached = 2, kNnNoBuild = 4 };

struct NnHeader {  // the first 256 bytes of the workspace
  unsigned kmin[3], kmax[3];
  unsigned status;   // build: kNnNonFinitePoint
  unsigned qstatus;  // query: kNnCapReached
  unsigned magic;
  int qok;
  long long N;
  double lo[3], hi[3];
  double h;
  int dims[3];
  int cells, maxdim;
};

__device__ __forceinline__ unsigned nn_key(float x) {  // order-preserving: x < y  <=>  key(x) < key(y)
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float nn_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ bool nn_finite3(float x, float y, float z) {
  return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;
}

struct NnGrid {
  double lo[3], h;
  int dims[3];
};

__device__ __forceinline__ NnGrid nn_grid(const NnHeader* __restrict__ hdr) {
  NnGrid g;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = hdr->lo[a];
    g.dims[a] = hdr->dims[a];
  }
  g.h = hdr->h;
  return g;
}

__device__ __forceinline__ int nn_coord(const NnGrid& g, int a, float x) {
  double v = floor(((double)x - g.lo[a]) / g.h);
  const double top = (double)(g.dims[a] - 1);
  v = v >= 0.0 ? v : 0.0;  // also NaN -> 0 (cannot happen: x, lo finite and h > 0)
  v = v <= top ? v : top;
  return (int)v;
}

__device__ __forceinline__ int nn_cell(const NnGrid& g, float x, float y, float z) {
  return (nn_coord(g, 2, z) * g.dims[1] + nn_coord(g, 1, y)) * g.dims[0] + nn_coord(g, 0, x);
}

__global__ void nn_init(NnHeader* __restrict__ hdr) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    hdr->kmin[a] = 0xffffffffu;
    hdr->kmax[a] = 0u;
  }
  hdr->status = 0;
  hdr->qstatus = 0;
  hdr->magic = 0;
  hdr->qok = 0;
}

// a grid of at most kNnBoundsGrid workgroups strides the points; one set of atomics per workgroup, and only
// where the header's value would move (a relaxed load may be stale, but a stale minimum is only ever too
// large and a stale maximum too small: the atomic is skipped only when it could not have changed anything)
__global__ __launch_bounds__(kNnWG) void nn_bounds(const float* __restrict__ pts, int64_t N,
                                                   NnHeader* __restrict__ hdr) {
  __shared__ unsigned lmn[kNnWG / 64][3], lmx[kNnWG / 64][3];
  __shared__ int lbad[kNnWG / 64];
  unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * kNnWG + threadIdx.x; i < N; i += (int64_t)gridDim.x * kNnWG) {
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    if (nn_finite3(p[0], p[1], p[2])) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const unsigned k = nn_key(p[a]);
        mn[a] = k < mn[a] ? k : mn[a];
        mx[a] = k > mx[a] ? k : mx[a];
      }
    } else {
      bad = true;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned lo = __shfl_xor(mn[a], off), hi = __shfl_xor(mx[a], off);
      mn[a] = lo < mn[a] ? lo : mn[a];
      mx[a] = hi > mx[a] ? hi : mx[a];
    }
  }
  const unsigned long long anybad = __ballot(bad);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lmn[wave][a] = mn[a];
      lmx[wave][a] = mx[a];
    }
    lbad[wave] = anybad ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    unsigned lo = lmn[0][a], hi = lmx[0][a];
#pragma unroll
    for (int w = 1; w < kNnWG / 64; ++w) {
      lo = lmn[w][a] < lo ? lmn[w][a] : lo;
      hi = lmx[w][a] > hi ? lmx[w][a] : hi;
    }
    if (hi != 0u) {  // the workgroup holds a finite point
      if (lo < __hip_atomic_load(&hdr->kmin[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&hdr->kmin[a], lo);
      if (hi > __hip_atomic_load(&hdr->kmax[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&hdr->kmax[a], hi);
    }
  } else if (threadIdx.x == 3) {
    int any = 0;
#pragma unroll
    for (int w = 0; w < kNnWG / 64; ++w) any |= lbad[w];
    if (any) atomicOr(&hdr->status, (unsigned)kNnNonFinitePoint);
  }
}

// box -> doubles; out (may be null): {lo xyz, hi xyz, 1 if any finite point else 0, status}
__global__ void nn_box(NnHeader* __restrict__ hdr, double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const bool any = hdr->kmax[0] != 0u;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    hdr->lo[a] = any ? (double)nn_unkey(hdr->kmin[a]) : 0.0;
    hdr->hi[a] = any ? (double)nn_unkey(hdr->kmax[a]) : 0.0;
  }
  if (out) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      out[a] = hdr->lo[a];
      out[3 + a] = hdr->hi[a];
    }
    out[6] = any ? 1.0 : 0.0;
    out[7] = (double)hdr->status;
  }
}

__global__ void nn_plan(NnHeader* __restrict__ hdr, double h, int64_t cap, int64_t N) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double d[3] = {1.0, 1.0, 1.0};
  bool fits = false;
  for (int it = 0; it < 2200 && !fits; ++it) {  // 2^2200 h is +inf: dims 1
    fits = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      d[a] = floor((hdr->hi[a] - hdr->lo[a]) / h) + 1.0;
      if (!(d[a] >= 1.0 && d[a] <= (double)cap)) fits = false;
    }
    if (fits && (d[0] * d[1]) * d[2] > (double)cap) fits = false;  // <= 2^78: exact enough, cap is an integer
    if (!fits) h = h * 2.0;
  }
  if (!fits) d[0] = d[1] = d[2] = 1.0;
  int64_t cells = 1;
  int maxdim = 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    hdr->dims[a] = (int)d[a];
    cells *= (int64_t)hdr->dims[a];
    maxdim = hdr->dims[a] > maxdim ? hdr->dims[a] : maxdim;
  }
  if (cells > cap) {  // cannot happen (the product test above is on exact integers below 2^53 when it passes)
    hdr->dims[0] = hdr->dims[1] = hdr->dims[2] = 1;
    cells = 1;
    maxdim = 1;
  }
  hdr->h = h;
  hdr->cells = (int)cells;
  hdr->maxdim = maxdim;
  hdr->N = N;
  hdr->magic = kNnMagic;
}

// the query side trusts the header only after this check
__global__ void nn_qinit(NnHeader* __restrict__ hdr, int64_t cap, int64_t N) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  bool ok = hdr->magic == kNnMagic && hdr->N == N && hdr->h > 0.0;
  if (ok) {
    const int64_t dx = hdr->dims[0], dy = hdr->dims[1], dz = hdr->dims[2];
    ok = dx >= 1 && dy >= 1 && dz >= 1 && dx <= cap && dy <= cap && dz <= cap && dx * dy <= cap &&
         dx * dy * dz <= cap && hdr->cells == dx * dy * dz && hdr->maxdim >= 1 && hdr->maxdim <= cap;
  }
  hdr->qok = ok ? 1 : 0;
  hdr->qstatus = 0;
}

// histogram of the finite items over the cells; with `index` (the query side) an item that is not binned
// gets its final answer here: -1 / +inf
__global__ __launch_bounds__(kNnWG) void nn_hist(const float* __restrict__ pts, int64_t n,
                                                 const NnHeader* __restrict__ hdr, int* __restrict__ table,
                                                 int query_side, int* __restrict__ index, double* __restrict__ d2) {
  const int64_t i = (int64_t)blockIdx.x * kNnWG + threadIdx.x;
  if (i >= n) return;
  const bool ok = query_side ? hdr->qok != 0 : true;
  const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
  if (!ok || !nn_finite3(x, y, z)) {
    if (query_side) {
      index[i] = -1;
      d2[i] = __longlong_as_double(0x7ff0000000000000ll);
    }
    return;
  }
  const NnGrid g = nn_grid(hdr);
  atomicAdd(table + nn_cell(g, x, y, z), 1);
}

// ---- exclusive scan of table[0 .. cells] in place (cells + 1 items: the last becomes the total) ----
__device__ __forceinline__ int nn_wave_incl(int v) {  // inclusive scan over the wave's 64 lanes
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

__global__ __launch_bounds__(kNnWG) void nn_scan_sums(const int* __restrict__ table,
                                                      const NnHeader* __restrict__ hdr, int* __restrict__ sums) {
  __shared__ int lds[kNnWG / 64];
  const int64_t n = (int64_t)hdr->cells + 1;
  const int64_t base = (int64_t)blockIdx.x * kNnScanItems;
  if (base >= n) return;
  int v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t j = base + 4 * threadIdx.x + k;
    v += j < n ? table[j] : 0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

// one workgroup; sums[b] = items before workgroup b
__global__ __launch_bounds__(kNnScanWG) void nn_scan_top(int* __restrict__ sums, const NnHeader* __restrict__ hdr) {
  __shared__ int s[kNnScanWG];
  const int64_t n = (int64_t)hdr->cells + 1;
  strip_scan<kNnScanWG>((n + kNnScanItems - 1) / kNnScanItems, s, [&](int64_t q) { return sums[q]; },
                        [&](int64_t q, int e) { sums[q] = e; });
}

__global__ __launch_bounds__(kNnWG) void nn_scan_fix(int* __restrict__ table, const NnHeader* __restrict__ hdr,
                                                     const int* __restrict__ sums) {
  __shared__ int lds[kNnWG / 64];
  const int64_t n = (int64_t)hdr->cells + 1;
  const int64_t base = (int64_t)blockIdx.x * kNnScanItems;
  if (base >= n) return;
  int c[4];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t j = base + 4 * threadIdx.x + k;
    c[k] = j < n ? table[j] : 0;
    mine += c[k];
  }
  const int incl = nn_wave_incl(mine);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) lds[wave] = incl;
  __syncthreads();
  int e = sums[blockIdx.x] + incl - mine;
#pragma unroll
  for (int w = 0; w < kNnWG / 64; ++w) e += w < wave ? lds[w] : 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t j = base + 4 * threadIdx.x + k;
    if (j < n) table[j] = e;
    e += c[k];
  }
}

// points: 16-byte records in cell order; queries (recs == null): order[slot] = query index
__global__ __launch_bounds__(kNnWG) void nn_scatter(const float* __restrict__ pts, int64_t n,
                                                    const NnHeader* __restrict__ hdr, int* __restrict__ table,
                                                    float4* __restrict__ recs, int* __restrict__ order,
                                                    int64_t capacity) {
  const int64_t i = (int64_t)blockIdx.x * kNnWG + threadIdx.x;
  if (i >= n) return;
  if (order && !hdr->qok) return;
  const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
  if (!nn_finite3(x, y, z)) return;
  const NnGrid g = nn_grid(hdr);
  const int slot = atomicAdd(table + nn_cell(g, x, y, z), 1);
  if (slot < 0 || slot >= capacity) return;  // cannot happen: the slots of the binned items are 0 .. their count - 1
  if (order) order[slot] = (int)i;
  else recs[slot] = make_float4(x, y, z, __int_as_float((int)i));
}

struct NnBest {
  double d2;
  int idx;
};

// the records [beg, end): lexicographic minimum of (d2, index)
__device__ __forceinline__ void nn_run(const float4* __restrict__ recs, int beg, int end, double qx, double qy,
                                       double qz, NnBest& best) {
  for (int j = beg; j < end; ++j) {
    const float4 p = recs[j];
    const double dx = qx - (double)p.x, dy = qy - (double)p.y, dz = qz - (double)p.z;
    const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
    const int idx = __float_as_int(p.w);
    if (d2 < best.d2 || (d2 == best.d2 && idx < best.idx)) {
      best.d2 = d2;
      best.idx = idx;
    }
  }
}

__global__ __launch_bounds__(kNnWG) void nn_query(const float* __restrict__ queries, int64_t M, int64_t N,
                                                  NnHeader* __restrict__ hdr, const int* __restrict__ ptable,
                                                  const int* __restrict__ qtable, const float4* __restrict__ recs,
                                                  const int* __restrict__ order, double max_dist,
                                                  int* __restrict__ index, double* __restrict__ d2_out) {
  const int64_t j = (int64_t)blockIdx.x * kNnWG + threadIdx.x;
  if (j >= M || !hdr->qok) return;
  const int cells = hdr->cells;
  if (j >= qtable[cells]) return;  // the binned (finite) queries; the others were answered by nn_hist
  const int qi = order[j];
  if (qi < 0 || qi >= M) return;
  const NnGrid g = nn_grid(hdr);
  const float fx = queries[3 * (int64_t)qi], fy = queries[3 * (int64_t)qi + 1], fz = queries[3 * (int64_t)qi + 2];
  const double qx = fx, qy = fy, qz = fz;
  const int cx = nn_coord(g, 0, fx), cy = nn_coord(g, 1, fy), cz = nn_coord(g, 2, fz);
  const int dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
  int rmax = cx > dx - 1 - cx ? cx : dx - 1 - cx;
  rmax = cy > rmax ? cy : rmax;
  rmax = dy - 1 - cy > rmax ? dy - 1 - cy : rmax;
  rmax = cz > rmax ? cz : rmax;
  rmax = dz - 1 - cz > rmax ? dz - 1 - cz : rmax;
  const int ring_cap = hdr->maxdim + 1;
  const int nrec = (int)(N < 0x7fffffff ? N : 0x7fffffff);
  NnBest best;
  best.d2 = __longlong_as_double(0x7ff0000000000000ll);
  best.idx = 0x7fffffff;
  for (int r = 0; r <= rmax; ++r) {
    if (r >= ring_cap) {  // rmax <= maxdim - 1: cannot happen (header comment)
      atomicOr(&hdr->qstatus, (unsigned)kNnCapReached);
      break;
    }
    const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < dz - 1 ? cz + r : dz - 1;
    const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < dy - 1 ? cy + r : dy - 1;
    const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < dx - 1 ? cx + r : dx - 1;
    for (int z = z0; z <= z1; ++z) {
      const bool zface = z - cz == r || cz - z == r;
      for (int y = y0; y <= y1; ++y) {
        const int row = (z * dy + y) * dx;
        if (zface || y - cy == r || cy - y == r) {  // the whole row x0 .. x1 belongs to the ring: one run
          const int a = row + x0, b = row + x1;
          int beg = a > 0 ? ptable[a - 1] : 0, end = ptable[b];
          beg = beg < 0 ? 0 : beg;
          end = end > nrec ? nrec : end;
          nn_run(recs, beg, end, qx, qy, qz, best);
        } else {  // only the two end cells, where they are inside the grid
          if (cx - r >= 0) {
            const int a = row + cx - r;
            int beg = a > 0 ? ptable[a - 1] : 0, end = ptable[a];
            beg = beg < 0 ? 0 : beg;
            end = end > nrec ? nrec : end;
            nn_run(recs, beg, end, qx, qy, qz, best);
          }
          if (cx + r <= dx - 1) {  // r >= 1 here (r == 0 makes every row a ring row)
            const int a = row + cx + r;
            int beg = a > 0 ? ptable[a - 1] : 0, end = ptable[a];
            beg = beg < 0 ? 0 : beg;
            end = end > nrec ? nrec : end;
            nn_run(recs, beg, end, qx, qy, qz, best);
          }
        }
      }
    }
    const double lim = ((double)r * g.h) * (1.0 - 9.5367431640625e-07);  // L_r, 2^-20
    if (best.d2 <= lim * lim) break;
    if (lim >= max_dist) break;
  }
  const bool keep = best.idx != 0x7fffffff && best.d2 <= max_dist * max_dist;
  index[qi] = keep ? best.idx : -1;
  d2_out[qi] = keep ? best.d2 : __longlong_as_double(0x7ff0000000000000ll);
}

__global__ void nn_qfinish(const NnHeader* __restrict__ hdr, int64_t* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  status[0] = (int64_t)((hdr->status & kNnNonFinitePoint) | (hdr->qstatus & kNnCapReached) |
                        (hdr->qok ? 0u : (unsigned)kNnNoBuild));
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct NnPlan {
  int64_t cap, nsb;  // cell cap, scan workgroups
  size_t o_ptable, o_qtable, o_sums, o_recs, o_order, build_total, total;
};

static bool nn_plan_host(int64_t N, int64_t M, NnPlan& p) {
  if (N < 0 || M < 0 || N > INT32_MAX || M > INT32_MAX) return false;
  p.cap = 4 * N < kNnMaxCells ? 4 * N : kNnMaxCells;
  if (p.cap < 1) p.cap = 1;
  p.nsb = (p.cap + 1 + kNnScanItems - 1) / kNnScanItems;
  size_t o = 256;  // NnHeader
  p.o_ptable = o; o += a256((size_t)(p.cap + 1) * 4);
  p.o_qtable = o; o += a256((size_t)(p.cap + 1) * 4);
  p.o_sums = o; o += a256((size_t)p.nsb * 4);
  p.o_recs = o; o += a256((size_t)N * 16);
  p.build_total = o;
  p.o_order = o; o += a256((size_t)M * 4);
  p.total = o;
  return true;
}

static_assert(sizeof(NnHeader) <= 256, "NnHeader must fit the workspace header");

static int nn_scan(const char* name, int* table, NnHeader* hdr, int* sums, const NnPlan& pl, hipStream_t st) {
  ProfScope prof(name, (double)(pl.cap + 1), st);
  hipLaunchKernelGGL(nn_scan_sums, dim3((unsigned)pl.nsb), dim3(kNnWG), 0, st, table, hdr, sums);
  hipLaunchKernelGGL(nn_scan_top, dim3(1), dim3(kNnScanWG), 0, st, sums, hdr);
  hipLaunchKernelGGL(nn_scan_fix, dim3((unsigned)pl.nsb), dim3(kNnWG), 0, st, table, hdr, sums);
  return 0;
}

static unsigned nn_blocks(int64_t n) { return (unsigned)((n + kNnWG - 1) / kNnWG); }

static unsigned nn_bounds_blocks(int64_t n) {
  const unsigned b = nn_blocks(n);
  return b < (unsigned)kNnBoundsGrid ? b : (unsigned)kNnBoundsGrid;
}

}  // namespace nr

using namespace nr;

extern "C" {

size_t nr_nn_workspace_bytes(int64_t N, int64_t M) {
  NnPlan pl;
  return nn_plan_host(N, M, pl) ? pl.total : 0;
}

int nr_nn_bounds(const float* points, int64_t N, double* bounds, void* workspace, size_t workspace_bytes,
                 void* stream) {
  NR_REQUIRE(N >= 0 && N <= INT32_MAX, NR_ERR_ARG, "nr_nn_bounds: the point count must be in [0, INT32_MAX]");
  NR_REQUIRE((points || N == 0) && bounds, NR_ERR_ARG, "nr_nn_bounds: null argument");
  NR_REQUIRE(workspace && workspace_bytes >= 256, NR_ERR_WORKSPACE, "nr_nn_bounds: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  NnHeader* hdr = (NnHeader*)workspace;
  hipLaunchKernelGGL(nn_init, dim3(1), dim3(64), 0, st, hdr);
  if (N > 0) NR_LAUNCH("nn_bounds", (double)N, nn_bounds, dim3(nn_bounds_blocks(N)), dim3(kNnWG), st, points, N, hdr);
  hipLaunchKernelGGL(nn_box, dim3(1), dim3(64), 0, st, hdr, bounds);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int nr_nn_build(const float* points, int64_t N, double h, void* workspace, size_t workspace_bytes, void* stream) {
  NnPlan pl;
  NR_REQUIRE(nn_plan_host(N, 0, pl), NR_ERR_ARG, "nr_nn_build: the point count must be in [0, INT32_MAX]");
  NR_REQUIRE(points || N == 0, NR_ERR_ARG, "nr_nn_build: null argument");
  NR_REQUIRE(h > 0.0 && h <= 1.79769313486231570e308, NR_ERR_ARG, "nr_nn_build: the cell size h must be finite and > 0");
  NR_REQUIRE(workspace && workspace_bytes >= pl.build_total, NR_ERR_WORKSPACE, "nr_nn_build: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  NnHeader* hdr = (NnHeader*)ws;
  int* ptable = (int*)(ws + pl.o_ptable);
  int* sums = (int*)(ws + pl.o_sums);
  float4* recs = (float4*)(ws + pl.o_recs);
  hipLaunchKernelGGL(nn_init, dim3(1), dim3(64), 0, st, hdr);
  NR_HIP_CHECK(hipMemsetAsync(ptable, 0, (size_t)(pl.cap + 1) * 4, st));
  if (N > 0) NR_LAUNCH("nn_bounds", (double)N, nn_bounds, dim3(nn_bounds_blocks(N)), dim3(kNnWG), st, points, N, hdr);
  hipLaunchKernelGGL(nn_box, dim3(1), dim3(64), 0, st, hdr, (double*)nullptr);
  hipLaunchKernelGGL(nn_plan, dim3(1), dim3(64), 0, st, hdr, h, pl.cap, N);
  NR_HIP_CHECK(hipGetLastError());
  if (N > 0)
    NR_LAUNCH("nn_hist", (double)N, nn_hist, dim3(nn_blocks(N)), dim3(kNnWG), st, points, N, hdr, ptable, 0, (int*)nullptr,
              (double*)nullptr);
  nn_scan("nn_scan", ptable, hdr, sums, pl, st);
  if (N > 0)
    NR_LAUNCH("nn_scatter", (double)N, nn_scatter, dim3(nn_blocks(N)), dim3(kNnWG), st, points, N, hdr, ptable, recs,
              (int*)nullptr, N);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int nr_nn_query(int64_t N, const float* queries, int64_t M, double max_dist, int32_t* index, double* d2,
                int64_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  NnPlan pl;
  NR_REQUIRE(nn_plan_host(N, M, pl), NR_ERR_ARG, "nr_nn_query: point and query counts must be in [0, INT32_MAX]");
  NR_REQUIRE(queries || M == 0, NR_ERR_ARG, "nr_nn_query: null argument");
  NR_REQUIRE(max_dist >= 0.0, NR_ERR_ARG, "nr_nn_query: max_dist must be >= 0 (+inf: no limit)");
  NR_REQUIRE(((index && d2) || M == 0) && status, NR_ERR_ARG, "nr_nn_query: null output");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_nn_query: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  NnHeader* hdr = (NnHeader*)ws;
  int* ptable = (int*)(ws + pl.o_ptable);
  int* qtable = (int*)(ws + pl.o_qtable);
  int* sums = (int*)(ws + pl.o_sums);
  float4* recs = (float4*)(ws + pl.o_recs);
  int* order = (int*)(ws + pl.o_order);
  hipLaunchKernelGGL(nn_qinit, dim3(1), dim3(64), 0, st, hdr, pl.cap, N);
  NR_HIP_CHECK(hipGetLastError());
  if (M > 0) {
    NR_HIP_CHECK(hipMemsetAsync(qtable, 0, (size_t)(pl.cap + 1) * 4, st));
    NR_LAUNCH("nn_qhist", (double)M, nn_hist, dim3(nn_blocks(M)), dim3(kNnWG), st, queries, M, hdr, qtable, 1, index, d2);
    nn_scan("nn_qscan", qtable, hdr, sums, pl, st);
    NR_LAUNCH("nn_qscatter", (double)M, nn_scatter, dim3(nn_blocks(M)), dim3(kNnWG), st, queries, M, hdr, qtable,
              (float4*)nullptr, order, M);
    NR_LAUNCH("nn_query", (double)M, nn_query, dim3(nn_blocks(M)), dim3(kNnWG), st, queries, M, N, hdr, ptable, qtable, recs,
              order, max_dist, index, d2);
  }
  hipLaunchKernelGGL(nn_qfinish, dim3(1), dim3(64), 0, st, hdr, status);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

}  // extern "C"
