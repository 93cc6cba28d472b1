// neurecon_amd — points on the surface of an indexed triangle mesh: the area-weighted, stratified sampler
// that feeds the mesh metrics (Chamfer distance, precision / recall / F-score of an extracted mesh against
// a ground-truth point cloud; neurecon_amd/mesh_metrics.py).  The neighbour search is nr_nn.hip.
//
// Every output is a pure function of the inputs (verts, faces, u): two runs are bit-identical.  All
// arithmetic is float64 with each operation rounded on its own: `#pragma clang fp contract(off)` below the
// includes and plain operators under it (why not the __d*_rn intrinsics: nr_common.h).  The float64 division and
// square root are correctly rounded, so tests/mesh_metrics_ref.py restates the sampler in numpy bit for bit.
//
// Definitions
//   Input (device): verts fp32 [V, 3], faces int32 [F, 3], u float64 [n, 3] uniforms in [0, 1).
//   Face area (ms_area, float64).  v0, v1, v2 the face's vertices widened to float64,
//       e1 = v1 - v0,  e2 = v2 - v0,  c = e1 x e2  (c.x = (e1.y e2.z) - (e1.z e2.y), cyclic)
//       a_f = 0.5 sqrt(((c.x c.x) + (c.y c.y)) + (c.z c.z))
//     A face with an index outside [0, V) is never dereferenced: a_f = 0 and status bit 0 is set.
//     A non-finite a_f (a NaN or inf coordinate) becomes 0 and sets status bit 1.
//   cdf [F] (float64): the inclusive prefix sum of the areas, in ONE fixed order of additions that depends on F
//     alone; total = cdf[F - 1] (0 when F == 0).  The order is a three-level chain, with a face's position
//     f = 2048 q + 8 t + i  (workgroup q, thread t of 256, element i of the thread's strip of 8):
//       s_0 = a_f0,  s_i = s_(i-1) + a_(f0+i)                 the strip, left to right;  S_t = s_7
//       T_0 = 0,     T_(t+1) = T_t + S_t                      the workgroup's 256 strips, left to right;  W_q = T_256
//       B_0 = 0,     B_(q+1) = B_q + W_q                      the workgroups, left to right
//       cdf[f] = B_q + (T_t + s_i)
//     Three launches in the shape of nr_mc_count / nr_mesh_filter_count: per-workgroup sums (ms_area), one
//     workgroup over those sums (ms_scan), a fix-up (ms_fix).  No workgroup waits for another.
//     Why the two upper levels are chains and not trees: cdf must be monotone, because the sampler searches
//     it.  Rounding is monotone (x <= y gives fl(x + z) <= fl(y + z)), so cdf is non-decreasing inside a strip.
//     The last element of strip t is B_q + (T_t + S_t) = B_q + T_(t+1), and the first of strip t + 1 is
//     B_q + (T_(t+1) + a) >= B_q + T_(t+1).  The last element of workgroup q is B_q + W_q = B_(q+1) and the first of
//     workgroup q + 1 is B_(q+1) + (0 + a) >= B_(q+1).  Both steps need the next base to be the very expression
//     that ends the previous run; a tree over the bases (B_(q+1) = fl(X + fl(e + W_q)) against
//     fl(fl(X + e) + W_q)) can fall one ulp short: X = 1, e = 1.1 2^-53, W = 1.8 2^-53.  The chain over the
//     workgroups costs one dependent addition per 2048 faces (1465 for a 3 M face mesh) in one thread.
//     Accuracy: cdf[f] is the sum of f + 1 areas by f additions, each off by at most 2^-53 of its result, so
//     |cdf[f] - exact| <= f 2^-53 total (1 + f 2^-53).
//   Sample k of n (ms_sample, one thread per sample), stratified:
//       t = ((k + u[k,0]) / n) total
//       face = the first f with cdf[f] > t, by binary search (lo = 0, hi = F; mid = (lo + hi) / 2;
//              cdf[mid] > t ? hi = mid : lo = mid + 1); when there is none (rounding pushed t to the end):
//              the first f with cdf[f] >= total, found the same way.
//     Either way cdf[face] > cdf[face - 1] (cdf[-1] = 0): by monotonicity cdf[face - 1] <= t < cdf[face] in the
//     first case, and in the second the first f that reaches total > 0 exceeds its predecessor.  A face of
//     area 0 (degenerate, invalid, non-finite) has cdf[f] == cdf[f - 1] and is never chosen, and the second
//     case names the last face with cdf[f] > cdf[f - 1].
//     Barycentrics without a square root:
//       (a, b) = (u[k,1], u[k,2]);  if a + b > 1: (a, b) = (1 - a, 1 - b);  b0 = (1 - a) - b
//       p = ((b0 v0) + (a v1)) + (b v2)  per component in float64, rounded once to fp32
//     Outputs: points fp32 [n, 3], face_id int32 [n].  total == 0 (or not finite: impossible, areas are finite
//     and a sum that overflows is refused) gives face_id -1 and a zero point for every sample; callers take
//     total == 0 or n == 0 as "no samples".  A chosen face is checked against V again before its vertices are
//     read, so a cdf that belongs to another mesh cannot cause an out-of-range read (face_id -1 then).
//   info (device float64 [2]): {total, status}.
// Workspace: 12 bytes per 2048 faces (W_q / B_q and a status word), each array rounded up to 256 bytes, at least 512.
#include "nr_meshcommon.h"

#pragma clang fp contract(off)  // no a * b + c -> fma anywhere in this file (header comment)

namespace nr {

constexpr int kMsWG = 256;                    // threads per workgroup
constexpr int kMsStrip = 8;                   // consecutive faces per thread
constexpr int kMsBlock = kMsWG * kMsStrip;    // faces per workgroup

enum { kMsBadIndex = 1, kMsNonFinite = 2 };

__device__ __forceinline__ double ms_area_of(const float* __restrict__ verts, int a, int b, int c) {
  const double x0 = verts[3 * (int64_t)a], y0 = verts[3 * (int64_t)a + 1], z0 = verts[3 * (int64_t)a + 2];
  const double e1x = (double)verts[3 * (int64_t)b] - x0, e1y = (double)verts[3 * (int64_t)b + 1] - y0,
               e1z = (double)verts[3 * (int64_t)b + 2] - z0;
  const double e2x = (double)verts[3 * (int64_t)c] - x0, e2y = (double)verts[3 * (int64_t)c + 1] - y0,
               e2z = (double)verts[3 * (int64_t)c + 2] - z0;
  const double cx = (e1y * e2z) - (e1z * e2y), cy = (e1z * e2x) - (e1x * e2z), cz = (e1x * e2y) - (e1y * e2x);
  return 0.5 * sqrt(((cx * cx) + (cy * cy)) + (cz * cz));
}

// cdf[f] = T_t + s_i (no workgroup base yet), wsum[q] = W_q, wstat[q] = the workgroup's status bits
__global__ __launch_bounds__(kMsWG) void ms_area(const float* __restrict__ verts, int64_t V,
                                                 const int* __restrict__ faces, int64_t F, double* __restrict__ cdf,
                                                 double* __restrict__ wsum, unsigned* __restrict__ wstat) {
  __shared__ double strip[kMsWG];
  __shared__ unsigned stat[kMsWG / 64];
  const int tid = threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.x * kMsBlock + (int64_t)tid * kMsStrip;
  double s[kMsStrip];
  unsigned status = 0;
  double run = 0.0;
#pragma unroll
  for (int i = 0; i < kMsStrip; ++i) {
    const int64_t f = f0 + i;
    double a = 0.0;
    if (f < F) {
      const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
      if (!face_valid(ia, ib, ic, V)) {
        status |= kMsBadIndex;
      } else {
        a = ms_area_of(verts, ia, ib, ic);
        if (!(a >= 0.0 && a <= 1.79769313486231570e308)) {
          a = 0.0;
          status |= kMsNonFinite;
        }
      }
    }
    run = i == 0 ? a : run + a;
    s[i] = run;
  }
  strip[tid] = run;
  // the workgroup's status: OR over the lanes of each wave, then over the waves
  unsigned w = status;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) w |= __shfl_xor(w, off);
  if ((tid & 63) == 0) stat[tid >> 6] = w;
  __syncthreads();
  if (tid == 0) {
    double T = 0.0;
    for (int t = 0; t < kMsWG; ++t) {  // the chain over the strips (header comment)
      const double S = strip[t];
      strip[t] = T;
      T = T + S;
    }
    wsum[blockIdx.x] = T;
    unsigned all = 0;
#pragma unroll
    for (int k = 0; k < kMsWG / 64; ++k) all |= stat[k];
    wstat[blockIdx.x] = all;
  }
  __syncthreads();
  const double T = strip[tid];
#pragma unroll
  for (int i = 0; i < kMsStrip; ++i)
    if (f0 + i < F) cdf[f0 + i] = T + s[i];
}

// one workgroup: wsum[q] = B_q in place (the chain over the workgroups, in thread 0, staged through LDS in
// pieces of 2048); info = {total, status}
__global__ __launch_bounds__(kMsWG) void ms_scan(double* __restrict__ wsum, const unsigned* __restrict__ wstat,
                                                 int64_t nb, double* __restrict__ info) {
  __shared__ double piece[kMsBlock];
  __shared__ double carry;
  __shared__ unsigned stat[kMsWG / 64];
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0.0;
  unsigned status = 0;
  for (int64_t base = 0; base < nb; base += kMsBlock) {
    const int64_t m = nb - base < kMsBlock ? nb - base : kMsBlock;
    for (int64_t j = tid; j < m; j += kMsWG) {
      piece[j] = wsum[base + j];
      status |= wstat[base + j];
    }
    __syncthreads();
    if (tid == 0) {
      double B = carry;
      for (int64_t j = 0; j < m; ++j) {
        const double W = piece[j];
        piece[j] = B;
        B = B + W;
      }
      carry = B;
    }
    __syncthreads();
    for (int64_t j = tid; j < m; j += kMsWG) wsum[base + j] = piece[j];
    __syncthreads();
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) status |= __shfl_xor(status, off);
  if ((tid & 63) == 0) stat[tid >> 6] = status;
  __syncthreads();
  if (tid == 0) {
    unsigned all = 0;
#pragma unroll
    for (int k = 0; k < kMsWG / 64; ++k) all |= stat[k];
    info[0] = carry;
    info[1] = (double)all;
  }
}

// cdf[f] = B_q + cdf[f]
__global__ __launch_bounds__(kMsWG) void ms_fix(double* __restrict__ cdf, int64_t F, const double* __restrict__ wsum) {
  const int64_t f = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (f < F) cdf[f] = wsum[f / kMsBlock] + cdf[f];
}

__global__ __launch_bounds__(kMsWG) void ms_sample(const float* __restrict__ verts, int64_t V,
                                                   const int* __restrict__ faces, int64_t F,
                                                   const double* __restrict__ cdf, const double* __restrict__ u,
                                                   int64_t n, float* __restrict__ points, int* __restrict__ face_id) {
  const int64_t k = (int64_t)blockIdx.x * kMsWG + threadIdx.x;
  if (k >= n) return;
  const double total = F > 0 ? cdf[F - 1] : 0.0;
  int64_t face = -1;
  if (total > 0.0 && total <= 1.79769313486231570e308) {
    const double t = (((double)k + u[3 * k]) / (double)n) * total;
    int64_t lo = 0, hi = F;
    while (lo < hi) {  // at most 32 steps
      const int64_t mid = (lo + hi) >> 1;
      if (cdf[mid] > t) hi = mid; else lo = mid + 1;
    }
    if (lo == F) {
      lo = 0, hi = F;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cdf[mid] >= total) hi = mid; else lo = mid + 1;
      }
    }
    face = lo < F ? lo : -1;
  }
  int ia = 0, ib = 0, ic = 0;
  if (face >= 0) {
    ia = faces[3 * face], ib = faces[3 * face + 1], ic = faces[3 * face + 2];
    if (!face_valid(ia, ib, ic, V)) face = -1;
  }
  if (face < 0) {
    points[3 * k] = 0.f, points[3 * k + 1] = 0.f, points[3 * k + 2] = 0.f;
    face_id[k] = -1;
    return;
  }
  double a = u[3 * k + 1], b = u[3 * k + 2];
  if (a + b > 1.0) {
    a = 1.0 - a;
    b = 1.0 - b;
  }
  const double b0 = (1.0 - a) - b;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v0 = verts[3 * (int64_t)ia + c], v1 = verts[3 * (int64_t)ib + c], v2 = verts[3 * (int64_t)ic + c];
    points[3 * k + c] = (float)(((b0 * v0) + (a * v1)) + (b * v2));
  }
  face_id[k] = (int)face;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct MsPlan {
  int64_t nb;
  size_t o_sum, o_stat, total;
};

static bool ms_plan(int64_t F, MsPlan& p) {
  if (F < 0 || F > INT32_MAX) return false;
  p.nb = (F + kMsBlock - 1) / kMsBlock;
  const size_t slots = (size_t)(p.nb > 0 ? p.nb : 1);
  size_t o = 0;
  p.o_sum = o; o += a256(slots * 8);
  p.o_stat = o; o += a256(slots * 4);
  p.total = o;
  return true;
}

}  // namespace nr

using namespace nr;

extern "C" {

size_t nr_mesh_sample_workspace_bytes(int64_t F) {
  MsPlan pl;
  return ms_plan(F, pl) ? pl.total : 0;
}

int nr_mesh_face_cdf(const float* verts, int64_t V, const int32_t* faces, int64_t F, double* cdf, double* info,
                     void* workspace, size_t workspace_bytes, void* stream) {
  MsPlan pl;
  NR_REQUIRE(V >= 0 && V <= INT32_MAX && ms_plan(F, pl), NR_ERR_ARG,
             "nr_mesh_face_cdf: vertex and face counts must be in [0, INT32_MAX]");
  NR_REQUIRE((verts || V == 0) && (faces || F == 0), NR_ERR_ARG, "nr_mesh_face_cdf: null argument");
  NR_REQUIRE((cdf || F == 0) && info, NR_ERR_ARG, "nr_mesh_face_cdf: null output");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_mesh_face_cdf: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* wsum = (double*)(ws + pl.o_sum);
  unsigned* wstat = (unsigned*)(ws + pl.o_stat);
  if (F > 0)
    NR_LAUNCH("mesh_area", (double)F, ms_area, dim3((unsigned)pl.nb), dim3(kMsWG), st, verts, V, faces, F, cdf, wsum, wstat);
  NR_LAUNCH("mesh_area_scan", (double)pl.nb, ms_scan, dim3(1), dim3(kMsWG), st, wsum, wstat, pl.nb, info);
  if (pl.nb > 1)  // a single workgroup has base 0: 0 + x == x
    NR_LAUNCH("mesh_area_fix", (double)F, ms_fix, dim3((unsigned)((F + kMsWG - 1) / kMsWG)), dim3(kMsWG), st, cdf, F, wsum);
  return NR_OK;
}

int nr_mesh_sample(const float* verts, int64_t V, const int32_t* faces, int64_t F, const double* cdf, const double* u,
                   int64_t n, float* points, int32_t* face_id, void* stream) {
  NR_REQUIRE(V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX, NR_ERR_ARG,
             "nr_mesh_sample: vertex and face counts must be in [0, INT32_MAX]");
  NR_REQUIRE(n >= 0 && n <= INT32_MAX, NR_ERR_ARG, "nr_mesh_sample: the sample count must be in [0, INT32_MAX]");
  NR_REQUIRE((verts || V == 0) && ((faces && cdf) || F == 0) && (u || n == 0), NR_ERR_ARG,
             "nr_mesh_sample: null argument");
  NR_REQUIRE((points && face_id) || n == 0, NR_ERR_ARG, "nr_mesh_sample: null output");
  if (n == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  NR_LAUNCH("mesh_sample", (double)n, ms_sample, dim3((unsigned)((n + kMsWG - 1) / kMsWG)), dim3(kMsWG), st, verts, V, faces,
            F, cdf, u, n, points, face_id);
  return NR_OK;
}

}  // extern "C"
