// neurecon_amd — culling an extracted mesh by what the training cameras constrain: the dilation of the
// cameras' object masks and the per-vertex, per-view test (in the image? inside the mask? in front of the
// mesh's own depth?) that the published DTU numbers of NeuS, VolSDF and UNISURF apply before the Chamfer
// distance is taken.  The counts feed mesh_cull.cull_mesh -> mesh_util.filter_mesh(vertex_mask=...).
//
// Every output is a pure function of the inputs: integers and bytes, decided by float64 arithmetic with each
// operation rounded on its own (dmul / dadd / ddiv of nr_common.h and the contract(off) pragma below) or by
// integer arithmetic.  tests/mesh_cull_ref.py restates both rules in numpy, operation for operation, and the
// device is compared to it by equality.
//
// Dilation (nr_mask_dilate).  in, out uint8 [B, H, W], not aliased; radius r >= 0.
//     out[b, j, i] = 1 iff some in-image pixel (j', i') with |j' - j| <= r and |i' - i| <= r has in[b, j', i'] != 0,
//     else 0: a square structuring element of side k = 2 r + 1, pixels outside the image count as 0 (what
//     cv2.dilate(mask, ones((k, k))) and scipy.ndimage.binary_dilation(structure=ones) give).  r = 0 copies in != 0.
//   Separable: the rows are dilated into `out`, then the columns of `out` in place (the second pass reads only the
//   workspace).  One pass over lines of length n (van Herk / Gil-Werman): the line is cut into blocks of k pixels
//   from its start; md_scan_rows / md_scan_cols give every pixel p two bits, g[p] = OR of the line from its block's
//   start to p and h[p] = OR from p to its block's end (columns: one thread per block walks it forwards and
//   backwards, at most k steps; rows: one wave per row walks it in chunks of 64 pixels, ceil(n / 64) steps each
//   way; whatever the data).  The window [lo, hi] = [max(p - r, 0), min(p + r, n - 1)] has at most k pixels, so it
//   touches at most two blocks, and md_combine reads
//       lo and hi in different blocks       h[lo] | g[hi]
//       the same block, lo its first pixel  g[hi]
//       the same block otherwise            h[lo]      (then hi = n - 1, the end of the last block: a window that
//                                                       is not clipped on the right and starts inside a block
//                                                       ends in the next one)
//   The cost per pixel does not depend on r.  Workspace: one byte per pixel, rounded up to 256 bytes.
//   Limits: 0 <= r < 2^15, H, W > 0, H W < 2^31, B >= 0, B H W < 2^32.
//
// View test (nr_mesh_view_test): the vertex stage of the renderer (nr_meshrender.hip, mr_setup) run against a
// batch of cameras.  cams float64 [n_views, 18]: W2C rows 0..2 (12 values), fx, fy, cx, cy, sk, near.  Per vertex
// (x, y, z) (fp32, widened) and view:
//       p_c[k] = (((W2C[k][0] x) + (W2C[k][1] y)) + (W2C[k][2] z)) + W2C[k][3]
//       x' = p_c.x / p_c.z,  y' = p_c.y / p_c.z
//       u = ((fx x') + (sk y')) + cx,  v = (fy y') + cy
//   in_image (bit 1) iff p_c.z, u, v are finite, p_c.z >= near, 0 <= u <= W - 1 and 0 <= v <= H - 1.
//   in_mask  (bit 2) iff in_image, masks are given and masks[view, (int) rint(v), (int) rint(u)] != 0: the nearest
//     pixel, round half to even; in range because of in_image.
//   visible  (bit 4) iff in_image, a depth frame is given and p_c.z <= zmax + depth_tol (one float64 addition);
//     zmax = the maximum over the samples (j0, i0), (j0, i1), (j1, i0), (j1, i1), i0 = floor(u), i1 = min(i0 + 1,
//     W - 1), j alike; a sample is +inf where face_id < 0 (a miss: nothing in front), else (double) zdepth.
//     The 2 x 2 footprint instead of the nearest pixel: a vertex of a locally planar visible surface lies within
//     the depth range of the four samples around its projection, so the tolerance absorbs curvature and
//     rounding, not slope x 1/2 pixel.  The price: at a silhouette a footprint that touches a miss says visible.
//   flags[view, vertex] = the OR of the bits; counts[vertex] = (n_in_image, n_in_mask, n_visible) over the views
//   of the call, added to what is there when `accumulate`.  One thread per vertex walks the views: no atomics,
//   the trip count is n_views.  There is no near-plane clipping: the limit is the renderer's.
//   Limits: 0 <= V <= INT32_MAX, n_views >= 0, H, W > 0, H W < 2^31.  V == 0 and n_views == 0 are valid.
#include "nr_meshcommon.h"

#pragma clang fp contract(off)  // no a * b + c -> fma anywhere in this file (header comment)

namespace nr {

constexpr int kMcWG = 256;

// the geometry of one pass: `lines` lines of n pixels, cut into nblk blocks of k; pixel p of line l is byte
// (l / inner) * outer + (l % inner) * lstep + p * step.  Rows: inner = 1 (outer = W, step = 1, n = W);
// columns: inner = W (outer = H W, lstep = 1, step = W, n = H).
struct MdPass {
  int64_t lines, inner, outer, lstep, step;
  int n, k, r, nblk;
};

__device__ __forceinline__ int64_t md_base(const MdPass& ps, int64_t line) {
  return (line / ps.inner) * ps.outer + (line % ps.inner) * ps.lstep;
}

// Rows: one wave per row walks it in chunks of 64 pixels, forwards for g and backwards for h, so every step is
// one contiguous run of bytes.  Inside a chunk the ORs are bit tests on the chunk's ballot; what a block
// carries across a chunk boundary is one bit, the g of the chunk's last pixel (the h of its first).  The rows
// are strided over a bounded grid; the trip counts are ceil(n / 64) and the rows per wave.
constexpr int kMdRowGrid = 1 << 20;

__global__ __launch_bounds__(kMcWG) void md_scan_rows(const uint8_t* __restrict__ in, uint8_t* __restrict__ gh,
                                                      int64_t rows, int n, int k) {
  const int l = threadIdx.x & 63;
  const int nchunk = (int)(((int64_t)n + 63) / 64);
  for (int64_t row = (int64_t)blockIdx.x * (kMcWG / 64) + (threadIdx.x >> 6); row < rows;  // wave-uniform
       row += (int64_t)gridDim.x * (kMcWG / 64)) {
    const uint8_t* src = in + row * n;
    uint8_t* dst = gh + row * n;
    unsigned carry = 0;
    for (int c = 0; c < nchunk; ++c) {
      const int64_t c0 = (int64_t)c * 64, p = c0 + l;
      const bool live = p < n;
      const unsigned long long bits = __ballot(live && src[p] != 0);
      unsigned g = 0;
      if (live) {
        const int64_t s = (p / k) * k;  // the block's first pixel
        const int lo = s > c0 ? (int)(s - c0) : 0;
        const unsigned long long m = bits & ((2ull << l) - 1ull) & ~((1ull << lo) - 1ull);  // lanes lo .. l
        g = (m != 0 || (s < c0 && carry != 0)) ? 1u : 0u;
        dst[p] = (uint8_t)g;
      }
      carry = __shfl(g, 63);
    }
    carry = 0;
    for (int c = nchunk - 1; c >= 0; --c) {
      const int64_t c0 = (int64_t)c * 64, p = c0 + l;
      const bool live = p < n;
      const unsigned long long bits = __ballot(live && src[p] != 0);
      unsigned h = 0;
      if (live) {
        const int64_t s = (p / k) * k;
        const int64_t last = (s + k < n ? s + k : (int64_t)n) - 1;  // the block's last pixel
        const int hi = last < c0 + 63 ? (int)(last - c0) : 63;
        const unsigned long long m = bits & ~((1ull << l) - 1ull) & ((2ull << hi) - 1ull);  // lanes l .. hi
        h = (m != 0 || (last > c0 + 63 && carry != 0)) ? 2u : 0u;
        dst[p] = (uint8_t)(dst[p] | h);  // this lane's own store above
      }
      carry = __shfl(h, 0);
    }
  }
}

// Columns: one thread per (column, block); consecutive threads take the same block of consecutive columns, so
// each step of a wave is one contiguous run of bytes.
__global__ __launch_bounds__(kMcWG) void md_scan_cols(const uint8_t* __restrict__ in, uint8_t* __restrict__ gh, MdPass ps) {
  const int64_t t = (int64_t)blockIdx.x * kMcWG + threadIdx.x;
  if (t >= ps.lines * ps.nblk) return;
  const int64_t line = t % ps.lines;
  const int blk = (int)(t / ps.lines);
  const int64_t base = md_base(ps, line);
  const int s = blk * ps.k, e = (int)min((int64_t)s + ps.k, (int64_t)ps.n);  // s <= n - 1
  unsigned acc = 0;
  for (int p = s; p < e; ++p) {
    const int64_t at = base + (int64_t)p * ps.step;
    acc |= in[at] != 0 ? 1u : 0u;
    gh[at] = (uint8_t)acc;
  }
  acc = 0;
  for (int p = e - 1; p >= s; --p) {
    const int64_t at = base + (int64_t)p * ps.step;
    acc |= in[at] != 0 ? 2u : 0u;
    gh[at] = (uint8_t)(gh[at] | acc);  // this thread's own store above
  }
}

// one thread per pixel, in memory order
template <bool ROWS>
__global__ __launch_bounds__(kMcWG) void md_combine(const uint8_t* __restrict__ gh, uint8_t* __restrict__ out, MdPass ps,
                                                    int64_t npix) {
  const int64_t t = (int64_t)blockIdx.x * kMcWG + threadIdx.x;
  if (t >= npix) return;
  int64_t line;
  int p;
  if (ROWS) {
    line = t / ps.n, p = (int)(t % ps.n);
  } else {  // t = (b H + j) W + i: line = b W + i, p = j
    const int64_t img = t / ps.outer, rem = t % ps.outer;
    line = img * ps.inner + rem % ps.inner, p = (int)(rem / ps.inner);
  }
  const int64_t base = md_base(ps, line);
  const int lo = max(p - ps.r, 0), hi = (int)min((int64_t)p + ps.r, (int64_t)ps.n - 1);
  const int bl = lo / ps.k, bh = hi / ps.k;
  const unsigned a = gh[base + (int64_t)lo * ps.step], b = gh[base + (int64_t)hi * ps.step];
  unsigned o;
  if (bl != bh)
    o = (a >> 1) | (b & 1u);
  else if (lo - bl * ps.k == 0)
    o = b & 1u;
  else
    o = a >> 1;
  out[t] = (uint8_t)(o & 1u);
}

__global__ __launch_bounds__(kMcWG) void mc_view_test(const float* __restrict__ verts, int64_t V, int64_t n_views,
                                                      const double* __restrict__ cams, int H, int W,
                                                      const uint8_t* __restrict__ masks, const float* __restrict__ zdepth,
                                                      const int* __restrict__ face_id, double depth_tol,
                                                      uint8_t* __restrict__ flags, int* __restrict__ counts,
                                                      int accumulate) {
  const int64_t t = (int64_t)blockIdx.x * kMcWG + threadIdx.x;
  if (t >= V) return;
  const double x = (double)verts[3 * t], y = (double)verts[3 * t + 1], z = (double)verts[3 * t + 2];
  const int64_t npix = (int64_t)H * W;
  const double umax = (double)(W - 1), vmax = (double)(H - 1);
  int n_image = 0, n_mask = 0, n_visible = 0;
  for (int64_t b = 0; b < n_views; ++b) {
    const double* c = cams + 18 * b;
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double* w = c + 4 * k;
      p[k] = dadd(dadd(dadd(dmul(w[0], x), dmul(w[1], y)), dmul(w[2], z)), w[3]);
    }
    const double fx = c[12], fy = c[13], cx = c[14], cy = c[15], sk = c[16], near = c[17];
    const double xp = ddiv(p[0], p[2]), yp = ddiv(p[1], p[2]);
    const double u = dadd(dadd(dmul(fx, xp), dmul(sk, yp)), cx);
    const double v = dadd(dmul(fy, yp), cy);
    const bool in_image = isfinite(p[2]) && isfinite(u) && isfinite(v) && p[2] >= near && u >= 0.0 && u <= umax &&
                          v >= 0.0 && v <= vmax;
    unsigned bits = 0;
    if (in_image) {
      bits = 1;
      const int64_t frame = b * npix;
      if (masks) {
        const int i = (int)rint(u), j = (int)rint(v);
        if (masks[frame + (int64_t)j * W + i] != 0) bits |= 2u;
      }
      if (zdepth) {
        const int i0 = (int)floor(u), j0 = (int)floor(v);
        const int i1 = min(i0 + 1, W - 1), j1 = min(j0 + 1, H - 1);
        const int64_t at[4] = {frame + (int64_t)j0 * W + i0, frame + (int64_t)j0 * W + i1, frame + (int64_t)j1 * W + i0,
                               frame + (int64_t)j1 * W + i1};
        double zmax = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double s = face_id[at[q]] < 0 ? (double)INFINITY : (double)zdepth[at[q]];
          zmax = (q == 0 || s > zmax) ? s : zmax;
        }
        if (p[2] <= dadd(zmax, depth_tol)) bits |= 4u;
      }
    }
    if (flags) flags[b * V + t] = (uint8_t)bits;
    n_image += (int)(bits & 1u);
    n_mask += (int)((bits >> 1) & 1u);
    n_visible += (int)((bits >> 2) & 1u);
  }
  if (counts) {
    int* o = counts + 3 * t;
    if (accumulate) n_image += o[0], n_mask += o[1], n_visible += o[2];
    o[0] = n_image, o[1] = n_mask, o[2] = n_visible;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static bool md_plan(int64_t B, int64_t H, int64_t W, int64_t& npix) {
  if (B < 0 || H <= 0 || W <= 0 || H > INT32_MAX || W > INT32_MAX) return false;
  if (H > INT32_MAX / W) return false;  // H W < 2^31
  if (B > ((int64_t)1 << 32) / (H * W)) return false;
  npix = B * H * W;
  return npix < ((int64_t)1 << 32);
}

template <bool ROWS>
static int md_pass(const uint8_t* in, uint8_t* out, uint8_t* gh, const MdPass& ps, int64_t npix, hipStream_t st) {
  if (ROWS) {
    const int64_t nwg = (ps.lines + kMcWG / 64 - 1) / (kMcWG / 64);
    NR_LAUNCH("md_scan_rows", (double)npix, md_scan_rows, dim3((unsigned)(nwg < kMdRowGrid ? nwg : kMdRowGrid)), dim3(kMcWG), st,
              in, gh, ps.lines, ps.n, ps.k);
  } else {
    const int64_t nscan = ps.lines * ps.nblk;  // <= B H W
    NR_LAUNCH("md_scan_cols", (double)npix, md_scan_cols, dim3((unsigned)((nscan + kMcWG - 1) / kMcWG)), dim3(kMcWG), st, in,
              gh, ps);
  }
  NR_LAUNCH(ROWS ? "md_combine_rows" : "md_combine_cols", (double)npix, md_combine<ROWS>,
            dim3((unsigned)((npix + kMcWG - 1) / kMcWG)), dim3(kMcWG), st, gh, out, ps, npix);
  return NR_OK;
}

}  // namespace nr

using namespace nr;

extern "C" {

size_t nr_mask_dilate_workspace_bytes(int64_t B, int64_t H, int64_t W) {
  int64_t npix;
  return md_plan(B, H, W, npix) ? a256((size_t)npix) : 0;
}

int nr_mask_dilate(const uint8_t* in, uint8_t* out, int64_t B, int64_t H, int64_t W, int64_t radius, void* workspace,
                   size_t workspace_bytes, void* stream) {
  NR_REQUIRE(H > 0 && W > 0, NR_ERR_ARG, "nr_mask_dilate: H and W must be positive");
  NR_REQUIRE(B >= 0, NR_ERR_ARG, "nr_mask_dilate: B must not be negative");
  NR_REQUIRE(radius >= 0 && radius < 32768, NR_ERR_ARG, "nr_mask_dilate: needs 0 <= radius < 2^15");
  int64_t npix;
  NR_REQUIRE(md_plan(B, H, W, npix), NR_ERR_ARG, "nr_mask_dilate: needs H * W < 2^31 and B * H * W < 2^32");
  if (npix == 0) return NR_OK;
  NR_REQUIRE(in && out, NR_ERR_ARG, "nr_mask_dilate: null in or out");
  {
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    NR_REQUIRE(a + (uintptr_t)npix <= b || b + (uintptr_t)npix <= a, NR_ERR_ARG, "nr_mask_dilate: in and out must not alias");
  }
  NR_REQUIRE(workspace && workspace_bytes >= a256((size_t)npix), NR_ERR_WORKSPACE, "nr_mask_dilate: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* gh = (uint8_t*)workspace;
  const int r = (int)radius, k = 2 * r + 1;
  MdPass rows;
  rows.lines = B * H, rows.inner = 1, rows.outer = W, rows.lstep = 0, rows.step = 1;
  rows.n = (int)W, rows.k = k, rows.r = r, rows.nblk = (int)((W + k - 1) / k);
  MdPass cols;
  cols.lines = B * W, cols.inner = W, cols.outer = H * W, cols.lstep = 1, cols.step = W;
  cols.n = (int)H, cols.k = k, cols.r = r, cols.nblk = (int)((H + k - 1) / k);
  int rc = md_pass<true>(in, out, gh, rows, npix, st);
  if (rc) return rc;
  return md_pass<false>(out, out, gh, cols, npix, st);
}

int nr_mesh_view_test(const NrMeshViewArgs* a, void* stream) {
  NR_REQUIRE(a, NR_ERR_ARG, "nr_mesh_view_test: null argument");
  NR_REQUIRE(a->V >= 0 && a->n_views >= 0, NR_ERR_ARG, "nr_mesh_view_test: vertex and view counts must not be negative");
  NR_REQUIRE(a->V <= INT32_MAX && a->n_views <= INT32_MAX, NR_ERR_ARG,
             "nr_mesh_view_test: needs V <= INT32_MAX and n_views <= INT32_MAX");
  NR_REQUIRE(a->H > 0 && a->W > 0, NR_ERR_ARG, "nr_mesh_view_test: H and W must be positive");
  NR_REQUIRE(a->H <= INT32_MAX && a->W <= INT32_MAX && a->H <= INT32_MAX / a->W, NR_ERR_ARG,
             "nr_mesh_view_test: needs H * W < 2^31");
  NR_REQUIRE((a->zdepth != nullptr) == (a->face_id != nullptr), NR_ERR_ARG,
             "nr_mesh_view_test: zdepth and face_id must be given together");
  NR_REQUIRE(a->depth_tol - a->depth_tol == 0.0 && a->depth_tol >= 0.0, NR_ERR_ARG,
             "nr_mesh_view_test: depth_tol must be finite and not negative");
  NR_REQUIRE(a->cams || a->n_views == 0, NR_ERR_ARG, "nr_mesh_view_test: null cams");
  NR_REQUIRE(a->verts || a->V == 0, NR_ERR_ARG, "nr_mesh_view_test: null verts");
  NR_REQUIRE(a->accumulate == 0 || a->accumulate == 1, NR_ERR_ARG, "nr_mesh_view_test: accumulate must be 0 or 1");
  if (a->V == 0 || (!a->flags && !a->counts)) return NR_OK;
  if (a->n_views == 0 && (!a->counts || a->accumulate)) return NR_OK;
  NR_LAUNCH("mc_view_test", (double)a->V * (double)a->n_views, mc_view_test,
            dim3((unsigned)((a->V + kMcWG - 1) / kMcWG)), dim3(kMcWG), (hipStream_t)stream, a->verts, a->V, a->n_views,
            a->cams, (int)a->H, (int)a->W, a->masks, a->zdepth, a->face_id, a->depth_tol, a->flags, a->counts,
            a->accumulate);
  return NR_OK;
}

}  // extern "C"
