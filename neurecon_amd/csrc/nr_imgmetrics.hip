// neurecon_amd — image metrics of rendered frames on the device: the error sums behind PSNR and the depth
// L1 / RMSE, the structural similarity (SSIM) and the cosine between two normal maps
// (neurecon_amd/image_metrics.py).  The image half of a published result, beside the mesh metrics of
// nr_meshsample.hip / nr_nn.hip.
//
// Every output is a pure function of the inputs: two runs are bit-identical.  All arithmetic that defines a
// result is float64 with each operation rounded on its own: `#pragma clang fp contract(off)` below the includes
// and plain operators under it (why not the __d*_rn intrinsics: nr_common.h), so nothing fuses into an FMA.
// The float64 division and square root are correctly rounded.  There are no float atomics: every sum is a fixed
// tree.  tests/image_metrics_ref.py restates the three rules in numpy; the maps are compared by equality.
//
// Inputs (device).  pred, gt: fp32 [F, H, W, C], contiguous, channel last, 1 <= C <= 4 (what render_mesh
// returns; volume_render's rgb after a reshape).  mask: uint8 [F, H, W] or NULL; a pixel passes when its byte is
// not 0 (or there is no mask).  F, H, W >= 1 and F H W C < 2^31.
//
// Error rule (nr_img_error; C = 3: RGB PSNR, C = 1: depth L1 / RMSE).
//   A pixel COUNTS iff it passes the mask and all 2 C of its values are finite.  A pixel that passes the mask
//   but holds a non-finite value is EXCLUDED.  Per counted value d = (double)p - (double)g (exact).
//   out float64 [F, 4] = {sum of d d, sum of |d|, n_used, n_excluded}, the two counts in pixels.
//   Order of the sums: a thread adds its pixels in ascending order (pixel 2048 q + 256 i + t for workgroup q,
//   thread t, i = 0..7), channel by channel, each product d d rounded and then added; the 64 lanes of a wave
//   are added by an xor butterfly (32, 16, .., 1), the four waves left to right, the workgroups of a frame
//   left to right.  The order depends on the shape alone.
//
// SSIM rule (nr_img_ssim): Wang et al. 2004, per channel, population covariances, over the valid region
//   only.  The caller passes the 1-D window w[0 .. win) of float64 (device; win odd, 1 <= win <= 33) and the
//   constants C1, C2 >= 0.  For the output position (r, c), 0 <= r <= H - win, 0 <= c <= W - win, and each of the
//   five fields a in {x, y, x x, y y, x y} (x = pred, y = gt widened to float64; the products of two widened fp32
//   values are exact):
//       horizontal first:  h[j] = sum_i w[i] a[r + j, c + i]      j = 0 .. win - 1
//       vertical second:   m    = sum_j w[j] h[j]
//   every sum sequential in ascending tap order, starting FROM w[0] a[0] (not from 0), every product and every
//   addition rounded separately.  With mx, my, exx, eyy, exy the five results:
//       vx = exx - (mx mx),  vy = eyy - (my my),  cxy = exy - (mx my)
//       S = ((2 (mx my) + C1) (2 cxy + C2)) / ((((mx mx) + (my my)) + C1) ((vx + vy) + C2))
//   map (optional, float64 [F, H - win + 1, W - win + 1, C]) = S.  A map value is NaN exactly where its window
//   covers a non-finite input: the arithmetic gives that by itself (inf - inf, 0 inf).
//   out float64 [F, 3] = {sum of S, n_used, n_nan}: over the map values of the frame whose CENTRE pixel
//   (r + win / 2, c + win / 2) passes the mask, the sum and the count of those that are not NaN, and the count
//   of those that are NaN.  Both counts are in map values (C per position).
//   H < win or W < win: the map is empty, out = {0, 0, 0}: no error.
//   Order of the sum: a thread adds its values channel by channel, and within a channel in ascending position
//   (tile position 512 i + t, row-major in the tile's 32 columns); then butterfly, the eight waves, the tiles of a
//   frame left to right (row-major over the tiles), as above.
//   This equals scikit-image's structural_similarity(gaussian_weights=True, use_sample_covariance=False) with
//   the window the caller passes: scikit-image crops the border its reflected filter touches, the same region.
//
// Normal rule (nr_img_normal_cos).  a, b fp32 [P, 3], mask uint8 [P] or NULL, out float64 [P]:
//       dot = ((ax bx) + (ay by)) + (az bz),  na = ((ax ax) + (ay ay)) + (az az),  nb likewise
//       cos = dot / sqrt(na nb), clamped to [-1, 1]
//   NaN where the mask is 0, where one of the six values is not finite, and where na nb == 0.
//
// The SSIM kernel (im_ssim).  One workgroup of 512 threads owns one output tile of TH rows x 32 columns of one
// frame and loops over the channels.  Per channel it stages the fp32 tile plus halo of both images in LDS
// ((TH + win - 1) x (31 + win) each, zero outside the image: never read from memory), runs the horizontal pass
// into five float64 planes of (TH + win - 1) x 32 in LDS, and the vertical pass from there; it writes the map
// if asked, and at the end one partial {sum, n_used, n_nan} per workgroup.  A one-workgroup pass (im_finish)
// adds the partials of every frame in index order.  Each input is read once plus halo.
//   CONDITION: a tile is at most 64 pixels in either dimension (it is at most 32 x 32).
//   Every loop is bounded by the shapes (win, C, TH, the tile counts); none has a data-dependent trip count.
//   LDS: (TH + win - 1) (8 (31 + win) + 1280) bytes of dynamic LDS, at most 63 KiB, plus under 400 bytes static:
//   two workgroups fit the 160 KiB of a CU.  TH = min(32, 64512 / (8 (31 + win) + 1280) - (win - 1)):
//   32 for win <= 9, 29 for win = 11 (63024 bytes), 4 for win = 33.
//   Banks: every plane keeps the column innermost, 32 float64 = 256 bytes = one bank row per plane row.  A
//   half-wave (the conflict group of ds_read_b64 / ds_write_b64) touches 32 consecutive float64, every bank
//   once, in both passes; the other half-wave sits one row further.  The fp32 reads of the horizontal pass are
//   32 consecutive floats per half-wave at offset i.  The window is read at one address by all lanes
//   (a broadcast).  No padding is needed.
// Workspace: 8 bytes x max(4 F ceil(H W / 2048), 3 F ceil(H / TH) ceil(W / 32)), rounded up to 256.
#include "nr_meshcommon.h"

#pragma clang fp contract(off)  // no a * b + c -> fma anywhere in this file (header comment)

namespace nr {

constexpr int kImWG = 256;                     // threads per workgroup
constexpr int kImSsimWG = 512;                 // ... of the SSIM kernel: eight waves share one tile's LDS
constexpr int kImTW = 32;                      // output columns per SSIM tile
constexpr int kImMaxTH = 32;                   // output rows per SSIM tile, at most
constexpr int kImMaxWin = 33;
constexpr int kImStrip = 8;                    // pixels per thread of the error kernel
constexpr int kImChunk = kImWG * kImStrip;     // pixels per workgroup of the error kernel
constexpr size_t kImLds = 65536 - 1024;        // dynamic LDS of im_ssim, at most

__device__ __forceinline__ bool im_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// Sum over the workgroup in a fixed tree: xor butterfly over each wave, then the waves left to right.  The
// result in every thread.  lds: WG / 64 slots.  Holds two barriers: every thread must call it.
template <int WG, class T>
__device__ __forceinline__ T im_wg_sum(T v, T* lds) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = lds[0];
#pragma unroll
  for (int w = 1; w < WG / 64; ++w) t = t + lds[w];
  __syncthreads();
  return t;
}

// partial[(f chunks + q) 4 + {0..3}] = {sum d d, sum |d|, n_used, n_excluded} of the workgroup's 2048 pixels
__global__ __launch_bounds__(kImWG) void im_error(const float* __restrict__ pred, const float* __restrict__ gt,
                                                  const uint8_t* __restrict__ mask, int64_t P, int C, int chunks,
                                                  double* __restrict__ partial) {
  __shared__ double red[kImWG / 64];
  __shared__ int redi[kImWG / 64];
  const int tid = threadIdx.x;
  const int q = blockIdx.x % chunks;
  const int64_t f = blockIdx.x / chunks;
  const int64_t base = (int64_t)q * kImChunk;
  double ss = 0.0, sa = 0.0;
  int nu = 0, ne = 0;
#pragma unroll
  for (int i = 0; i < kImStrip; ++i) {
    const int64_t px = base + (int64_t)i * kImWG + tid;
    if (px >= P) continue;
    const int64_t at = f * P + px;
    if (mask && mask[at] == 0) continue;
    double d[4];
    bool fin = true;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      d[c] = 0.0;
      if (c < C) {
        const float p = pred[at * C + c], g = gt[at * C + c];
        fin = fin && im_finite(p) && im_finite(g);
        d[c] = (double)p - (double)g;
      }
    }
    if (!fin) {
      ++ne;
      continue;
    }
    ++nu;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) {
        ss = ss + d[c] * d[c];
        sa = sa + fabs(d[c]);
      }
  }
  ss = im_wg_sum<kImWG>(ss, red);
  sa = im_wg_sum<kImWG>(sa, red);
  nu = im_wg_sum<kImWG>(nu, redi);
  ne = im_wg_sum<kImWG>(ne, redi);
  if (tid == 0) {
    double* o = partial + (int64_t)blockIdx.x * 4;
    o[0] = ss, o[1] = sa, o[2] = (double)nu, o[3] = (double)ne;
  }
}

// one workgroup: out[f K + k] = the partials [f][0 .. per_frame)[k] added left to right
__global__ __launch_bounds__(kImWG) void im_finish(const double* __restrict__ partial, int64_t per_frame, int K,
                                                   int64_t n, double* __restrict__ out) {
  for (int64_t i = threadIdx.x; i < n; i += kImWG) {
    const int64_t f = i / K;
    const int k = (int)(i - f * K);
    const double* p = partial + f * per_frame * K + k;
    double acc = 0.0;
    int64_t t = 0;
    for (; t + 16 <= per_frame; t += 16) {  // 16 loads in flight, then the 16 additions in order
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = p[(t + u) * K];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc = acc + v[u];
    }
    for (; t < per_frame; ++t) acc = acc + p[t * K];
    out[i] = acc;
  }
}

__global__ __launch_bounds__(kImSsimWG) void im_ssim(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const uint8_t* __restrict__ mask, int H, int W, int C, int win,
                                                     int TH, int tiles_x, int tiles_y,
                                                     const double* __restrict__ window, double C1, double C2,
                                                     double* __restrict__ map, double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char im_lds[];
  __shared__ double sw[kImMaxWin];
  __shared__ double red[kImSsimWG / 64];
  __shared__ int redi[kImSsimWG / 64];
  const int tid = threadIdx.x;
  const int Ho = H - win + 1, Wo = W - win + 1;
  const int rows_in = TH + win - 1, cols_in = kImTW + win - 1;
  const int plane = rows_in * kImTW;
  double* hf = (double*)im_lds;                    // [5][rows_in][kImTW]
  float* sx = (float*)(hf + 5 * plane);            // [rows_in][cols_in]
  float* sy = sx + rows_in * cols_in;
  int b = blockIdx.x;
  const int c0 = (b % tiles_x) * kImTW;
  b /= tiles_x;
  const int r0 = (b % tiles_y) * TH;
  const int64_t f = b / tiles_y;
  const int64_t frame = f * H * W;                 // in pixels
  if (tid < win) sw[tid] = window[tid];
  double sum = 0.0;
  int nu = 0, nn = 0;
  for (int ch = 0; ch < C; ++ch) {
    // the tile plus halo of both images; zero outside the image (those results are never written)
    for (int it = tid; it < rows_in * cols_in; it += kImSsimWG) {
      const int rr = it / cols_in, cc = it - rr * cols_in;
      const int y = r0 + rr, x = c0 + cc;
      float p = 0.f, g = 0.f;
      if (y < H && x < W) {
        const int64_t at = (frame + (int64_t)y * W + x) * C + ch;
        p = pred[at], g = gt[at];
      }
      sx[it] = p, sy[it] = g;
    }
    __syncthreads();
    // horizontal pass: the five fields of every staged row at the tile's 32 columns
    for (int it = tid; it < plane; it += kImSsimWG) {
      const int rr = it / kImTW, cc = it - rr * kImTW;
      const float* px = sx + rr * cols_in + cc;
      const float* py = sy + rr * cols_in + cc;
      double w = sw[0], x = px[0], y = py[0];
      double hx = w * x, hy = w * y, hxx = w * (x * x), hyy = w * (y * y), hxy = w * (x * y);
      for (int i = 1; i < win; ++i) {
        w = sw[i], x = px[i], y = py[i];
        hx = hx + w * x;
        hy = hy + w * y;
        hxx = hxx + w * (x * x);
        hyy = hyy + w * (y * y);
        hxy = hxy + w * (x * y);
      }
      hf[it] = hx, hf[plane + it] = hy, hf[2 * plane + it] = hxx, hf[3 * plane + it] = hyy, hf[4 * plane + it] = hxy;
    }
    __syncthreads();
    // vertical pass and the formula
    for (int it = tid; it < TH * kImTW; it += kImSsimWG) {
      const int r = it / kImTW, c = it - r * kImTW;
      const int orow = r0 + r, ocol = c0 + c;
      if (orow >= Ho || ocol >= Wo) continue;
      double m[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) m[k] = sw[0] * hf[k * plane + it];
      for (int j = 1; j < win; ++j) {
        const double w = sw[j];
#pragma unroll
        for (int k = 0; k < 5; ++k) m[k] = m[k] + w * hf[k * plane + it + j * kImTW];
      }
      const double mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
      const double vx = m[2] - mxx, vy = m[3] - myy, cxy = m[4] - mxy;
      const double S = ((2.0 * mxy + C1) * (2.0 * cxy + C2)) / (((mxx + myy) + C1) * ((vx + vy) + C2));
      if (map) map[(((f * Ho + orow) * Wo + ocol)) * C + ch] = S;
      if (mask && mask[frame + (int64_t)(orow + win / 2) * W + (ocol + win / 2)] == 0) continue;
      if (S == S) {
        sum = sum + S;
        ++nu;
      } else {
        ++nn;
      }
    }
    // no barrier here: the next channel's staging writes sx / sy only, last read before the barrier above, and
    // its own barrier stands between this vertical pass and the next write of hf
  }
  sum = im_wg_sum<kImSsimWG>(sum, red);
  nu = im_wg_sum<kImSsimWG>(nu, redi);
  nn = im_wg_sum<kImSsimWG>(nn, redi);
  if (tid == 0) {
    double* o = partial + (int64_t)blockIdx.x * 3;
    o[0] = sum, o[1] = (double)nu, o[2] = (double)nn;
  }
}

__global__ __launch_bounds__(kImWG) void im_normal_cos(const float* __restrict__ a, const float* __restrict__ b,
                                                       const uint8_t* __restrict__ mask, int64_t P,
                                                       double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kImWG + threadIdx.x;
  if (i >= P) return;
  const float fa[3] = {a[3 * i], a[3 * i + 1], a[3 * i + 2]}, fb[3] = {b[3 * i], b[3 * i + 1], b[3 * i + 2]};
  bool ok = !mask || mask[i] != 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && im_finite(fa[k]) && im_finite(fb[k]);
  const double ax = fa[0], ay = fa[1], az = fa[2], bx = fb[0], by = fb[1], bz = fb[2];
  const double dot = ((ax * bx) + (ay * by)) + (az * bz);
  const double na = ((ax * ax) + (ay * ay)) + (az * az), nb = ((bx * bx) + (by * by)) + (bz * bz);
  const double den = na * nb;
  double c = __builtin_nan("");
  if (ok && den != 0.0) {
    c = dot / __dsqrt_rn(den);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
  }
  out[i] = c;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int im_tile_rows(int64_t win) {
  const size_t per_row = 8 * (size_t)(kImTW + win - 1) + 5 * 8 * kImTW;
  const int64_t rows = (int64_t)(kImLds / per_row) - (win - 1);  // >= 4 for win <= 33
  return (int)(rows > kImMaxTH ? kImMaxTH : rows);
}

static size_t im_lds_bytes(int TH, int64_t win) {
  return (size_t)(TH + win - 1) * (8 * (size_t)(kImTW + win - 1) + 5 * 8 * kImTW);
}

// the shape checks every entry shares; false with the text in `why`
static bool im_shape_ok(int64_t F, int64_t H, int64_t W, int64_t C, const char*& why) {
  if (C < 1 || C > 4) {
    why = "C must be in 1..4";
    return false;
  }
  if (F < 1 || H < 1 || W < 1) {
    why = "F, H and W must be positive";
    return false;
  }
  const int64_t lim = (int64_t)1 << 31;
  if (F >= lim || H >= lim || W >= lim || F * H >= lim || F * H * W >= lim || F * H * W * C >= lim) {
    why = "F H W C must be below 2^31";
    return false;
  }
  return true;
}

static bool im_win_ok(int64_t win) { return win >= 1 && win <= kImMaxWin && (win & 1) == 1; }

static int64_t im_error_slots(int64_t F, int64_t H, int64_t W) { return F * ((H * W + kImChunk - 1) / kImChunk) * 4; }

static int64_t im_ssim_slots(int64_t F, int64_t H, int64_t W, int64_t win) {
  const int TH = im_tile_rows(win);
  return F * ((H + TH - 1) / TH) * ((W + kImTW - 1) / kImTW) * 3;
}

}  // namespace nr

using namespace nr;

extern "C" {

size_t nr_img_workspace_bytes(int64_t F, int64_t H, int64_t W, int64_t C, int64_t win) {
  const char* why = nullptr;
  if (!im_shape_ok(F, H, W, C, why) || !im_win_ok(win)) return 0;
  const int64_t e = im_error_slots(F, H, W), s = im_ssim_slots(F, H, W, win);
  return a256(8 * (size_t)(e > s ? e : s));
}

int nr_img_error(const float* pred, const float* gt, const uint8_t* mask, int64_t F, int64_t H, int64_t W, int64_t C,
                 double* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* why = nullptr;
  NR_REQUIRE(pred && gt, NR_ERR_ARG, "nr_img_error: null argument");
  NR_REQUIRE(out, NR_ERR_ARG, "nr_img_error: null output");
  NR_REQUIRE(im_shape_ok(F, H, W, C, why), NR_ERR_ARG, std::string("nr_img_error: ") + why);
  const int64_t chunks = (H * W + kImChunk - 1) / kImChunk;
  NR_REQUIRE(workspace && workspace_bytes >= a256(8 * (size_t)im_error_slots(F, H, W)), NR_ERR_WORKSPACE,
             "nr_img_error: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  NR_LAUNCH("img_error", (double)(F * H * W), im_error, dim3((unsigned)(F * chunks)), dim3(kImWG), st, pred, gt, mask,
            H * W, (int)C, (int)chunks, partial);
  NR_LAUNCH("img_finish", (double)(F * chunks), im_finish, dim3(1), dim3(kImWG), st, partial, chunks, 4, F * 4, out);
  return NR_OK;
}

int nr_img_ssim(const float* pred, const float* gt, const uint8_t* mask, int64_t F, int64_t H, int64_t W, int64_t C,
                const double* window, int64_t win, double C1, double C2, double* map, double* out, void* workspace,
                size_t workspace_bytes, void* stream) {
  const char* why = nullptr;
  NR_REQUIRE(pred && gt, NR_ERR_ARG, "nr_img_ssim: null argument");
  NR_REQUIRE(window, NR_ERR_ARG, "nr_img_ssim: null window");
  NR_REQUIRE(out, NR_ERR_ARG, "nr_img_ssim: null output");
  NR_REQUIRE(im_shape_ok(F, H, W, C, why), NR_ERR_ARG, std::string("nr_img_ssim: ") + why);
  NR_REQUIRE(im_win_ok(win), NR_ERR_ARG, "nr_img_ssim: win must be odd and in 1..33");
  NR_REQUIRE(C1 >= 0.0 && C2 >= 0.0 && C1 <= 1.79769313486231570e308 && C2 <= 1.79769313486231570e308, NR_ERR_ARG,
             "nr_img_ssim: C1 and C2 must be finite and >= 0");
  NR_REQUIRE(workspace && workspace_bytes >= a256(8 * (size_t)im_ssim_slots(F, H, W, win)), NR_ERR_WORKSPACE,
             "nr_img_ssim: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  const int TH = im_tile_rows(win);
  int64_t tiles_x = 0, tiles_y = 0;
  if (H >= win && W >= win) {
    tiles_y = (H - win + 1 + TH - 1) / TH;
    tiles_x = (W - win + 1 + kImTW - 1) / kImTW;
    const size_t lds = im_lds_bytes(TH, win);
    {
      ProfScope prof("img_ssim", (double)(F * H * W * C), st);
      hipLaunchKernelGGL(im_ssim, dim3((unsigned)(F * tiles_y * tiles_x)), dim3(kImSsimWG), lds, st, pred, gt, mask,
                         (int)H, (int)W, (int)C, (int)win, TH, (int)tiles_x, (int)tiles_y, window, C1, C2, map,
                         partial);
    }
    NR_HIP_CHECK(hipGetLastError());
  }
  NR_LAUNCH("img_finish", (double)(F * tiles_y * tiles_x), im_finish, dim3(1), dim3(kImWG), st, partial,
            tiles_y * tiles_x, 3, F * 3, out);
  return NR_OK;
}

int nr_img_normal_cos(const float* a, const float* b, const uint8_t* mask, int64_t P, double* out, void* stream) {
  NR_REQUIRE(P >= 0 && P <= INT32_MAX / 3, NR_ERR_ARG, "nr_img_normal_cos: 3 P must be in [0, 2^31)");
  NR_REQUIRE((a && b) || P == 0, NR_ERR_ARG, "nr_img_normal_cos: null argument");
  NR_REQUIRE(out || P == 0, NR_ERR_ARG, "nr_img_normal_cos: null output");
  if (P == 0) return NR_OK;
  hipStream_t st = (hipStream_t)stream;
  NR_LAUNCH("img_normal_cos", (double)P, im_normal_cos, dim3((unsigned)((P + kImWG - 1) / kImWG)), dim3(kImWG), st, a,
            b, mask, P, out);
  return NR_OK;
}

}  // extern "C"
