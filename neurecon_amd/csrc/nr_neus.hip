// neurecon_amd — NeuS render path for gfx950: per-ray sampling / compositing kernels and the
// orchestration of one ray chunk (models/frameworks/neus.py:118-397, render mode).
//
// Per-ray state is stored sample-major ([sample][ray]) so the one-thread-per-ray kernels read
// and write coalesced lines; the MLP kernels see a flat point list p = sample * Rc + ray.
// Scans (cumsum / cumprod) accumulate in fp64 exactly like ATen's CPU kernels
// (acc_type<float, is_cuda=false> = double), each prefix rounded to fp32.
#include <algorithm>
#include <cstdint>
#include <mutex>

#include "nr_common.h"
#include "nr_composite.h"
#include "nr_mlp.h"
#include "nr_neus.h"
#include "nr_render.h"

namespace nr {

__device__ __forceinline__ float4 load3(const float* p) { return make_float4(p[0], p[1], p[2], 0.f); }

// ---------------------------------------------------------------------------------------------
// prologue: normalize rays_d (neus.py:169-172), near/far (rend_util.py:167-185), coarse depths
// (neus.py:209-210) and their points (neus.py:251)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void neus_prologue(NeusChunk c, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                              const float* __restrict__ t_coarse, float r_obj, float near_bypass, float far_bypass) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= c.R) return;
  const float ox = rays_o[r * 3 + 0], oy = rays_o[r * 3 + 1], oz = rays_o[r * 3 + 2];
  float dx = rays_d[r * 3 + 0], dy = rays_d[r * 3 + 1], dz = rays_d[r * 3 + 2];
  normalize3(dx, dy, dz);
  c.ro[r * 3 + 0] = ox; c.ro[r * 3 + 1] = oy; c.ro[r * 3 + 2] = oz;
  c.rd[r * 3 + 0] = dx; c.rd[r * 3 + 1] = dy; c.rd[r * 3 + 2] = dz;
  const float mid = -fadd(fadd(fmul(ox, dx), fmul(oy, dy)), fmul(oz, dz));
  float nr = fmaxf(fsub(mid, r_obj), 0.0f);
  float fr = fmaxf(fadd(mid, r_obj), r_obj);
  if (!__builtin_isnan(near_bypass)) nr = near_bypass;
  if (!__builtin_isnan(far_bypass)) fr = far_bypass;
  c.near[r] = nr;
  c.far[r] = fr;
  for (int s = 0; s < c.N_samples; ++s) {
    const float t = t_coarse[s];
    const float d = fadd(fmul(nr, fsub(1.0f, t)), fmul(fr, t));
    const int64_t q = (int64_t)s * c.R + r;
    c.dv[q] = d;
    if (c.idv) c.idv[q] = s;
    c.pts[q * 3 + 0] = fadd(ox, fmul(dx, d));
    c.pts[q * 3 + 1] = fadd(oy, fmul(dy, d));
    c.pts[q * 3 + 2] = fadd(oz, fmul(dz, d));
  }
}

// sample_pdf(bins=dv[0..L), weights=wtmp[0..L-1) (already +1e-5), N=n, u) -> out[k*R + r]
// total = sum of the (+1e-5) weights.  rend_util.py:255-292.
__device__ void sample_pdf_ray(const float* __restrict__ bins, const float* __restrict__ w, int64_t stride, int L,
                               float total, const float* __restrict__ u, int n, float* __restrict__ out,
                               int64_t out_stride) {
  // w[i] are the raw weights; the +1e-5 of rend_util.py:259 is applied on the fly
  int k = 0;
  const float b_first = bins[0];
  while (k < n && u[k] <= 0.0f) {  // searchsorted -> 0: below = above = 0
    out[k * out_stride] = invert_one(u[k], 0.0f, 0.0f, b_first, b_first);
    ++k;
  }
  double acc = 0.0;
  float c_prev = 0.0f, b_prev = b_first;
  for (int i = 0; i < L - 1 && k < n; ++i) {
    acc += (double)fdiv(fadd(w[i * stride], 1e-5f), total);
    const float c_next = (float)acc;
    const float b_next = bins[(i + 1) * stride];
    while (k < n && u[k] <= c_next) {
      out[k * out_stride] = invert_one(u[k], c_prev, c_next, b_prev, b_next);
      ++k;
    }
    c_prev = c_next;
    b_prev = b_next;
  }
  // u above every cdf value: searchsorted -> L, below = above = L-1 (c_prev = cdf[L-1] here)
  for (; k < n; ++k) out[k * out_stride] = invert_one(u[k], c_prev, c_prev, b_prev, b_prev);
}

// sample_pdf with det=False (rend_util.py:268-290): the caller's uniforms u[0..n) are in any order,
// so each draw does its own searchsorted(cdf, u, right=False).  The cdf overwrites the weights in
// place (w[i] <- cdf[i+1], same fp64 running sum as above) and is binary-searched per draw.
__device__ void sample_pdf_ray_rand(const float* __restrict__ bins, float* __restrict__ w, int64_t stride, int L,
                                    float total, const float* __restrict__ u, int n, float* __restrict__ out,
                                    int64_t out_stride) {
  double acc = 0.0;
  for (int i = 0; i < L - 1; ++i) {
    acc += (double)fdiv(fadd(w[i * stride], 1e-5f), total);
    w[i * stride] = (float)acc;
  }
  auto cdf = [&](int j) { return j == 0 ? 0.0f : w[(int64_t)(j - 1) * stride]; };
  for (int k = 0; k < n; ++k) {
    const float uk = u[k];
    int lo = 0, hi = L;  // first j in [0, L) with cdf[j] >= uk, L if none
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (cdf(m) >= uk) hi = m; else lo = m + 1;
    }
    const int below = lo > 0 ? lo - 1 : 0, above = lo < L - 1 ? lo : L - 1;
    out[k * out_stride] = invert_one(uk, cdf(below), cdf(above), bins[below * stride], bins[above * stride]);
  }
}

// one "official_solution" upsampling round (neus.py:252-276): RPW rays per wave (64 / RPW lanes each).  The per-interval
// work (slopes, logistic CDFs, alpha) runs across the lanes; the three order-sensitive scans
// (transmittance cumprod, the ATen-order weight sum, the CDF cumsum) run on lane 0 over LDS with
// exactly the arithmetic of the per-ray version; the n_up inverse-CDF draws run across lanes.
// u: the round's uniforms, u[r * u_stride + k] (u_stride 0: the shared deterministic linspace)
template <int RPW>
__global__ __launch_bounds__(64) void neus_upsample(NeusChunk c, int it, const float* __restrict__ u, int64_t u_stride) {
  extern __shared__ float lds[];
  constexpr int NL = 64 / RPW;  // lanes per ray
  const int r = blockIdx.x * RPW + (int)threadIdx.x / NL, l = (int)threadIdx.x % NL;
  const int L = c.N_samples + it * c.n_up;  // last round's samples were merged by neus_merge
  const int64_t R = c.R;
  const bool live = r < R;
  const int Ll = live ? L : 0;  // a ray past the chunk's end only joins the barriers
  float* sz = lds + ((int)threadIdx.x / NL) * (5 * c.S + 1);  // depths [L]
  float* ss = sz + c.S;      // sdf [L]
  float* sa = ss + c.S;      // alpha, then weights [L-1]
  float* scdf = sa + c.S;    // (1 - alpha + 1e-10) factors [L-1], then the cdf [L]
  float* sq = scdf + c.S;    // normalised weights [L-1]
  float* stot = sq + c.S;    // [1] weight total
  for (int i = l; i < Ll; i += NL) {
    sz[i] = c.dv[i * R + r];
    ss[i] = c.sv[i * R + r];
  }
  __syncthreads();
  const float S = (float)(64 << it);  // 64 * 2**i
  for (int i = l; i < Ll - 1; i += NL) {
    const float s0 = ss[i], s1 = ss[i + 1], z0 = sz[i], z1 = sz[i + 1];
    const float mid = fmul(fadd(s0, s1), 0.5f);
    const float slope = fdiv(fsub(s1, s0), fadd(fsub(z1, z0), 1e-5f));
    const float prev_slope = i > 0 ? fdiv(fsub(s0, ss[i - 1]), fadd(fsub(z0, sz[i - 1]), 1e-5f)) : 0.0f;
    float m = fminf(prev_slope, slope);
    m = fminf(fmaxf(m, -10.0f), 0.0f);
    const float dist = fsub(z1, z0);
    const float md = fmul(fmul(m, dist), 0.5f);
    const float c0 = sigmoidf_ref(fmul(fsub(mid, md), S));
    const float c1 = sigmoidf_ref(fmul(fadd(mid, md), S));
    const float alpha = fdiv(fadd(fsub(c0, c1), 1e-5f), fadd(c0, 1e-5f));
    sa[i] = alpha;
    scdf[i] = transparency(alpha);  // the transmittance factor, off the serial chain
  }
  __syncthreads();
  if (l == 0 && live) {
    double T = 1.0;
    for (int i = 0; i < L - 1; ++i) {
      sa[i] = fmul(sa[i], (float)T);
      T *= (double)scdf[i];
    }
    stot[0] = aten_row_sum(L - 1, [&](int i) { return fadd(sa[i], 1e-5f); });
  }
  __syncthreads();
  {  // sample_pdf's normalised weights (rend_util.py:259-264) across the lanes
    const float total = stot[0];
    for (int i = l; i < Ll - 1; i += NL) sq[i] = fdiv(fadd(sa[i], 1e-5f), total);
  }
  __syncthreads();
  if (l == 0 && live) {  // ... and their fp64 running sum
    double acc = 0.0;
    scdf[0] = 0.0f;
    for (int i = 0; i < L - 1; ++i) {
      acc += (double)sq[i];
      scdf[i + 1] = (float)acc;
    }
  }
  __syncthreads();
  if (!live) return;
  const float ox = c.ro[r * 3], oy = c.ro[r * 3 + 1], oz = c.ro[r * 3 + 2];
  const float dx = c.rd[r * 3], dy = c.rd[r * 3 + 1], dz = c.rd[r * 3 + 2];
  for (int k = l; k < c.n_up; k += NL) {
    const float uk = u[r * u_stride + k];
    float d;
    if (uk <= 0.0f) {  // searchsorted -> 0: below = above = 0
      d = invert_one(uk, 0.0f, 0.0f, sz[0], sz[0]);
    } else {
      int lo = 0, hi = L - 1;  // first interval i with uk <= cdf[i+1]
      while (lo < hi) {
        const int mm = (lo + hi) >> 1;
        if (uk <= scdf[mm + 1]) hi = mm; else lo = mm + 1;
      }
      d = lo < L - 1 ? invert_one(uk, scdf[lo], scdf[lo + 1], sz[lo], sz[lo + 1])
                     : invert_one(uk, scdf[L - 1], scdf[L - 1], sz[L - 1], sz[L - 1]);  // above every cdf
    }
    const int64_t q = k * R + r;
    c.dnew[q] = d;
    c.pts[q * 3 + 0] = fadd(ox, fmul(dx, d));
    c.pts[q * 3 + 1] = fadd(oy, fmul(dy, d));
    c.pts[q * 3 + 2] = fadd(oz, fmul(dz, d));
  }
}

template __global__ void neus_upsample<1>(NeusChunk, int, const float*, int64_t);
template __global__ void neus_upsample<4>(NeusChunk, int, const float*, int64_t);

// merge (neus.py:276: cat + sort + gather) of the sorted list (dv, sv, idv)[0..L) with the n_up new
// samples (dnew, snew) into (dv2, sv2, idv2)[0..L+n_up), one thread per (output element, ray):
// old element i lands at i + #(new < d_i), new element j at rank_j + #(old <= d_j) (stable; ties put
// new after old) — the order of a stable sort of the concatenation.
// sort key: NaN after everything (torch.sort order), so positions stay a permutation for any input
__device__ __forceinline__ float merge_key(float v) { return v != v ? __builtin_inff() : v; }

__global__ void neus_merge(NeusChunk c, int L, float* __restrict__ dv2, float* __restrict__ sv2,
                           int* __restrict__ idv2) {
  const int64_t R = c.R;
  const int n = c.n_up;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)(L + n) * R) return;
  const int64_t e = t / R, r = t - e * R;
  if (e < L) {
    const int64_t q = e * R + r;
    const float d = c.dv[q], kd = merge_key(d);
    int cnt = 0;
    for (int k = 0; k < n; ++k) cnt += merge_key(c.dnew[k * R + r]) < kd ? 1 : 0;
    const int64_t qo = (e + cnt) * R + r;
    dv2[qo] = d;
    sv2[qo] = c.sv[q];
    if (idv2) idv2[qo] = c.idv[q];
  } else {
    const int j = (int)(e - L);
    const float d = c.dnew[j * R + r], kd = merge_key(d);
    int rank = 0;
    for (int k = 0; k < n; ++k) {
      const float v = merge_key(c.dnew[k * R + r]);
      rank += (v < kd || (v == kd && k < j)) ? 1 : 0;
    }
    int lo = 0, hi = L;  // upper bound of d in the sorted old list
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (merge_key(c.dv[m * R + r]) <= kd) lo = m + 1; else hi = m;
    }
    const int64_t qo = (int64_t)(rank + lo) * R + r;
    dv2[qo] = d;
    sv2[qo] = c.snew[j * R + r];
    if (idv2) idv2[qo] = L + j;  // new samples were evaluated in slots L .. L+n-1
  }
}

// per (sample, ray) after the final merge: sample points (or, fused, the sorted nablas) and the
// S-1 mid-points d_mid = (d_s + d_{s-1}) / 2 (neus.py:284-288); sample-major, fully parallel
// gather = 0: the fused path's nablas are gathered later (neus_gather_nablas: the deferred reverse
// pass of a NeRF++ render runs after the background net)
__global__ void neus_expand(NeusChunk c, int gather) {
  const int64_t R = c.R;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)c.S * R) return;
  const int64_t s = q / R, r = q - s * R;
  const float ox = c.ro[r * 3], oy = c.ro[r * 3 + 1], oz = c.ro[r * 3 + 2];
  const float dx = c.rd[r * 3], dy = c.rd[r * 3 + 1], dz = c.rd[r * 3 + 2];
  const float d = c.dv[q];
  if (c.idv) {  // fused: nablas of the sorted samples from their evaluation slots
    if (gather) {
      const int64_t qs = (int64_t)c.idv[q] * R + r;
#pragma unroll
      for (int e = 0; e < 3; ++e) c.nab_f[q * 3 + e] = c.nraw[qs * 3 + e];
    }
  } else {
    c.pts[q * 3 + 0] = fadd(ox, fmul(dx, d));
    c.pts[q * 3 + 1] = fadd(oy, fmul(dy, d));
    c.pts[q * 3 + 2] = fadd(oz, fmul(dz, d));
  }
  if (s > 0) {
    const float dm = fmul(0.5f, fadd(d, c.dv[q - R]));
    const int64_t qm = q - R;
    c.dmid[qm] = dm;
    c.mids[qm * 3 + 0] = fadd(ox, fmul(dx, dm));
    c.mids[qm * 3 + 1] = fadd(oy, fmul(dy, dm));
    c.mids[qm * 3 + 2] = fadd(oz, fmul(dz, dm));
  }
}

// the fused path's sample nablas into sorted order (neus_expand's gather, run on its own)
__global__ void neus_gather_nablas(NeusChunk c) {
  const int64_t R = c.R;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)c.S * R) return;
  const int64_t r = q - (q / R) * R;
  const int64_t qs = (int64_t)c.idv[q] * R + r;
#pragma unroll
  for (int e = 0; e < 3; ++e) c.nab_f[q * 3 + e] = c.nraw[qs * 3 + e];
}

// compositing (neus.py:296, :346-380), RPW rays per wave (64 / RPW lanes each): logistic CDFs,
// alpha, radiance and unit normals per sample across the ray's lanes (LDS); the transmittance product
// and the fp64 rgb / acc / normal / depth accumulations on the ray's first lane in sample order,
// exactly as the per-ray version did.  RPW 4: the serial scans of four rays share one wave's issue.
// s = exp(ln_s * speed_factor) (neus.py:108-109): *s_dev when given (device scalar, no host sync), else s_val
template <int RPW>
__global__ __launch_bounds__(64) void neus_composite(NeusChunk c, NeusOut o, const float* __restrict__ s_dev,
                                                     float s_val, int calc_normal, int white_bkgd) {
  extern __shared__ float lds[];
  constexpr int NL = 64 / RPW;  // lanes per ray
  const float s_inv = s_dev ? *s_dev : s_val;
  const int r = blockIdx.x * RPW + (int)threadIdx.x / NL, l = (int)threadIdx.x % NL;
  const int S = c.S;
  const int64_t R = c.R;
  const bool live = r < R;
  const int Sl = live ? S : 0;    // a ray past the chunk's end only joins the barriers
  const int64_t ro = o.ray0 + r;  // global ray index for outputs
  float* scdf = lds + ((int)threadIdx.x / NL) * 9 * S;  // [S]
  float* sal = scdf + S;      // [S-1] alpha, then weights
  float* srad = sal + S;      // [S-1][3]
  float* snrm = srad + 3 * S; // [S-1][3] unit nablas
  float* sdm = snrm + 3 * S;  // [S-1] mid-point depths (the serial depth sum reads LDS, not HBM)
  for (int i = l; i < Sl; i += NL) {
    const float cdf = neus_cdf(c.sdf_f[i * R + r], s_inv);
    scdf[i] = cdf;
    if (o.cdf) o.cdf[ro * S + i] = cdf;
  }
  __syncthreads();
  for (int i = l; i < Sl - 1; i += NL) {
    const float alpha = neus_alpha(scdf[i], scdf[i + 1]);
    sal[i] = alpha;
    if (o.alpha) o.alpha[ro * (S - 1) + i] = alpha;
    const int64_t q = i * R + r;
    sdm[i] = c.dmid[q];
#pragma unroll
    for (int e = 0; e < 3; ++e) srad[i * 3 + e] = c.rad_m[q * 3 + e];
    if (calc_normal) {
      float x = c.nab_f[q * 3 + 0], y = c.nab_f[q * 3 + 1], z = c.nab_f[q * 3 + 2];
      normalize3(x, y, z);
      snrm[i * 3 + 0] = x;
      snrm[i * 3 + 1] = y;
      snrm[i * 3 + 2] = z;
    }
  }
  __syncthreads();
  Composite A;
  if (l == 0 && live) {
    for (int i = 0; i < S - 1; ++i) {
      const float w = A.weight(sal[i]);
      A.add(w, srad + i * 3);
      if (calc_normal) A.add_normal(w, snrm[i * 3 + 0], snrm[i * 3 + 1], snrm[i * 3 + 2]);
      sal[i] = w;
    }
    scdf[0] = A.denom();  // the depth normaliser for the ray's lanes (the cdf is no longer read)
  }
  __syncthreads();
  // depth terms w_i / (acc + 1e-10) * d_mid_i across the ray's lanes, into scdf[1 ..] (the CDFs
  // are no longer read; scdf[0] holds the normaliser)
  {
    const float denom = scdf[0];
    __syncthreads();  // every lane has its normaliser before scdf[1 ..] is overwritten
    for (int i = l; i < Sl - 1; i += NL) scdf[i + 1] = fmul(fdiv(sal[i], denom), sdm[i]);
  }
  __syncthreads();
  if (l == 0 && live) {
    double depth = 0.0;
    for (int i = 0; i < S - 1; ++i) depth += (double)scdf[i + 1];
    A.finish((float)depth, white_bkgd, ro, o.rgb, o.depth, o.acc, calc_normal ? o.normals : nullptr);
  }
  __syncthreads();
  // detailed per-sample outputs, ray-major
  for (int i = l; i < Sl; i += NL) {
    const int64_t q = i * R + r;
    if (o.sdf) o.sdf[ro * S + i] = c.sdf_f[q];
    if (o.nablas) copy3(o.nablas + (ro * S + i) * 3, c.nab_f + q * 3);
    if (i < S - 1) {
      if (o.weights) o.weights[ro * (S - 1) + i] = sal[i];
      if (o.d_final) o.d_final[ro * (S - 1) + i] = c.dmid[q];
      if (o.radiance) copy3(o.radiance + (ro * (S - 1) + i) * 3, srad + i * 3);
    }
  }
}

template __global__ void neus_composite<1>(NeusChunk, NeusOut, const float*, float, int, int);
template __global__ void neus_composite<4>(NeusChunk, NeusOut, const float*, float, int, int);

// ---------------------------------------------------------------------------------------------
// 'direct_use' / 'direct_more' upsampling (neus.py:215-243): one sample_pdf of N_importance over
// the visibility weights of the coarse (or N_nograd_samples uniform) depths, s = 1/fixed_s_recp
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void neus_nograd_points(NeusChunk c) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= c.R) return;
  const int64_t R = c.R;
  const float ox = c.ro[r * 3], oy = c.ro[r * 3 + 1], oz = c.ro[r * 3 + 2];
  const float dx = c.rd[r * 3], dy = c.rd[r * 3 + 1], dz = c.rd[r * 3 + 2];
  const float nr = c.near[r], fr = c.far[r];
  for (int k = 0; k < c.n_nog; ++k) {
    const float t = c.t_nog[k];
    const float d = fadd(fmul(nr, fsub(1.0f, t)), fmul(fr, t));
    const int64_t q = (int64_t)k * R + r;
    c.pts_nog[q * 3 + 0] = fadd(ox, fmul(d, dx));
    c.pts_nog[q * 3 + 1] = fadd(oy, fmul(d, dy));
    c.pts_nog[q * 3 + 2] = fadd(oz, fmul(d, dz));
  }
}

__global__ __launch_bounds__(64) void neus_direct_upsample(NeusChunk c, int more, const float* __restrict__ u,
                                                         int64_t u_stride) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= c.R) return;
  const int64_t R = c.R;
  const int L = more ? c.n_nog : c.N_samples;
  const float nr = c.near[r], fr = c.far[r];
  // bins: the coarse depths (dv) or the nograd depths (recomputed, never stored)
  float* bins = c.dv + r;
  if (more) {
    bins = c.d_out + r;  // scratch column of >= n_nog floats
    for (int k = 0; k < L; ++k) {
      const float t = c.t_nog[k];
      bins[(int64_t)k * R] = fadd(fmul(nr, fsub(1.0f, t)), fmul(fr, t));
    }
  }
  const float* sdf = more ? c.s_nog + r : c.sv + r;
  // sdf_to_w (neus.py:37-70): logistic cdf, alpha = max((c_i - c_i+1)/(c_i + 1e-10), 0), cumprod
  double T = 1.0;
  float cprev = neus_cdf(sdf[0], c.fixed_s);
  for (int i = 0; i < L - 1; ++i) {
    const float cn = neus_cdf(sdf[(int64_t)(i + 1) * R], c.fixed_s);
    const float alpha = neus_alpha(cprev, cn);
    c.wtmp[(int64_t)i * R + r] = fmul(alpha, (float)T);
    T *= (double)transparency(alpha);
    cprev = cn;
  }
  float* wr = c.wtmp + r;
  const float total = aten_row_sum(L - 1, [&](int i) { return fadd(wr[(int64_t)i * R], 1e-5f); });
  float* dn = c.dnew + r;
  if (u_stride) sample_pdf_ray_rand(bins, wr, R, L, total, u + r * u_stride, c.n_imp, dn, R);
  else sample_pdf_ray(bins, wr, R, L, total, u, c.n_imp, dn, R);
  // sort(cat([d_coarse, d_fine])) (neus.py:227-228): insertion-sort the new column, merge in place
  const int n = c.n_imp;
  for (int k = 1; k < n; ++k) {
    const float v = dn[(int64_t)k * R];
    int j = k - 1;
    while (j >= 0 && dn[(int64_t)j * R] > v) {
      dn[(int64_t)(j + 1) * R] = dn[(int64_t)j * R];
      --j;
    }
    dn[(int64_t)(j + 1) * R] = v;
  }
  int i = c.N_samples - 1, j = n - 1;
  for (int k = c.N_samples + n - 1; k >= 0 && j >= 0; --k) {
    const float di = i >= 0 ? c.dv[(int64_t)i * R + r] : 0.f;
    const float dj = dn[(int64_t)j * R];
    if (i >= 0 && di > dj) {
      c.dv[(int64_t)k * R + r] = di;
      --i;
    } else {
      c.dv[(int64_t)k * R + r] = dj;
      --j;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// NeRF++ background (neus.py:303-343)
// ---------------------------------------------------------------------------------------------
// d_vals_out = cat([d_mid, far / flip(linspace(0,1,N_out+2)[1:-1])]); x_out = [p / |p|, 1 / |p|]
// perturb (neus.py:306-311): d_k = lower_k + (upper_k - lower_k) * t_rand[r][k] with the mid-point
// brackets of the deterministic inverted-sphere depths (t_rand: the caller's uniforms, or null)
__global__ __launch_bounds__(64) void neus_outside_points(NeusChunk c, const float* __restrict__ t_rand) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= c.R) return;
  const int64_t R = c.R;
  const int S1 = c.S - 1, M = S1 + c.N_out;
  const float ox = c.ro[r * 3], oy = c.ro[r * 3 + 1], oz = c.ro[r * 3 + 2];
  const float dx = c.rd[r * 3], dy = c.rd[r * 3 + 1], dz = c.rd[r * 3 + 2];
  const float fr = c.far[r];
  const int No = c.N_out;
  auto dvo = [&](int j) { return fdiv(fr, c.t_out[No - j]); };  // far / flip(linspace(0,1,No+2)[1:-1])[j]
  for (int k = 0; k < M; ++k) {
    float d;
    if (k < S1) {
      d = c.dmid[(int64_t)k * R + r];
    } else {
      const int j = k - S1;
      d = dvo(j);
      if (t_rand) {
        const float lower = j > 0 ? fmul(0.5f, fadd(dvo(j), dvo(j - 1))) : dvo(0);
        const float upper = j + 1 < No ? fmul(0.5f, fadd(dvo(j + 1), dvo(j))) : dvo(No - 1);
        d = fadd(lower, fmul(fsub(upper, lower), t_rand[(int64_t)r * No + j]));
      }
    }
    const int64_t q = (int64_t)k * R + r;
    c.d_out[q] = d;
    const float px = fadd(ox, fmul(dx, d)), py = fadd(oy, fmul(dy, d)), pz = fadd(oz, fmul(dz, d));
    const float rr = norm3_ref(px, py, pz);
    *(float4*)(c.x4 + q * 4) = make_float4(fdiv(px, rr), fdiv(py, rr), fdiv(pz, rr), fdiv(1.0f, rr));
  }
}

// Workgroup-aggregated append (blockDim.x a multiple of 64, at most 1024): one atomicAdd per
// workgroup instead of one per wave -- the per-wave atomics on the one counter serialised (~8 ns
// each, 8 k of them per config-(b) mid-point pass).  Returns the lane's compact index when need.
// Every thread of the block must call it (barriers inside).
__device__ __forceinline__ int64_t block_append(bool need, int* __restrict__ count) {
  __shared__ int wcnt[16];
  __shared__ int bbase;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint64_t bal = __ballot(need);
  if (lane == 0) wcnt[w] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < nw; ++i) {
      const int v = wcnt[i];
      wcnt[i] = t;
      t += v;
    }
    bbase = t ? atomicAdd(count, t) : 0;
  }
  __syncthreads();
  return (int64_t)bbase + wcnt[w] + __popcll(bal & ((1ull << lane) - 1ull));
}

// The background values the compositing reads (neus.py:325-343): every inverted-sphere sample, and the
// mid-points outside the bounding sphere -- the ones inside take the SDF's alpha and radiance, so the
// reference's background evaluation there is discarded.  Without detailed outputs only these points
// go through the NeRF++ net: appended (one atomic per workgroup) to x4c / vdc, slot[q] = compact index or
// -1.
__global__ void neus_outside_compact(NeusChunk c, int* __restrict__ count, int* __restrict__ slot,
                                     float* __restrict__ x4c, float* __restrict__ vdc) {
  const int64_t R = c.R;
  const int S1 = c.S - 1, M = S1 + c.N_out;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = q < (int64_t)M * R;
  int64_t r = 0;
  bool need = false;
  if (in_range) {
    const int k = (int)(q / R);
    r = q - (int64_t)k * R;
    if (k >= S1) {
      need = true;
    } else {
      need = !inside_sphere(c.ro, c.rd, r, c.dmid[q], c.r_obj);
    }
  }
  const int64_t ja = block_append(need, count);
  if (!in_range) return;
  if (need) {
    const int j = (int)ja;
    slot[q] = j;
    *(float4*)(x4c + (int64_t)j * 4) = *(const float4*)(c.x4 + q * 4);
    vdc[(int64_t)j * 3 + 0] = c.rd[r * 3 + 0];
    vdc[(int64_t)j * 3 + 1] = c.rd[r * 3 + 1];
    vdc[(int64_t)j * 3 + 2] = c.rd[r * 3 + 2];
  } else {
    slot[q] = -1;
  }
}

// Mid-point i of a ray contributes w_i * radiance_i with w_i = alpha_i T_i, and alpha_i = max((c_i -
// c_{i+1}) / (c_i + 1e-10), 0) is exactly 0 wherever the SDF does not decrease from sample i to i+1
// (neus.py:28-35): there the radiance (and the mid-point's SDF, nablas and feature that feed it) is
// multiplied by an exact zero.  Without detailed outputs only the mid-points with alpha != 0
// (neus_alpha, as the compositing forms it) go through the SDF + radiance nets; the others get radiance 0.
__global__ void neus_mid_compact(NeusChunk c, const float* __restrict__ s_dev, float s_val, int* __restrict__ count,
                                 int* __restrict__ slot, float* __restrict__ midc, float* __restrict__ vdc) {
  const int64_t R = c.R;
  const int S1 = c.S - 1;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = q < (int64_t)S1 * R;
  int64_t r = 0;
  bool need = false;
  if (in_range) {
    const float s_inv = s_dev ? *s_dev : s_val;
    const int i = (int)(q / R);
    r = q - (int64_t)i * R;
    const float cp = neus_cdf(c.sdf_f[(int64_t)i * R + r], s_inv);
    const float cn = neus_cdf(c.sdf_f[(int64_t)(i + 1) * R + r], s_inv);
    need = !(neus_alpha(cp, cn) == 0.0f);
    // NeRF++: a mid-point outside the bounding sphere takes the background's alpha and colour
    if (need && c.N_out > 0) need = inside_sphere(c.ro, c.rd, r, c.dmid[q], c.r_obj);
  }
  const int64_t j = block_append(need, count);
  if (!in_range) return;
  if (need) {
    slot[q] = (int)j;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      midc[j * 3 + e] = c.mids[q * 3 + e];
      vdc[j * 3 + e] = c.rd[r * 3 + e];
    }
  } else {
    slot[q] = -1;
  }
}

// deferred sample nablas: flag the 16-slot tile (evaluation order) of every sorted sample i < S-1 whose
// interval alpha is not exactly 0 -- neus_composite weights sample i's unit nabla by w_i = alpha_i T_i
// (neus.py:364-368), so the others contribute exactly 0 (their nablas stay 0, normalize(0) = 0).
__global__ void neus_sample_need(NeusChunk c, const float* __restrict__ s_dev, float s_val) {
  const int64_t R = c.R;
  const int S1 = c.S - 1;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)S1 * R) return;
  const float s_inv = s_dev ? *s_dev : s_val;
  const int i = (int)(q / R);
  const int64_t r = q - (int64_t)i * R;
  const float cp = neus_cdf(c.sdf_f[(int64_t)i * R + r], s_inv);
  const float cn = neus_cdf(c.sdf_f[(int64_t)(i + 1) * R + r], s_inv);
  if (!(neus_alpha(cp, cn) == 0.0f)) c.tflag[((int64_t)c.idv[q] * R + r) >> c.tshift] = 1;
}

// the same with the NeRF++ background (neus_composite_outside): sample k < S weights its unit nabla by
// w_k = alpha_k T_k, alpha_k the SDF alpha of interval k if mid-point k is inside the bounding sphere,
// else the background's 1 - exp(-softplus(sigma) dist) -- also for k = S-1, whose weight is the first
// inverted-sphere sample's (neus.py:364-366 pairs min(#weights, #nablas) = S of them).  Runs after the
// background net (sig_o); a tile is flagged if any alpha != 0.
__global__ void neus_sample_need_outside(NeusChunk c, const float* __restrict__ s_dev, float s_val) {
  const int64_t R = c.R;
  const int S = c.S, S1 = S - 1, M = S1 + c.N_out;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)S * R) return;
  const int k = (int)(q / R);
  const int64_t r = q - (int64_t)k * R;
  bool inside = false;
  float alpha = 0.0f;
  if (k < S1) {
    const float s_inv = s_dev ? *s_dev : s_val;
    const float cp = neus_cdf(c.sdf_f[(int64_t)k * R + r], s_inv);
    const float cn = neus_cdf(c.sdf_f[(int64_t)(k + 1) * R + r], s_inv);
    alpha = neus_alpha(cp, cn);
    inside = inside_sphere(c.ro, c.rd, r, c.dmid[q], c.r_obj);
  }
  if (!inside) {
    const float dist = nerfpp_dist(c.d_out[q], c.d_out, q + R, k + 1 < M);
    alpha = nerfpp_alpha(c.sig_o[q], dist);
  }
  if (!(alpha == 0.0f)) c.tflag[((int64_t)c.idv[q] * R + r) >> c.tshift] = 1;
}

// flagged sample slots -> list for the compacted reverse pass (sdf4_kernel STAGE 4): each 1024-slot
// workgroup appends its flagged slots in slot order as one segment padded with -1 to a multiple of 16
// entries (one atomic per workgroup), so the 16 entries a wave takes come from one 1024-slot range:
// within 64 tiles of the segment's first entry (the kernel's per-lane slab offsets stay small)
__global__ __launch_bounds__(1024) void neus_point_list(NeusChunk c, int64_t n_slots) {
  __shared__ int wcnt[16];
  __shared__ int bbase, btot;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool need = t < n_slots && c.tflag[t] != 0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint64_t bal = __ballot(need);
  if (lane == 0) wcnt[w] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < nw; ++i) {
      const int v = wcnt[i];
      wcnt[i] = s;
      s += v;
    }
    btot = s;
    bbase = s ? atomicAdd(c.tcnt, (s + 15) & ~15) : 0;
  }
  __syncthreads();
  if (need) c.tiles[(int64_t)bbase + wcnt[w] + __popcll(bal & ((1ull << lane) - 1ull))] = (int)t;
  const int pad = ((btot + 15) & ~15) - btot;
  if ((int)threadIdx.x < pad) c.tiles[(int64_t)bbase + btot + threadIdx.x] = -1;
}

// flagged tiles -> list (any order: each tile's nablas depend on that tile alone)
__global__ void neus_tile_list(NeusChunk c, int64_t n_tiles) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool need = t < n_tiles && c.tflag[t] != 0;
  const int64_t j = block_append(need, c.tcnt);
  if (need) c.tiles[j] = (int)t;
}

__global__ void neus_mid_scatter(const int* __restrict__ slot, const float* __restrict__ radc, int64_t n,
                                 float* __restrict__ rad_m) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int j = slot[q];
#pragma unroll
  for (int e = 0; e < 3; ++e) rad_m[q * 3 + e] = j < 0 ? 0.0f : radc[(int64_t)j * 3 + e];
}

__global__ void neus_outside_scatter(const int* __restrict__ slot, const float* __restrict__ sigc,
                                     const float* __restrict__ radc, int64_t n, float* __restrict__ sig_o,
                                     float* __restrict__ rad_o) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int j = slot[q];
  if (j < 0) return;
  sig_o[q] = sigc[j];
  rad_o[q * 3 + 0] = radc[(int64_t)j * 3 + 0];
  rad_o[q * 3 + 1] = radc[(int64_t)j * 3 + 1];
  rad_o[q * 3 + 2] = radc[(int64_t)j * 3 + 2];
}


// compositing with the background merged in, RPW rays per wave (neus_composite's structure): the
// per-sample CDFs, the inside test, the inside / background alphas, radiance and unit nablas across the
// ray's lanes into LDS; the transmittance product and the fp64 sums on the ray's first lane in sample
// order (neus_composite_outside, one thread per ray, remains the fallback when the LDS staging does not
// fit).  LDS per ray: 6 M + 4 S floats.
template <int RPW>
__global__ __launch_bounds__(64) void neus_composite_outside_w(NeusChunk c, NeusOut o, const float* __restrict__ s_dev,
                                                               float s_val, int calc_normal, int white_bkgd) {
  extern __shared__ float lds[];
  constexpr int NL = 64 / RPW;
  const float s_inv = s_dev ? *s_dev : s_val;
  const int r = blockIdx.x * RPW + (int)threadIdx.x / NL, l = (int)threadIdx.x % NL;
  const int S = c.S, S1 = S - 1, M = S1 + c.N_out;
  const int Nn = M < S ? M : S;  // normals use min(#weights, #nablas) samples (neus.py:364-366)
  const int64_t R = c.R;
  const bool live = r < R;
  const int Sl = live ? S : 0, Ml = live ? M : 0, Nl = live ? Nn : 0;
  const int64_t ro = o.ray0 + r;
  float* scdf = lds + ((int)threadIdx.x / NL) * (6 * M + 4 * S);  // [S]
  float* sal = scdf + S;       // [M] alpha, then weights
  float* srad = sal + M;       // [M][3]
  float* sdo = srad + 3 * M;   // [M] d_out
  float* dum = sdo + M;        // [M] (pad)
  float* snrm = dum + M;       // [S][3] unit nablas
  for (int i = l; i < Sl; i += NL) {
    const float cdf = neus_cdf(c.sdf_f[(int64_t)i * R + r], s_inv);
    scdf[i] = cdf;
    if (o.cdf) o.cdf[ro * S + i] = cdf;
  }
  __syncthreads();
  for (int k = l; k < Ml; k += NL) {
    const int64_t q = (int64_t)k * R + r;
    const float dk = c.d_out[q];
    sdo[k] = dk;
    bool inside = false;
    float a_in = 0.0f;
    if (k < S1) {
      a_in = neus_alpha(scdf[k], scdf[k + 1]);
      inside = inside_sphere(c.ro, c.rd, r, c.dmid[q], c.r_obj);
    }
    float alpha;
    if (inside) {
      alpha = a_in;
#pragma unroll
      for (int e = 0; e < 3; ++e) srad[k * 3 + e] = c.rad_m[q * 3 + e];
    } else {
      const float dist = nerfpp_dist(dk, c.d_out, q + R, k + 1 < M);
      alpha = nerfpp_alpha(c.sig_o[q], dist);
#pragma unroll
      for (int e = 0; e < 3; ++e) srad[k * 3 + e] = c.rad_o[q * 3 + e];
    }
    sal[k] = alpha;
    if (o.alpha) o.alpha[ro * M + k] = alpha;
  }
  if (calc_normal) {
    for (int k = l; k < Nl; k += NL) {
      const int64_t q = (int64_t)k * R + r;
      float x = c.nab_f[q * 3 + 0], y = c.nab_f[q * 3 + 1], z = c.nab_f[q * 3 + 2];
      normalize3(x, y, z);
      snrm[k * 3 + 0] = x;
      snrm[k * 3 + 1] = y;
      snrm[k * 3 + 2] = z;
    }
  }
  __syncthreads();
  if (l == 0 && live) {
    Composite A;
    for (int k = 0; k < M; ++k) {
      const float w = A.weight(sal[k]);
      A.add(w, srad + k * 3);
      if (calc_normal && k < Nn) A.add_normal(w, snrm[k * 3 + 0], snrm[k * 3 + 1], snrm[k * 3 + 2]);
      sal[k] = w;
    }
    const float denom = A.denom();
    double depth = 0.0;
    for (int k = 0; k < M; ++k) depth += (double)fmul(fdiv(sal[k], denom), sdo[k]);
    A.finish((float)depth, white_bkgd, ro, o.rgb, o.depth, o.acc, calc_normal ? o.normals : nullptr);
  }
  __syncthreads();
  // detailed per-sample outputs, ray-major
  for (int k = l; k < Ml; k += NL) {
    const int64_t q = (int64_t)k * R + r;
    if (o.weights) o.weights[ro * M + k] = sal[k];
    if (o.d_final) o.d_final[ro * M + k] = sdo[k];
    if (o.radiance) copy3(o.radiance + (ro * M + k) * 3, srad + k * 3);
    if (o.sigma_out) o.sigma_out[ro * M + k] = c.sig_o[q];
    if (o.radiance_bg) copy3(o.radiance_bg + (ro * M + k) * 3, c.rad_o + q * 3);
  }
  for (int i = l; i < Sl; i += NL) {
    const int64_t q = (int64_t)i * R + r;
    if (o.sdf) o.sdf[ro * S + i] = c.sdf_f[q];
    if (o.nablas) copy3(o.nablas + (ro * S + i) * 3, c.nab_f + q * 3);
  }
}

template __global__ void neus_composite_outside_w<1>(NeusChunk, NeusOut, const float*, float, int, int);
template __global__ void neus_composite_outside_w<4>(NeusChunk, NeusOut, const float*, float, int, int);

// compositing with the background merged in (neus.py:325-343, :346-380)
__global__ __launch_bounds__(64) void neus_composite_outside(NeusChunk c, NeusOut o, const float* __restrict__ s_dev,
                                                             float s_val, int calc_normal, int white_bkgd) {
  const float s_inv = s_dev ? *s_dev : s_val;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= c.R) return;
  const int S = c.S, S1 = S - 1, M = S1 + c.N_out;
  const int64_t R = c.R;
  const int64_t ro = o.ray0 + r;
  const float ro3[3] = {c.ro[r * 3], c.ro[r * 3 + 1], c.ro[r * 3 + 2]};
  const float rd3[3] = {c.rd[r * 3], c.rd[r * 3 + 1], c.rd[r * 3 + 2]};
  Composite A;
  float cprev = neus_cdf(c.sdf_f[r], s_inv);
  if (o.cdf) o.cdf[ro * S] = cprev;
  const int Nn = M < S ? M : S;  // normals use min(#weights, #nablas) samples (neus.py:364-366)
  for (int k = 0; k < M; ++k) {
    const int64_t q = (int64_t)k * R + r;
    const float dk = c.d_out[q];
    const float dist = nerfpp_dist(dk, c.d_out, q + R, k + 1 < M);
    const float a_out = nerfpp_alpha(c.sig_o[q], dist);
    float alpha, col[3];
    bool inside = false;
    float a_in = 0.f;
    if (k < S1) {
      const float cn = neus_cdf(c.sdf_f[(int64_t)(k + 1) * R + r], s_inv);
      a_in = neus_alpha(cprev, cn);
      if (o.cdf) o.cdf[ro * S + k + 1] = cn;
      cprev = cn;
      inside = inside_sphere(ro3, rd3, 0, c.dmid[q], c.r_obj);
    }
    if (inside) {
      alpha = a_in;
      col[0] = c.rad_m[q * 3 + 0]; col[1] = c.rad_m[q * 3 + 1]; col[2] = c.rad_m[q * 3 + 2];
    } else {
      alpha = a_out;
      col[0] = c.rad_o[q * 3 + 0]; col[1] = c.rad_o[q * 3 + 1]; col[2] = c.rad_o[q * 3 + 2];
    }
    const float w = A.weight(alpha);
    A.add(w, col);
    if (calc_normal && k < Nn) {
      float x = c.nab_f[(int64_t)k * R * 3 + r * 3 + 0], y = c.nab_f[(int64_t)k * R * 3 + r * 3 + 1],
            z = c.nab_f[(int64_t)k * R * 3 + r * 3 + 2];
      normalize3(x, y, z);
      A.add_normal(w, x, y, z);
    }
    c.wtmp[q] = w;
    if (o.alpha) o.alpha[ro * M + k] = alpha;
    if (o.weights) o.weights[ro * M + k] = w;
    if (o.d_final) o.d_final[ro * M + k] = dk;
    if (o.radiance) copy3(o.radiance + (ro * M + k) * 3, col);
    if (o.sigma_out) o.sigma_out[ro * M + k] = c.sig_o[q];
    if (o.radiance_bg) copy3(o.radiance_bg + (ro * M + k) * 3, c.rad_o + q * 3);
  }
  const float denom = A.denom();
  double depth = 0.0;
  for (int k = 0; k < M; ++k) {
    const int64_t q = (int64_t)k * R + r;
    depth += (double)fmul(fdiv(c.wtmp[q], denom), c.d_out[q]);
  }
  A.finish((float)depth, white_bkgd, ro, o.rgb, o.depth, o.acc, calc_normal ? o.normals : nullptr);
  for (int i = 0; i < S; ++i) {
    const int64_t q = (int64_t)i * R + r;
    if (o.sdf) o.sdf[ro * S + i] = c.sdf_f[q];
    if (o.nablas) copy3(o.nablas + (ro * S + i) * 3, c.nab_f + q * 3);
  }
}

// sorted sample depths, sample-major [S][R] -> ray-major rows of the output (training sample pass)
__global__ void neus_write_dall(const float* __restrict__ dv, int64_t R, int S, int64_t ray0, float* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)S * R) return;
  const int64_t s = q / R, r = q - s * R;
  out[(ray0 + r) * S + s] = dv[q];
}

// ---------------------------------------------------------------------------------------------
// generic sample_pdf entry (rend_util.py:255-292), bins/weights ray-major [R][L], u [N]
// ---------------------------------------------------------------------------------------------
// u: shared sorted uniforms (u_stride 0, det=True) or per-row uniforms u[r * u_stride + k] in any
// order (det=False): each of those is inverted by its own cumsum walk (weights stay read-only)
__global__ void sample_pdf_kernel(const float* __restrict__ bins, const float* __restrict__ weights, int64_t R, int L,
                                  const float* __restrict__ u, int64_t u_stride, int N, float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* wr = weights + r * (L - 1);
  const float total = aten_row_sum(L - 1, [&](int i) { return fadd(wr[i], 1e-5f); });
  if (!u_stride) {
    sample_pdf_ray(bins + r * L, wr, 1, L, total, u, N, out + r * N, 1);
    return;
  }
  const float* br = bins + r * L;
  for (int k = 0; k < N; ++k) {
    const float uk = u[r * u_stride + k];
    sample_pdf_ray(br, wr, 1, L, total, &uk, 1, out + r * N + k, 1);
  }
}

// ---------------------------------------------------------------------------------------------
// host orchestration: workspace binding, one ray chunk, chunk size, argument checks, entry points
// ---------------------------------------------------------------------------------------------
// official_solution, render mode without the per-sample nablas (detailed outputs), the f16x3 softplus
// net, and slots that tile exactly (R % 16 == 0: every launch starts a tile).  With NeRF++ the tiles
// are flagged after the background net (neus_sample_need_outside); not with its detailed outputs.
static bool neus_deferred(const NrNeusArgs& a, int64_t R) {
  return a.upsample_algo == NR_UPSAMPLE_OFFICIAL && !a.sample_only && !a.nablas_out && !a.no_mid_skip &&
         !a.no_defer && !(a.N_outside > 0 && (a.sigma_out || a.radiance_bg_out || a.radiance_out)) && a.sdf &&
         a.sdf->precision == NR_PREC_F16X3 && !a.sdf->siren && R > 0 && R % 16 == 0;
}

// Fills the chunk view `c` (sample counts, workspace pointers) and the host-only buffers `h` for chunks of
// up to Rc rays carved from `base`, and returns the workspace bytes they need.  base == nullptr sizes only.
// The arrays are [sample][R] with the chunk's own R, so one binding serves every chunk of a call.
static size_t neus_bind(const NrNeusArgs& a, int64_t Rc, char* base, NeusChunk& c, NeusHost& h) {
  const bool direct = a.upsample_algo != NR_UPSAMPLE_OFFICIAL;
  const int n_up = direct ? 0 : (a.N_upsample_iters > 0 ? a.N_importance / a.N_upsample_iters : 0);
  c = NeusChunk{};
  h = NeusHost{};
  c.N_samples = a.N_samples;
  c.n_up = n_up;
  c.n_iters = direct ? 0 : a.N_upsample_iters;
  c.S = direct ? a.N_samples + a.N_importance : a.N_samples + a.N_upsample_iters * n_up;
  c.n_imp = a.N_importance;
  c.n_nog = a.upsample_algo == NR_UPSAMPLE_DIRECT_MORE ? a.N_nograd_samples : 0;
  c.fixed_s = a.fixed_s;
  c.t_nog = a.t_nograd;
  c.N_out = a.N_outside;
  c.r_obj = a.obj_bounding_radius;
  c.t_out = a.t_outside;
  const size_t S = c.S, n_nog = c.n_nog, n_new = direct ? a.N_importance : n_up;
  Carve cv{base, 0};
  c.ro = cv.take(Rc * 3);
  c.rd = cv.take(Rc * 3);
  c.near = cv.take(Rc);
  c.far = cv.take(Rc);
  c.dv = cv.take(S * Rc);
  c.sv = cv.take(S * Rc);
  c.wtmp = cv.take(std::max(S, n_nog) * Rc);  // dead when N_outside > 0 (re-carved below); no total may shift
  c.dnew = cv.take(std::max<size_t>(n_new, 1) * Rc);
  c.snew = cv.take(std::max<size_t>(n_new, 1) * Rc);
  c.pts = cv.take(S * Rc * 3);
  c.mids = cv.take((S - 1) * Rc * 3);
  c.dmid = cv.take((S - 1) * Rc);
  c.sdf_f = cv.take(S * Rc);
  c.nab_f = cv.take(S * Rc * 3);
  c.sdf_m = cv.take((S - 1) * Rc);
  c.nab_m = cv.take((S - 1) * Rc * 3);
  c.feat_m = cv.take((S - 1) * Rc * 256);
  c.rad_m = cv.take((S - 1) * Rc * 3);
  const bool bg = a.N_outside > 0;
  const size_t M = S - 1 + a.N_outside;
  // weights of all M samples; direct_more also writes its n_nog-1 no-grad weights here first
  if (bg) c.wtmp = cv.take(std::max(M, n_nog) * Rc);
  c.d_out = cv.take((bg ? std::max(M, n_nog) : std::max<size_t>(n_nog, 1)) * Rc);
  const size_t Mo = (bg ? M : 1) * Rc;
  c.x4 = cv.take(Mo * 4);
  c.sig_o = cv.take(Mo);
  c.rad_o = cv.take(Mo * 3);
  h.slot = cv.take<int>(Mo);  // NeRF++: compacted background points
  h.x4c = cv.take(Mo * 4);
  h.vdc = cv.take(Mo * 3);
  h.sigc = cv.take(Mo);
  h.radc = cv.take(Mo * 3);
  h.cnt = cv.take<int>(1);
  const size_t Mm = (S - 1) * Rc;
  h.mslot = cv.take<int>(Mm);  // mid-points of non-zero alpha (compacted)
  h.midc = cv.take(Mm * 3);
  h.mvd = cv.take(Mm * 3);
  h.mrad = cv.take(Mm * 3);
  h.mcnt = cv.take<int>(3);  // the count, then the mid-point and radiance launches' tile claims (one memset)
  c.pts_nog = cv.take(std::max<size_t>(n_nog, 1) * Rc * 3);
  c.s_nog = cv.take(std::max<size_t>(n_nog, 1) * Rc);
  c.idv = cv.take<int>(S * Rc);
  float* nsort = cv.take(S * Rc * 3);
  h.dv2 = cv.take(S * Rc);  // merge ping-pong buffers
  h.sv2 = cv.take(S * Rc);
  h.idv2 = cv.take<int>(S * Rc);
  // official_solution evaluates every final sample exactly once, when it is drawn: the coarse and
  // upsampled points are bit-identical to the final `pts` (neus.py:284 recomputes o + d*dir from
  // the same depths), so one SDF+nabla launch per round replaces the forward-only round launches
  // plus the reference's second pass over all samples (neus.py:294).  sdf rides along the sorted
  // merges (sv); nablas stay in evaluation order (nraw) and are gathered once by neus_points.
  h.fused = !direct && !a.sample_only;  // the sample pass needs no nablas
  if (h.fused) {
    c.nraw = c.nab_f;
    c.sdf_f = c.sv;
    c.nab_f = nsort;
  } else {
    c.idv = h.idv2 = nullptr;
  }
  // deferred sample nablas (NeusChunk::slabs); a chunk that does not defer ignores them
  const bool defer = neus_deferred(a, Rc);
  const size_t slots = defer ? S * Rc : 1;
  c.slabs = cv.take<float4>(defer ? (slots + 15) / 16 * (kSlabColBytes / 16) : 1);  // 100 KB per 16-slot tile
  // flags per sample slot; the list (neus_point_list) pads each 1024-slot segment to 16 entries
  c.tflag = cv.take<int>(slots);
  c.tiles = cv.take<int>(slots + 16 * ((slots + 1023) / 1024));
  c.tcnt = cv.take<int>(2);  // the list's length, then the reverse pass's tile claims (one memset)
  h.mlp_ws = base ? base + cv.off : nullptr;
  h.mlp_bytes = base ? a.workspace_bytes - cv.off : 0;
  return cv.off + nr_mlp_workspace_bytes(1);
}

// The side stream of the two-branch chunk (neus_chunk): one per device, non-blocking, created at its first
// use and kept for the life of the process, with the two events of its fork and join.
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
constexpr int kMaxSideDev = 64;
static std::mutex g_side_mu;
static SideStream g_side[kMaxSideDev];

static int side_stream(SideStream& out) {
  int dev = 0;
  NR_HIP_CHECK(hipGetDevice(&dev));
  NR_REQUIRE(dev >= 0 && dev < kMaxSideDev, NR_ERR_UNSUPPORTED, "nr_neus_render: device index beyond the side streams");
  std::lock_guard<std::mutex> lk(g_side_mu);
  SideStream& g = g_side[dev];
  if (!g.s) {
    SideStream n;
    NR_HIP_CHECK(hipStreamCreateWithFlags(&n.s, hipStreamNonBlocking));
    NR_HIP_CHECK(hipEventCreateWithFlags(&n.fork, hipEventDisableTiming));
    NR_HIP_CHECK(hipEventCreateWithFlags(&n.join, hipEventDisableTiming));
    g = n;
  }
  out = g;
  return NR_OK;
}

// `to` waits for what `from` holds now.  The record and the wait are one step under the lock: two host
// threads rendering on one device share the events, and a wait must see its own thread's record.
static int stream_after(hipStream_t to, hipStream_t from, hipEvent_t ev) {
  std::lock_guard<std::mutex> lk(g_side_mu);
  NR_HIP_CHECK(hipEventRecord(ev, from));
  NR_HIP_CHECK(hipStreamWaitEvent(to, ev, 0));
  return NR_OK;
}

// A fork that always joins: a chunk that fails between the two still leaves `st` ordered after the side
// stream's work on its workspace.
struct SideJoin {
  hipStream_t st;
  SideStream side;
  bool open = false;
  int join() {
    if (!open) return NR_OK;
    open = false;
    return stream_after(st, side.s, side.join);
  }
  ~SideJoin() { (void)join(); }
};

static bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {  // e.g. the legacy stream beside a capture: stay in order
    (void)hipGetLastError();
    return true;
  }
  return cs != hipStreamCaptureStatusNone;
}

static int neus_chunk(const NrNeusArgs& a, NeusChunk c, const NeusHost& h, int64_t ray0, int R, hipStream_t st) {
  const bool direct = a.upsample_algo != NR_UPSAMPLE_OFFICIAL, fused = h.fused;
  const int n_up = c.n_up;
  c.R = R;
  // deferred sample nablas (NeusChunk::slabs): sample launches leave per-tile slabs, the reverse pass
  // runs after the sampling on the tiles of non-zero weight
  const bool defer = fused && neus_deferred(a, R);
  if (!defer) {
    c.slabs = nullptr;
    c.tflag = c.tiles = c.tcnt = nullptr;
  }
  void* const mlp_ws = h.mlp_ws;
  const size_t mlp_bytes = h.mlp_bytes;
  const SdfLayout SL = sdf_layout(*a.sdf);
  const RadLayout RL = rad_layout(*a.rad);
  // SDF of P sample points at evaluation slot slot0 (coarse: 0; round it: (N_samples + it n_up) R)
  auto sample_sdf = [&](const float* pts, int64_t P, float* sdf_out, int64_t slot0) -> int {
    if (defer)
      return launch_sdf_deferred(SL, a.sdf_packed, pts, P, sdf_out, nullptr, a.sdf->multires,
                                 (float4*)((char*)c.slabs + (size_t)(slot0 / 16) * kSlabColBytes), nullptr, nullptr,
                                 1, st);
    return launch_sdf(SL, a.sdf_packed, pts, P, sdf_out, fused ? c.nraw + slot0 * 3 : nullptr, nullptr,
                      a.sdf->multires, fused ? mlp_ws : nullptr, fused ? mlp_bytes : 0, st);
  };
  const dim3 blk(64), grd((R + 63) / 64);  // one wave per block: a 4096-ray chunk spreads over 64 CUs
  int rc;

  {
  ProfScope prof("neus_prologue", (double)R, st);
  hipLaunchKernelGGL(neus_prologue, grd, blk, 0, st, c, a.rays_o + ray0 * 3, a.rays_d + ray0 * 3, a.t_coarse,
                     a.obj_bounding_radius, a.near_bypass, a.far_bypass);
  }
  NR_HIP_CHECK(hipGetLastError());
  // coarse SDF (no grad, neus.py:220 / :251); direct_more uses its own uniform depths instead
  if (a.upsample_algo != NR_UPSAMPLE_DIRECT_MORE && (rc = sample_sdf(c.pts, (int64_t)a.N_samples * R, c.sv, 0)))
    return rc;
  if (a.upsample_algo == NR_UPSAMPLE_DIRECT_MORE) {  // SDF at N_nograd_samples uniform depths
    hipLaunchKernelGGL(neus_nograd_points, grd, blk, 0, st, c);
    NR_HIP_CHECK(hipGetLastError());
    if ((rc = launch_sdf(SL, a.sdf_packed, c.pts_nog, (int64_t)c.n_nog * R, c.s_nog, nullptr, nullptr,
                         a.sdf->multires, nullptr, 0, st)))
      return rc;
  }
  if (direct) {
    ProfScope prof("neus_upsample", (double)R, st);
    // perturb: this chunk's rows of the caller's [n_rays][N_importance] uniforms
    const float* u = a.u_rand ? a.u_rand + ray0 * a.N_importance : a.u_fine;
    hipLaunchKernelGGL(neus_direct_upsample, grd, blk, 0, st, c, (int)(a.upsample_algo == NR_UPSAMPLE_DIRECT_MORE), u,
                       (int64_t)(a.u_rand ? a.N_importance : 0));
  }
  NR_HIP_CHECK(hipGetLastError());
  // sorted sample lists ping-pong between two buffers; each merge writes the other one
  float* dvb[2] = {c.dv, h.dv2};
  float* svb[2] = {c.sv, h.sv2};
  int* idb[2] = {c.idv, h.idv2};
  int cur = 0;
  auto merge = [&](int L) -> int {
    ProfScope prof("neus_merge", (double)R, st);
    const int64_t nt = (int64_t)(L + n_up) * R;
    hipLaunchKernelGGL(neus_merge, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, c, L, dvb[cur ^ 1],
                       svb[cur ^ 1], idb[cur ^ 1]);
    cur ^= 1;
    c.dv = dvb[cur];
    c.sv = svb[cur];
    c.idv = idb[cur];
    if (fused) c.sdf_f = c.sv;
    NR_HIP_CHECK(hipGetLastError());
    return NR_OK;
  };
  for (int it = 0; it < c.n_iters; ++it) {
    if (it > 0 && (rc = merge(a.N_samples + (it - 1) * n_up))) return rc;
    const int64_t slot0 = (int64_t)(a.N_samples + it * n_up) * R;
    // deferred: every round's points stay at their evaluation slots (the reverse pass reads them)
    NeusChunk cu = c;
    if (defer) cu.pts = c.pts + slot0 * 3;
    {
      ProfScope prof("neus_upsample", (double)R, st);
      // perturb: round it's [n_rays][n_up] block of the caller's uniforms
      const float* u = a.u_rand ? a.u_rand + ((int64_t)it * a.n_rays + ray0) * n_up : a.u_fine;
      const size_t lds1 = (5 * (size_t)c.S + 1) * sizeof(float);  // four rays per wave when their staging fits
      if (4 * lds1 <= 65536)
        hipLaunchKernelGGL((neus_upsample<4>), dim3((unsigned)((R + 3) / 4)), dim3(64), 4 * lds1, st, cu, it, u,
                           (int64_t)(a.u_rand ? n_up : 0));
      else
        hipLaunchKernelGGL((neus_upsample<1>), dim3((unsigned)R), dim3(64), lds1, st, cu, it, u,
                           (int64_t)(a.u_rand ? n_up : 0));
    }
    NR_HIP_CHECK(hipGetLastError());
    if ((rc = sample_sdf(cu.pts, (int64_t)n_up * R, c.snew, slot0))) return rc;
  }
  if (c.n_iters > 0 && (rc = merge(c.S - n_up))) return rc;
  // Tile claims (nr_mlp.h) of the three persistent launches behind the sampling, unless the caller asked for
  // the serial order: the counters share the memsets of the counts they follow (neus_bind).
  const bool claims = !a.serial_order;
  // Two branches (deferred nablas, no NeRF++): the sample nablas -- flags, list, compacted reverse pass, all
  // writing nraw / tflag / tiles / tcnt alone -- run on the side stream beside the mid-point -> radiance chain
  // on st, which reads none of them; st joins before neus_gather_nablas.  With claimed tiles the reverse
  // pass's workgroups take the compute units that the other branch's last round leaves idle.  A stream
  // under capture keeps the one-stream order.
  const bool two = defer && claims && a.calc_normal && a.N_outside == 0 && !stream_capturing(st);
  SideJoin sj{st};
  if (defer) {  // nablas of the tiles holding a sample of non-zero interval weight; the rest stay 0
    const int64_t nslot = (int64_t)c.S * R;
    c.tshift = 0;  // flags per sample slot, the reverse pass on the listed samples (sdf4_kernel STAGE 4)
    hipStream_t sr = st;  // the stream of the sample nablas
    if (two) {
      if ((rc = side_stream(sj.side)) || (rc = stream_after(sj.side.s, st, sj.side.fork))) return rc;
      sj.open = true;
      sr = sj.side.s;
    }
    NR_HIP_CHECK(hipMemsetAsync(c.nraw, 0, (size_t)nslot * 3 * sizeof(float), sr));
    if (a.calc_normal && a.N_outside == 0) {  // normals_volume is the only reader of the sample nablas here
      // (with NeRF++ the flags need the background's alphas: after the background net, below)
      NR_HIP_CHECK(hipMemsetAsync(c.tflag, 0, (size_t)nslot * sizeof(int), sr));
      NR_HIP_CHECK(hipMemsetAsync(c.tcnt, 0, (claims ? 2 : 1) * sizeof(int), sr));
      const int64_t nq = (int64_t)(c.S - 1) * R;
      hipLaunchKernelGGL(neus_sample_need, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, sr, c, a.s_dev, a.s);
      NR_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(neus_point_list, dim3((unsigned)((nslot + 1023) / 1024)), dim3(1024), 0, sr, c, nslot);
      NR_HIP_CHECK(hipGetLastError());
      if ((rc = launch_sdf_deferred(SL, a.sdf_packed, c.pts, nslot, nullptr, c.nraw, a.sdf->multires, c.slabs, c.tiles,
                                    c.tcnt, 4, sr, claims ? c.tcnt + 1 : nullptr)))
        return rc;
    }
  }
  if (a.sample_only) {  // training: the sorted depths are the whole output (neus.py:279)
    hipLaunchKernelGGL(neus_write_dall, dim3((unsigned)(((int64_t)c.S * R + 255) / 256)), dim3(256), 0, st, c.dv,
                       (int64_t)R, c.S, ray0, a.d_all_out);
    NR_HIP_CHECK(hipGetLastError());
    return NR_OK;
  }
  {
    ProfScope prof("neus_points", (double)R, st);
    hipLaunchKernelGGL(neus_expand, dim3((unsigned)(((int64_t)c.S * R + 255) / 256)), dim3(256), 0, st, c,
                       (int)!(defer && (a.N_outside > 0 || two)));
  }
  NR_HIP_CHECK(hipGetLastError());
  // SDF + nablas at the samples (neus.py:294); already in sv / nv on the fused path
  if (!fused && (rc = launch_sdf(SL, a.sdf_packed, c.pts, (int64_t)c.S * R, c.sdf_f, c.nab_f, nullptr,
                                 a.sdf->multires, mlp_ws, mlp_bytes, st)))
    return rc;
  // SDF + nablas + geometry feature at the mid-points, then the radiance net (neus.py:103-106, :298)
  const int64_t Pm = (int64_t)(c.S - 1) * R;
  // with a fold pack, feat_m carries u (F8' in F8's place) and the radiance net's layer 0 is R0'
  const char* f8p = nullptr;
  const char* r0p = nullptr;
  if (a.fold_packed) {
    const FoldLayout FL = fold_layout(RL);
    f8p = (const char*)a.fold_packed + FL.f8_off;
    r0p = (const char*)a.fold_packed + FL.r0_off;
  }
  int* const claim_mid = claims ? h.mcnt + 1 : nullptr;
  int* const claim_rad = claims ? h.mcnt + 2 : nullptr;
  if (a.radiance_out || a.no_mid_skip) {  // every mid-point, as the reference
    if (claims) NR_HIP_CHECK(hipMemsetAsync(h.mcnt, 0, 3 * sizeof(int), st));
    if ((rc = launch_sdf(SL, a.sdf_packed, c.mids, Pm, c.sdf_m, c.nab_m, c.feat_m, a.sdf->multires, mlp_ws, mlp_bytes,
                         st, nullptr, 0, f8p, claim_mid)))
      return rc;
    if ((rc = launch_radiance(RL, a.rad_packed, c.mids, c.rd, 1, R, c.nab_m, c.feat_m, Pm, c.rad_m,
                              a.rad->multires_view, st, nullptr, r0p, claim_rad)))
      return rc;
  } else {  // only the mid-points whose alpha is not exactly 0 (neus_mid_compact); bit-identical maps
    NR_HIP_CHECK(hipMemsetAsync(h.mcnt, 0, (claims ? 3 : 1) * sizeof(int), st));
    const dim3 g1((unsigned)((Pm + 255) / 256));
    hipLaunchKernelGGL(neus_mid_compact, dim3((unsigned)((Pm + 1023) / 1024)), dim3(1024), 0, st, c, a.s_dev, a.s,
                       h.mcnt, h.mslot, h.midc, h.mvd);
    NR_HIP_CHECK(hipGetLastError());
    if ((rc = launch_sdf(SL, a.sdf_packed, h.midc, Pm, c.sdf_m, c.nab_m, c.feat_m, a.sdf->multires, mlp_ws, mlp_bytes,
                         st, h.mcnt, 1, f8p, claim_mid)))
      return rc;
    if ((rc = launch_radiance(RL, a.rad_packed, h.midc, h.mvd, 1, INT64_MAX, c.nab_m, c.feat_m, Pm, h.mrad,
                              a.rad->multires_view, st, h.mcnt, r0p, claim_rad)))
      return rc;
    hipLaunchKernelGGL(neus_mid_scatter, g1, dim3(256), 0, st, h.mslot, h.mrad, Pm, c.rad_m);
    NR_HIP_CHECK(hipGetLastError());
  }
  if (two) {  // join: the sample nablas are complete; into sorted order (neus_expand left them out)
    if ((rc = sj.join())) return rc;
    hipLaunchKernelGGL(neus_gather_nablas, dim3((unsigned)(((int64_t)c.S * R + 255) / 256)), dim3(256), 0, st, c);
    NR_HIP_CHECK(hipGetLastError());
  }
  NeusOut o{ray0, a.rgb, a.depth, a.acc, a.normals, a.d_final, a.sdf_out, a.nablas_out,
            a.radiance_out, a.alpha_out, a.cdf_out, a.weights_out, a.sigma_out, a.radiance_bg_out};
  if (a.N_outside > 0) {  // NeRF++ background on [mid-points ; inverted-sphere samples]
    hipLaunchKernelGGL(neus_outside_points, grd, blk, 0, st, c,
                       a.t_out_rand ? a.t_out_rand + ray0 * a.N_outside : (const float*)nullptr);
    NR_HIP_CHECK(hipGetLastError());
    const int64_t Po = (int64_t)(c.S - 1 + a.N_outside) * R;
    if (a.sigma_out || a.radiance_bg_out) {  // detailed outputs: the background at every sample, as the reference
      if ((rc = launch_nerf(nerf_layout(*a.nerf), a.nerf_packed, c.x4, c.rd, 1, R, Po, c.sig_o, c.rad_o, st)))
        return rc;
    } else {  // only the background values the compositing reads (neus_outside_compact)
      NR_HIP_CHECK(hipMemsetAsync(h.cnt, 0, sizeof(int), st));
      const dim3 g1((unsigned)((Po + 255) / 256));
      hipLaunchKernelGGL(neus_outside_compact, dim3((unsigned)((Po + 1023) / 1024)), dim3(1024), 0, st, c, h.cnt,
                         h.slot, h.x4c, h.vdc);
      NR_HIP_CHECK(hipGetLastError());
      if ((rc = launch_nerf(nerf_layout(*a.nerf), a.nerf_packed, h.x4c, h.vdc, 1, INT64_MAX, Po, h.sigc, h.radc, st,
                            h.cnt)))
        return rc;
      hipLaunchKernelGGL(neus_outside_scatter, g1, dim3(256), 0, st, h.slot, h.sigc, h.radc, Po, c.sig_o, c.rad_o);
      NR_HIP_CHECK(hipGetLastError());
    }
    if (defer) {  // deferred sample nablas: samples (or tiles) whose (inside or background) alpha != 0
      const int64_t nslot = (int64_t)c.S * R;
      c.tshift = 0;
      if (a.calc_normal) {
        NR_HIP_CHECK(hipMemsetAsync(c.tflag, 0, (size_t)nslot * sizeof(int), st));
        NR_HIP_CHECK(hipMemsetAsync(c.tcnt, 0, sizeof(int), st));
        hipLaunchKernelGGL(neus_sample_need_outside, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, st, c,
                           a.s_dev, a.s);
        NR_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(neus_point_list, dim3((unsigned)((nslot + 1023) / 1024)), dim3(1024), 0, st, c, nslot);
        NR_HIP_CHECK(hipGetLastError());
        if ((rc = launch_sdf_deferred(SL, a.sdf_packed, c.pts, nslot, nullptr, c.nraw, a.sdf->multires, c.slabs,
                                      c.tiles, c.tcnt, 4, st)))
          return rc;
      }
      hipLaunchKernelGGL(neus_gather_nablas, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, st, c);
      NR_HIP_CHECK(hipGetLastError());
    }
    ProfScope prof("neus_composite", (double)R, st);
    const int M = c.S - 1 + a.N_outside;
    const size_t lds1 = (6 * (size_t)M + 4 * (size_t)c.S) * sizeof(float);  // wave-per-ray staging of one ray
    if (4 * lds1 <= 65536)
      hipLaunchKernelGGL((neus_composite_outside_w<4>), dim3((unsigned)((R + 3) / 4)), dim3(64), 4 * lds1, st, c, o,
                         a.s_dev, a.s, a.calc_normal, a.white_bkgd);
    else if (lds1 <= 65536)
      hipLaunchKernelGGL((neus_composite_outside_w<1>), dim3((unsigned)R), dim3(64), lds1, st, c, o, a.s_dev, a.s,
                         a.calc_normal, a.white_bkgd);
    else
      hipLaunchKernelGGL(neus_composite_outside, grd, blk, 0, st, c, o, a.s_dev, a.s, a.calc_normal, a.white_bkgd);
  } else {
    ProfScope prof("neus_composite", (double)R, st);
    const size_t lds1 = 9 * (size_t)c.S * sizeof(float);  // four rays per wave when four rays' staging fits
    if (4 * lds1 <= 65536)  // the dynamic-LDS limit per workgroup (nr_neus_render checks lds1 against it)
      hipLaunchKernelGGL((neus_composite<4>), dim3((unsigned)((R + 3) / 4)), dim3(64), 4 * lds1, st, c, o, a.s_dev, a.s,
                         a.calc_normal, a.white_bkgd);
    else
      hipLaunchKernelGGL((neus_composite<1>), dim3((unsigned)R), dim3(64), lds1, st, c, o, a.s_dev, a.s, a.calc_normal,
                         a.white_bkgd);
  }
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

// rays per chunk: at most 16384, the caller's max_chunk_rays (its rayschunk) -- with no explicit
// workspace budget a hint floored at NR_MIN_CHUNK_RAYS (the reference's validation rayschunk of 256
// would leave the per-ray kernels a few CUs; memory is bounded by the default budget), exact when the
// caller also set max_workspace_bytes -- and as many as keep the workspace within
// max_workspace_bytes (the binding is affine in the chunk's ray count); deferred chunks (8 KB of slabs
// per sample) are a multiple of 16 rays, so that every launch starts a tile
static int64_t neus_chunk_rays(const NrNeusArgs* a) {
  const int64_t n = a->n_rays > 0 ? a->n_rays : 1;
  int64_t cap = 16384;
  // the floor applies to a caller that left the memory bound to the library (max_workspace_bytes 0); one
  // that set a workspace budget gets its max_chunk_rays exactly, as the reference's rayschunk loop
  if (a->max_chunk_rays > 0)
    cap = std::min(cap, a->max_workspace_bytes ? a->max_chunk_rays : std::max<int64_t>(a->max_chunk_rays, NR_MIN_CHUNK_RAYS));
  const size_t budget = a->max_workspace_bytes ? a->max_workspace_bytes : NR_DEFAULT_WORKSPACE_BYTES;
  const bool defer = neus_deferred(*a, 16);
  NeusChunk c;
  NeusHost h;  // two sizing passes, deferral decided as for a 16-ray-multiple chunk
  const size_t t1 = neus_bind(*a, 1024, nullptr, c, h), t2 = neus_bind(*a, 2048, nullptr, c, h);
  const size_t per_ray = (t2 - t1) / 1024 + 1, fixed = t1 > 1024 * per_ray ? t1 - 1024 * per_ray : 0;
  const int64_t fit = budget > fixed ? (int64_t)((budget - fixed) / per_ray) : 0;
  cap = std::min(cap, std::max<int64_t>(fit, 16));
  // deferred chunks tile exactly: a ray count that is not a multiple of 16 renders as 16-multiple
  // chunks (deferred) plus a < 16-ray tail (nablas when drawn)
  if (defer && n > 16 && n % 16) cap = std::min(cap, n / 16 * 16);
  if (n <= cap) return n;
  if (defer && cap >= 16) cap = cap / 16 * 16;
  return std::max<int64_t>(cap, 1);
}

static int check_neus(const NrNeusArgs* a) {
  static const char* const kName = "nr_neus_render";
  int rc = check_render_common(kName, a);
  if (rc) return rc;
  NR_REQUIRE(a->sdf_packed && a->rad && (a->rad_packed || a->sample_only) && a->t_coarse, NR_ERR_ARG,
             "nr_neus_render: null argument");
  NR_REQUIRE(!a->fold_packed || fold_applies(*a->sdf, *a->rad), NR_ERR_ARG,
             "nr_neus_render: a fold pack needs the f16x3 softplus SDF net and a f16x3 ReLU D=4 radiance net");
  NR_REQUIRE(a->N_samples >= 2, NR_ERR_ARG, "nr_neus_render: N_samples must be >= 2");
  if ((rc = check_render_normals(kName, a))) return rc;
  NR_REQUIRE(a->N_outside >= 0, NR_ERR_ARG, "nr_neus_render: N_outside must be >= 0");
  if (a->N_outside > 0) {
    if ((rc = check_nerf_desc(a->nerf))) return rc;
    NR_REQUIRE(a->nerf_packed && a->t_outside, NR_ERR_ARG, "nr_neus_render: N_outside > 0 needs the NeRF++ net");
  }
  NR_REQUIRE(a->upsample_algo >= NR_UPSAMPLE_OFFICIAL && a->upsample_algo <= NR_UPSAMPLE_DIRECT_MORE, NR_ERR_ARG,
             "nr_neus_render: unknown upsample_algo");
  if (a->upsample_algo != NR_UPSAMPLE_OFFICIAL) {
    NR_REQUIRE(a->N_importance >= 1 && a->u_fine && a->fixed_s > 0.f, NR_ERR_ARG,
               "nr_neus_render: direct upsampling needs N_importance >= 1, u_fine and fixed_s > 0");
    NR_REQUIRE(a->upsample_algo != NR_UPSAMPLE_DIRECT_MORE || (a->N_nograd_samples >= 2 && a->t_nograd), NR_ERR_ARG,
               "nr_neus_render: direct_more needs N_nograd_samples >= 2 and t_nograd");
  } else if (a->N_upsample_iters > 0) {
    const int n_up = a->N_importance / a->N_upsample_iters;
    NR_REQUIRE(n_up >= 1 && n_up <= kMaxUp && a->u_fine, NR_ERR_UNSUPPORTED,
               "nr_neus_render: N_importance/N_upsample_iters must be in [1, 32]");
  }
  return NR_OK;
}

}  // namespace nr

using namespace nr;

extern "C" size_t nr_neus_workspace_bytes(const NrNeusArgs* a) {
  if (!a) return 0;
  NeusChunk c;
  NeusHost h;
  return neus_bind(*a, neus_chunk_rays(a), nullptr, c, h);
}

extern "C" int nr_neus_render(const NrNeusArgs* a, void* stream) {
  int rc = check_neus(a);
  if (rc || a->n_rays <= 0) return rc;
  const int64_t Rc = neus_chunk_rays(a);
  NeusChunk c;
  NeusHost h;
  const size_t total = neus_bind(*a, Rc, (char*)a->workspace, c, h);
  NR_REQUIRE(a->workspace && a->workspace_bytes >= total, NR_ERR_WORKSPACE, "nr_neus_render: workspace too small");
  // the wave-per-ray upsampling / compositing kernels stage S samples per ray in LDS
  size_t lds_max;
  if ((rc = lds_limit(lds_max))) return rc;
  NR_REQUIRE((size_t)9 * c.S * sizeof(float) <= lds_max, NR_ERR_UNSUPPORTED,
             "nr_neus_render: N_samples + N_importance too large for the per-ray LDS staging of the compositing");
  return for_chunks(a->n_rays, Rc, [&](int64_t r0, int R) { return neus_chunk(*a, c, h, r0, R, (hipStream_t)stream); });
}

