// neurecon_amd — the volume-rendering integral, written once for the render kernels (nr_neus.hip,
// nr_volsdf.hip, nr_unisurf.hip) and the training compositing kernels (nr_train.hip): the per-sample
// opacity formulas, the transmittance / weight step with its fp64 sums and epilogue, the part of the
// backward that all four frameworks' kernels share, and the wave scans of the lane-parallel kernels.
// The mid-point compaction and the deferred-nabla flags skip a sample exactly when the compositing's
// alpha is 0.0f, and the training forward reproduces the render kernels' rounding: both hold because
// every kernel calls these helpers.  Scalars and plain pointers only (no chunk structs).
#pragma once
#include "nr_common.h"

namespace nr {

// ---------------------------------------------------------------------------------------------
// per-sample formulas
// ---------------------------------------------------------------------------------------------
// F.normalize(v, dim=-1): v / max(||v||_2, 1e-12)
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
  const float n = norm3_ref(x, y, z);
  const float d = fmaxf(n, 1e-12f);
  x = fdiv(x, d);
  y = fdiv(y, d);
  z = fdiv(z, d);
}

// one 3-vector of a ray-major detailed output
__device__ __forceinline__ void copy3(float* dst, const float* src) {
  dst[0] = src[0];
  dst[1] = src[1];
  dst[2] = src[2];
}

// NeuS (neus.py:28-35): logistic CDF of the scaled SDF, alpha = max((c_i - c_{i+1}) / (c_i + 1e-10), 0)
__device__ __forceinline__ float neus_cdf(float sdf, float s) { return sigmoidf_ref(fmul(sdf, s)); }
__device__ __forceinline__ float neus_alpha(float cp, float cn) {
  return fmaxf(fdiv(fsub(cp, cn), fadd(cp, 1e-10f)), 0.0f);
}

// NeuS + NeRF++ (neus.py:325-343): |o_r + d_r dm| <= r_obj, the mid-point takes the SDF's alpha and colour
// (ro, rd: [R][3], r of the kernel's own index type)
template <class Index>
__device__ __forceinline__ bool inside_sphere(const float* ro, const float* rd, Index r, float dm, float r_obj) {
  const float px = fadd(ro[r * 3], fmul(rd[r * 3], dm)), py = fadd(ro[r * 3 + 1], fmul(rd[r * 3 + 1], dm)),
              pz = fadd(ro[r * 3 + 2], fmul(rd[r * 3 + 2], dm));
  return norm3_ref(px, py, pz) <= r_obj;
}

// F.softplus (beta 1, threshold 20) and its derivative (softplus_backward)
__device__ __forceinline__ float softplus1(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
__device__ __forceinline__ double softplus1_grad(float x) { return x > 20.0f ? 1.0 : 1.0 / (1.0 + exp(-(double)x)); }

// NeRF++ background sample: alpha = 1 - exp(-softplus(sigma) dist), dist = d_{k+1} - d_k (1e10 for the last)
// (dk = d[k]; d[next] is sample k + 1 in the kernel's layout, read only if has_next)
template <class Index>
__device__ __forceinline__ float nerfpp_dist(float dk, const float* d, Index next, bool has_next) {
  return has_next ? fsub(d[next], dk) : 1e10f;
}
__device__ __forceinline__ float nerfpp_alpha(float sigma, float dist) {
  return fsub(1.0f, expf(fmul(-softplus1(sigma), dist)));
}

// UNISURF (unisurf.py:53-62): alpha = odds / (1 + odds), odds = exp(-logit)
__device__ __forceinline__ float uni_alpha(float lg) {
  const float odds = expf(-lg);
  return fdiv(odds, fadd(1.0f, odds));
}

// the shifted transparency 1 - alpha + 1e-10: a factor of the transmittance cumprod (neus.py:67,
// unisurf.py:226), and VolSDF's opacity 1 - p + 1e-10 of an interval (volsdf.py:484)
__device__ __forceinline__ float transparency(float alpha) { return fadd(fsub(1.0f, alpha), 1e-10f); }

// VolSDF sdf_to_sigma (volsdf.py:16-35): alpha * (sdf >= 0 ? 0.5 exp(-|sdf|/beta) : 1 - 0.5 exp(-|sdf|/beta))
__device__ __forceinline__ float vs_sigma(float s, float alpha, float beta) {
  const float e = fmul(0.5f, expf(fdiv(-fabsf(s), beta)));
  return fmul(alpha, s >= 0.0f ? e : fsub(1.0f, e));
}
// builtin background sphere (volsdf.py:317-325): a sample whose r_bg - |x| is smaller takes that value
// (masked: it then passes no gradient to the network); |x| as torch forms it (norm3_ref)
__device__ __forceinline__ float vs_sdf_bg(float v, const float* x, int use_bg, float r_bg, bool& masked) {
  masked = false;
  if (use_bg) {
    const float dbg = fsub(r_bg, norm3_ref(x[0], x[1], x[2]));
    if (dbg < v) {
      v = dbg;
      masked = true;
    }
  }
  return v;
}
// p_i = exp(-relu(sigma_i delta_i)), tau_i = (1 - p_i + 1e-10) T_i (volsdf.py:481-487)
__device__ __forceinline__ float vs_p(float sigma, float delta) { return expf(-fmaxf(fmul(sigma, delta), 0.0f)); }
__device__ __forceinline__ float vs_tau(float p, float T) { return fmul(transparency(p), T); }

// ---------------------------------------------------------------------------------------------
// the accumulator: transmittance, colour / opacity / normal sums in fp64 (ATen's CPU accumulation
// type), each term rounded to fp32 first, and the epilogue of a ray.  The serial kernels step it per
// sample; the lane-parallel ones fill the sums from their wave reductions and share denom / finish.
// ---------------------------------------------------------------------------------------------
struct Composite {
  double T = 1.0, acc = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
  float accf = 0.0f;

  // w_i = alpha_i T_i, T_{i+1} = T_i (1 - alpha_i + 1e-10)
  __device__ __forceinline__ float weight(float alpha) {
    const float w = fmul(alpha, (float)T);
    T *= (double)transparency(alpha);
    return w;
  }
  // VolSDF: tau_i = (1 - p_i + 1e-10) T_i, T_{i+1} = T_i p_i
  __device__ __forceinline__ float weight_tau(float p) {
    const float tau = vs_tau(p, (float)T);
    T *= (double)p;
    return tau;
  }
  __device__ __forceinline__ void add(float w, const float* col) {
    c0 += (double)fmul(w, col[0]);
    c1 += (double)fmul(w, col[1]);
    c2 += (double)fmul(w, col[2]);
    acc += (double)w;
  }
  __device__ __forceinline__ void add_normal(float w, float x, float y, float z) {  // unit normal
    n0 += (double)fmul(x, w);
    n1 += (double)fmul(y, w);
    n2 += (double)fmul(z, w);
  }
  // the depth normaliser acc + 1e-10 (depth = sum_i w_i / denom d_i, summed by the kernel)
  __device__ __forceinline__ float denom() {
    accf = (float)acc;
    return fadd(accf, 1e-10f);
  }
  // after denom(): white background rgb += 1 - acc, and the maps of ray r (normals: NULL for none)
  __device__ __forceinline__ void finish(float depth_r, int white_bkgd, int64_t r, float* rgb, float* depth,
                                         float* acc_map, float* normals) const {
    float q0 = (float)c0, q1 = (float)c1, q2 = (float)c2;
    if (white_bkgd) {
      const float bg = fsub(1.0f, accf);
      q0 = fadd(q0, bg); q1 = fadd(q1, bg); q2 = fadd(q2, bg);
    }
    rgb[r * 3 + 0] = q0;
    rgb[r * 3 + 1] = q1;
    rgb[r * 3 + 2] = q2;
    depth[r] = depth_r;
    acc_map[r] = accf;
    if (normals) {
      normals[r * 3 + 0] = (float)n0;
      normals[r * 3 + 1] = (float)n1;
      normals[r * 3 + 2] = (float)n2;
    }
  }
};

// ---------------------------------------------------------------------------------------------
// what the four backward kernels share: the incoming gradients of ray r (NULL as a zero tensor), the
// adjoint of weight w_i and d radiance_i = w_i g_rgb
// ---------------------------------------------------------------------------------------------
struct CompositeGrads {
  float gr0, gr1, gr2;
  double gd, ga;
  __device__ __forceinline__ CompositeGrads(const float* g_rgb, const float* g_depth, const float* g_acc, int64_t r,
                                            int white_bkgd) {
    gr0 = g_rgb ? g_rgb[r * 3 + 0] : 0.f, gr1 = g_rgb ? g_rgb[r * 3 + 1] : 0.f, gr2 = g_rgb ? g_rgb[r * 3 + 2] : 0.f;
    gd = g_depth ? (double)g_depth[r] : 0.0;
    // white_bkgd: rgb += 1 - acc -> acc receives -sum(g_rgb)
    ga = (g_acc ? (double)g_acc[r] : 0.0) - (white_bkgd ? (double)gr0 + gr1 + gr2 : 0.0);
  }
  // dL/dw_i: colour col, depth d, A = acc + 1e-10, wd = sum_j w_j d_j; g_w: direct weight gradients or NULL
  __device__ __forceinline__ double weight_adjoint(const float* col, double d, double A, double wd, const float* g_w,
                                                   int64_t q) const {
    double v = (double)gr0 * col[0] + (double)gr1 * col[1] + (double)gr2 * col[2] + ga;
    v += gd * (d / A - wd / (A * A));
    if (g_w) v += (double)g_w[q];
    return v;
  }
  __device__ __forceinline__ void d_radiance(float w, float* d_rad) const {
    d_rad[0] = fmul(w, gr0);
    d_rad[1] = fmul(w, gr1);
    d_rad[2] = fmul(w, gr2);
  }
};

// ---------------------------------------------------------------------------------------------
// fp64 scans and sums over the 64 lanes of a one-wave workgroup
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_scan_mul(double v) {  // inclusive prefix product
  const int l = threadIdx.x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o);
    if (l >= o) v *= t;
  }
  return v;
}
__device__ __forceinline__ double wave_scan_add_rev(double v) {  // inclusive sum over lanes >= l
  const int l = threadIdx.x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_down(v, o);
    if (l + o < 64) v += t;
  }
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {  // fixed butterfly: every lane gets the same sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace nr
