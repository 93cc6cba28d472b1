// neurecon_amd — VolSDF render path internals (models/frameworks/volsdf.py, render mode).
#pragma once
#include "nr_common.h"

namespace nr {

// Device views of one ray chunk.  Per-ray sample lists are ray-major ([ray][cap]) and are
// processed one wave (= one 64-thread workgroup) per ray; the MLP kernels see flat point lists.
struct VolChunk {
  int R;          // rays in this chunk
  int N0;         // initial samples of the error-bounded sampler (4 * N_samples)
  int N_up;       // samples added per round (4 * N_samples)
  int cap;        // list capacity = N0 + max_iter * N_up
  int N_samples;  // coarse samples (final pass)
  int N_imp;      // fine samples (final pass)
  int S;          // N_samples + N_imp
  int max_iter, max_bisect;
  float alpha_net, beta_net, beta_plus0, eps;
  float near, far, r_bg;
  int use_bg;
  float* ro; float* rd;            // [R][3] (rd normalised)
  float* Ld[2]; float* Ls[2];      // ping-pong sample lists [R][cap]
  float* dnew[2];                  // ping-pong new samples [R][N_up] (by active slot)
  float* pts;                      // MLP input, flat
  float* sraw;                     // MLP output, flat
  int* act[2];                     // ping-pong active ray lists
  int* cnt;                        // [max_iter + 1] active counts (zeroed per chunk)
  float* beta;                     // [R] current beta+
  float* fine;                     // [R][N_imp] final fine depths
  float* usage;                    // [R] iter_usage
  float* bmap;                     // [R] beta_map
  // final pass (ray-major [R][S])
  float* d_all; float* pts_f; float* sdf_f; float* nab_f; float* feat_f; float* rad_f;
  const float* t_coarse; const float* t_init; const float* u_up; const float* u_fine;
  const float* u_rand;             // perturb: [R][N_imp] per-ray sorted uniforms of the final sample_cdf
  const float* u_out;              // perturb: [R][N_out] NeRF++ strata uniforms
  // NeRF++ background (N_out > 0): per-ray far (sphere exit) and beta+ init, outside samples
  int N_out;
  float beta_k;                    // float32(4 (N0 - 1) log(1 + eps))
  float* farr;                     // [R] far per ray
  float* bp0;                      // [R] beta+ init per ray
  const float* rs_out;             // [N_out] radii of the background spheres
  float* d_out;                    // [R][N_out] background depths
  float* x4;                       // [R][N_out][4] NeRF input [p / r, 1 / r]
  float* sig_o; float* rad_o;      // [R][N_out], [R][N_out][3] NeRF outputs
};

struct VolOut {
  int64_t ray0;
  float* rgb; float* depth; float* acc; float* normals;
  float* d_vals; float* sdf; float* nablas; float* radiance; float* alpha; float* p_i; float* weights;
  float* sigma; float* beta_map; float* iter_usage;
  float* sigma_bg; float* radiance_bg;
};

// what only the host orchestration reads (nr_volsdf.hip volsdf_bind / volsdf_chunk)
struct VolHost {
  void* mlp_ws; size_t mlp_bytes;  // the MLP kernels' reverse-pass scratch: the rest of the workspace
  size_t lds_bytes;                // dynamic LDS of the per-ray kernels
};

__global__ void volsdf_prologue(VolChunk c, const float* rays_o, const float* rays_d);
__global__ void volsdf_first(VolChunk c);
__global__ void volsdf_iter(VolChunk c, int it);
__global__ void volsdf_points(VolChunk c);
__global__ void volsdf_outside(VolChunk c);
__global__ void volsdf_composite(VolChunk c, VolOut o, int calc_normal, int white_bkgd);

}  // namespace nr
