// neurecon_amd — C-ABI entry points (include/neurecon_hip.h) that belong to no single framework:
// the net descriptors and their checks, the packed-weight layouts and packs, the per-net forward and
// training entry points, the NeuS fold entries and nr_sample_pdf.  The render entry points
// (nr_*_workspace_bytes, nr_*_render) live with their framework: nr_neus.hip, nr_volsdf.hip,
// nr_unisurf.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "nr_common.h"
#include "nr_mlp.h"
#include "nr_neus.h"
#include "nr_tgemm.h"

namespace nr {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

static int64_t chunk_bytes_host(int KB) { return (int64_t)(2 * KB + 1) * 1024; }

// ---------------------------------------------------------------------------------------------
// descriptors
// ---------------------------------------------------------------------------------------------
int check_sdf_desc(const NrSdfDesc* d) {
  NR_REQUIRE(d, NR_ERR_ARG, "null NrSdfDesc");
  if (d->siren) {
    NR_REQUIRE(d->D == 5 && d->W == 256 && d->skip < 0 && d->multires < 0 && d->W_geo_feat == 256,
               NR_ERR_UNSUPPORTED,
               "SIREN SDF net: only D=5, W=256, skips=[], embed_multires=-1, W_geo_feat=256 (configs/volsdf_siren.yaml)");
    NR_REQUIRE(d->precision == NR_PREC_FP32 || d->precision == NR_PREC_F16X3, NR_ERR_UNSUPPORTED,
               "SDF net: unknown precision mode");
    return NR_OK;
  }
  NR_REQUIRE(d->D == 8 && d->W == 256 && d->skip == 4 && d->multires == 6 && d->W_geo_feat == 256,
             NR_ERR_UNSUPPORTED,
             "SDF net: only D=8, W=256, skips=[4], embed_multires=6, W_geo_feat=256 are implemented");
  NR_REQUIRE(d->precision == NR_PREC_FP32 || d->precision == NR_PREC_F16X3, NR_ERR_UNSUPPORTED,
             "SDF net: unknown precision mode");
  return NR_OK;
}

int check_rad_desc(const NrRadDesc* d) {
  NR_REQUIRE(d, NR_ERR_ARG, "null NrRadDesc");
  NR_REQUIRE((d->D == 4 || d->D == 5) && d->W == 256 && d->multires < 0 && d->W_geo_feat == 256 &&
                 d->multires_view <= 7,
             NR_ERR_UNSUPPORTED,
             "radiance net: only D=4 or 5, W=256, embed_multires=-1, embed_multires_view<=7, W_geo_feat=256");
  NR_REQUIRE(d->precision == NR_PREC_FP32 || d->precision == NR_PREC_F16X3, NR_ERR_UNSUPPORTED,
             "radiance net: unknown precision mode");
  return NR_OK;
}


SdfLayout sdf_layout(const NrSdfDesc& d) {
  SdfLayout L{};
  L.prec = d.precision;
  L.siren = d.siren ? 1 : 0;
  const int nops = L.siren ? kSirenOps : kSdfOps;
  const int* KB = L.siren ? kSirenKB : kSdfKB;
  const int* NBO = L.siren ? kSirenNBO : kSdfNBO;
  size_t off = 0;
  for (int i = 0; i < nops; ++i) {
    L.op_bytes[i] = (2 * KB[i] + 1) * 1024;
    L.op_off[i] = (uint32_t)off;
    off += (size_t)(NBO[i] / 2) * L.op_bytes[i];
  }
  static_assert(sdf_op_off(kSdfOps - 1) + (kSdfNBO[kSdfOps - 1] / 2) * (2 * kSdfKB[kSdfOps - 1] + 1) * 1024 > 0, "");
  L.scale_off = (uint32_t)off;
  L.winv_off = L.scale_off + 128;  // inside scale_off's 256 bytes: the pack's size and offsets stay
  static_assert(kSdfOps * 4 <= 128, "max |W| and 1 / weight scale share 256 bytes");
  off = align256(off + 128 + kSdfOps * 4);
  L.bound_off = (uint32_t)off;
  off = align256(off + kSdfOps * 8);
  L.w8row0_off = (uint32_t)off;
  off = align256(off + 256 * 4);
  L.misc_off = (uint32_t)off;
  off = align256(off + 16);
  L.total = (uint32_t)off;
  return L;
}

// small input columns of layer 0 ahead of the feature: x, then (use_view_dirs) embed_view(v), normals
static int rad_small(const NrRadDesc& d) {
  return d.no_view_dirs ? 3 : 3 + (d.multires_view < 0 ? 3 : 3 + 6 * d.multires_view) + 3;
}

RadLayout rad_layout(const NrRadDesc& d) {
  RadLayout L{};
  L.prec = d.precision;
  L.n_small = rad_small(d);
  L.view = d.no_view_dirs ? 0 : 1;
  L.D = d.D;
  L.siren = d.siren ? 1 : 0;
  L.kbs = L.n_small <= 32 ? 2 : 4;
  size_t off = 0;
  for (int i = 0; i < L.D; ++i) {
    const int kb = i == 0 ? 16 + L.kbs : 16;
    L.op_bytes[i] = (2 * kb + 1) * 1024;
    L.op_off[i] = (uint32_t)off;
    off += 8 * (size_t)L.op_bytes[i];
  }
  L.scale_off = (uint32_t)off;
  off = align256(off + 5 * 4);
  L.bound_off = (uint32_t)off;
  off = align256(off + 5 * 2 * 4);
  L.head_off = (uint32_t)off;
  off = align256(off + (3 * 256 + 4) * 4);
  L.total = (uint32_t)off;
  return L;
}

bool fold_applies(const NrSdfDesc& sd, const NrRadDesc& rd) {
  return sd.precision == NR_PREC_F16X3 && !sd.siren && sd.W_geo_feat == 256 && rd.precision == NR_PREC_F16X3 &&
         !rd.siren && rd.D == 4 && rd.W_geo_feat == 256;
}

FoldLayout fold_layout(const RadLayout& RL) {
  FoldLayout F{};
  F.kbs = RL.kbs;
  size_t off = 0;
  F.f8_off = (uint32_t)off;
  off += 8 * (size_t)chunk_bytes_host(16);
  F.r0_off = (uint32_t)off;
  off += 8 * (size_t)chunk_bytes_host(RL.kbs);
  F.scale_off = (uint32_t)off;
  off = align256(off + 2 * 4);
  F.bound_off = (uint32_t)off;
  off = align256(off + 2 * 2 * 4);
  F.u_off = (uint32_t)off;
  off = align256(off + (256 * 256 + 256) * 4);
  F.total = (uint32_t)off;
  return F;
}

int check_nerf_desc(const NrNerfDesc* d) {
  NR_REQUIRE(d, NR_ERR_ARG, "null NrNerfDesc");
  NR_REQUIRE(d->D == 8 && d->W == 256 && d->skip == 4 && d->input_ch == 4 && d->multires == 10 &&
                 d->multires_view == 4,
             NR_ERR_UNSUPPORTED,
             "NeRF net: only the NeRF++ background configuration (D=8, W=256, skips=[4], input_ch=4, "
             "multires=10, multires_view=4, use_view_dirs) is implemented");
  NR_REQUIRE(d->precision == NR_PREC_FP32 || d->precision == NR_PREC_F16X3, NR_ERR_UNSUPPORTED,
             "NeRF net: unknown precision mode");
  return NR_OK;
}

// (input blocks, output blocks) of each NeRF GEMM op: N0..N7, feature, views
static const int kNerfKB[kNerfOps] = {6, 16, 16, 16, 16, 22, 16, 16, 16, 18};
static const int kNerfNBO[kNerfOps] = {16, 16, 16, 16, 16, 16, 16, 16, 16, 8};

// output blocks of NeRF op i: f16x3's NF also carries alpha_linear (blocks 16-17, row 0 = sigma)
static int nerf_nbo(int i, int prec) { return (i == NF && prec == NR_PREC_F16X3) ? 18 : kNerfNBO[i]; }

NerfLayout nerf_layout(const NrNerfDesc& d) {
  NerfLayout L{};
  L.prec = d.precision;
  size_t off = 0;
  for (int i = 0; i < kNerfOps; ++i) {
    L.op_bytes[i] = (2 * kNerfKB[i] + 1) * 1024;
    L.op_off[i] = (uint32_t)off;
    off += (size_t)(nerf_nbo(i, d.precision) / 2) * L.op_bytes[i];
  }
  L.scale_off = (uint32_t)off;
  off = align256(off + kNerfOps * 4);
  L.bound_off = (uint32_t)off;
  off = align256(off + kNerfOps * 2 * 4);
  L.alpha_off = (uint32_t)off;
  off = align256(off + 257 * 4);
  L.rgb_off = (uint32_t)off;
  off = align256(off + (3 * 128 + 3) * 4);
  L.total = (uint32_t)off;
  return L;
}

static PackSeg seg(int nblk, int off, int nvalid) { return PackSeg{nblk, off, nvalid}; }
static PackOp mkop(const float* W, const float* bias, int rows, int ld, int tr, PackSeg o0, PackSeg o1, PackSeg i0,
                   PackSeg i1, float scale, int prec, float* wmax) {
  PackOp op{};
  op.W = W; op.bias = bias; op.wn = (int64_t)rows * ld; op.ld = ld; op.transpose = tr;
  op.out[0] = o0; op.out[1] = o1; op.in[0] = i0; op.in[1] = i1;
  op.scale = scale; op.prec = prec; op.wmax = wmax;
  return op;
}
static PackSeg none() { return PackSeg{0, 0, 0}; }

static size_t scratch_bytes() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return (size_t)cus * kScratchPerWG;
}

}  // namespace nr

using namespace nr;

extern "C" {

int nr_version(void) { return 1; }
#ifndef NR_BUILD_ID
#define NR_BUILD_ID "unknown-source00"
#endif
// the marker lets neurecon_amd/build.py read the ID from the file without loading it
__attribute__((used)) static const char kBuildIdMarker[] = "NR_BUILD_ID=" NR_BUILD_ID;
const char* nr_build_id(void) { return kBuildIdMarker + 12; }
const char* nr_last_error(void) { return g_err.c_str(); }

int nr_set_workgroup_cap(int n) {
  NR_REQUIRE(n >= 0, NR_ERR_ARG, "nr_set_workgroup_cap: the cap must be >= 0");
  set_workgroup_cap(n);
  return NR_OK;
}

size_t nr_sdf_packed_bytes(const NrSdfDesc* d) {
  if (check_sdf_desc(d)) return 0;
  return sdf_layout(*d).total;
}

int nr_sdf_pack(const NrSdfDesc* d, const float* const* W, const float* const* b, void* packed, void* stream) {
  int rc = check_sdf_desc(d);
  if (rc) return rc;
  NR_REQUIRE(W && b && packed, NR_ERR_ARG, "nr_sdf_pack: null argument");
  for (int l = 0; l <= d->D; ++l) NR_REQUIRE(W[l] && b[l], NR_ERR_ARG, "nr_sdf_pack: null layer pointer");
  hipStream_t st = (hipStream_t)stream;
  const SdfLayout L = sdf_layout(*d);
  char* P = (char*)packed;
  if (L.siren) {  // S0..S4, SF, SB4..SB0 (nr_mlp.h SirenOp); layer 5 = Linear(256 -> 257)
    const int prec = d->precision;
    float* wmax = (float*)(P + L.scale_off);
    float* bound = (float*)(P + L.bound_off);
    PackOp ops[kSirenOps];
    ops[S0] = mkop(W[0], b[0], 256, 3, 0, seg(16, 0, 256), none(), seg(4, 0, 3), none(), 1.0f, prec, wmax + S0);
    for (int l = 1; l < 5; ++l)
      ops[S0 + l] = mkop(W[l], b[l], 256, 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec,
                         wmax + S0 + l);
    ops[SF] = mkop(W[5], b[5], 257, 256, 0, seg(16, 1, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + SF);
    for (int l = 4; l >= 1; --l)
      ops[SB4 + (4 - l)] = mkop(W[l], nullptr, 256, 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f,
                                prec, wmax + SB4 + (4 - l));
    ops[SB0] = mkop(W[0], nullptr, 256, 3, 1, seg(4, 0, 3), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + SB0);
    char* dst[kSirenOps];
    for (int i = 0; i < kSirenOps; ++i) {
      ops[i].bound = bound + 2 * i;
      dst[i] = P + L.op_off[i];
    }
    if ((rc = launch_pack_ops(ops, dst, kSirenOps, st))) return rc;
    if ((rc = launch_pack_vec(W[5], 0, 256, 256, P + L.w8row0_off, st))) return rc;
    return launch_pack_vec(b[5], 0, 1, 4, P + L.misc_off, st);
  }
  const int in0 = 39, n3 = 217;
  const float isq2 = 1.0f / 1.41421356237309504880f;
  const int prec = d->precision;
  float* wmax = (float*)(P + L.scale_off);
  auto ROWS = [&](int l) { return l == 3 ? n3 : (l == 8 ? 257 : 256); };
  PackOp ops[kSdfOps];
  // forward
  ops[F0] = mkop(W[0], b[0], ROWS(0), in0, 0, seg(16, 0, 256), none(), seg(4, 0, in0), none(), 1.0f, prec, wmax + F0);
  ops[F1] = mkop(W[1], b[1], ROWS(1), 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + F1);
  ops[F2] = mkop(W[2], b[2], ROWS(2), 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + F2);
  ops[F3] = mkop(W[3], b[3], ROWS(3), 256, 0, seg(14, 0, n3), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + F3);
  ops[F4] = mkop(W[4], b[4], ROWS(4), 256, 0, seg(16, 0, 256), none(), seg(14, 0, n3), seg(4, n3, in0), isq2, prec, wmax + F4);
  ops[F5] = mkop(W[5], b[5], ROWS(5), 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + F5);
  ops[F6] = mkop(W[6], b[6], ROWS(6), 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + F6);
  ops[F7] = mkop(W[7], b[7], ROWS(7), 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + F7);
  ops[F8] = mkop(W[8], b[8], ROWS(8), 256, 0, seg(16, 1, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + F8);
  // backward (transposed)
  ops[B7] = mkop(W[7], nullptr, ROWS(7), 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + B7);
  ops[B6] = mkop(W[6], nullptr, ROWS(6), 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + B6);
  ops[B5] = mkop(W[5], nullptr, ROWS(5), 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + B5);
  ops[B4] = mkop(W[4], nullptr, ROWS(4), 256, 1, seg(14, 0, n3), seg(4, n3, in0), seg(16, 0, 256), none(), isq2, prec, wmax + B4);
  ops[B3] = mkop(W[3], nullptr, ROWS(3), 256, 1, seg(16, 0, 256), none(), seg(14, 0, n3), none(), 1.0f, prec, wmax + B3);
  ops[B2] = mkop(W[2], nullptr, ROWS(2), 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + B2);
  ops[B1] = mkop(W[1], nullptr, ROWS(1), 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + B1);
  ops[B0] = mkop(W[0], nullptr, ROWS(0), in0, 1, seg(4, 0, in0), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + B0);
  float* bound = (float*)(P + L.bound_off);
  for (int i = 0; i < kSdfOps; ++i) ops[i].bound = bound + 2 * i;
  // per-op scalar table of the lean ops (sdf4_kernel's reverse pass): 1 / weight scale beside (R, B)
  for (int i = 0; i < kSdfOps; ++i) ops[i].winv = (float*)(P + L.winv_off) + i;
  ops[F7].aux = W[8];  // sdf row W8[0, :] rides with F7's chunks (F7Epi4's running dot product)
  char* dst[kSdfOps];
  for (int i = 0; i < kSdfOps; ++i) dst[i] = P + L.op_off[i];
  if ((rc = launch_pack_ops(ops, dst, kSdfOps, st))) return rc;
  if ((rc = launch_pack_vec(W[8], 0, 256, 256, P + L.w8row0_off, st))) return rc;
  if ((rc = launch_pack_vec(b[8], 0, 1, 4, P + L.misc_off, st))) return rc;
  return NR_OK;
}

size_t nr_mlp_workspace_bytes(int with_backward) { return with_backward ? scratch_bytes() : 0; }

int nr_sdf_forward(const NrSdfDesc* d, const void* packed, const float* pts, int64_t P, float* sdf, float* nabla,
                   float* feature, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_sdf_desc(d);
  if (rc) return rc;
  NR_REQUIRE(packed && pts && sdf && P >= 0, NR_ERR_ARG, "nr_sdf_forward: null argument");
  return launch_sdf(sdf_layout(*d), packed, pts, P, sdf, nabla, feature, d->multires, workspace, workspace_bytes,
                    (hipStream_t)stream);
}

size_t nr_nerf_packed_bytes(const NrNerfDesc* d) {
  if (check_nerf_desc(d)) return 0;
  return nerf_layout(*d).total;
}

int nr_nerf_pack(const NrNerfDesc* d, const float* const* W, const float* const* b, void* packed, void* stream) {
  int rc = check_nerf_desc(d);
  if (rc) return rc;
  NR_REQUIRE(W && b && packed, NR_ERR_ARG, "nr_nerf_pack: null argument");
  for (int l = 0; l < 12; ++l) NR_REQUIRE(W[l] && b[l], NR_ERR_ARG, "nr_nerf_pack: null layer pointer");
  hipStream_t st = (hipStream_t)stream;
  const NerfLayout L = nerf_layout(*d);
  char* P = (char*)packed;
  const int prec = d->precision;
  float* wmax = (float*)(P + L.scale_off);
  const int in0 = 84, inv = 27;
  PackOp ops[kNerfOps];
  ops[N0] = mkop(W[0], b[0], 256, in0, 0, seg(16, 0, 256), none(), seg(6, 0, in0), none(), 1.0f, prec, wmax + N0);
  for (int i = 1; i < 8; ++i) {
    if (i == 5)  // Linear(W + input_ch, W): columns [input_pts(84) | h(256)] -> K blocks [h ; input_pts]
      ops[i] = mkop(W[i], b[i], 256, 256 + in0, 0, seg(16, 0, 256), none(), seg(16, in0, 256), seg(6, 0, in0), 1.0f,
                    prec, wmax + i);
    else
      ops[i] = mkop(W[i], b[i], 256, 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + i);
  }
  if (prec == NR_PREC_F16X3) {  // [feature_linear; alpha_linear]: sigma = row 0 of output block 16
    ops[NF] = mkop(W[8], b[8], 256, 256, 0, seg(16, 0, 256), seg(2, 0, 1), seg(16, 0, 256), none(), 1.0f, prec,
                   wmax + NF);
    ops[NF].W2 = W[10];
    ops[NF].bias2 = b[10];
    ops[NF].wn2 = 256;
    ops[NF].ld2 = 256;
  } else {
    ops[NF] = mkop(W[8], b[8], 256, 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + NF);
  }
  ops[NV] = mkop(W[9], b[9], 128, 256 + inv, 0, seg(8, 0, 128), none(), seg(16, 0, 256), seg(2, 256, inv), 1.0f, prec,
                 wmax + NV);
  float* bound = (float*)(P + L.bound_off);
  char* dst[kNerfOps];
  for (int i = 0; i < kNerfOps; ++i) {
    ops[i].bound = bound + 2 * i;
    dst[i] = P + L.op_off[i];
  }
  if ((rc = launch_pack_ops(ops, dst, kNerfOps, st))) return rc;
  if ((rc = launch_pack_vec(W[10], 0, 256, 256, P + L.alpha_off, st))) return rc;
  if ((rc = launch_pack_vec(b[10], 0, 1, 1, P + L.alpha_off + 256 * 4, st))) return rc;
  if ((rc = launch_pack_vec(W[11], 0, 384, 384, P + L.rgb_off, st))) return rc;
  if ((rc = launch_pack_vec(b[11], 0, 3, 3, P + L.rgb_off + 384 * 4, st))) return rc;
  return NR_OK;
}

int nr_nerf_forward(const NrNerfDesc* d, const void* packed, const float* x4, const float* vdir, int64_t vdir_div,
                    int64_t P, float* sigma, float* rgb, void* stream) {
  int rc = check_nerf_desc(d);
  if (rc) return rc;
  NR_REQUIRE(packed && x4 && vdir && sigma && rgb && vdir_div > 0 && P >= 0, NR_ERR_ARG,
             "nr_nerf_forward: bad argument");
  return launch_nerf(nerf_layout(*d), packed, x4, vdir, vdir_div, INT64_MAX, P, sigma, rgb, (hipStream_t)stream);
}

size_t nr_radiance_packed_bytes(const NrRadDesc* d) {
  if (check_rad_desc(d)) return 0;
  return rad_layout(*d).total;
}

int nr_radiance_pack(const NrRadDesc* d, const float* const* W, const float* const* b, void* packed, void* stream) {
  int rc = check_rad_desc(d);
  if (rc) return rc;
  NR_REQUIRE(W && b && packed, NR_ERR_ARG, "nr_radiance_pack: null argument");
  for (int l = 0; l <= d->D; ++l) NR_REQUIRE(W[l] && b[l], NR_ERR_ARG, "nr_radiance_pack: null layer pointer");
  hipStream_t st = (hipStream_t)stream;
  const RadLayout L = rad_layout(*d);
  char* P = (char*)packed;
  const int ns = L.n_small, ld0 = ns + 256;
  PackOp ops[5];
  const int prec = d->precision;
  float* wmax = (float*)(P + L.scale_off);
  ops[0] = mkop(W[0], b[0], 256, ld0, 0, seg(16, 0, 256), none(), seg(16, ns, 256), seg(L.kbs, 0, ns), 1.0f, prec, wmax);
  for (int i = 1; i < L.D; ++i)
    ops[i] = mkop(W[i], b[i], 256, 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + i);
  float* bound = (float*)(P + L.bound_off);
  char* dst[5];
  for (int i = 0; i < L.D; ++i) {
    ops[i].bound = bound + 2 * i;
    dst[i] = P + L.op_off[i];
  }
  if ((rc = launch_pack_ops(ops, dst, L.D, st))) return rc;
  if ((rc = launch_pack_vec(W[L.D], 0, 768, 768, P + L.head_off, st))) return rc;
  if ((rc = launch_pack_vec(b[L.D], 0, 3, 4, P + L.head_off + 768 * 4, st))) return rc;
  return NR_OK;
}

int nr_radiance_forward(const NrRadDesc* d, const void* packed, const float* x, const float* vdir, int64_t vdir_div,
                        const float* normals, const float* feature, int64_t P, float* rgb, void* stream) {
  int rc = check_rad_desc(d);
  if (rc) return rc;
  NR_REQUIRE(packed && x && (d->no_view_dirs || (vdir && normals)) && feature && rgb && vdir_div > 0, NR_ERR_ARG,
             "nr_radiance_forward: bad argument");
  return launch_radiance(rad_layout(*d), packed, x, vdir, vdir_div, INT64_MAX, normals, feature, P, rgb,
                         d->multires_view, (hipStream_t)stream);
}

int nr_radiance_train_fwd32(const NrRadDesc* d, const void* packed, const float* feat, const float* small,
                            int64_t ld_small, int64_t P, float* h0, float* h1, float* h2, float* h3, float* rgb,
                            void* stream) {
  int rc = check_rad_desc(d);
  if (rc) return rc;
  NR_REQUIRE(P >= 0, NR_ERR_ARG, "nr_radiance_train_fwd32: negative P");
  if (P == 0) return NR_OK;
  NR_REQUIRE(packed && feat && small && h0 && h1 && h2 && h3 && rgb, NR_ERR_ARG,
             "nr_radiance_train_fwd32: null argument");
  const RadLayout L = rad_layout(*d);
  NR_REQUIRE(ld_small >= L.n_small, NR_ERR_ARG, "nr_radiance_train_fwd32: ld_small below the small-input count");
  float* const h[4] = {h0, h1, h2, h3};
  return launch_radiance_train32(L, packed, feat, small, ld_small, L.n_small, P, h, rgb, (hipStream_t)stream);
}

// ---- NeRF++ net in the training step (nr_mlp.hip nerf_train32_*_kernel) ---------------------------
static NerfBwdLayout nerf_bwd_layout() {
  NerfBwdLayout B{};
  size_t off = 0;
  for (int i = 0; i < kNerfBwdOps; ++i) {
    B.op_bytes[i] = (2 * (i == NBV ? 8 : 16) + 1) * 1024;
    B.op_off[i] = (uint32_t)off;
    off += 8 * (size_t)B.op_bytes[i];  // 16 output blocks = 8 chunks
  }
  B.scale_off = (uint32_t)off;
  off = align256(off + kNerfBwdOps * 4);
  B.wr_off = (uint32_t)off;
  off = align256(off + 3 * 128 * 4);
  B.wa_off = (uint32_t)off;
  off = align256(off + 256 * 4);
  B.total = (uint32_t)off;
  return B;
}

size_t nr_nerf_train_packed_bytes(const NrNerfDesc* d) {
  if (check_nerf_desc(d)) return 0;
  return nerf_bwd_layout().total;
}

int nr_nerf_train_pack(const NrNerfDesc* d, const float* const* W, const float* const* b, void* packed, void* stream) {
  int rc = check_nerf_desc(d);
  if (rc) return rc;
  NR_REQUIRE(W && b && packed, NR_ERR_ARG, "nr_nerf_train_pack: null argument");
  for (int l = 0; l < 12; ++l) NR_REQUIRE(W[l], NR_ERR_ARG, "nr_nerf_train_pack: null layer pointer");
  hipStream_t st = (hipStream_t)stream;
  const NerfBwdLayout B = nerf_bwd_layout();
  char* P = (char*)packed;
  float* wmax = (float*)(P + B.scale_off);
  const int prec = d->precision == NR_PREC_F16X3 ? NR_PREC_F16X3 : NR_PREC_FP32, in0 = 84, inv = 27;
  PackOp ops[kNerfBwdOps];
  // views_linears[0]^T restricted to the feature columns: [128][256 + 27] -> out 256 (feature), in 128
  ops[NBV] = mkop(W[9], nullptr, 128, 256 + inv, 1, seg(16, 0, 256), none(), seg(8, 0, 128), none(), 1.0f, prec,
                  wmax + NBV);
  ops[NBF] = mkop(W[8], nullptr, 256, 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec,
                  wmax + NBF);
  for (int i = 7; i >= 1; --i) {
    const int o = NB7 + (7 - i);
    if (i == 5)  // input cat([x_emb(84), h4(256)]): the h4 columns 84..339
      ops[o] = mkop(W[5], nullptr, 256, 256 + in0, 1, seg(16, in0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec,
                    wmax + o);
    else
      ops[o] = mkop(W[i], nullptr, 256, 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, prec, wmax + o);
  }
  char* dst[kNerfBwdOps];
  for (int i = 0; i < kNerfBwdOps; ++i) dst[i] = P + B.op_off[i];
  if ((rc = launch_pack_ops(ops, dst, kNerfBwdOps, st))) return rc;
  if ((rc = launch_pack_vec(W[11], 0, 384, 384, P + B.wr_off, st))) return rc;
  if ((rc = launch_pack_vec(W[10], 0, 256, 256, P + B.wa_off, st))) return rc;
  return NR_OK;
}

int nr_nerf_train_fwd32(const NrNerfDesc* d, const void* packed, const float* x_emb, const float* v_emb, int64_t P,
                        float* const* h, float* feat, float* hv, float* sigma, float* rgb, void* stream) {
  int rc = check_nerf_desc(d);
  if (rc) return rc;
  NR_REQUIRE(d->precision == NR_PREC_FP32, NR_ERR_ARG, "nr_nerf_train_fwd32: the desc / pack must be NR_PREC_FP32");
  NR_REQUIRE(P >= 0, NR_ERR_ARG, "nr_nerf_train_fwd32: negative P");
  if (P == 0) return NR_OK;
  NR_REQUIRE(packed && x_emb && v_emb && h && feat && hv && sigma && rgb, NR_ERR_ARG,
             "nr_nerf_train_fwd32: null argument");
  for (int i = 0; i < 8; ++i) NR_REQUIRE(h[i], NR_ERR_ARG, "nr_nerf_train_fwd32: null activation pointer");
  NR_REQUIRE(((uintptr_t)x_emb & 15) == 0, NR_ERR_ARG, "nr_nerf_train_fwd32: x_emb must be 16-byte aligned");
  return launch_nerf_train32_fwd(nerf_layout(*d), packed, x_emb, v_emb, P, h, feat, hv, sigma, rgb,
                                 (hipStream_t)stream);
}

int nr_nerf_train_bwd32(const NrNerfDesc* d, const void* train_packed, const float* rgb, const float* hv,
                        const float* const* h, const float* g_rgb, const float* g_sigma, int64_t P, float* g3,
                        float* ghv, float* g_feat, float* const* gz, void* stream) {
  int rc = check_nerf_desc(d);
  if (rc) return rc;
  NR_REQUIRE(P >= 0, NR_ERR_ARG, "nr_nerf_train_bwd32: negative P");
  if (P == 0) return NR_OK;
  NR_REQUIRE(train_packed && rgb && hv && h && g3 && ghv && g_feat && gz, NR_ERR_ARG,
             "nr_nerf_train_bwd32: null argument");
  for (int i = 0; i < 8; ++i) NR_REQUIRE(h[i] && gz[i], NR_ERR_ARG, "nr_nerf_train_bwd32: null layer pointer");
  return launch_nerf_train32_bwd(nerf_bwd_layout(), train_packed, rgb, hv, h, g_rgb, g_sigma, P, g3, ghv, g_feat, gz,
                                 (hipStream_t)stream, d->precision == NR_PREC_F16X3);
}

// ---- training layer GEMMs (nr_mlp.hip tgemm_kernel) ---------------------------------------------
int nr_train_gemm(const NrTrainGemm* a, int KB, int KB2, int NBO, int NB2, void* stream) {
  NR_REQUIRE(a, NR_ERR_ARG, "nr_train_gemm: null argument");
  return launch_tgemm(*a, KB, KB2, NBO, NB2, (hipStream_t)stream);
}

static int softplus_net(const NrSdfDesc* d) {
  int rc = check_sdf_desc(d);
  if (rc) return rc;
  NR_REQUIRE(!d->siren && d->precision == NR_PREC_F16X3, NR_ERR_UNSUPPORTED,
             "training GEMMs: f16x3 softplus SDF nets only (SIREN / fp32 nets train on nr_gemm32)");
  return NR_OK;
}

int nr_sdf_op_info(const NrSdfDesc* d, int op, int64_t* offset, int* kb, int* nbo) {
  int rc = softplus_net(d);
  if (rc) return rc;
  NR_REQUIRE(offset && kb && nbo && op >= 0 && op <= kSdfOps, NR_ERR_ARG, "nr_sdf_op_info: bad argument");
  if (op == kSdfOps) {  // B8 = W8^T of the training pack
    *offset = 0; *kb = 18; *nbo = 16;
    return NR_OK;
  }
  const SdfLayout L = sdf_layout(*d);
  *offset = L.op_off[op]; *kb = kSdfKB[op]; *nbo = kSdfNBO[op];
  return NR_OK;
}

size_t nr_sdf_train_packed_bytes(const NrSdfDesc* d) {
  if (softplus_net(d)) return 0;
  return align256((size_t)8 * chunk_bytes_host(18) + 4) + 256;
}

// W8^T [256 x 257]: output rows = the 256 inputs of layer 8 (h7), input blocks [feature rows (16) ;
// sdf row (2 blocks, 1 valid)]; per-row vector W8[0, :] (g_7 of the nabla chain, nr_train.hip)
int nr_sdf_train_pack(const NrSdfDesc* d, const float* const* W, const float* const* b, void* packed, void* stream) {
  int rc = softplus_net(d);
  if (rc) return rc;
  NR_REQUIRE(W && b && packed && W[8], NR_ERR_ARG, "nr_sdf_train_pack: null argument");
  char* P = (char*)packed;
  float* wmax = (float*)(P + (size_t)8 * chunk_bytes_host(18));
  PackOp op = mkop(W[8], nullptr, 257, 256, 1, seg(16, 0, 256), none(), seg(16, 1, 256), seg(2, 0, 1), 1.0f,
                   NR_PREC_F16X3, wmax);
  op.aux = W[8];
  return launch_pack_op(op, P, (hipStream_t)stream);
}

static int train_radiance(const NrRadDesc* d) {
  int rc = check_rad_desc(d);
  if (rc) return rc;
  NR_REQUIRE(!d->siren && d->D == 4 && d->precision == NR_PREC_F16X3, NR_ERR_UNSUPPORTED,
             "training GEMMs: f16x3 ReLU radiance nets with D = 4 only");
  return NR_OK;
}

// training pack of a radiance net: head^T (KB 2), W3^T, W2^T, W1^T (16 x 16), W0^T (out 16 + kbs)
static void rad_train_layout(const RadLayout& L, int64_t (&off)[5], int (&kb)[5], int (&nbo)[5], int64_t& total) {
  const int KBs[5] = {2, 16, 16, 16, 16};
  const int NBOs[5] = {16, 16, 16, 16, 16 + L.kbs};
  int64_t o = 0;
  for (int i = 0; i < 5; ++i) {
    off[i] = o; kb[i] = KBs[i]; nbo[i] = NBOs[i];
    o += (int64_t)(NBOs[i] / 2) * chunk_bytes_host(KBs[i]);
  }
  total = o;
}

int nr_radiance_op_info(const NrRadDesc* d, int op, int64_t* offset, int* kb, int* nbo) {
  int rc = train_radiance(d);
  if (rc) return rc;
  NR_REQUIRE(offset && kb && nbo && op >= 0 && op <= 2 * d->D + 1, NR_ERR_ARG, "nr_radiance_op_info: bad argument");
  const RadLayout L = rad_layout(*d);
  if (op < d->D) {
    *offset = L.op_off[op]; *kb = op == 0 ? 16 + L.kbs : 16; *nbo = 16;
  } else if (op == d->D) {
    *offset = L.head_off; *kb = 0; *nbo = 0;
  } else {
    int64_t off[5], total;
    int kbs[5], nbos[5];
    rad_train_layout(L, off, kbs, nbos, total);
    const int i = op - d->D - 1;
    *offset = off[i]; *kb = kbs[i]; *nbo = nbos[i];
  }
  return NR_OK;
}

size_t nr_radiance_train_packed_bytes(const NrRadDesc* d) {
  if (train_radiance(d)) return 0;
  int64_t off[5], total;
  int kb[5], nbo[5];
  rad_train_layout(rad_layout(*d), off, kb, nbo, total);
  return align256((size_t)total + 5 * 4) + 256;
}

int nr_radiance_train_pack(const NrRadDesc* d, const float* const* W, const float* const* b, void* packed,
                           void* stream) {
  int rc = train_radiance(d);
  if (rc) return rc;
  NR_REQUIRE(W && b && packed, NR_ERR_ARG, "nr_radiance_train_pack: null argument");
  for (int l = 0; l <= d->D; ++l) NR_REQUIRE(W[l], NR_ERR_ARG, "nr_radiance_train_pack: null layer pointer");
  hipStream_t st = (hipStream_t)stream;
  const RadLayout L = rad_layout(*d);
  int64_t off[5], total;
  int kb[5], nbo[5];
  rad_train_layout(L, off, kb, nbo, total);
  char* P = (char*)packed;
  float* wmax = (float*)(P + total);
  const int ns = L.n_small, ld0 = ns + 256;
  PackOp ops[5];
  ops[0] = mkop(W[4], nullptr, 3, 256, 1, seg(16, 0, 256), none(), seg(2, 0, 3), none(), 1.0f, NR_PREC_F16X3, wmax);
  for (int i = 1; i <= 3; ++i)  // W3^T, W2^T, W1^T
    ops[i] = mkop(W[4 - i], nullptr, 256, 256, 1, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f,
                  NR_PREC_F16X3, wmax + i);
  ops[4] = mkop(W[0], nullptr, 256, ld0, 1, seg(16, ns, 256), seg(L.kbs, 0, ns), seg(16, 0, 256), none(), 1.0f,
                NR_PREC_F16X3, wmax + 4);
  char* dst[5];
  for (int i = 0; i < 5; ++i) dst[i] = P + off[i];
  if ((rc = launch_pack_ops(ops, dst, 5, st))) return rc;
  return NR_OK;
}

// Fold of the geometry-feature layer (base.py:255-256: no activation) into the radiance net's layer 0
// (base.py:382: a Linear over cat([x, embed_view(v), n, feature])): U = W0f W8[1:], bu = W0f b8[1:] + b0
static int check_fold(const NrSdfDesc* sd, const NrRadDesc* rd) {
  int rc = check_sdf_desc(sd);
  if (rc) return rc;
  if ((rc = check_rad_desc(rd))) return rc;
  NR_REQUIRE(fold_applies(*sd, *rd), NR_ERR_UNSUPPORTED,
             "NeuS fold: needs the f16x3 softplus SDF net and a f16x3 ReLU D=4 radiance net");
  return NR_OK;
}

size_t nr_neus_fold_packed_bytes(const NrSdfDesc* sd, const NrRadDesc* rd) {
  if (!sd || !rd || check_sdf_desc(sd) || check_rad_desc(rd) || !fold_applies(*sd, *rd)) return 0;
  return fold_layout(rad_layout(*rd)).total;
}

int nr_neus_fold_pack(const NrSdfDesc* sd, const NrRadDesc* rd, const float* W8, const float* b8, const float* W0,
                      const float* b0, void* packed, void* stream) {
  int rc = check_fold(sd, rd);
  if (rc) return rc;
  NR_REQUIRE(W8 && b8 && W0 && b0 && packed, NR_ERR_ARG, "nr_neus_fold_pack: null argument");
  hipStream_t st = (hipStream_t)stream;
  const RadLayout RL = rad_layout(*rd);
  const FoldLayout F = fold_layout(RL);
  char* P = (char*)packed;
  const int ns = RL.n_small, ld0 = ns + 256;
  float* U = (float*)(P + F.u_off);
  float* bu = U + 256 * 256;
  // exact fp32 products, fp64 sums, one rounding (nr_gemm32's default mode); b0 added last
  if ((rc = nr_gemm32(W0 + ns, ld0, W8 + 256, 256, 0, nullptr, U, 256, 256, 256, 256, 0, stream))) return rc;
  if ((rc = nr_gemm32(b8 + 1, 256, W0 + ns, ld0, 1, b0, bu, 256, 1, 256, 256, 0, stream))) return rc;
  float* wmax = (float*)(P + F.scale_off);
  float* bound = (float*)(P + F.bound_off);
  PackOp ops[2];
  ops[0] = mkop(U, bu, 256, 256, 0, seg(16, 0, 256), none(), seg(16, 0, 256), none(), 1.0f, NR_PREC_F16X3, wmax);
  ops[1] = mkop(W0, nullptr, 256, ld0, 0, seg(16, 0, 256), none(), seg(RL.kbs, 0, ns), none(), 1.0f, NR_PREC_F16X3,
                wmax + 1);
  char* dst[2] = {P + F.f8_off, P + F.r0_off};
  for (int i = 0; i < 2; ++i) ops[i].bound = bound + 2 * i;
  return launch_pack_ops(ops, dst, 2, st);
}

int nr_neus_fold_forward(const NrSdfDesc* sd, const void* sdf_packed, const NrRadDesc* rd, const void* rad_packed,
                         const void* fold_packed, const float* pts, const float* vdir, int64_t vdir_div,
                         const float* normals, int64_t P, float* u, float* sdf_out, float* rgb, void* stream) {
  int rc = check_fold(sd, rd);
  if (rc) return rc;
  NR_REQUIRE(sdf_packed && rad_packed && fold_packed && pts && (rd->no_view_dirs || (vdir && normals)) && u &&
                 sdf_out && rgb && vdir_div > 0 && P >= 0,
             NR_ERR_ARG, "nr_neus_fold_forward: bad argument");
  const RadLayout RL = rad_layout(*rd);
  const FoldLayout F = fold_layout(RL);
  const char* fp = (const char*)fold_packed;
  if ((rc = launch_sdf(sdf_layout(*sd), sdf_packed, pts, P, sdf_out, nullptr, u, sd->multires, nullptr, 0,
                       (hipStream_t)stream, nullptr, 0, fp + F.f8_off)))
    return rc;
  return launch_radiance(RL, rad_packed, pts, vdir, vdir_div, INT64_MAX, normals, u, P, rgb, rd->multires_view,
                         (hipStream_t)stream, nullptr, fp + F.r0_off);
}

int nr_sample_pdf(const float* bins, const float* weights, int64_t R, int L, const float* u, int64_t u_stride, int N,
                  float* out, void* stream) {
  NR_REQUIRE(bins && weights && u && out && L >= 2 && N >= 1 && u_stride >= 0, NR_ERR_ARG,
             "nr_sample_pdf: bad argument");
  if (R <= 0) return NR_OK;
  hipLaunchKernelGGL(sample_pdf_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bins,
                     weights, R, L, u, u_stride, N, out);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

}  // extern "C"
