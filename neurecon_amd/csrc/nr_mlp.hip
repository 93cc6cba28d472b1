// neurecon_amd — fused SDF / radiance MLP kernels for gfx950 (MI355X, CDNA4).
//
// Replaces ImplicitSurface.forward / forward_with_nablas (models/base.py:243-282) and
// RadianceNet.forward (models/base.py:372-391) of SuwoongHeo/neurecon.
//
// Design:
//  * Transposed GEMM formulation: activations are held as Xᵀ [features x points]; one wave owns a
//    tile of 16 points, a workgroup of 8 waves owns 128 points.  With v_mfma_f32_16x16x4_f32 the
//    accumulator of layer l (rows = output features, cols = points) is *directly* the B operand of
//    layer l+1: register r of 16-feature block b in lane-group g holds feature 16b+4g+r, which is
//    the k-index g of k-step (b,r).  No LDS round trip or shuffle between layers; the weight
//    packing (host side) applies the matching k permutation.
//  * Weights are streamed through LDS in chunks of 2 output blocks (32 output features x K) by
//    global_load_lds (LDS-DMA), double buffered, shared by the 8 waves.
//  * Softplus(beta=100) keeps exp(100 z) per element; the reverse pass (nablas) reloads it from a
//    per-wave scratch slab and applies torch's softplus_backward formula g*e/(e+1).
//  * Everything per point (embedding, nabla chain rule through sin/cos, sdf row dot product,
//    sigmoid head) is VALU work in the same kernel.
#include <algorithm>
#include <atomic>
#include <type_traits>
#include "nr_common.h"
#include "nr_mlp.h"
#include "nr_tgemm.h"

namespace nr {

using lds_ptr = __attribute__((address_space(3))) void*;

// ---------------------------------------------------------------------------------------------
// LDS weight stream: a ring of kRing chunk buffers filled by LDS-DMA (global_load_lds, 16 B/lane),
// issued kRing-1 = 2 chunks ahead of the chunk being computed
// ---------------------------------------------------------------------------------------------
// The DMA is issued from inline asm so that hipcc does not treat it as a pending LDS store
// (with the builtin it puts `s_waitcnt vmcnt(0)` in front of the next ds_read, i.e. every chunk
// would wait for the newest DMA).  Completion is counted by hand: at the end of chunk c, flip()
// waits until only the DMA instructions of chunk c+2 (issued last) may still be outstanding --
// vmcnt retires in issue order on gfx9 -- then barriers, so chunk c+1 has landed for all waves.
// Everything a chunk needs from global memory besides the weights (the softplus' slab of the
// reverse pass) also travels by LDS-DMA, so no compiler-visible load is ever waited on behind
// an in-flight weight DMA.
__device__ __forceinline__ void glds16(const char* gsrc, uint32_t lds_addr) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_addr)
      : "memory");
}

// LDS-DMA with a wave-uniform 64-bit base in SGPRs and a 32-bit per-lane offset: keeps address
// math out of the (full) VGPR file -- a spilled address would be reloaded with a vmcnt(0) that
// also waits for every in-flight weight DMA
__device__ __forceinline__ void glds16s(const char* sbase, uint32_t voff, uint32_t lds_addr) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_addr)
      : "memory");
}

// ... with M0 declared clobbered instead of saved and restored around every piece (the v3 kernel
// issues ~9 pieces per chunk per wave; the compiler re-materialises M0 where it needs it)
__device__ __forceinline__ void glds16m(const char* sbase, uint32_t voff, uint32_t lds_addr) {
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %1"
      :
      : "v"(voff), "s"(sbase), "s"(lds_addr)
      : "memory", "m0");
}

// a pointer every lane of the wave agrees on, forced into SGPRs
template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (T*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

// s_waitcnt vmcnt(n) for a runtime n (the immediate must be a constant)
__device__ __forceinline__ void wait_vmcnt(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
    case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
    case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
    case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); break;
    case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
    case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); break;
    case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
    case 21: asm volatile("s_waitcnt vmcnt(21)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(22)" ::: "memory"); break;  // callers stay <= 22
  }
}

__device__ __forceinline__ uint32_t lds_u32(const void* p) {
  return (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)p);
}

constexpr int kRing = 3;
constexpr int kSlabChunk = kWaves * 2 * 64 * 16;  // softplus' of 2 blocks for every wave: 16 KB

template <int CBMAX>
struct WStream {
  char* lds;   // kRing x CBMAX weight buffers
  char* slab;  // 2 x kSlabChunk staged softplus' values (reverse pass), or null
  int cur;     // ring slot of the chunk being computed
  int pend;    // DMA instructions of the newest issued chunk (this wave)
  int ecur;    // slab slot of the chunk being computed
  __device__ __forceinline__ static int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
  __device__ __forceinline__ int dma(const char* gsrc, int bytes, int slot) {
    const int wave = wave_id();
    const uint32_t voff = (threadIdx.x & 63) * 16;
    const char* g = uniform_ptr(gsrc);
    const uint32_t base = __builtin_amdgcn_readfirstlane(lds_u32(lds) + (uint32_t)(slot * CBMAX));
    int n = 0;
    for (int off = wave * 1024; off < bytes; off += kThreads * 16, ++n) glds16s(g + off, voff, base + off);
    return n;
  }
  // chunks 0 and 1 of the stream; returns once chunk 0 is in LDS for every wave
  __device__ __forceinline__ void start(const char* g0, int b0, const char* g1, int b1) {
    cur = 0;
    ecur = 0;
    dma(g0, b0, 0);
    pend = dma(g1, b1, 1);
    wait_vmcnt(pend);
    __syncthreads();
  }
  // the chunk two ahead of the current one: the last VMEM of a chunk
  __device__ __forceinline__ void issue(const char* gsrc, int bytes) { pend = dma(gsrc, bytes, (cur + 2) % kRing); }
  __device__ __forceinline__ void none() { pend = 0; }
  // softplus' blocks (b, b+1) of this wave's slab for the NEXT chunk (before issue())
  __device__ __forceinline__ void slab_next(const float4* e, int b) {
    const int wave = wave_id();
    const uint32_t voff = (threadIdx.x & 63) * 16;
    const char* g = (const char*)uniform_ptr(e + b * 64);
    const uint32_t base = __builtin_amdgcn_readfirstlane(lds_u32(slab) + (uint32_t)((ecur ^ 1) * kSlabChunk + wave * 2048));
    glds16s(g, voff, base);
    glds16s(g + 1024, voff, base + 1024);
  }
  // ... or for the CURRENT chunk, waiting for it (once per tile, before the first reverse op)
  __device__ __forceinline__ void slab_now(const float4* e, int b) {
    ecur ^= 1;
    slab_next(e, b);
    ecur ^= 1;
    wait_vmcnt(0);
  }
  __device__ __forceinline__ const float4* slab_cur() const {
    return (const float4*)(slab + ecur * kSlabChunk + wave_id() * 2048);
  }
  __device__ __forceinline__ const float4* buf() const { return (const float4*)(lds + cur * CBMAX); }
  __device__ __forceinline__ void flip() {
    wait_vmcnt(pend);  // everything older than the newest chunk's DMA has landed (this wave)
    __syncthreads();   // ... for every wave
    cur = (cur + 1) % kRing;
    ecur ^= 1;
  }
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 tof(float4 v) { return f32x4{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ float4 fromf(f32x4 v) { return make_float4(v[0], v[1], v[2], v[3]); }

// One chunk = 2 output blocks.  A layout in LDS: [obl(2)][b(KB)][lane(64)] float4 (r = .x.y.z.w)
// Software-pipelined one input block deep: the A fragments of block b+1 are read from LDS while
// block b's 8 MFMAs issue; sched_barrier stops hipcc from hoisting every LDS read of the chunk
// (which would cost ~128 VGPRs and force spills at 2 waves/SIMD).
template <int KBX, int KBE, int NE>
__device__ __forceinline__ void mma_chunk(const float4* __restrict__ A, const float4 (&X)[16], const float4 (&E)[NE],
                                          f32x4& acc0, f32x4& acc1, int lane) {
  constexpr int KB = KBX + KBE;
  float4 n0 = A[lane], n1 = A[KB * 64 + lane];
#pragma unroll
  for (int b = 0; b < KB; ++b) {
    const float4 a0 = n0, a1 = n1;
    if (b + 1 < KB) {
      n0 = A[(b + 1) * 64 + lane];
      n1 = A[(KB + b + 1) * 64 + lane];
    }
    const float4 x = b < KBX ? X[b < KBX ? b : 0] : E[b < KBX ? 0 : b - KBX];
    acc0 = mfma4(a0.x, x.x, acc0);
    acc1 = mfma4(a1.x, x.x, acc1);
    acc0 = mfma4(a0.y, x.y, acc0);
    acc1 = mfma4(a1.y, x.y, acc1);
    acc0 = mfma4(a0.z, x.z, acc0);
    acc1 = mfma4(a1.z, x.z, acc1);
    acc0 = mfma4(a0.w, x.w, acc0);
    acc1 = mfma4(a1.w, x.w, acc1);
    if (b + 1 < KB) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // next block's reads first
    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// rotate-in a pair of output blocks: after N/2 pushes Y[0..N-1] holds the outputs in order
template <int N>
__device__ __forceinline__ void push2(float4 (&Y)[16], float4 a, float4 b) {
#pragma unroll
  for (int i = 0; i + 2 < N; ++i) Y[i] = Y[i + 2];
  Y[N - 2] = a;
  Y[N - 1] = b;
}
// same over the concatenation [Y[0..N1-1], Z[0..N2-1]]
template <int N1, int N2>
__device__ __forceinline__ void push2cat(float4 (&Y)[16], float4 (&Z)[4], float4 a, float4 b) {
  constexpr int N = N1 + N2;
#pragma unroll
  for (int i = 0; i + 2 < N; ++i) {
    const float4 v = (i + 2 < N1) ? Y[i + 2] : Z[i + 2 - N1];
    if (i < N1) Y[i] = v; else Z[i - N1] = v;
  }
  if (N - 2 < N1) Y[N - 2] = a; else Z[N - 2 - N1] = a;
  if (N - 1 < N1) Y[N - 1] = b; else Z[N - 1 - N1] = b;
}

// ---------------------------------------------------------------------------------------------
// activations (torch CPU semantics, models/base.py:202, :361-363)
// ---------------------------------------------------------------------------------------------
// Softplus(beta=100, threshold=20): y = (100 z > 20) ? z : log1p(exp(100 z)) / 100.
// e = exp(100 z) is kept for the backward (softplus_backward: g * e / (e + 1)); +inf marks the
// linear branch (gradient passes through unchanged).
//  P = NR_PREC_FP32 : libm-accurate expf/log1pf and IEEE division, op order of the reference.
//  P = NR_PREC_F16X3: hardware v_exp_f32 / v_log_f32 / v_rcp_f32 (~1e-6 rel), for the fast mode.
template <int P>
__device__ __forceinline__ void softplus_fwd(float z, float& y, float& e) {
  const float t = fmul(z, 100.0f);
  const bool lin = t > 20.0f;
  if constexpr (P == NR_PREC_FP32) {
    const float ex = expf(t);
    y = lin ? z : fdiv(log1pf(ex), 100.0f);
    e = lin ? __builtin_inff() : ex;
  } else {
    const float ex = __builtin_amdgcn_exp2f(t * 1.44269504088896341f);
    y = lin ? z : __builtin_amdgcn_logf(1.0f + ex) * (0.693147180559945309f * 0.01f);
    e = lin ? __builtin_inff() : ex;
  }
}
template <int P>
__device__ __forceinline__ float softplus_bwd(float g, float e) {
  if constexpr (P == NR_PREC_FP32) return __builtin_isinf(e) ? g : fdiv(fmul(g, e), fadd(e, 1.0f));
  else return __builtin_isinf(e) ? g : g * e * __builtin_amdgcn_rcpf(e + 1.0f);
}

enum { ACT_NONE = 0, ACT_SOFTPLUS = 1, ACT_RELU = 2, ACT_SINE = 3 };

// SirenLayer (base.py:84-115): h = sin(w0 z), w0 = 30, the argument rounded as torch's w0 * x.
// The slab keeps cos(w0 z); autograd's backward is (g * cos(w0 z)) * w0 (SinBackward, then MulBackward)
constexpr float kSirenW0 = 30.0f;
__device__ __forceinline__ void sine_fwd(float z, float& y, float& e) {
  const float t = fmul(kSirenW0, z);
  y = sinf(t);
  e = cosf(t);
}
__device__ __forceinline__ float sine_bwd(float g, float e) { return fmul(fmul(g, e), kSirenW0); }
template <int P, int ACT>
__device__ __forceinline__ float act_bwd(float g, float e) {
  if constexpr (ACT == ACT_SINE) return sine_bwd(g, e);
  else return softplus_bwd<P>(g, e);
}

// chunk = [A: 2*KB KB][bias slot: 32 floats (2 output blocks), [32] = 1/weight-scale; 1 KB]
__host__ __device__ constexpr int chunk_bytes(int KB) { return (2 * KB + 1) * 1024; }
// ... without the bias slot: what a lean op (op4) fetches of each chunk
__host__ __device__ constexpr int weight_bytes(int KB) { return 2 * KB * 1024; }

// ---------------------------------------------------------------------------------------------
// split-fp16 x3 operands: v = (hi + lo) * 2^-k with hi = f16(v 2^k), lo = f16(v 2^k - hi).
// One power-of-two scale per point (column of the B operand) keeps |hi| < 2^13 and lo normal.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 mfma16h(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f16x8 as_h8(float4 v) { return __builtin_bit_cast(f16x8, v); }

__device__ __forceinline__ float amax4(float4 v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}
// max over the 4 lane groups of a point (lanes l, l^16, l^32, l^48) without ds_bpermute: no
// address VGPRs to keep live (they would be spilled and reloaded behind the in-flight DMA)
__device__ __forceinline__ float max4_groups(float m) {
  m = fmaxf(m, __uint_as_float(__builtin_amdgcn_ds_swizzle(__float_as_uint(m), 0x401F)));  // lane ^ 16
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));                              // lane ^ 32
}
// 2^(13 - e) with m = f 2^e, f in [0.5, 1): m * scale < 2^13
__device__ __forceinline__ float pow2_scale(float m) {
  if (!(m > 0.0f) || __builtin_isinf(m)) return 1.0f;
  return __builtin_ldexpf(1.0f, 13 - __builtin_amdgcn_frexp_expf(m));
}
__device__ __forceinline__ void split8(float4 lo4, float4 hi4, float sc, f16x8& h, f16x8& l) {
  const float v[8] = {lo4.x * sc, lo4.y * sc, lo4.z * sc, lo4.w * sc, hi4.x * sc, hi4.y * sc, hi4.z * sc, hi4.w * sc};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 hh = (_Float16)v[e];
    h[e] = hh;
    l[e] = (_Float16)(v[e] - (float)hh);
  }
}
// B operand of a layer whose input is [X[0..KBX) ; E[0..KBE)] (16-feature blocks, acc layout):
// k-step s pairs blocks 2s, 2s+1.  Returns 1/scale of this lane's point.
template <int KBX, int KBE, int NE>
__device__ __forceinline__ float make_b16(const float4 (&X)[16], const float4 (&E)[NE], f16x8 (&bh)[12],
                                          f16x8 (&bl)[12]) {
  constexpr int KB = KBX + KBE;
  static_assert(KB % 2 == 0 && KB <= 24, "bad block count");
  float m = 0.0f;
#pragma unroll
  for (int b = 0; b < KBX; ++b) m = fmaxf(m, amax4(X[b]));
#pragma unroll
  for (int b = 0; b < KBE; ++b) m = fmaxf(m, amax4(E[b]));
  m = max4_groups(m);
  const float sc = pow2_scale(m);
#pragma unroll
  for (int s = 0; s < KB / 2; ++s) {
    const int b0 = 2 * s, b1 = 2 * s + 1;
    const float4 v0 = b0 < KBX ? X[b0 < KBX ? b0 : 0] : E[b0 < KBX ? 0 : b0 - KBX];
    const float4 v1 = b1 < KBX ? X[b1 < KBX ? b1 : 0] : E[b1 < KBX ? 0 : b1 - KBX];
    split8(v0, v1, sc, bh[s], bl[s]);
    // opaque to the optimiser: otherwise hipcc keeps X live and re-splits it inside every chunk
    // of the layer (~200 VALU per chunk) to save the 8 extra VGPRs the halves need over X
    asm volatile("" : "+v"(bh[s]), "+v"(bl[s]));
  }
  return 1.0f / sc;
}
// A layout (f16x3): [obl(2)][s(NS)][hl(2)][lane(64)] x 16 B (8 halves).
// Software-pipelined one k-step deep (the 4 A fragments of step s+1 are read while step s's 6
// MFMAs issue); sched_barrier keeps hipcc from re-serialising each read behind an lgkmcnt(0).
template <int NS>
__device__ __forceinline__ void mma_chunk_h3(const float4* __restrict__ A, const f16x8 (&bh)[12],
                                             const f16x8 (&bl)[12], f32x4& acc0, f32x4& acc1, int lane) {
  f16x8 nh0 = as_h8(A[0 * 64 + lane]), nl0 = as_h8(A[1 * 64 + lane]);
  f16x8 nh1 = as_h8(A[(NS * 2) * 64 + lane]), nl1 = as_h8(A[(NS * 2 + 1) * 64 + lane]);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const f16x8 h0 = nh0, l0 = nl0, h1 = nh1, l1 = nl1;
    if (s + 1 < NS) {
      nh0 = as_h8(A[((s + 1) * 2) * 64 + lane]);
      nl0 = as_h8(A[((s + 1) * 2 + 1) * 64 + lane]);
      nh1 = as_h8(A[((NS + s + 1) * 2) * 64 + lane]);
      nl1 = as_h8(A[((NS + s + 1) * 2 + 1) * 64 + lane]);
    }
    acc0 = mfma16h(l0, bh[s], acc0);
    acc1 = mfma16h(l1, bh[s], acc1);
    acc0 = mfma16h(h0, bl[s], acc0);
    acc1 = mfma16h(h1, bl[s], acc1);
    acc0 = mfma16h(h0, bh[s], acc0);
    acc1 = mfma16h(h1, bh[s], acc1);
    // issue order: the next step's LDS reads first, then this step's MFMAs
    if (s + 1 < NS) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Forward GEMM layer: Y[0..NBO) = act(W · [X[0..KBX) ; E[0..KBE)] + bias).
// `op` chunks are consumed from the stream; `nxt` (chunks of nxt_bytes) is the op that follows.
template <int P, int KBX, int KBE, int NBO, int ACT, int NE, class WS>
__device__ __forceinline__ void gemm_fwd(WS& ws, const char* __restrict__ op, const char* nxt, int nxt_bytes,
                                         const float4 (&X)[16], const float4 (&E)[NE], float4 (&Y)[16],
                                         float4* __restrict__ e_out, float* __restrict__ feat_out, bool feat_ok,
                                         int lane) {
  constexpr int KB = KBX + KBE;
  constexpr int CB = chunk_bytes(KB);
  constexpr int NCH = NBO / 2;
  static_assert(NCH >= 2, "the 2-ahead stream needs >= 2 chunks per op");
  const int g = lane >> 4;
  f16x8 bh[12], bl[12];
  float xinv = 1.0f;
  if constexpr (P == NR_PREC_F16X3) xinv = make_b16<KBX, KBE, NE>(X, E, bh, bl);
  // global stores of chunk c are issued at the start of chunk c+1, *before* that chunk's DMA, so
  // flip()'s wait never stands behind a store younger than the weights it waits for
  float4 p0 = make_float4(0, 0, 0, 0), p1 = p0;
  int pc = -1;
  auto drain = [&]() {
    if (pc >= 0) {
      if constexpr (ACT == ACT_SOFTPLUS || ACT == ACT_SINE) {
        if (e_out) {  // streamed: non-temporal so the slab does not evict the weights from L2
          using gf4 = __attribute__((address_space(1))) f32x4;
          gf4* eb = (gf4*)uniform_ptr(e_out + (2 * pc) * 64);
          __builtin_nontemporal_store(tof(p0), eb + lane);
          __builtin_nontemporal_store(tof(p1), eb + 64 + lane);
        }
      } else {
        if (feat_out && feat_ok) {  // row-major [P][256] feature rows of that chunk
          *(float4*)(feat_out + (2 * pc) * 16 + g * 4) = p0;
          *(float4*)(feat_out + (2 * pc + 1) * 16 + g * 4) = p1;
        }
      }
    }
    pc = -1;
  };
#pragma unroll 1
  for (int c = 0; c < NCH; ++c) {
    drain();
    if (c + 2 < NCH) ws.issue(op + (c + 2) * CB, CB);
    else if (nxt) ws.issue(nxt + (c + 2 - NCH) * nxt_bytes, nxt_bytes);
    else ws.none();
    const float4* A = ws.buf();
    const f32x4 b0 = tof(A[2 * KB * 64 + g]), b1 = tof(A[2 * KB * 64 + 4 + g]);
    f32x4 acc0, acc1;
    if constexpr (P == NR_PREC_FP32) {
      acc0 = b0;
      acc1 = b1;
      mma_chunk<KBX, KBE, NE>(A, X, E, acc0, acc1, lane);
    } else {
      acc0 = f32x4{0, 0, 0, 0};
      acc1 = f32x4{0, 0, 0, 0};
      mma_chunk_h3<KB / 2>(A, bh, bl, acc0, acc1, lane);
      const float inv = xinv * A[2 * KB * 64 + 8].x;  // 1/(x scale * w scale), exact powers of two
      acc0 = acc0 * inv + b0;
      acc1 = acc1 * inv + b1;
    }
    float4 y0, y1;
    if constexpr (ACT == ACT_SOFTPLUS) {
      softplus_fwd<P>(acc0[0], y0.x, p0.x); softplus_fwd<P>(acc0[1], y0.y, p0.y);
      softplus_fwd<P>(acc0[2], y0.z, p0.z); softplus_fwd<P>(acc0[3], y0.w, p0.w);
      softplus_fwd<P>(acc1[0], y1.x, p1.x); softplus_fwd<P>(acc1[1], y1.y, p1.y);
      softplus_fwd<P>(acc1[2], y1.z, p1.z); softplus_fwd<P>(acc1[3], y1.w, p1.w);
      pc = c;
    } else if constexpr (ACT == ACT_SINE) {
      sine_fwd(acc0[0], y0.x, p0.x); sine_fwd(acc0[1], y0.y, p0.y);
      sine_fwd(acc0[2], y0.z, p0.z); sine_fwd(acc0[3], y0.w, p0.w);
      sine_fwd(acc1[0], y1.x, p1.x); sine_fwd(acc1[1], y1.y, p1.y);
      sine_fwd(acc1[2], y1.z, p1.z); sine_fwd(acc1[3], y1.w, p1.w);
      pc = c;
    } else if constexpr (ACT == ACT_RELU) {
      y0 = make_float4(fmaxf(acc0[0], 0.f), fmaxf(acc0[1], 0.f), fmaxf(acc0[2], 0.f), fmaxf(acc0[3], 0.f));
      y1 = make_float4(fmaxf(acc1[0], 0.f), fmaxf(acc1[1], 0.f), fmaxf(acc1[2], 0.f), fmaxf(acc1[3], 0.f));
    } else {
      y0 = fromf(acc0);
      y1 = fromf(acc1);
      p0 = y0;
      p1 = y1;
      pc = c;
    }
    push2<NBO>(Y, y0, y1);
    ws.flip();
  }
  drain();
}

// Backward GEMM layer: out = Wᵀ · G (no bias).  The first NBO1 output blocks are scaled by
// act'(z) of the previous layer (slab e_cur, staged into LDS one chunk ahead) and rotated
// into Y; the remaining NBO2 blocks are gradients w.r.t. the positional encoding and are handed to
// `emb(block, value)` as produced.  The last chunk stages e_next blocks 0,1 for the next op.
template <int P, int KBG, int NBO1, int NBO2, int ACTB = ACT_SOFTPLUS, class WS, class EmbFn>
__device__ __forceinline__ void gemm_bwd(WS& ws, const char* __restrict__ op, const char* nxt, int nxt_bytes,
                                         const float4 (&G)[16], float4 (&Y)[16], const float4* __restrict__ e_cur,
                                         const float4* __restrict__ e_next, int lane, EmbFn&& emb) {
  constexpr int NBO = NBO1 + NBO2;
  constexpr int NCH = NBO / 2;
  static_assert(NBO1 % 2 == 0 && NBO2 % 2 == 0, "output segments must be chunk aligned");
  static_assert(NCH >= 2, "the 2-ahead stream needs >= 2 chunks per op");
  constexpr int CB = chunk_bytes(KBG);
  const float4 dummy[4] = {};
  f16x8 bh[12], bl[12];
  float ginv = 1.0f;
  if constexpr (P == NR_PREC_F16X3) ginv = make_b16<KBG, 0, 4>(G, dummy, bh, bl);
#pragma unroll 1
  for (int c = 0; c < NCH; ++c) {
    const bool main = 2 * c < NBO1;
    if (2 * c + 2 < NBO1) {
      if (e_cur) ws.slab_next(e_cur, 2 * c + 2);
    } else if (c + 1 == NCH && e_next) {
      ws.slab_next(e_next, 0);
    }
    if (c + 2 < NCH) ws.issue(op + (c + 2) * CB, CB);
    else if (nxt) ws.issue(nxt + (c + 2 - NCH) * nxt_bytes, nxt_bytes);
    else ws.none();
    const float4* A = ws.buf();
    f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
    if constexpr (P == NR_PREC_FP32) {
      mma_chunk<KBG, 0, 4>(A, G, dummy, acc0, acc1, lane);
    } else {
      mma_chunk_h3<KBG / 2>(A, bh, bl, acc0, acc1, lane);
      const float inv = ginv * A[2 * KBG * 64 + 8].x;
      acc0 = acc0 * inv;
      acc1 = acc1 * inv;
    }
    float4 y0 = fromf(acc0), y1 = fromf(acc1);
    if (main) {
      if (e_cur) {
        const float4* eb = ws.slab_cur();
        const float4 e0 = eb[lane], e1 = eb[64 + lane];
        y0 = make_float4(act_bwd<P, ACTB>(y0.x, e0.x), act_bwd<P, ACTB>(y0.y, e0.y), act_bwd<P, ACTB>(y0.z, e0.z),
                         act_bwd<P, ACTB>(y0.w, e0.w));
        y1 = make_float4(act_bwd<P, ACTB>(y1.x, e1.x), act_bwd<P, ACTB>(y1.y, e1.y), act_bwd<P, ACTB>(y1.z, e1.z),
                         act_bwd<P, ACTB>(y1.w, e1.w));
      }
      if constexpr (NBO1 > 0) push2<NBO1>(Y, y0, y1);
    } else {
      emb(2 * c - NBO1, y0);
      emb(2 * c + 1 - NBO1, y1);
    }
    ws.flip();
  }
}

// ---------------------------------------------------------------------------------------------
// positional encoding (models/base.py:14-81): feature f of [x, sin(x), cos(x), sin(2x), ...]
// ---------------------------------------------------------------------------------------------
// noinline: the accurate sinf/cosf expansions are large; one call per feature keeps code and
// register pressure of the (once per tile) encoding small
__device__ __noinline__ float embed_feature(int f, float x0, float x1, float x2, int nfreq) {
  if (f < 3) return f == 0 ? x0 : (f == 1 ? x1 : x2);
  const int fp = f - 3;
  if (fp >= 6 * nfreq) return 0.0f;
  const int band = fp / 6, m = fp - band * 6, c = m % 3;
  const float xc = c == 0 ? x0 : (c == 1 ? x1 : x2);
  const float v = fmul(xc, (float)(1 << band));
  return m < 3 ? sinf(v) : cosf(v);
}
// d/dx of the embedding, applied to the gradient gf of feature f (autograd: Sin/CosBackward
// then MulBackward by freq), accumulated into n[c]
__device__ __noinline__ void embed_backward(int f, float gf, float x0, float x1, float x2, int nfreq, float& n0,
                                            float& n1, float& n2) {
  float contrib;
  int c;
  if (f < 3) {
    contrib = gf;
    c = f;
  } else {
    const int fp = f - 3;
    if (fp >= 6 * nfreq) return;
    const int band = fp / 6, m = fp - band * 6;
    c = m % 3;
    const float freq = (float)(1 << band);
    const float xc = c == 0 ? x0 : (c == 1 ? x1 : x2);
    const float v = fmul(xc, freq);
    contrib = m < 3 ? fmul(fmul(gf, cosf(v)), freq) : fmul(fmul(gf, -sinf(v)), freq);
  }
  if (c == 0) n0 = fadd(n0, contrib);
  else if (c == 1) n1 = fadd(n1, contrib);
  else n2 = fadd(n2, contrib);
}

__device__ __forceinline__ float wave_sum4(float v) {  // sum over the 4 lane-groups of a point
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// ---------------------------------------------------------------------------------------------
// positional encoding of sdf4_kernel's render launches (6 bands: the only SDF net the library admits)
// ---------------------------------------------------------------------------------------------
// A point's 64 operand rows sit in its four lanes (lane group g holds rows 16 b + 4 g + r), and one
// embed_feature / embed_backward call per row makes every lane run sinf and cosf 12 times for the 36
// values the point has.  Here each of the point's 18 arguments a = 3 band + c is evaluated once, sin
// and cos together, by lane group a & 3 in slot a >> 2 (5 calls per lane: 20 evaluations, the last two
// of arguments no row has), and a row's value comes from the lane that holds it (ds_bpermute: no LDS
// memory).  A launch with both passes evaluates them at the tile start and again at the tile end, as
// before.  The values are sinf / cosf of the same fp32 argument as in embed_feature / embed_backward,
// so they are theirs bit for bit.
constexpr int kEncSlots = 5, kEncBands = 6;
struct Enc4 {
  float s[kEncSlots], c[kEncSlots];  // sin, cos of this lane's arguments g + 4 slot
};
__device__ __noinline__ float2 embed_sincos(float v) { return make_float2(sinf(v), cosf(v)); }
__device__ __forceinline__ void enc_eval(Enc4& t, const float (&x)[3], int g) {
  float x0 = x[0], x1 = x[1], x2 = x[2];
  asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2));  // values in registers: selected below, not branched on
#pragma unroll
  for (int s = 0; s < kEncSlots; ++s) {
    // a = 18, 19 (band 6): evaluated, fetched by no row
    const uint32_t a = (uint32_t)g + 4u * s, band = (a * 11u) >> 5 /* a / 3, a < 22 */, c = a - 3u * band;
    float xc = c == 1u ? x1 : x0;
    xc = c == 2u ? x2 : xc;
    const float2 r = embed_sincos(fmul(xc, __uint_as_float(0x3f800000u + (band << 23))));
    t.s[s] = r.x;
    t.c[s] = r.y;
  }
}
// where row f's trig value is: lane group | slot << 2 | (cos ? 32 : 0), or 0xff for a row without one;
// deriv: the value of its derivative instead (cos for a sin row, sin for a cos row)
constexpr uint32_t enc_src(int f, bool deriv) {
  const int fp = f - 3;
  if (fp < 0 || fp >= 6 * kEncBands) return 0xffu;
  const int band = fp / 6, m = fp % 6, a = band * 3 + m % 3;
  return (uint32_t)((a & 3) | ((a >> 2) << 2) | (((m >= 3) != deriv) ? 32 : 0));
}
// what the chain rule needs of row f: coordinate | band << 2 | (cos row ? 32 : 0) | (raw coordinate ? 64 : 0),
// or 0xff for a row that is always zero
constexpr uint32_t enc_meta(int f) {
  if (f < 3) return (uint32_t)(f | 64);
  const int fp = f - 3;
  if (fp >= 6 * kEncBands) return 0xffu;
  const int band = fp / 6, m = fp % 6;
  return (uint32_t)((m % 3) | (band << 2) | (m >= 3 ? 32 : 0));
}
// the value of row F0 + 4 g from the lane that evaluated it (0 where the row has none); j = lane & 15
template <int F0, bool DERIV>
__device__ __forceinline__ float enc_pull(const Enc4& t, int g, int j) {
  constexpr uint32_t c0 = enc_src(F0, DERIV), c1 = enc_src(F0 + 4, DERIV), c2 = enc_src(F0 + 8, DERIV),
                     c3 = enc_src(F0 + 12, DERIV);
  constexpr uint32_t word = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
  const uint32_t code = (word >> (8 * g)) & 0xffu;
  const int addr = (int)((((code & 3u) << 4) | (uint32_t)j) << 2);
  float out = 0.0f;
#pragma unroll
  for (uint32_t id = 0; id < 16; ++id) {  // id = slot | (cos ? 8 : 0): only the ones some lane group asks for
    if ((c0 >> 2) != id && (c1 >> 2) != id && (c2 >> 2) != id && (c3 >> 2) != id) continue;
    const float src = (id & 8) ? t.c[id & 7] : t.s[id & 7];
    const float v = __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(src)));
    out = (code >> 2) == id ? v : out;
  }
  return out;
}
// rows 16 b + 4 g + r of the encoding, r = 0..3 (embed_feature's values)
template <int B>
__device__ __forceinline__ float4 enc_rows(const Enc4& t, const float (&x)[3], int g, int j) {
  if constexpr (16 * B + 3 >= 3 + 6 * kEncBands + 12) {  // no lane group has a row
    float z = 0.0f;  // made per tile: a constant would be hoisted out of the tile loop into 4 more registers
    asm volatile("" : "+v"(z));
    return make_float4(z, z, z, z);
  }
  float v[4];
  v[0] = enc_pull<16 * B + 0, false>(t, g, j);
  v[1] = enc_pull<16 * B + 1, false>(t, g, j);
  v[2] = enc_pull<16 * B + 2, false>(t, g, j);
  v[3] = enc_pull<16 * B + 3, false>(t, g, j);
  if constexpr (B == 0) {  // rows 0..2: the coordinates themselves
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r] = g == 0 ? x[r] : v[r];
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}
// embed_backward for row F0 + 4 g: the same fmul / fadd on the same values, into the same n
template <int F0>
__device__ __forceinline__ void enc_row_bwd(const Enc4& t, float gf, int g, int j, float& n0, float& n1,
                                            float& n2) {
  constexpr uint32_t m0 = enc_meta(F0), m1 = enc_meta(F0 + 4), m2 = enc_meta(F0 + 8), m3 = enc_meta(F0 + 12);
  if constexpr (m0 == 0xffu && m1 == 0xffu && m2 == 0xffu && m3 == 0xffu) return;
  constexpr uint32_t word = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
  const uint32_t meta = (word >> (8 * g)) & 0xffu;
  // d cos = -sin: the cos rows' bit 5 becomes the sign bit
  const float tv = __uint_as_float(__float_as_uint(enc_pull<F0, true>(t, g, j)) ^ ((meta & 32u) << 26));
  const float freq = __uint_as_float(0x3f800000u + (((meta >> 2) & 7u) << 23));
  const float contrib = (meta & 64u) ? gf : fmul(fmul(gf, tv), freq);
  // selects, not conditional stores (those get merged into one store through a selected pointer, which
  // puts n0..n2 into scratch memory); a row that is always zero has c = 3 and adds to none
  const uint32_t c = meta & 3u;
  const float s0 = fadd(n0, contrib), s1 = fadd(n1, contrib), s2 = fadd(n2, contrib);
  n0 = c == 0u ? s0 : n0;
  n1 = c == 1u ? s1 : n1;
  n2 = c == 2u ? s2 : n2;
}

// =============================================================================================
// SDF kernel
// =============================================================================================
struct SdfKArgs {
  const char* packed;
  SdfLayout L;
  const float* pts;
  int64_t P;
  float* sdf;
  float* nabla;
  float* feature;
  float4* scratch;  // [grid*8 waves][8 layers][16 blocks][64 lanes] float4
  int nfreq;
  const int* P_dev;  // optional device-side point count (x P_mult), bounded by P
  int P_mult;
  float4* slabs;      // deferred nablas: per 16-point tile of the launch, kSlabColBytes (nr_mlp.h layout)
  const int* tiles;   // STAGE 2: 16-point tiles to run the reverse pass on
  const int* n_tiles; //   ... and their count (device)
  const char* f8_alt; // sdf4_kernel: a packed op to run in F8's place (the NeuS fold's F8', nr_neus_fold_pack), or null
};
// ... of the sdf4_kernel instances that can claim their tiles (kSdfClaim): the others keep SdfKArgs, and with
// it their kernel arguments' layout and their instructions
struct SdfKArgsC : SdfKArgs {
  int* claim;  // tile claim counter (nr_mlp.h), or null
};

template <int P, bool NABLA>
__global__ __launch_bounds__(kThreads) void sdf_kernel(SdfKArgs a) {
  constexpr int CB = chunk_bytes(18);  // largest SDF op chunk (F4: 14 + 4 input blocks)
  __shared__ __attribute__((aligned(16))) char smem[kRing * CB + (NABLA ? 2 * kSlabChunk : 0)];
  WStream<CB> ws{smem, NABLA ? smem + kRing * CB : nullptr, 0, 0, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const SdfLayout& L = a.L;
  const char* W = a.packed;
  auto OP = [&](int i) { return W + L.op_off[i]; };
  auto OPB = [&](int i) { return (int)L.op_bytes[i]; };
  const float* w8 = (const float*)(W + L.w8row0_off);
  const float b8 = *(const float*)(W + L.misc_off);
  float4* escr = uniform_ptr(a.scratch + (size_t)(blockIdx.x * kWaves + wave) * (8 * 16 * 64));
  const bool want_feat = a.feature != nullptr;

  ws.start(OP(F0), OPB(F0), OP(F0) + OPB(F0), OPB(F0));

  const int64_t Pn = a.P_dev ? min(a.P, (int64_t)(*a.P_dev) * a.P_mult) : a.P;
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < Pn; base += (int64_t)gridDim.x * kPointsPerWG) {
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < Pn;
    const int64_t p = base + wave * kTile + j;
    const bool valid = p < Pn;
    const int64_t pc = valid ? p : Pn - 1;
    const float x0 = a.pts[pc * 3 + 0], x1 = a.pts[pc * 3 + 1], x2 = a.pts[pc * 3 + 2];

    float4 E[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int f = 16 * b + 4 * g;
      E[b] = make_float4(embed_feature(f + 0, x0, x1, x2, a.nfreq), embed_feature(f + 1, x0, x1, x2, a.nfreq),
                         embed_feature(f + 2, x0, x1, x2, a.nfreq), embed_feature(f + 3, x0, x1, x2, a.nfreq));
    }
    float4 X[16], Y[16];
    float4* e_l[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) e_l[l] = NABLA ? escr + l * 16 * 64 : nullptr;

    // ---- forward (base.py:243-257) -----------------------------------------------------------
    gemm_fwd<P, 0, 4, 16, ACT_SOFTPLUS>(ws, OP(F0), OP(F1), OPB(F1), X, E, Y, e_l[0], nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_SOFTPLUS>(ws, OP(F1), OP(F2), OPB(F2), Y, E, X, e_l[1], nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_SOFTPLUS>(ws, OP(F2), OP(F3), OPB(F3), X, E, Y, e_l[2], nullptr, false, lane);
    gemm_fwd<P, 16, 0, 14, ACT_SOFTPLUS>(ws, OP(F3), OP(F4), OPB(F4), Y, E, X, e_l[3], nullptr, false, lane);
    gemm_fwd<P, 14, 4, 16, ACT_SOFTPLUS>(ws, OP(F4), OP(F5), OPB(F5), X, E, Y, e_l[4], nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_SOFTPLUS>(ws, OP(F5), OP(F6), OPB(F6), Y, E, X, e_l[5], nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_SOFTPLUS>(ws, OP(F6), OP(F7), OPB(F7), X, E, Y, e_l[6], nullptr, false, lane);
    {
      const char* n = want_feat ? OP(F8) : (NABLA ? OP(B7) : (has_next ? OP(F0) : nullptr));
      const int nb = want_feat ? OPB(F8) : (NABLA ? OPB(B7) : OPB(F0));
      gemm_fwd<P, 16, 0, 16, ACT_SOFTPLUS>(ws, OP(F7), n, nb, Y, E, X, e_l[7], nullptr, false, lane);
    }
    // ---- last layer, row 0 = sdf (VALU dot product) ---------------------------------------------
    float part = 0.0f;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const float4 w = *(const float4*)(w8 + 16 * b + 4 * g);
      part = fmaf(X[b].x, w.x, part);
      part = fmaf(X[b].y, w.y, part);
      part = fmaf(X[b].z, w.z, part);
      part = fmaf(X[b].w, w.w, part);
    }
    const float sdf = wave_sum4(part) + b8;
    if (valid && g == 0) a.sdf[p] = sdf;
    // ---- geometry feature rows 1..256 -------------------------------------------------------------
    if (want_feat) {
      const char* n = NABLA ? OP(B7) : (has_next ? OP(F0) : nullptr);
      const int nb = NABLA ? OPB(B7) : OPB(F0);
      gemm_fwd<P, 16, 0, 16, ACT_NONE>(ws, OP(F8), n, nb, X, E, Y, nullptr, a.feature + pc * 256, valid,
                                    lane);
    }
    if constexpr (NABLA) {
      // ---- reverse pass (autograd.grad of sdf w.r.t. x, base.py:265-282) ---------------------------
      // d sdf / d h7 = W8[0,:], scaled by softplus'(z7); h7 (X) is dead now and holds the gradient
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const float4 w = *(const float4*)(w8 + 16 * b + 4 * g);
        const float4 e = e_l[7][b * 64 + lane];
        X[b] = make_float4(softplus_bwd<P>(w.x, e.x), softplus_bwd<P>(w.y, e.y), softplus_bwd<P>(w.z, e.z),
                           softplus_bwd<P>(w.w, e.w));
      }
      // gradients w.r.t. the positional encoding (skip layer + first layer) are parked in the
      // (already consumed) layer-7 slab and folded into the nabla after the GEMM chain
      float4* park = e_l[7];
      auto emb_skip = [&](int eb, float4 gv) { park[eb * 64 + lane] = gv; };
      auto emb_first = [&](int eb, float4 gv) { park[(4 + eb) * 64 + lane] = gv; };
      auto noemb = [](int, float4) {};
      ws.slab_now(e_l[6], 0);  // softplus'(z6) blocks 0,1 for B7's first chunk
      gemm_bwd<P, 16, 16, 0>(ws, OP(B7), OP(B6), OPB(B6), X, Y, e_l[6], e_l[5], lane, noemb);
      gemm_bwd<P, 16, 16, 0>(ws, OP(B6), OP(B5), OPB(B5), Y, X, e_l[5], e_l[4], lane, noemb);
      gemm_bwd<P, 16, 16, 0>(ws, OP(B5), OP(B4), OPB(B4), X, Y, e_l[4], e_l[3], lane, noemb);
      // skip layer: rows 0..216 -> h3 (scaled by softplus'(z3)), rows 217..255 -> embedding
      gemm_bwd<P, 16, 14, 4>(ws, OP(B4), OP(B3), OPB(B3), Y, X, e_l[3], e_l[2], lane, emb_skip);
      gemm_bwd<P, 14, 16, 0>(ws, OP(B3), OP(B2), OPB(B2), X, Y, e_l[2], e_l[1], lane, noemb);
      gemm_bwd<P, 16, 16, 0>(ws, OP(B2), OP(B1), OPB(B1), Y, X, e_l[1], e_l[0], lane, noemb);
      gemm_bwd<P, 16, 16, 0>(ws, OP(B1), OP(B0), OPB(B0), X, Y, e_l[0], nullptr, lane, noemb);
      gemm_bwd<P, 16, 0, 4>(ws, OP(B0), has_next ? OP(F0) : nullptr, OPB(F0), Y, X, nullptr, nullptr, lane,
                            emb_first);
      // chain rule through the positional encoding (autograd sums both uses of embed(x))
      float n0 = 0.f, n1 = 0.f, n2 = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float4 u = park[b * 64 + lane], v = park[(4 + b) * 64 + lane];
        const int f = 16 * b + 4 * g;
        embed_backward(f + 0, fadd(v.x, u.x), x0, x1, x2, a.nfreq, n0, n1, n2);
        embed_backward(f + 1, fadd(v.y, u.y), x0, x1, x2, a.nfreq, n0, n1, n2);
        embed_backward(f + 2, fadd(v.z, u.z), x0, x1, x2, a.nfreq, n0, n1, n2);
        embed_backward(f + 3, fadd(v.w, u.w), x0, x1, x2, a.nfreq, n0, n1, n2);
      }
      n0 = wave_sum4(n0);
      n1 = wave_sum4(n1);
      n2 = wave_sum4(n2);
      if (valid && g == 0) {
        a.nabla[p * 3 + 0] = n0;
        a.nabla[p * 3 + 1] = n1;
        a.nabla[p * 3 + 2] = n2;
      }
    }
  }
  wait_vmcnt(0);  // a block without tiles still has the prologue's second chunk in flight
}

// =============================================================================================
// f16x3 operand helpers of the v3 SDF pipeline (sdf4_kernel, below)
// A wave of sdf4_kernel owns kNC = 1 16-point MFMA column: 8 waves of 16 points, two waves per SIMD
// with up to 256 registers each, every operand in VGPRs (no AGPR moves); the two waves of a SIMD hide
// each other's DMA / LDS / barrier stalls.  Measured on config (b): ~5 % faster than 4 waves of 32
// points (one per SIMD, B operands in AGPRs, each weight fragment feeding two columns).
// =============================================================================================
// What changes against sdf_kernel<F16X3> (which stays the reference design for the radiance and
// NeRF++ kernels):
//  * The B operand of op l+1 is split into f16 hi/lo fragments by op l's epilogue, one k-step per
//    chunk (chunk c of op l produces exactly k-step c of op l+1), instead of in one burst of
//    ~300 VALU per layer in which every wave of the workgroup idles its matrix core.  The per-point
//    power-of-two scale this needs is fixed *before* op l runs, from a bound on its outputs:
//    |out| <= R_l * max|in| + B_l (R_l = max row L1 norm of the op's effective matrix, B_l = max
//    |bias|, both computed at pack time; softplus(z) <= max(z, 0) + ln2/100; the backward factor
//    softplus' <= 1).  The scale puts the bound at 2^14 < f16 max, so hi never overflows, and the
//    bound is loose by ~10-50x in practice, leaving the outputs near 2^9..2^10 where hi + lo still
//    carry 22 significant bits (lo turns subnormal only 2^-17 below the bound).
//  * No fp32 copy of the activations is kept, chunk loops are fully unrolled (no register
//    rotation), and every DMA count is a compile-time constant.
//  * The reverse pass stores softplus'(z) = sigmoid(100 z) itself (1 on torch's linear branch),
//    so the backward epilogue is one multiply.
typedef float f2v __attribute__((ext_vector_type(2)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t cvt_pk_h(float a, float b) {  // v_cvt_pk_f16_f32 (RNE)
  const h2v h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(uint32_t, h);
}
// 8 values of one k-step (block 2s: a, block 2s+1: b), scaled by sc, into f16 hi / lo fragments
__device__ __forceinline__ void split8s(float4 a, float4 b, float sc, f16x8& h, f16x8& l) {
  const f2v s2 = {sc, sc};
  const f2v v[4] = {f2v{a.x, a.y} * s2, f2v{a.z, a.w} * s2, f2v{b.x, b.y} * s2, f2v{b.z, b.w} * s2};
  uint32_t hw[4], lw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t hh = cvt_pk_h(v[i].x, v[i].y);
    asm volatile("" : "+v"(hh));  // widen the packed halves back (not a second pair of converts)
    const h2v hv = __builtin_bit_cast(h2v, hh);
    const f2v r = v[i] - f2v{(float)hv.x, (float)hv.y};
    hw[i] = hh;
    lw[i] = cvt_pk_h(r.x, r.y);
  }
  h = __builtin_bit_cast(f16x8, make_uint4(hw[0], hw[1], hw[2], hw[3]));
  l = __builtin_bit_cast(f16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
}
// ... with both halves from v_fma_mix, written straight into the packed f16 pairs: hi = f16(v*sc)
// (one rounding of the exact product), lo = f16(v*sc - hi); no packed-fp32 multiply (v_pk_mul_f32
// issued beside MFMAs costs ~22 cycles more than scalar VALU, MI355X_MICROARCH.md)
__device__ __forceinline__ void split8a(float4 a, float4 b, float sc, f16x8& h, f16x8& l) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t hw[4], lw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t hh;
    asm volatile("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hh) : "v"(v[2 * i]), "v"(sc));
    asm volatile("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hh) : "v"(v[2 * i + 1]), "v"(sc));
    uint32_t lo;
    asm volatile("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(v[2 * i]), "v"(sc), "v"(hh));
    asm volatile("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
                 : "+v"(lo)
                 : "v"(v[2 * i + 1]), "v"(sc), "v"(hh));
    hw[i] = hh;
    lw[i] = lo;
  }
  h = __builtin_bit_cast(f16x8, make_uint4(hw[0], hw[1], hw[2], hw[3]));
  l = __builtin_bit_cast(f16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
}
__device__ __forceinline__ float max3abs(float m, float a, float b) {
  return __builtin_fmaxf(m, __builtin_fmaxf(fabsf(a), fabsf(b)));  // -> v_max3_f32 with |.| modifiers
}
__device__ __forceinline__ float amax8(float m, float4 a, float4 b) {
  m = max3abs(m, a.x, a.y);
  m = max3abs(m, a.z, a.w);
  m = max3abs(m, b.x, b.y);
  return max3abs(m, b.z, b.w);
}
// power-of-two scale putting a bound M at < 2^14 (1 for M = 0, inf or NaN)
__device__ __forceinline__ float bound_scale(float M) {
  if (!(M > 0.0f) || __builtin_isinf(M)) return 1.0f;
  return __builtin_ldexpf(1.0f, 14 - __builtin_amdgcn_frexp_expf(M));
}
// softplus(beta=100, threshold=20) (base.py:202) and its derivative sigmoid(100 z) (1 on the linear
// branch, as torch's softplus_backward passes the gradient through there)
template <bool DERIV>
__device__ __forceinline__ void softplus3(float z, float& y, float& s) {
  const float t = z * 100.0f;
  const bool lin = t > 20.0f;
  const float ex = __builtin_amdgcn_exp2f(t * 1.44269504088896341f);
  const float u = 1.0f + ex;
  const float yy = __builtin_amdgcn_logf(u) * (0.693147180559945309f * 0.01f);
  y = lin ? z : yy;
  if constexpr (DERIV) s = lin ? 1.0f : ex * __builtin_amdgcn_rcpf(u);
}
// the same on a pair with 100 log2(e) folded into one multiply (the linear-branch test t > 20
// becomes t log2(e) > 20 log2(e); differs from softplus3 by rounding only).  Scalar fp32 on purpose:
// this runs beside MFMAs, where packed fp32 VALU costs ~22 extra cycles (MI355X_MICROARCH.md)
__device__ __forceinline__ void softplus1(float z, float& y, float& s) {
  const float t = z * 144.269504088896341f;
  const float ex = __builtin_amdgcn_exp2f(t);
  const float u = ex + 1.0f;
  const bool lin = t > 28.8539008f;
  y = lin ? z : __builtin_amdgcn_logf(u) * (0.693147180559945309f * 0.01f);
  s = lin ? 1.0f : ex * __builtin_amdgcn_rcpf(u);
}
template <bool DERIV>
__device__ __forceinline__ void softplus_pk(float z0, float z1, float& y0, float& y1, float& s0, float& s1) {
  float d0, d1;
  softplus1(z0, y0, d0);
  softplus1(z1, y1, d1);
  if constexpr (DERIV) {
    s0 = d0;
    s1 = d1;
  }
}
// a * m + b per component as scalar FMAs (nr_mlp.hip is built without SLP vectorisation, so these
// stay v_fma_f32: packed fp32 beside MFMAs is an anti-lever, MI355X_MICROARCH.md)
__device__ __forceinline__ float4 fma4s(f32x4 a, float m, float4 b) {
  return make_float4(__builtin_fmaf(a[0], m, b.x), __builtin_fmaf(a[1], m, b.y), __builtin_fmaf(a[2], m, b.z),
                     __builtin_fmaf(a[3], m, b.w));
}

using gf4 = __attribute__((address_space(1))) f32x4;

// =============================================================================================
// f16x3 SDF pipeline v3 (sdf4_kernel): kNC 16-point columns per wave, 128-point tile
// =============================================================================================
// * 8 waves x 16 points (two per SIMD, 256 registers each): the B operands of the op being computed
//   AND of the op being produced stay in registers.
// * Chunk c's epilogue (bias, activation, slab I/O, per-chunk operand split) is issued in the same
//   basic block as chunk c+1's MFMAs, so the wave's VALU work fills the matrix core's issue gaps.
// * The operand split uses per-point power-of-two scales fixed before the op runs, from a bound on
//   its outputs (see the operand-helper notes above: split8a / bound_scale).
constexpr int kNC = 1;            // 16-point MFMA columns per wave (two waves per SIMD)
constexpr int kW4 = 8 / kNC;      // waves per workgroup: the tile stays 128 points
constexpr int kT4 = 64 * kW4;
constexpr int kWPE = kW4 / 4;     // waves per SIMD
// one chunk's slab codes of one wave in LDS: 2 blocks x kNC columns x 64 lanes x 16 B (the LDS-DMA of
// global_load_lds_dwordx3 lands lane l's 12 B at l x 16, the 4th dword untouched: tools/probes/ldsdma_x3)
constexpr int kSlabW = 2 * kNC * 1024;
constexpr int kSlab4 = kW4 * kSlabW;        // ... of the workgroup: 16 KB
constexpr int kLoad = 8;                    // waves that issue the weight stream (the last kLoad)
static_assert(kLoad >= 1 && kLoad <= kW4, "loader waves");

// Deferred stores of one chunk (up to 4 x 16 B per lane), issued at the start of the next chunk
// before its weight DMA, so flip()'s counted wait never stands behind a store younger than the
// weights it waits for.  Wave-uniform base (SGPR) + per-lane 32-bit float4 offsets.
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
struct Pend4 {
  float4* base;  // null: nothing pending
  uint32_t o[4];  // float4 index, or with b96 a byte offset
  float4 v[4];    // with b96: the 3 dwords in .x .y .z (bit patterns)
  int n;
  bool nt;
  bool b96;       // 12-byte stores (24-bit slab codes)
  // global_store_dwordx4 with an SGPR base and a 32-bit VGPR byte offset (saddr form), from asm:
  // compiler-built 64-bit per-lane addresses get hoisted out of the tile loop and spilled
  __device__ __forceinline__ int flush() {
    int issued = 0;
    if (base) {
      issued = n;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < n) {
          // s_nop: the store-data hazard (a VALU may not overwrite a >8-byte store's data VGPRs in
          // the next cycle) is not tracked through inline asm
          if (b96) {
            const uint32_t off = o[i];
            const u32x3 d = {__float_as_uint(v[i].x), __float_as_uint(v[i].y), __float_as_uint(v[i].z)};
            if (nt) asm volatile("global_store_dwordx3 %0, %1, %2 nt\n\ts_nop 1" : : "v"(off), "v"(d), "s"(base) : "memory");
            else asm volatile("global_store_dwordx3 %0, %1, %2\n\ts_nop 1" : : "v"(off), "v"(d), "s"(base) : "memory");
          } else {
            const uint32_t off = o[i] * 16u;
            const f32x4 d = tof(v[i]);
            if (nt) asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" : : "v"(off), "v"(d), "s"(base) : "memory");
            else asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(off), "v"(d), "s"(base) : "memory");
          }
        }
      }
      base = nullptr;
    }
    return issued;
  }
  __device__ __forceinline__ void put(float4* b, int cnt, bool nontemporal, bool bytes96 = false) {
    base = b;
    n = cnt;
    nt = nontemporal;
    b96 = bytes96;
  }
};

constexpr int kSlabRing = 3;  // softplus' slabs in LDS: one being read, one landing, one being staged
constexpr int kFwdRing = 4;   // weight-ring slots of the forward-only sdf4_kernel launches
constexpr int kTabBytes = 8 * 512;  // one op's bias table: 8 chunks x 512 B (WStream4::dma_tab)
// cache policy of the forward softplus slab stores (read back by the reverse pass of the same tile)
constexpr bool kSlabNT = true;
// ... of the geometry-feature and d sdf / d z7 stores
constexpr bool kFeatNT = false;

// RING: weight-ring slots, issued RING - 1 chunks ahead of the chunk being computed.  3 wherever the
// slab ring shares the LDS (reverse passes); 4 in the forward-only launches, whose LDS holds the
// weight ring alone (a 37 KB chunk x 4 = 148 KB): three chunks in flight instead of two against the
// L2 latency of the stream
// NW: waves of the workgroup (kW4; 4 in the narrow forward-only launches, sdf4_kernel), every one of
// them a loader when NW != kW4
template <int CBMAX, int RING = 3, int NW = kW4>
struct WStream4 {
  static_assert(RING == 3 || RING == 4, "weight ring depth");
  static constexpr int kRingN = RING;
  static constexpr int kLd = NW == kW4 ? kLoad : NW;  // loader waves
  char* lds;
  char* slab;  // kSlabRing x kSlab4
  int cur;     // ring slot of the chunk being computed
  int es;      // slab slot the next stage_slab() writes
  int er;      // slab slot the next consumed chunk's epilogue reads
  int prev;    // RING 4: VMEM instructions this wave issued in the previous chunk iteration
  char* tab;   // bias table (op4's kTab mode): 2 buffers x kTabBytes, or null
  int tcur;    // table buffer of the op being computed
  __device__ __forceinline__ static int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
  __device__ __forceinline__ static int next3(int i) { return i == 2 ? 0 : i + 1; }
  __device__ __forceinline__ static int nextr(int i) { return i == RING - 1 ? 0 : i + 1; }
  // the slot chunk c + RING - 1 goes into: the one chunk c - 1 left (every wave is past it)
  __device__ __forceinline__ int ahead_slot() const { return cur == 0 ? RING - 1 : cur - 1; }
  // BYTES/1 KB pieces; every loader wave (the last kLd of the workgroup) issues ceil(pieces/kLd)
  // (a wave past the end repeats the last piece: identical bytes to the same LDS address) so the
  // count is one constant in every loader wave
  template <int BYTES>
  __device__ __forceinline__ static constexpr int pieces() { return (BYTES / 1024 + kLd - 1) / kLd; }
  __device__ __forceinline__ static int loader() { return wave_id() - (NW - kLd); }  // < 0: no DMA
  template <int BYTES>
  __device__ __forceinline__ static int npieces() { return loader() >= 0 ? pieces<BYTES>() : 0; }
  // Each wave moves a contiguous run of NPW pieces (the last wave's run is shifted back to end at
  // the chunk's end; overlapping pieces are identical bytes to the same LDS address), up to 4 per
  // M0 setting: the instruction offset steps the global and the LDS address together.
  template <int BYTES>
  __device__ __forceinline__ void dma(const char* gsrc, int slot) {
    constexpr int NB = BYTES / 1024, NPW = pieces<BYTES>();
    const int wave = loader();
    if (wave < 0) return;
    const uint32_t voff = (threadIdx.x & 63) * 16;
    const int first = __builtin_amdgcn_readfirstlane(min(wave * NPW, NB - NPW));
    const char* g = uniform_ptr(gsrc) + first * 1024;
    const uint32_t base =
        __builtin_amdgcn_readfirstlane(lds_u32(lds) + (uint32_t)(slot * CBMAX) + (uint32_t)(first * 1024));
#pragma unroll
    for (int j = 0; j < NPW; j += 4) {
      const char* gj = g + j * 1024;
      const uint32_t mj = base + j * 1024;
      if (NPW - j >= 4)
        asm volatile(
            "s_mov_b32 m0, %2\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %0, %1\n\t"
            "global_load_lds_dwordx4 %0, %1 offset:1024\n\t"
            "global_load_lds_dwordx4 %0, %1 offset:2048\n\t"
            "global_load_lds_dwordx4 %0, %1 offset:3072"
            :
            : "v"(voff), "s"(gj), "s"(mj)
            : "memory", "m0");
      else if (NPW - j == 3)
        asm volatile(
            "s_mov_b32 m0, %2\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %0, %1\n\t"
            "global_load_lds_dwordx4 %0, %1 offset:1024\n\t"
            "global_load_lds_dwordx4 %0, %1 offset:2048"
            :
            : "v"(voff), "s"(gj), "s"(mj)
            : "memory", "m0");
      else if (NPW - j == 2)
        asm volatile(
            "s_mov_b32 m0, %2\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %0, %1\n\t"
            "global_load_lds_dwordx4 %0, %1 offset:1024"
            :
            : "v"(voff), "s"(gj), "s"(mj)
            : "memory", "m0");
      else
        glds16m(gj, voff, mj);
    }
  }
  template <int B0, int B1>
  __device__ __forceinline__ void start(const char* g0, const char* g1) {
    static_assert(RING == 3, "start: the first RING - 1 chunks");
    cur = 0;
    es = 0;
    er = 0;
    prev = 0;
    dma<B0>(g0, 0);
    dma<B1>(g1, 1);
    wait_vmcnt(npieces<B1>());
    __syncthreads();
  }
  // The bias table of one op: the first 512 B (float4 0..31: bias, scalars, aux, TS bias) of the bias slot
  // of each of its chunks, entry c at c x 512.  One instruction moves two entries: lanes 0-31 read chunk
  // 2p's slot, lanes 32-63 chunk 2p+1's (per-lane source, lane-linear destination).  Every loader wave
  // issues one: wave w pair w & 3 (waves 4-7: identical bytes to the same address), 8 entries in all (a
  // 7-chunk op's last entry is the following op's first bytes, inside the pack and never read).
  // gop: the op's first chunk, CBN its chunk stride.
  template <int CBN>
  __device__ __forceinline__ void dma_tab(const char* gop, int buf) {
    const int wave = loader();
    if (wave < 0) return;
    const uint32_t l = threadIdx.x & 63;
    const uint32_t voff = (l & 31) * 16 + (l >> 5) * (uint32_t)CBN;
    const int pair = wave & 3;
    const char* g = uniform_ptr(gop) + (CBN - 1024) + pair * 2 * CBN;
    const uint32_t base =
        __builtin_amdgcn_readfirstlane(lds_u32(tab) + (uint32_t)(buf * kTabBytes) + (uint32_t)(pair * 1024));
    glds16m(g, voff, base);
  }
  __device__ __forceinline__ static int ntab() { return loader() >= 0 ? 1 : 0; }
  // entry c of the op being computed
  __device__ __forceinline__ const float4* tab_entry(int c) const {
    uint32_t off = tcur * kTabBytes;
    asm volatile("" : "+s"(off));
    return (const float4*)(tab + off + c * 512);
  }
  template <int B0, int B1, int B2>
  __device__ __forceinline__ void start(const char* g0, const char* g1, const char* g2) { start<B0, B1, B2, 0>(g0, g1, g2, nullptr); }
  // CBT != 0: also the bias table of the first op (gt, chunk stride CBT), behind chunk 0 and ahead of the
  // chunks the wait leaves in flight
  template <int B0, int B1, int B2, int CBT>
  __device__ __forceinline__ void start(const char* g0, const char* g1, const char* g2, const char* gt) {
    static_assert(RING == 4, "start: the first RING - 1 chunks");
    cur = 0;
    es = 0;
    er = 0;
    tcur = 0;
    dma<B0>(g0, 0);
    if constexpr (CBT != 0) dma_tab<CBT>(gt, 0);
    dma<B1>(g1, 1);
    dma<B2>(g2, 2);
    prev = npieces<B2>();
    wait_vmcnt(npieces<B1>() + npieces<B2>());
    __syncthreads();
  }
  template <int BYTES>
  __device__ __forceinline__ void issue(const char* gsrc) { dma<BYTES>(gsrc, ahead_slot()); }
  // this wave's softplus' slab of chunk c (blocks 2c, 2c+1, all kNC columns: 2 kNC pieces, contiguous in
  // global memory) -> the next slab slot.  Staged two chunk-iterations before the epilogue that reads it.  Returns the DMA instructions issued.
  // e: byte base of the layer's slab (24-bit codes, kSlab24Chunk per column and chunk)
  __device__ __forceinline__ int stage_slab(const float4* e, int c) {
    return stage_slab(e, c, (threadIdx.x & 63) * kSlabVB);
  }
  // voff: this lane's byte offset from e (lane x kSlabVB; the compacted reverse pass gathers each lane's
  // codes from its point's own tile)
  __device__ __forceinline__ int stage_slab(const float4* e, int c, uint32_t voff) {
    // global: 768 B per piece (64 lanes x 12 B); LDS: 1 KB per piece (lane stride 16 B), so each piece
    // gets its own global base and M0 (the instruction offset would step both by the same amount).
    // nt: the codes are read once, so they should not evict the weight stream's lines from L2
    // (3.80 -> 3.74 ms per 524 k-point nabla + feature launch)
    const char* g = uniform_ptr((const char*)e + kNC * kSlab24Chunk * c);
    const uint32_t base =
        __builtin_amdgcn_readfirstlane(lds_u32(slab) + (uint32_t)(es * kSlab4 + wave_id() * kSlabW));
#pragma unroll
    for (int piece = 0; piece < 2 * kNC; ++piece) {
      const char* gp = g + piece * 768;
      asm volatile(
          "s_mov_b32 m0, %2\n\ts_nop 0\n\t"
          "global_load_lds_dwordx3 %0, %1 nt"
          :
          : "v"(voff), "s"(gp), "s"(base + piece * 1024)
          : "memory", "m0");
    }
    es = next3(es);
    return 2 * kNC;
  }
  // the slab of the chunk whose epilogue runs now (staged two iterations ago)
  __device__ __forceinline__ const float4* slab_read() const {
    uint32_t off = er * kSlab4 + wave_id() * kSlabW;
    asm volatile("" : "+s"(off));
    return (const float4*)(slab + off);
  }
  __device__ __forceinline__ void slab_consumed() { er = next3(er); }
  __device__ __forceinline__ const float4* buf() const {
    uint32_t off = cur * CBMAX;
    asm volatile("" : "+s"(off));
    return (const float4*)(lds + off);
  }
  // n: DMA / store instructions this wave issued in the current iteration (vmcnt retires in issue
  // order: everything older -- the current-plus-one chunk's weights and slab -- has landed after it).
  // RING 4: chunk c+1 went out two iterations ago, so the previous iteration's instructions may stay
  // in flight too (after a vmcnt(0) drain the count only over-allows instructions that have landed)
  __device__ __forceinline__ void flip(int n) {
    if constexpr (RING == 4) {
      wait_vmcnt(n + prev);
      prev = n;
    } else {
      wait_vmcnt(n);
    }
    __syncthreads();
    cur = nextr(cur);
  }
  // the caller has waited for everything the next chunk needs (tgemm_kernel's counted waits)
  __device__ __forceinline__ void flip_nowait() {
    __syncthreads();
    cur = nextr(cur);
  }
};

// one k-step pair of output blocks x kNC point columns: 6 kNC MFMAs per k-step
// Software-pipelined one k-step deep (step s+1's 4 fragments are read while step s's MFMAs
// issue).  stage(s) is VALU work of the previous chunk's epilogue placed in k-step s's scheduling
// region, so it fills the matrix core's issue gaps instead of running before or after the MFMAs.
__device__ __forceinline__ f16x8 rd_frag(const float4* __restrict__ A, int i, int lane) {
  return as_h8(A[i * 64 + lane]);
}
template <int NS, class Stage>
__device__ __forceinline__ void mma4(const float4* __restrict__ A, const f16x8 (&bh)[kNC][12],
                                     const f16x8 (&bl)[kNC][12], f32x4 (&acc)[kNC][2], int lane, Stage&& stage) {
  f16x8 nh0 = rd_frag(A, 0, lane), nl0 = rd_frag(A, 1, lane);
  f16x8 nh1 = rd_frag(A, NS * 2, lane), nl1 = rd_frag(A, NS * 2 + 1, lane);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const f16x8 h0 = nh0, l0 = nl0, h1 = nh1, l1 = nl1;
    if (s + 1 < NS) {
      nh0 = rd_frag(A, (s + 1) * 2, lane);
      nl0 = rd_frag(A, (s + 1) * 2 + 1, lane);
      nh1 = rd_frag(A, (NS + s + 1) * 2, lane);
      nl1 = rd_frag(A, (NS + s + 1) * 2 + 1, lane);
    }
    stage(s);
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      acc[q][0] = mfma16h(l0, bh[q][s], acc[q][0]);
      acc[q][1] = mfma16h(l1, bh[q][s], acc[q][1]);
      acc[q][0] = mfma16h(h0, bl[q][s], acc[q][0]);
      acc[q][1] = mfma16h(h1, bl[q][s], acc[q][1]);
      acc[q][0] = mfma16h(h0, bh[q][s], acc[q][0]);
      acc[q][1] = mfma16h(h1, bh[q][s], acc[q][1]);
    }
    // the next step's 4 fragment reads ahead of this step's MFMAs (a whole region of prefetch
    // distance); the epilogue VALU is left to the scheduler
    if (s + 1 < NS) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 6 * kNC, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Pre-activations of one chunk: z[q][o] = column q, output block 2c+o; aux[o] = the op's per-row
// vector (bias-slot floats 64..95) for block o
struct Z4 {
  float4 z[kNC][2];
  float4 aux[2];
};

// One GEMM op: out = W · B (+ bias), NBO/2 chunks, fully unrolled; chunk c's epilogue runs in chunk
// c+1's iteration (after its DMA issue, beside its MFMAs).
//  pre(c): issued right after chunk c's weight DMA (slab staging for a later chunk's epilogue);
//          returns the DMA instructions it issued
//  TS:     the epilogue wants t = 100 log2(e) z instead of z (forward softplus ops: the bias slot's
//          floats 96..127 hold bias * 100 log2(e), packed by pack_ops_kernel)
// kT ~ 100 log2(e) and kC ~ ln2 / 100 as a float pair whose product is 1 within 2e-10: on softplus'
// linear branch the value path is t * kC = z * kT * kC, so the correctly rounded constants
// (product 1 - 4.7e-8) would shrink every positive activation by that factor per layer, a bias that
// compounds over the network's 8 layers.  kT sits 4.5e-7 relative below 100 log2(e) (softplus' beta
// moves by that much: <= 3e-9 absolute on its output).  pack_ops_kernel packs bias * kT.
constexpr float kT = 144.26944f;
constexpr float kC = 0.0069314749f;

#ifdef NR_EXP_STAMPS
// stamps build: per-wave shader-clock totals of the four phases of a chunk iteration (VMEM
// issue, MFMA loop + epilogue stages, bias + vmcnt wait, barrier), copied out at the end of the launch
// sdf4_kernel also stamps the whole tile: 6 = tile start (loop top to the first op), 7 = tile end (last op's
// return to the loop's end), 8 = the tile; what 8 has beyond 0..3, 6 and 7 is the op boundaries and the
// forward -> reverse turn
constexpr int kStampPh = 9;  // 4 phases + iteration count (tgemm_kernel: tile start) + tgemm's epilogue + 3
constexpr int kStampSlot = 2048 * 8 * kStampPh;  // one launch's stamps
// slot 0: the last launch of any stamped kernel; slot 1 + STAGE_: the last sdf4_kernel launch of that STAGE_
// (a render runs several instances back to back)
__device__ unsigned long long g_nr_stamps[6 * kStampSlot];
__device__ __forceinline__ unsigned long long* stamp_lds() {
  __shared__ unsigned long long s_stamp[kW4 * kStampPh];
  return s_stamp;
}
__device__ __forceinline__ uint64_t stamp_now() { return __builtin_amdgcn_s_memtime(); }
__device__ __forceinline__ void stamp_add(int ph, uint64_t dt) {
  if ((threadIdx.x & 63) == 0) stamp_lds()[(threadIdx.x >> 6) * kStampPh + ph] += dt;
}
#define NR_STAMP(var) const uint64_t var = stamp_now()
#define NR_STAMP_VAR(var) uint64_t var = 0
#define NR_STAMP_SET(var) var = stamp_now()
#define NR_STAMP_ADD(ph, dt) stamp_add(ph, dt)
#else
#define NR_STAMP(var)
#define NR_STAMP_VAR(var)
#define NR_STAMP_SET(var)
#define NR_STAMP_ADD(ph, dt)
#endif

// MODE: where the op's bias-slot data comes from (NXT_MODE: the same for the next op, whose first chunks
// this op issues).
// kSlot: the whole chunk is fetched and the bias slot read from the ring slot.
// kLean: the op has no per-row data in its bias slots (transposed ops: no bias, no aux).  Only the 2 KB
// weight pieces of each chunk are fetched, from the unchanged global address (the chunk stride stays
// CB) into the unchanged ring slot, so every loader wave issues 2 KB / kLd pieces and none twice for
// KB 16; the op's one scalar, 1 / weight scale, comes in as winv (per-op table of the pack's tail).
// kTab (forward ops of the launches whose LDS holds the weight ring alone): the chunks are fetched as in
// kLean; bias, scalars and aux come from the op's bias table in LDS (WStream4::dma_tab), fetched once
// per op by the op before it, in the iteration that issues this op's chunk 0 (start() for the first
// op), into the table buffer the op before that one has left.
enum { kSlot = 0, kLean = 1, kTab = 2 };
template <int KB, int NBO, int NXT_CB, bool AUX, bool TS, int MODE = kSlot, int NXT_MODE = kSlot, class WS,
          class Pre, class Epi>
__device__ __forceinline__ void op4(WS& ws, const char* __restrict__ op, const char* nxt, const f16x8 (&bh)[kNC][12],
                                    const f16x8 (&bl)[kNC][12], const float (&xinv)[kNC], Pend4& pd, Pre&& pre,
                                    Epi&& epi, int lane, float winv = 0.0f) {
  constexpr int CB = chunk_bytes(KB);
  constexpr bool LEAN = MODE == kLean;
  constexpr int FB = MODE != kSlot ? weight_bytes(KB) : CB;             // bytes fetched per chunk
  constexpr int NXT_FB = NXT_MODE != kSlot ? NXT_CB - 1024 : NXT_CB;    // ... of the next op
  static_assert(!LEAN || (!AUX && !TS), "lean ops carry no per-row data");
  constexpr int NCH = NBO / 2;
  static_assert(MODE != kTab || NCH * 512 <= kTabBytes, "bias table entries");
  constexpr int LA = WS::kRingN - 1;  // chunks issued ahead of the one being computed
  static_assert(NCH >= 2, "the 2-ahead stream needs >= 2 chunks per op");
  // (a 4-slot ring's lookahead reaches chunk 2 of the next op: forward ops only, all >= 7 chunks)
  const int g = lane >> 4;
  Z4 zq{};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    // opaque per chunk: keeps the scheduler from computing every chunk's address up front
    const char* opc = op;
    const char* nxc = nxt;
    asm volatile("" : "+s"(opc), "+s"(nxc));
    NR_STAMP(t0);
    int npend = 0;
    if (c + LA < NCH) {
      ws.template issue<FB>(opc + (c + LA) * CB);
      npend = WS::template npieces<FB>();
    } else if (nxc) {
      ws.template issue<NXT_FB>(nxc + (c + LA - NCH) * NXT_CB);
      npend = WS::template npieces<NXT_FB>();
      if constexpr (NXT_MODE == kTab) {
        if (c + LA == NCH) {  // (compile time) the next op's chunk 0 went out just now: its table with it
          ws.template dma_tab<NXT_CB>(nxc, ws.tcur ^ 1);
          npend += WS::ntab();
        }
      }
    }
    npend += pre(c);
    // the previous chunk's stores go out after this chunk's DMA: this chunk's flip does not wait for
    // them (the next one does, two chunk-times after issue)
    npend += pd.flush();
    NR_STAMP(t1);
    const float4* A = ws.buf();
    f32x4 acc[kNC][2] = {};
    // the previous chunk's epilogue, 8 stages spread over this chunk's KB/2 k-steps
    mma4<KB / 2>(A, bh, bl, acc, lane, [&](int st) {
      if (c > 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e * (KB / 2) / 8 == st) epi(c - 1, zq, e);
      }
    });
    NR_STAMP(t2);
    float wi;
    float4 b0, b1;
    if constexpr (LEAN) {  // + 0 kept: an accumulator of -0 comes out +0, as with the slot's zero bias
      wi = winv;
      b0 = b1 = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const float4* S = MODE == kTab ? ws.tab_entry(c) : A + 2 * KB * 64;  // the chunk's bias slot
      wi = S[8].x;
      if constexpr (TS) wi *= kT;
      b0 = S[(TS ? 24 : 0) + g];
      b1 = S[(TS ? 28 : 4) + g];
    }
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      const float inv = xinv[q] * wi;
      zq.z[q][0] = fma4s(acc[q][0], inv, b0);
      zq.z[q][1] = fma4s(acc[q][1], inv, b1);
    }
    if constexpr (AUX) {
      const float4* S = MODE == kTab ? ws.tab_entry(c) : A + 2 * KB * 64;
      zq.aux[0] = S[16 + g];
      zq.aux[1] = S[20 + g];
    }
#ifdef NR_EXP_STAMPS
    wait_vmcnt(npend);
    NR_STAMP(t3);
    ws.flip(npend);
    NR_STAMP(t4);
    stamp_add(0, t1 - t0);
    stamp_add(1, t2 - t1);
    stamp_add(2, t3 - t2);
    stamp_add(3, t4 - t3);
    stamp_add(4, 1);
#else
    ws.flip(npend);
#endif
  }
  pd.flush();  // chunk NCH-2's stores, put by its epilogue in the last iteration
  if constexpr (MODE == kTab) ws.tcur ^= 1;  // the next op's table
#pragma unroll
  for (int e = 0; e < 8; ++e) epi(NCH - 1, zq, e);
}

// ---- staged epilogues: operator()(c, z, st) does stage st (0..7) of chunk c's epilogue; stages
// 4q..4q+3 handle column q (two values each, the fourth also splits the column's 8 outputs) ----
template <bool NABLA>
__device__ __forceinline__ void sp_pair(const Z4& zz, int q, int k, float4 (&y)[2], float4& s0, float4& s1) {
  const int o = k >> 1;
  const float4 z = zz.z[q][o];
  float4& s = o ? s1 : s0;
  if ((k & 1) == 0) softplus_pk<NABLA>(z.x, z.y, y[o].x, y[o].y, s.x, s.y);
  else softplus_pk<NABLA>(z.z, z.w, y[o].z, y[o].w, s.z, s.w);
}
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
// slab layout [block][column][lane]: the chunk's blocks 2c, 2c+1 of all kNC columns = 2 kNC KB
__device__ __forceinline__ uint32_t opaque_lane(int lane) {  // not hoistable: offsets built at use
  uint32_t l = (uint32_t)lane;
  asm volatile("" : "+v"(l));
  return l;
}
// pd.v[o * kNC + q] (block first_blk + o, column q) -> its slab slot
__device__ __forceinline__ void pend_chunk(Pend4& pd, float4* base, int first_blk, int lane, bool nt) {
  const uint32_t l = opaque_lane(lane);
#pragma unroll
  for (int i = 0; i < 2 * kNC; ++i) pd.o[i] = (kNC * first_blk + i) * 64 + l;
  pd.put(base, 2 * kNC, nt);
}
// 24-bit slab codes of chunk c: pd.v[o * kNC + q] (3 dwords: block 2c + o, column q) -> byte offset
// c kNC 1536 + ((o kNC + q) 64 + lane) 12 of the layer's slab (the chunk's kNC x 1536 B stay contiguous
// for the reverse pass's staging DMA)
__device__ __forceinline__ void pend_chunk24(Pend4& pd, float4* layer, int c, int lane, bool nt) {
  const uint32_t l = opaque_lane(lane);
#pragma unroll
  for (int i = 0; i < 2 * kNC; ++i) pd.o[i] = (uint32_t)(c * kNC * kSlab24Chunk) + ((uint32_t)i * 64 + l) * 12u;
  pd.put(layer, 2 * kNC, nt, true);
}
// softplus' = 1 - 2^-L is kept as the 24-bit code of c = 2^-L = 1 / (1 + 2^t): u = floor(c 2^23 + 0.5)
// (c in [0, 1], 2^23 fits in 24 bits).  The code's absolute error 2^-24 matches fp32's rounding of
// softplus' near 1 (and of the old 1 - 2^-L cancellation near 0); exact 1 (u = 0) wherever 2^-L < 2^-24,
// which covers torch's linear branch (100 z > 20: 2^-L < 2^-28.8).  4 codes -> 3 dwords.
__device__ __forceinline__ uint32_t code24(float c) { return (uint32_t)__builtin_fmaf(c, 8388608.0f, 0.5f); }
__device__ __forceinline__ float4 pack24(float c0, float c1, float c2, float c3) {
  const uint32_t u0 = code24(c0), u1 = code24(c1), u2 = code24(c2), u3 = code24(c3);
  return make_float4(__uint_as_float(u0 | (u1 << 24)), __uint_as_float((u1 >> 8) | (u2 << 16)),
                     __uint_as_float((u2 >> 16) | (u3 << 8)), 0.0f);
}
// g * softplus' = g - g c for the 4 codes in (w0, w1, w2)
__device__ __forceinline__ float4 unpack24_mul(uint32_t w0, uint32_t w1, uint32_t w2, float4 g) {
  const float u0 = (float)(w0 & 0xFFFFFFu);
  const float u1 = (float)(__builtin_amdgcn_alignbit(w1, w0, 24) & 0xFFFFFFu);
  const float u2 = (float)(__builtin_amdgcn_alignbit(w2, w1, 16) & 0xFFFFFFu);
  const float u3 = (float)(w2 >> 8);
  constexpr float k = 1.0f / 8388608.0f;
  return make_float4(__builtin_fmaf(-(g.x * k), u0, g.x), __builtin_fmaf(-(g.y * k), u1, g.y),
                     __builtin_fmaf(-(g.z * k), u2, g.z), __builtin_fmaf(-(g.w * k), u3, g.w));
}

// forward softplus op: out -> next operand (k-step c of oh/ol), slab <- L = log2(1 + 2^t).
// Staged by operation, not by value: each stage applies one step to all 16 values of the chunk
// (2 columns x 2 blocks x 4), so the VALU a k-step region receives is independent work that issues
// between its MFMAs.  Input t = 100 log2(e) z (op4's TS mode), then
//   L = log2(1 + 2^min(t, 126)),  y = max(L, t) * ln2/100
// equals torch's softplus(beta=100, threshold=20) up to ~1e-10 relative (on the linear branch,
// 100 z > 20, L exceeds t by log2(1 + 2^-t) < 3e-9; where the clamp bites (z > 0.873) the max returns
// t itself).  The backward needs softplus' = sigmoid(100 z) = 1 - 2^-L: the slab stores L and the
// backward epilogue forms g - g 2^-L with one exp2 + one fma (no reciprocal here: the forward
// epilogue, which carries the heavier VALU load, issues 2 transcendentals per value instead of 3).
// The running max tracks max(L, t) >= 0; finish() scales it by ln2/100.

template <bool NABLA>
struct FwdEpi4 {
  static constexpr int NV = 8 * kNC;  // values per lane and chunk
  f16x8 (&oh)[kNC][12];
  f16x8 (&ol)[kNC][12];
  const float (&sc)[kNC];  // operand scale of y (the split multiplies max(L, t) by sc * ln2/100)
  float4* sl;
  float (&mrun)[kNC];
  Pend4& pd;
  int lane;
  float e[NV], L[NV], m[NV];  // value i = (2q + o) * 4 + r: column q, block o, register r
  __device__ __forceinline__ static float zval(const Z4& zz, int i) {
    const float4 v = zz.z[i >> 3][(i >> 2) & 1];
    const int r = i & 3;
    return r == 0 ? v.x : (r == 1 ? v.y : (r == 2 ? v.z : v.w));
  }
  __device__ __forceinline__ void operator()(int c, const Z4& zz, int st) {
    if (st == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) e[i] = fminf(zval(zz, i), 126.0f);
    } else if (st == 1) {
#pragma unroll
      for (int i = 0; i < NV; ++i) e[i] = __builtin_amdgcn_exp2f(e[i]);
    } else if (st == 2) {
#pragma unroll
      for (int i = 0; i < NV; ++i) e[i] = e[i] + 1.0f;
#pragma unroll
      for (int i = 0; i < NV / 2; ++i) L[i] = __builtin_amdgcn_logf(e[i]);
    } else if (st == 3) {
#pragma unroll
      for (int i = NV / 2; i < NV; ++i) L[i] = __builtin_amdgcn_logf(e[i]);
      if constexpr (NABLA) {  // c = 2^-L = 1 / (1 + 2^t) for the slab codes (e no longer needed)
#pragma unroll
        for (int i = 0; i < NV / 2; ++i) e[i] = __builtin_amdgcn_rcpf(e[i]);
      }
    } else if (st == 4) {
#pragma unroll
      for (int i = 0; i < NV; ++i) m[i] = fmaxf(L[i], zval(zz, i));
      if constexpr (NABLA) {
#pragma unroll
        for (int i = NV / 2; i < NV; ++i) e[i] = __builtin_amdgcn_rcpf(e[i]);
      }
    } else if (st == 5) {
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        const int i = 8 * q;
        float r = mrun[q];
        r = __builtin_fmaxf(r, __builtin_fmaxf(m[i + 0], m[i + 1]));
        r = __builtin_fmaxf(r, __builtin_fmaxf(m[i + 2], m[i + 3]));
        r = __builtin_fmaxf(r, __builtin_fmaxf(m[i + 4], m[i + 5]));
        r = __builtin_fmaxf(r, __builtin_fmaxf(m[i + 6], m[i + 7]));
        mrun[q] = r;
      }
      if constexpr (NABLA) {  // 24-bit codes of 2^-L straight into the pending-store slots ([block][column])
#pragma unroll
        for (int q = 0; q < kNC; ++q)
#pragma unroll
          for (int o = 0; o < 2; ++o) {
            const int i = (2 * q + o) * 4;
            pd.v[kNC * o + q] = pack24(e[i], e[i + 1], e[i + 2], e[i + 3]);
          }
      }
    } else if (st == 6) {
      split8a(make_float4(m[0], m[1], m[2], m[3]), make_float4(m[4], m[5], m[6], m[7]), sc[0] * kC, oh[0][c],
              ol[0][c]);
    } else {
      if constexpr (NABLA) pend_chunk24(pd, sl, c, lane, kSlabNT);
    }
  }
};

// F7: softplus, sdf row (aux = W8[0, :]) as a running dot product, d sdf / d z7 parked in slab 7,
// h7 split for F8 when the geometry feature is wanted
template <bool NABLA, bool FEAT>
struct F7Epi4 {
  f16x8 (&oh)[kNC][12];
  f16x8 (&ol)[kNC][12];
  const float (&sc)[kNC];
  float4* g7;
  float (&mrun)[kNC];
  float (&sdf_part)[kNC];
  Pend4& pd;
  int lane;
  float4 y[kNC][2], s[kNC][2];
  __device__ __forceinline__ void operator()(int c, const Z4& zz, int st) {
    // stages 4q..4q+3: column q (one column per wave: stages 4..7 only finish the chunk)
    const int q = st >> 2, k = st & 3;
    if (q < kNC) sp_pair<NABLA>(zz, q, k, y[q], s[q][0], s[q][1]);
    if (q < kNC && k == 3) {
      const float4 w0 = zz.aux[0], w1 = zz.aux[1];
      float sp = sdf_part[q];
      sp = fmaf(y[q][0].x, w0.x, sp); sp = fmaf(y[q][0].y, w0.y, sp);
      sp = fmaf(y[q][0].z, w0.z, sp); sp = fmaf(y[q][0].w, w0.w, sp);
      sp = fmaf(y[q][1].x, w1.x, sp); sp = fmaf(y[q][1].y, w1.y, sp);
      sp = fmaf(y[q][1].z, w1.z, sp); sp = fmaf(y[q][1].w, w1.w, sp);
      sdf_part[q] = sp;
      if constexpr (NABLA) {
        pd.v[q] = mul4(w0, s[q][0]);
        pd.v[kNC + q] = mul4(w1, s[q][1]);
      }
      if constexpr (FEAT) {
        mrun[q] = amax8(mrun[q], y[q][0], y[q][1]);
        split8a(y[q][0], y[q][1], sc[q], oh[q][c], ol[q][c]);
      }
    }
    if constexpr (NABLA)
      if (st == 7) pend_chunk(pd, g7, 2 * c, lane, kFeatNT);
  }
};

// backward op: out = Wᵀ G scaled by softplus'(z) of the layer below (slab staged into LDS in the
// chunk's own iteration, read here, one iteration later); chunks >= NMAIN/2 are embedding
// gradients, parked in fp32 from block park_blk on
template <int NMAIN, class WS>
struct BwdEpi4 {
  f16x8 (&oh)[kNC][12];
  f16x8 (&ol)[kNC][12];
  const float (&sc)[kNC];
  WS& ws;
  float4* park;
  int park_blk;
  float (&mrun)[kNC];
  Pend4& pd;
  int lane;
  int plane;  // this lane's float4 index in the parked embedding gradients (lane; compacted: its point's)
  float4 y[kNC][2];
  __device__ __forceinline__ void operator()(int c, const Z4& zz, int st) {
    if (2 * c < NMAIN) {
      const int q = st >> 2, k = st & 3;
      if (q >= kNC) return;
      if (k < 2) {  // g * softplus'(z) = g - g 2^-L  (FwdEpi4's 24-bit codes of 2^-L)
        const uint4 sw = *(const uint4*)((const char*)ws.slab_read() + ((kNC * k + q) * 64 + lane) * 16);
        y[q][k] = unpack24_mul(sw.x, sw.y, sw.z, zz.z[q][k]);
      } else if (k == 2) {
        mrun[q] = amax8(mrun[q], y[q][0], y[q][1]);
      } else {
        split8a(y[q][0], y[q][1], sc[q], oh[q][c], ol[q][c]);
        if (q == kNC - 1) ws.slab_consumed();
      }
    } else if (st == 7) {
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        pd.v[q] = zz.z[q][0];
        pd.v[kNC + q] = zz.z[q][1];
      }
      pend_chunk(pd, park, park_blk + 2 * c - NMAIN, plane, false);
    }
  }
};

struct NoPre4 {
  __device__ __forceinline__ int operator()(int) const { return 0; }
};

// STAGE 0: forward (+ reverse pass with NABLA) on consecutive 128-point tiles.  The deferred-nabla
// pair (NABLA, no feature): STAGE 1 runs the forward and leaves each 16-point tile's slabs (softplus
// log2 terms, d sdf / d z7) in a.slabs at the tile's index; STAGE 2 runs only the reverse pass, on the
// 16-point tiles of the device list a.tiles[0 .. *a.n_tiles) (nablas of those points).
// tile claims (nr_mlp.h, SdfKArgsC::claim): the instances that run behind a render's sampling -- the mid-point
// launch and the reverse-only launches
template <bool NABLA, bool FEAT, int STAGE_>
constexpr bool kSdfClaim = NABLA && (STAGE_ == 2 || STAGE_ == 4 || (FEAT && STAGE_ == 0));

template <bool NABLA, bool FEAT, int STAGE_>
__global__ __attribute__((amdgpu_flat_work_group_size(STAGE_ == 3 ? 256 : kT4, STAGE_ == 3 ? 256 : kT4),
                          amdgpu_waves_per_eu(kWPE, kWPE)))
void sdf4_kernel(std::conditional_t<kSdfClaim<NABLA, FEAT, STAGE_>, SdfKArgsC, SdfKArgs> a) {
  // STAGE_ 3: the forward of a small launch (launch_sdf: at most 64 points per CU) on 64-point tiles of 4
  // waves, one per SIMD -- twice the CUs of 128-point tiles, half the matrix work per CU and chunk (each
  // workgroup streams the whole net once per tile either way); otherwise STAGE 0, the same per-point code
  // STAGE_ 4: STAGE 2 over a device list of points instead of tiles (each wave 16 listed points, every
  // lane reading its point's slab codes from that point's own tile)
  constexpr int STAGE = STAGE_ == 3 ? 0 : (STAGE_ == 4 ? 2 : STAGE_);
  constexpr bool COMPACT = STAGE_ == 4;
  constexpr bool CLAIM = kSdfClaim<NABLA, FEAT, STAGE_>;  // the others keep the fixed stride and their instructions
  constexpr int NW = STAGE_ == 3 ? 4 : kW4;  // waves per workgroup
  static_assert(STAGE_ != 3 || (!NABLA && !FEAT), "narrow tiles: forward-only launches");
  static_assert(STAGE == 0 || (NABLA && !FEAT), "deferred nablas: no feature");
  constexpr int PPW = 16 * kNC * NW;  // points per workgroup tile
  // positional encoding: one evaluation per argument (Enc4) in the render launches that run a reverse pass
  // -- the mid-point launch <true, true, 0> and the reverse-only <true, false, 2 / 4>, whose chain rule stood
  // bare at the tile end.  The forward-only instances keep one call per row (the sample launch measured no
  // faster with Enc4: profiles/tile_turns/ab.txt), and so does the fused nabla launch without the feature,
  // which holds the others to embed_feature's and embed_backward's values.
#ifdef NR_EXP_ROW_ENC  // variant builds: every instance on the per-row calls, for an A/B of the encoding alone
  constexpr bool ENC4 = false;
#else
  constexpr bool ENC4 = NABLA && STAGE != 1 && !(!FEAT && STAGE_ == 0);
#endif
  constexpr int CB = chunk_bytes(18);  // largest SDF op chunk (F4: 14 + 4 input blocks)
  constexpr int C16 = chunk_bytes(16), C4 = chunk_bytes(4), C14 = chunk_bytes(14), C18 = chunk_bytes(18);
  // launches with a reverse pass share the LDS with the slab ring (3 weight slots); forward-only
  // launches (STAGE 1 included: its slabs go straight to HBM) stream through a 4-slot ring
  static_assert((size_t)kW4 * kNC * kSlabColBytes <= kScratchPerWG, "per-workgroup slab scratch");
  constexpr bool SLABS = NABLA && STAGE != 1;
  constexpr int RING = SLABS ? 3 : kFwdRing;
  // the launches without a slab ring have room for the forward ops' bias table beside the weight ring
  // (4 x 37 KB + 2 x 4 KB): their forward ops run in op4's kTab mode, the others' on the slot path
  constexpr bool TABF = !SLABS;
  constexpr int FM = TABF ? kTab : kSlot;  // mode of the forward ops
  constexpr int LDSB = RING * CB + (SLABS ? kSlabRing * kSlab4 : 0) + (TABF ? 2 * kTabBytes : 0);
  __shared__ __attribute__((aligned(16))) char smem[LDSB + (CLAIM ? 16 : 0)];  // CLAIM: the claimed tile index
  static_assert(LDSB + (CLAIM ? 16 : 0) <= 160 * 1024, "LDS budget");
  static_assert(!TABF || RING * CB + 2 * kTabBytes == LDSB, "the bias table follows the weight ring");
  WStream4<CB, RING, NW> ws{smem, SLABS ? smem + RING * CB : nullptr, 0, 0, 0, 0, TABF ? smem + RING * CB : nullptr, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const char* W = a.packed;
  // addresses are rebuilt from an opaque base at each use: hoisted out of the tile loop, the ~50
  // chunk / slab addresses would pin (and spill) registers for the whole kernel
  auto OP = [&](int i) {  // ops packed back to back (nr_mlp.h)
    const char* w = W;
    asm volatile("" : "+s"(w));
    return w + sdf_op_off(i);
  };
  // F8, or the op the launch runs in its place (same shape: KB 16, NBO 16)
  auto OPF8 = [&]() {
    const char* w = a.f8_alt;
    asm volatile("" : "+s"(w));
    return w ? w : OP(F8);
  };
  const float b8 = *(const float*)(W + a.L.misc_off);
  // this wave's slabs: [layer 8][block 16][column kNC][lane 64] float4 (128 KB per column); the
  // deferred stages keep them per 16-point tile of the launch (set per tile below)
  float4* escr = uniform_ptr((float4*)((char*)a.scratch + (size_t)(blockIdx.x * kW4 + wave) * (kNC * kSlabColBytes)));
  // layer l's slab (byte base): layers 0..6 24-bit codes (kNC x 12 KB), layer 7 fp32 (kNC x 16 KB)
  auto slab = [&](int l) {
    char* e = (char*)escr;
    asm volatile("" : "+s"(e));
    return (float4*)(e + l * kNC * kSlab24Layer);
  };

#ifdef NR_EXP_STAMPS
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < kStampPh; ++i) stamp_lds()[wave * kStampPh + i] = 0;
#endif
  // The reverse ops run in op4's kLean mode (no bias piece) in the reverse-only launches and in the
  // nabla + feature launch.  The fused nabla launch without the feature keeps the slot path: lean, it
  // spills 59 registers instead of 24 (profiles/lean_stream/registers.txt).
  constexpr bool LEANR = STAGE == 2 || (NABLA && FEAT);
  constexpr int W16 = weight_bytes(16);  // a lean chunk of B7
  if constexpr (STAGE == 2) ws.template start<W16, W16>(OP(B7), OP(B7) + C16);
  else if constexpr (TABF)
    ws.template start<weight_bytes(4), weight_bytes(4), weight_bytes(4), C4>(OP(F0), OP(F0) + C4, OP(F0) + 2 * C4, OP(F0));
  else ws.template start<C4, C4>(OP(F0), OP(F0) + C4);
  Pend4 pd{};
  NoPre4 nopre;
  const float kSpSlack = 0.0070f;  // softplus(z) <= max(z, 0) + ln2/100

  // STAGE 2 walks the tile list, 8 tiles (one per wave) per workgroup iteration
  const int64_t Pn = COMPACT      ? ((int64_t)(*a.n_tiles) + 15) / 16 * 16
                     : STAGE == 2 ? (int64_t)(*a.n_tiles) * kPointsPerWG / kW4
                                  : (a.P_dev ? min(a.P, (int64_t)(*a.P_dev) * a.P_mult) : a.P);
  // Claimed tiles: thread 0 draws the next tile's index at the tile start, ahead of the point loads (whose
  // wait then covers the atomic's return), and leaves it in LDS; every wave reads it before the tile's last
  // op, which needs has_next -- the chunk barriers of the ops between order the write before those reads,
  // the last op's barriers order the reads before the next tile's write.
  int* claim = nullptr;  // the counter; stays null in the instances that cannot claim (no new code there)
  if constexpr (CLAIM) claim = a.claim;
  int* const claim_lds = (int*)(smem + LDSB);
  int64_t next = 0;  // the next tile's first point (claimed)
  for (int64_t base = (int64_t)blockIdx.x * PPW; base < Pn; base = claim ? next : base + (int64_t)gridDim.x * PPW) {
    bool has_next = base + (int64_t)gridDim.x * PPW < Pn;
    int claimed = 0;
    if (claim && threadIdx.x == 0) claimed = atomicAdd(claim, 1);
    NR_STAMP_VAR(ts0);
    NR_STAMP_VAR(ts1);  // the first op starts
    NR_STAMP_VAR(te0);  // the last op has returned
    NR_STAMP_SET(ts0);
    int64_t p0 = base + wave * 16 * kNC;  // this wave's first point
    int plane = lane;                      // float4 index of this lane's slab-7 / parked entries
    uint32_t soff = 0;                     // byte offset of this lane's slab codes (COMPACT)
    int64_t pl = 0;                        // this lane's listed point (COMPACT)
    bool listed = true;
    if constexpr (COMPACT) {  // list entries [p0, p0 + 16): one slot per lane j, -1 = padding (invalid)
      // neus_point_list: the 16 entries of a wave are one segment's, in slot order, the first one a slot,
      // all within 64 tiles of it -- which is the wave's slab base (past the list's end: the last wave's)
      const int64_t n = *a.n_tiles;
      const int64_t w0 = p0 < n ? p0 : n - 16;
      const int e = a.tiles[w0 + j];
      const int e0 = __builtin_amdgcn_readfirstlane(a.tiles[w0]);
      listed = p0 < n && e >= 0;
      pl = e >= 0 ? e : e0;
      const uint32_t rt = (uint32_t)((pl >> 4) - (e0 >> 4)), js = (uint32_t)(pl & 15);  // rt < 64
      plane = (int)(rt * (uint32_t)(kSlabColBytes / 16) + js + 16u * (uint32_t)g);
      soff = rt * (uint32_t)kSlabColBytes + (js + 16u * (uint32_t)g) * (uint32_t)kSlabVB;
      escr = uniform_ptr((float4*)((char*)a.slabs + (size_t)(e0 >> 4) * kSlabColBytes));
    } else if constexpr (STAGE == 2) {  // this wave's tile (the last one again past the list's end: nothing stored)
      const int64_t ti = min(p0 / 16, (int64_t)(*a.n_tiles) - 1);
      const int64_t tile = a.tiles[ti];
      escr = uniform_ptr((float4*)((char*)a.slabs + (size_t)tile * kSlabColBytes));
      p0 = p0 / 16 < (int64_t)(*a.n_tiles) ? tile * 16 : a.P;  // a.P: every point invalid
    } else if constexpr (STAGE == 1) {
      escr = uniform_ptr((float4*)((char*)a.slabs + (size_t)(p0 / 16) * kSlabColBytes));
    }
    const int64_t Pv = STAGE == 2 ? a.P : Pn;  // points of the launch (validity of this wave's points)
    int64_t pq[kNC];
    bool valid[kNC];
    float xs[kNC][3];
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      const int64_t p = p0 + 16 * q + j;
      if constexpr (COMPACT) {
        valid[q] = listed;
        pq[q] = pl;
      } else {
        valid[q] = p < Pv;
        pq[q] = valid[q] ? p : Pv - 1;
      }
      xs[q][0] = a.pts[pq[q] * 3 + 0];
      xs[q][1] = a.pts[pq[q] * 3 + 1];
      xs[q][2] = a.pts[pq[q] * 3 + 2];
    }
    if (claim && threadIdx.x == 0) *claim_lds = claimed;
    float4 E[kNC][4];
    float mE[kNC], xinv[kNC];
    f16x8 Uh[kNC][12], Ul[kNC][12], Vh[kNC][12], Vl[kNC][12];
    float mrun[kNC], m_in[kNC];  // running max |output| of the op being computed (lane's values),
                                 // max |input| of the op being computed (per point)
    // (R, B) of the op about to run ride in its chunks' bias slot (floats 33, 34); its chunk 0 is
    // the current ring slot when it starts (TABF: entry 0 of its bias table, current since the op
    // before it ended)
    auto next_scales = [&](int kb, float extra, const float (&floor_max)[kNC], float (&sc)[kNC]) {
      const float4 v = TABF ? ws.tab_entry(0)[8] : ws.buf()[2 * kb * 64 + 8];
#pragma unroll
      for (int q = 0; q < kNC; ++q) sc[q] = bound_scale(fmaxf(fmaf(v.y, m_in[q], v.z) + extra, floor_max[q]));
    };
    // The reverse ops fetch no bias slot (op4's kLean mode): their three scalars -- 1 / weight scale and
    // (R, B), the words 32..34 of every one of their slots -- come from the per-op tables of the pack's
    // tail through a wave-uniform pointer (scalar loads, as b8), one op ahead of their use.
    struct OpScal {
      float winv, R, B;
    };
    auto op_scal = [&](int opi) {
      const char* w = W;
      asm volatile("" : "+s"(w));
      // constant address space: scalar loads wherever they stand (the pack is not written while a
      // render kernel runs), never a vector load that a counted vmcnt wait would have to count
      typedef __attribute__((address_space(4))) const float cfloat;
      cfloat* rb = (cfloat*)(w + a.L.bound_off + 8 * opi);
      return OpScal{*(cfloat*)(w + a.L.winv_off + 4 * opi), rb[0], rb[1]};
    };
    // end of an op: its output becomes the next operand; mscale converts the running max to output
    // units (forward softplus epilogues track max(L, t), i.e. y / (ln2/100))
    auto finish = [&](const float (&sc)[kNC], float mscale = 1.0f) {
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        m_in[q] = max4_groups(mrun[q]) * mscale;
        mrun[q] = 0.0f;
        xinv[q] = 1.0f / sc[q];
      }
    };
    float zero2[kNC];
#pragma unroll
    for (int q = 0; q < kNC; ++q) zero2[q] = 0.0f;
    if constexpr (STAGE != 2) {
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      if constexpr (ENC4) {
        // lane group and column rebuilt opaquely: hoisted out of the tile loop, the rows' source lanes and
        // select masks would sit in registers for the whole kernel
        const int ge = (int)opaque_lane(g), je = (int)opaque_lane(j);
        Enc4 t;
        enc_eval(t, xs[q], ge);
        E[q][0] = enc_rows<0>(t, xs[q], ge, je);
        E[q][1] = enc_rows<1>(t, xs[q], ge, je);
        E[q][2] = enc_rows<2>(t, xs[q], ge, je);
        E[q][3] = enc_rows<3>(t, xs[q], ge, je);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int f = 16 * b + 4 * g;
          E[q][b] = make_float4(embed_feature(f + 0, xs[q][0], xs[q][1], xs[q][2], a.nfreq),
                                embed_feature(f + 1, xs[q][0], xs[q][1], xs[q][2], a.nfreq),
                                embed_feature(f + 2, xs[q][0], xs[q][1], xs[q][2], a.nfreq),
                                embed_feature(f + 3, xs[q][0], xs[q][1], xs[q][2], a.nfreq));
        }
      }
      mE[q] = max4_groups(amax8(amax8(0.0f, E[q][0], E[q][1]), E[q][2], E[q][3]));
      const float sE = bound_scale(mE[q]);  // exact-max scale for the embedding operand of F0
      split8a(E[q][0], E[q][1], sE, Uh[q][0], Ul[q][0]);
      split8a(E[q][2], E[q][3], sE, Uh[q][1], Ul[q][1]);
      xinv[q] = 1.0f / sE;
    }
    // F4 (skip layer) needs the embedding again, split at F3's output scale: with a slab workspace
    // it waits there (slab 7, blocks 12-15, free until F7) instead of in 32 registers
    float4* epark = slab(7);
    if constexpr (NABLA) {
      const uint32_t l = opaque_lane(lane);
#pragma unroll
      for (int q = 0; q < kNC; ++q)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t off = (((12 + b) * kNC + q) * 64 + l) * 16u;
          const f32x4 d = tof(E[q][b]);
          asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(off), "v"(d), "s"(epark) : "memory");
        }
    }
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      mrun[q] = 0.0f;
      m_in[q] = mE[q];
    }
    auto fwd_epi = [&](f16x8(&oh)[kNC][12], f16x8(&ol)[kNC][12], const float (&sc)[kNC], float4* sl) {
      return FwdEpi4<NABLA>{oh, ol, sc, sl, mrun, pd, lane};
    };

    // ---- forward (base.py:243-257) -------------------------------------------------------------
    NR_STAMP_SET(ts1);
    {
      float sc[kNC];
      next_scales(4, kSpSlack, zero2, sc);
      op4<4, 16, C16, false, true, FM, FM>(ws, OP(F0), OP(F1), Uh, Ul, xinv, pd, nopre, fwd_epi(Vh, Vl, sc, slab(0)), lane);
      finish(sc, kC);
    }
    {
      float sc[kNC];
      next_scales(16, kSpSlack, zero2, sc);
      op4<16, 16, C16, false, true, FM, FM>(ws, OP(F1), OP(F2), Vh, Vl, xinv, pd, nopre, fwd_epi(Uh, Ul, sc, slab(1)), lane);
      finish(sc, kC);
    }
    {
      float sc[kNC];
      next_scales(16, kSpSlack, zero2, sc);
      op4<16, 16, C16, false, true, FM, FM>(ws, OP(F2), OP(F3), Uh, Ul, xinv, pd, nopre, fwd_epi(Vh, Vl, sc, slab(2)), lane);
      finish(sc, kC);
    }
    {
      // F3's outputs (h3: 217 rows in 14 blocks) and the embedding form F4's operand: one scale
      float sc[kNC];
      next_scales(16, kSpSlack, mE, sc);
      op4<16, 14, C18, false, true, FM, FM>(ws, OP(F3), OP(F4), Vh, Vl, xinv, pd, nopre, fwd_epi(Uh, Ul, sc, slab(3)), lane);
      if constexpr (NABLA) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < kNC; ++q)
#pragma unroll
          for (int b = 0; b < 4; ++b) E[q][b] = fromf(*((const gf4*)epark + ((12 + b) * kNC + q) * 64 + lane));
      }
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        split8a(E[q][0], E[q][1], sc[q], Uh[q][7], Ul[q][7]);
        split8a(E[q][2], E[q][3], sc[q], Uh[q][8], Ul[q][8]);
        mrun[q] = fmaxf(mrun[q], mE[q] * (1.0f / kC));  // mrun is in max(L, t) units here
      }
      finish(sc, kC);
    }
    {
      float sc[kNC];
      next_scales(18, kSpSlack, zero2, sc);
      op4<18, 16, C16, false, true, FM, FM>(ws, OP(F4), OP(F5), Uh, Ul, xinv, pd, nopre, fwd_epi(Vh, Vl, sc, slab(4)), lane);
      finish(sc, kC);
    }
    {
      float sc[kNC];
      next_scales(16, kSpSlack, zero2, sc);
      op4<16, 16, C16, false, true, FM, FM>(ws, OP(F5), OP(F6), Vh, Vl, xinv, pd, nopre, fwd_epi(Uh, Ul, sc, slab(5)), lane);
      finish(sc, kC);
    }
    {
      float sc[kNC];
      next_scales(16, kSpSlack, zero2, sc);
      op4<16, 16, C16, false, true, FM, FM>(ws, OP(F6), OP(F7), Uh, Ul, xinv, pd, nopre, fwd_epi(Vh, Vl, sc, slab(6)), lane);
      finish(sc, kC);
    }
    // F7: softplus, sdf row (aux = W8[0, :]) as a running dot product, d sdf / d z7 parked in slab 7,
    // h7 split for F8 when the geometry feature is wanted
    float sdf_part[kNC];
#pragma unroll
    for (int q = 0; q < kNC; ++q) sdf_part[q] = 0.0f;
    {
      float sc[kNC];
      next_scales(16, kSpSlack, zero2, sc);
      F7Epi4<NABLA, FEAT> epi{Uh, Ul, sc, slab(7), mrun, sdf_part, pd, lane};
      constexpr int NXT = ((NABLA && STAGE == 0) || FEAT) ? C16 : C4;
      const char* n;
      if constexpr (FEAT) n = OPF8();
      else n = (NABLA && STAGE == 0) ? OP(B7) : (has_next ? OP(F0) : nullptr);
      // next: F8 (forward), B7 (here only on the slot path: LEANR needs FEAT), or the next tile's F0
      op4<16, 16, NXT, true, false, FM, FM>(ws, OP(F7), n, Vh, Vl, xinv, pd, nopre, epi, lane);
      finish(sc);
    }
    NR_STAMP_SET(te0);
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      const float sdf = wave_sum4(sdf_part[q]) + b8;
      if (valid[q] && g == 0) a.sdf[p0 + 16 * q + j] = sdf;
    }
    // ---- geometry feature rows 1..256 (no activation) ------------------------------------------
    if constexpr (FEAT) {
      const int64_t pf = p0 < Pn ? p0 : Pn - 1;
      float4* fb = uniform_ptr((float4*)(a.feature + pf * 256));
      // clamped lanes (past the end) rewrite the last point's row with that point's own values
      uint32_t frow[kNC];
#pragma unroll
      for (int q = 0; q < kNC; ++q) frow[q] = (uint32_t)(pq[q] - pf);
      auto epi = [&](int c, const Z4& zz, int st) {
        if (st != 7) return;
#pragma unroll
        for (int q = 0; q < kNC; ++q) {
          pd.v[2 * q] = zz.z[q][0];
          pd.v[2 * q + 1] = zz.z[q][1];
          const uint32_t r = opaque_lane(frow[q] * 64 + g);
          pd.o[2 * q] = r + (2 * c) * 4;
          pd.o[2 * q + 1] = r + (2 * c + 1) * 4;
        }
        pd.put(fb, 2 * kNC, kFeatNT);
      };
      constexpr int NXT = NABLA ? C16 : C4;
      const char* n = NABLA ? OP(B7) : (has_next ? OP(F0) : nullptr);
      op4<16, 16, NXT, false, false, FM, NABLA ? (LEANR ? kLean : kSlot) : FM>(ws, OPF8(), n, Uh, Ul, xinv, pd, nopre, epi,
                                                                               lane);
      NR_STAMP_SET(te0);
    }
    }  // STAGE != 2: forward
    if constexpr (NABLA && STAGE == 1) {  // the slabs stay for the reverse-pass launch
      pd.flush();
    }
    if constexpr (NABLA && STAGE != 1) {
      // ---- reverse pass (autograd.grad of sdf w.r.t. x, base.py:265-282) ------------------------
      pd.flush();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      OpScal osn{};  // the scalars of the op about to run, loaded while the previous one runs
      if constexpr (LEANR) osn = op_scal(B7);
      float4* g7 = slab(7);
#pragma unroll
      for (int q = 0; q < kNC; ++q) {  // d sdf / d z7 from slab 7, split with the exact max scale
        float4 G[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) G[b] = fromf(*((const gf4*)g7 + (kNC * b + q) * 64 + (COMPACT ? plane : lane)));
        float m = 0.0f;
#pragma unroll
        for (int b = 0; b < 16; b += 2) m = amax8(m, G[b], G[b + 1]);
        m_in[q] = max4_groups(m);
        mrun[q] = 0.0f;  // B7's running max starts here (STAGE 2 skips the forward that zeroes it)
        const float sc = bound_scale(m_in[q]);
#pragma unroll
        for (int s = 0; s < 8; ++s) split8a(G[2 * s], G[2 * s + 1], sc, Uh[q][s], Ul[q][s]);
        xinv[q] = 1.0f / sc;
      }
      float4* park = slab(7);  // embedding gradients [block 8][column 2][lane]: skip layer 0-3, first layer 4-7
      // backward op: out = Wᵀ G, scaled by softplus'(z) of the layer below (its slab, staged into LDS
      // two chunk-iterations ahead of the epilogue that reads it: chunk c+1's slab goes out right after
      // chunk c's weight DMA, the next op's chunk 0 during this op's last chunk); output chunks >=
      // NMAIN/2 are embedding gradients, parked in fp32
      if constexpr (COMPACT) ws.stage_slab(slab(6), 0, soff);  // B7's chunk 0 (consumed in B7's second iteration)
      else ws.stage_slab(slab(6), 0);
      auto bwd = [&](auto kb_tag, auto nbo_tag, auto nmain_tag, auto nxt_tag, auto nxl_tag, int opi, const char* nxt,
                     f16x8(&ih)[kNC][12], f16x8(&il)[kNC][12], f16x8(&oh)[kNC][12], f16x8(&ol)[kNC][12], int lcur,
                     int park_blk, int lnext) {
        constexpr int KBo = decltype(kb_tag)::value, NBOo = decltype(nbo_tag)::value;
        constexpr int NMAIN = decltype(nmain_tag)::value, NXC = decltype(nxt_tag)::value;
        constexpr bool NXL = decltype(nxl_tag)::value;
        const OpScal os = osn;
        float sc[kNC];
        if constexpr (LEANR) {
          if (opi != B0) osn = op_scal(opi + 1);  // B7..B0 are consecutive in stream order
#pragma unroll
          for (int q = 0; q < kNC; ++q) sc[q] = bound_scale(fmaxf(fmaf(os.R, m_in[q], os.B) + 0.0f, zero2[q]));
        } else {
          next_scales(KBo, 0.0f, zero2, sc);
        }
        auto pre = [&](int c) -> int {
          if constexpr (COMPACT) {
            if (2 * (c + 1) < NMAIN) return ws.stage_slab(slab(lcur), c + 1, soff);
            if (c + 1 == NBOo / 2 && lnext >= 0) return ws.stage_slab(slab(lnext), 0, soff);
          } else {
            if (2 * (c + 1) < NMAIN) return ws.stage_slab(slab(lcur), c + 1);
            if (c + 1 == NBOo / 2 && lnext >= 0) return ws.stage_slab(slab(lnext), 0);
          }
          return 0;
        };
        BwdEpi4<NMAIN, decltype(ws)> epi{oh, ol, sc, ws, park, park_blk, mrun, pd, lane, COMPACT ? plane : lane};
        constexpr int RM = LEANR ? kLean : kSlot, RMN = (LEANR && NXL) ? kLean : kSlot;
        op4<KBo, NBOo, NXC, false, false, RM, RMN>(ws, OP(opi), nxt, ih, il, xinv, pd, pre, epi, lane, os.winv);
        finish(sc);
      };
      using I0 = std::integral_constant<int, 0>;
      using I4 = std::integral_constant<int, 4>;
      using I14 = std::integral_constant<int, 14>;
      using I16 = std::integral_constant<int, 16>;
      using I18 = std::integral_constant<int, 18>;
      using IC16 = std::integral_constant<int, C16>;
      using IC14 = std::integral_constant<int, C14>;
      using IC4 = std::integral_constant<int, C4>;
      using LeanNext = std::true_type;   // the next op is a reverse op too
      using SlotNext = std::false_type;  // ... the next tile's F0
      if constexpr (STAGE == 2) {
        NR_STAMP_SET(ts1);
      }
      bwd(I16{}, I16{}, I16{}, IC16{}, LeanNext{}, B7, OP(B6), Uh, Ul, Vh, Vl, 6, 0, 5);
      bwd(I16{}, I16{}, I16{}, IC16{}, LeanNext{}, B6, OP(B5), Vh, Vl, Uh, Ul, 5, 0, 4);
      bwd(I16{}, I16{}, I16{}, IC16{}, LeanNext{}, B5, OP(B4), Uh, Ul, Vh, Vl, 4, 0, 3);
      // skip layer: rows 0..216 -> h3 (scaled by softplus'(z3)), rows 217..255 -> embedding
      bwd(I16{}, I18{}, I14{}, IC14{}, LeanNext{}, B4, OP(B3), Vh, Vl, Uh, Ul, 3, 0, 2);
      bwd(I14{}, I16{}, I16{}, IC16{}, LeanNext{}, B3, OP(B2), Uh, Ul, Vh, Vl, 2, 0, 1);
      bwd(I16{}, I16{}, I16{}, IC16{}, LeanNext{}, B2, OP(B1), Vh, Vl, Uh, Ul, 1, 0, 0);
      bwd(I16{}, I16{}, I16{}, IC16{}, LeanNext{}, B1, OP(B0), Uh, Ul, Vh, Vl, 0, 0, -1);
      if (claim) {
        next = (int64_t)(gridDim.x + __builtin_amdgcn_readfirstlane(*claim_lds)) * PPW;
        has_next = next < Pn;
      }
      if constexpr (STAGE == 2) bwd(I16{}, I4{}, I0{}, IC16{}, LeanNext{}, B0, has_next ? OP(B7) : nullptr, Vh, Vl, Uh, Ul, 0, 4, -1);
      else bwd(I16{}, I4{}, I0{}, IC4{}, SlotNext{}, B0, has_next ? OP(F0) : nullptr, Vh, Vl, Uh, Ul, 0, 4, -1);
      NR_STAMP_SET(te0);
      pd.flush();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // chain rule through the positional encoding (autograd sums both uses of embed(x))
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        float n0 = 0.f, n1 = 0.f, n2 = 0.f;
        auto grad = [&](int b) {  // the gradient of rows 16 b + 4 g + r: skip layer's + first layer's
          const float4 u = fromf(*((const gf4*)park + (kNC * b + q) * 64 + (COMPACT ? plane : lane)));
          const float4 v = fromf(*((const gf4*)park + (kNC * (4 + b) + q) * 64 + (COMPACT ? plane : lane)));
          return make_float4(fadd(v.x, u.x), fadd(v.y, u.y), fadd(v.z, u.z), fadd(v.w, u.w));
        };
        if constexpr (ENC4) {  // rows in embed_backward's order
          const int ge = (int)opaque_lane(g), je = (int)opaque_lane(j);  // (as at the tile start)
          Enc4 t;
          enc_eval(t, xs[q], ge);
          const float4 g0 = grad(0), g1 = grad(1), g2 = grad(2);
          enc_row_bwd<0>(t, g0.x, ge, je, n0, n1, n2);
          enc_row_bwd<1>(t, g0.y, ge, je, n0, n1, n2);
          enc_row_bwd<2>(t, g0.z, ge, je, n0, n1, n2);
          enc_row_bwd<3>(t, g0.w, ge, je, n0, n1, n2);
          enc_row_bwd<16>(t, g1.x, ge, je, n0, n1, n2);
          enc_row_bwd<17>(t, g1.y, ge, je, n0, n1, n2);
          enc_row_bwd<18>(t, g1.z, ge, je, n0, n1, n2);
          enc_row_bwd<19>(t, g1.w, ge, je, n0, n1, n2);
          enc_row_bwd<32>(t, g2.x, ge, je, n0, n1, n2);
          enc_row_bwd<33>(t, g2.y, ge, je, n0, n1, n2);
          enc_row_bwd<34>(t, g2.z, ge, je, n0, n1, n2);
          enc_row_bwd<35>(t, g2.w, ge, je, n0, n1, n2);  // rows 48..63: none within 6 bands
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const float4 gr = grad(b);
            const int f = 16 * b + 4 * g;
            embed_backward(f + 0, gr.x, xs[q][0], xs[q][1], xs[q][2], a.nfreq, n0, n1, n2);
            embed_backward(f + 1, gr.y, xs[q][0], xs[q][1], xs[q][2], a.nfreq, n0, n1, n2);
            embed_backward(f + 2, gr.z, xs[q][0], xs[q][1], xs[q][2], a.nfreq, n0, n1, n2);
            embed_backward(f + 3, gr.w, xs[q][0], xs[q][1], xs[q][2], a.nfreq, n0, n1, n2);
          }
        }
        n0 = wave_sum4(n0);
        n1 = wave_sum4(n1);
        n2 = wave_sum4(n2);
        if (valid[q] && g == 0) {
          const int64_t p = COMPACT ? pq[q] : p0 + 16 * q + j;
          a.nabla[p * 3 + 0] = n0;
          a.nabla[p * 3 + 1] = n1;
          a.nabla[p * 3 + 2] = n2;
        }
      }
    }
    NR_STAMP(te1);
    NR_STAMP_ADD(6, ts1 - ts0);
    NR_STAMP_ADD(7, te1 - te0);
    NR_STAMP_ADD(8, te1 - ts0);
  }
  pd.flush();
  wait_vmcnt(0);  // a block without tiles still has the prologue's second chunk in flight
#ifdef NR_EXP_STAMPS
  if ((threadIdx.x & 63) == 0 && blockIdx.x < 2048)
    for (int i = 0; i < kStampPh; ++i) {
      const unsigned long long v = stamp_lds()[wave * kStampPh + i];
      g_nr_stamps[(blockIdx.x * kW4 + wave) * kStampPh + i] = v;
      g_nr_stamps[(1 + STAGE_) * kStampSlot + (blockIdx.x * kW4 + wave) * kStampPh + i] = v;
    }
#endif
}


// =============================================================================================
// SIREN SDF kernel (base.py:84-115 SirenLayer, ImplicitSurface(use_siren=True) with
// configs/volsdf_siren.yaml's D=5, skips=[], embed_multires=-1): h_{l+1} = sin(30 (W_l h_l + b_l)),
// l = 0..4, then Linear(256 -> 257): row 0 = sdf, rows 1..256 = geometry feature.  The reverse pass
// (autograd.grad of sdf w.r.t. x, base.py:265-282) runs back through the transposed layers with
// the cos(30 z) slabs; the gradient w.r.t. the 3 raw coordinates is the nabla (identity embedding).
// Same streamed-weight GEMM building blocks as sdf_kernel.
// =============================================================================================
template <int P, bool NABLA>
__global__ __launch_bounds__(kThreads) void siren_sdf_kernel(SdfKArgs a) {
  constexpr int CB = chunk_bytes(16);
  __shared__ __attribute__((aligned(16))) char smem[kRing * CB + (NABLA ? 2 * kSlabChunk : 0)];
  WStream<CB> ws{smem, NABLA ? smem + kRing * CB : nullptr, 0, 0, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const SdfLayout& L = a.L;
  const char* W = a.packed;
  auto OP = [&](int i) { return W + L.op_off[i]; };
  auto OPB = [&](int i) { return (int)L.op_bytes[i]; };
  const float* wl = (const float*)(W + L.w8row0_off);  // row 0 of the last layer
  const float bl = *(const float*)(W + L.misc_off);
  float4* escr = uniform_ptr(a.scratch + (size_t)(blockIdx.x * kWaves + wave) * (8 * 16 * 64));
  const bool want_feat = a.feature != nullptr;

  ws.start(OP(S0), OPB(S0), OP(S0) + OPB(S0), OPB(S0));

  const int64_t Pn = a.P_dev ? min(a.P, (int64_t)(*a.P_dev) * a.P_mult) : a.P;
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < Pn; base += (int64_t)gridDim.x * kPointsPerWG) {
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < Pn;
    const int64_t p = base + wave * kTile + j;
    const bool valid = p < Pn;
    const int64_t pc = valid ? p : Pn - 1;
    const float x0 = a.pts[pc * 3 + 0], x1 = a.pts[pc * 3 + 1], x2 = a.pts[pc * 3 + 2];
    // identity embedding: features 0..2 of block 0 (lane group 0), zero padding elsewhere
    float4 E[4];
    E[0] = g == 0 ? make_float4(x0, x1, x2, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int b = 1; b < 4; ++b) E[b] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 X[16], Y[16];
    float4* e_l[5];
#pragma unroll
    for (int l = 0; l < 5; ++l) e_l[l] = NABLA ? escr + l * 16 * 64 : nullptr;

    // ---- forward: 5 sine layers --------------------------------------------------------------
    gemm_fwd<P, 0, 4, 16, ACT_SINE>(ws, OP(S0), OP(S1), OPB(S1), X, E, Y, e_l[0], nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_SINE>(ws, OP(S1), OP(S2), OPB(S2), Y, E, X, e_l[1], nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_SINE>(ws, OP(S2), OP(S3), OPB(S3), X, E, Y, e_l[2], nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_SINE>(ws, OP(S3), OP(S4), OPB(S4), Y, E, X, e_l[3], nullptr, false, lane);
    {
      const char* n = want_feat ? OP(SF) : (NABLA ? OP(SB4) : (has_next ? OP(S0) : nullptr));
      const int nb = want_feat ? OPB(SF) : (NABLA ? OPB(SB4) : OPB(S0));
      gemm_fwd<P, 16, 0, 16, ACT_SINE>(ws, OP(S4), n, nb, X, E, Y, e_l[4], nullptr, false, lane);
    }
    // ---- last layer row 0 = sdf (VALU dot product over h5 = Y) ----------------------------------
    float part = 0.0f;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const float4 w = *(const float4*)(wl + 16 * b + 4 * g);
      part = fmaf(Y[b].x, w.x, part);
      part = fmaf(Y[b].y, w.y, part);
      part = fmaf(Y[b].z, w.z, part);
      part = fmaf(Y[b].w, w.w, part);
    }
    const float sdf = wave_sum4(part) + bl;
    if (valid && g == 0) a.sdf[p] = sdf;
    if (want_feat) {  // rows 1..256 (X is free: only the feature stores are kept)
      const char* n = NABLA ? OP(SB4) : (has_next ? OP(S0) : nullptr);
      const int nb = NABLA ? OPB(SB4) : OPB(S0);
      gemm_fwd<P, 16, 0, 16, ACT_NONE>(ws, OP(SF), n, nb, Y, E, X, nullptr, a.feature + pc * 256, valid, lane);
    }
    if constexpr (NABLA) {
      // d sdf / d z4 = W5[0, :] * 30 cos(30 z4)
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const float4 w = *(const float4*)(wl + 16 * b + 4 * g);
        const float4 e = e_l[4][b * 64 + lane];
        X[b] = make_float4(sine_bwd(w.x, e.x), sine_bwd(w.y, e.y), sine_bwd(w.z, e.z), sine_bwd(w.w, e.w));
      }
      auto noemb = [](int, float4) {};
      // d sdf / d x: features 0..2 of block 0 (lane group 0) of W0^T g
      auto coords = [&](int eb, float4 gv) {
        if (eb == 0 && g == 0 && valid) {
          a.nabla[p * 3 + 0] = gv.x;
          a.nabla[p * 3 + 1] = gv.y;
          a.nabla[p * 3 + 2] = gv.z;
        }
      };
      ws.slab_now(e_l[3], 0);
      gemm_bwd<P, 16, 16, 0, ACT_SINE>(ws, OP(SB4), OP(SB3), OPB(SB3), X, Y, e_l[3], e_l[2], lane, noemb);
      gemm_bwd<P, 16, 16, 0, ACT_SINE>(ws, OP(SB3), OP(SB2), OPB(SB2), Y, X, e_l[2], e_l[1], lane, noemb);
      gemm_bwd<P, 16, 16, 0, ACT_SINE>(ws, OP(SB2), OP(SB1), OPB(SB1), X, Y, e_l[1], e_l[0], lane, noemb);
      gemm_bwd<P, 16, 16, 0, ACT_SINE>(ws, OP(SB1), OP(SB0), OPB(SB0), Y, X, e_l[0], nullptr, lane, noemb);
      gemm_bwd<P, 16, 0, 4, ACT_SINE>(ws, OP(SB0), has_next ? OP(S0) : nullptr, OPB(S0), X, Y, nullptr, nullptr,
                                      lane, coords);
    }
  }
  wait_vmcnt(0);  // a block without tiles still has the prologue's second chunk in flight
}

// =============================================================================================
// Radiance kernel (RadianceNet): cat([x, embed_view(v), normals, feature]) -> D x ReLU(256) -> 3
// (D = 4), or D = 5 SirenLayers sin(30 z) (base.py:357-361, configs/volsdf_siren.yaml)
// =============================================================================================
struct RadKArgs {
  const char* packed;
  RadLayout L;
  const float* x;
  const float* vdir;
  int64_t vdiv;
  int64_t vmod;
  const float* normals;
  const float* feature;
  int64_t P;
  float* rgb;
  int nfreq_view;  // <0: identity
  const int* P_dev;  // optional device count: the first min(P, *P_dev) points are evaluated
  const char* r0_fold;  // rad4_kernel<KBS, true>: the fold pack's R0' (then `feature` holds u), or null
};
// ... of rad4_kernel<KBS, true>, the render's instances, which can claim their tiles
struct RadKArgsC : RadKArgs {
  int* claim;  // tile claim counter (nr_mlp.h), or null
};

// small input features [x(3), view-embedding(3+6F or 3), normals(3)] in block layout ([x(3)] only
// without view dirs)
__device__ __forceinline__ float rad_small_feature(int f, const float (&x)[3], const float (&v)[3],
                                                   const float (&n)[3], int nfreq_view, bool view) {
  if (f < 3) return x[f];
  if (!view) return 0.0f;
  f -= 3;
  const int nv = nfreq_view < 0 ? 3 : 3 + 6 * nfreq_view;
  if (f < nv) return embed_feature(f, v[0], v[1], v[2], nfreq_view < 0 ? 0 : nfreq_view);
  f -= nv;
  if (f < 3) return n[f];
  return 0.0f;
}

template <int P, int KBS, int ACT, int D>
__global__ __launch_bounds__(kThreads) void radiance_kernel(RadKArgs a) {
  static_assert(D == 4 || D == 5, "radiance net depth");
  constexpr int CB = chunk_bytes(16 + KBS);
  __shared__ __attribute__((aligned(16))) char smem[kRing * CB];
  WStream<CB> ws{smem, nullptr, 0, 0, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const RadLayout& L = a.L;
  const char* W = a.packed;
  auto OP = [&](int i) { return W + L.op_off[i]; };
  auto OPB = [&](int i) { return (int)L.op_bytes[i]; };
  const float* head = (const float*)(W + L.head_off);  // [3][256] weights then [3] bias
  const bool view = L.view != 0;

  ws.start(OP(0), OPB(0), OP(0) + OPB(0), OPB(0));
  const int64_t Pn = a.P_dev ? min(a.P, (int64_t)*a.P_dev) : a.P;
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < Pn; base += (int64_t)gridDim.x * kPointsPerWG) {
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < Pn;
    const int64_t p = base + wave * kTile + j;
    const bool valid = p < Pn;
    const int64_t pc = valid ? p : Pn - 1;
    float xs[3], vs[3] = {0.f, 0.f, 0.f}, ns[3] = {0.f, 0.f, 0.f};
    const int64_t pv = (pc / a.vdiv) % a.vmod;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xs[c] = a.x[pc * 3 + c];
      if (view) {
        vs[c] = a.vdir[pv * 3 + c];
        ns[c] = a.normals[pc * 3 + c];
      }
    }
    float4 S[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int f = 16 * b + 4 * g;
      S[b] = b < KBS ? make_float4(rad_small_feature(f, xs, vs, ns, a.nfreq_view, view),
                                   rad_small_feature(f + 1, xs, vs, ns, a.nfreq_view, view),
                                   rad_small_feature(f + 2, xs, vs, ns, a.nfreq_view, view),
                                   rad_small_feature(f + 3, xs, vs, ns, a.nfreq_view, view))
                     : make_float4(0, 0, 0, 0);
    }
    float4 X[16], Y[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) X[b] = *(const float4*)(a.feature + pc * 256 + 16 * b + 4 * g);

    gemm_fwd<P, 16, KBS, 16, ACT>(ws, OP(0), OP(1), OPB(1), X, S, Y, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT>(ws, OP(1), OP(2), OPB(2), Y, S, X, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT>(ws, OP(2), OP(3), OPB(3), X, S, Y, nullptr, nullptr, false, lane);
    if constexpr (D == 4) {
      gemm_fwd<P, 16, 0, 16, ACT>(ws, OP(3), has_next ? OP(0) : nullptr, OPB(0), Y, S, X, nullptr, nullptr, false,
                                  lane);
    } else {
      gemm_fwd<P, 16, 0, 16, ACT>(ws, OP(3), OP(4), OPB(4), Y, S, X, nullptr, nullptr, false, lane);
      gemm_fwd<P, 16, 0, 16, ACT>(ws, OP(4), has_next ? OP(0) : nullptr, OPB(0), X, S, Y, nullptr, nullptr, false,
                                  lane);
    }
    const float4(&H)[16] = D == 4 ? X : Y;  // last hidden layer
    // head: Linear(256 -> 3) + sigmoid  (VALU dot products)
    float r[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float part = 0.f;
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const float4 w = *(const float4*)(head + o * 256 + 16 * b + 4 * g);
        part = fmaf(H[b].x, w.x, part);
        part = fmaf(H[b].y, w.y, part);
        part = fmaf(H[b].z, w.z, part);
        part = fmaf(H[b].w, w.w, part);
      }
      r[o] = sigmoidf_ref(wave_sum4(part) + head[3 * 256 + o]);
    }
    if (valid && g == 0) {
      a.rgb[p * 3 + 0] = r[0];
      a.rgb[p * 3 + 1] = r[1];
      a.rgb[p * 3 + 2] = r[2];
    }
  }
  wait_vmcnt(0);
}

// =============================================================================================
// Training forward of the ReLU radiance net with exact fp32 products (RadianceTG.forward,
// base.py:372-391 with a graph): the fp32 render kernel's layer chain (radiance_kernel<FP32>: the
// activations stay in registers from layer to layer, v_mfma_f32_16x16x4_f32 over an fp32 pack) with
// every hidden activation h_l stored ([P, 256] row-major, after the ReLU) for the backward, the small
// inputs read from the training input tensor (nr_radiance_input's [x, embed_view(v), normals] columns,
// the same values the backward's weight gradient of layer 0 reads) and the feature from its own
// [P, 256] tensor; rgb = sigmoid(head).  The ReLU masks come from fp32 pre-activations as in the
// reference (an f16x3 z flips a few masks per step); one launch replaces the four
// hipBLASLt GEMMs, their ReLU launches and the head.
// =============================================================================================
struct RadTrainArgs {
  const char* packed;
  RadLayout L;
  const float* feat;   // [P][256]
  const float* small;  // small[p * ld_small + f], f < n_small
  int64_t ld_small;
  int n_small;
  int64_t P;
  float* h[4];         // [P][256] each
  float* rgb;          // [P][3]
};

template <int KBS>
__global__ __launch_bounds__(kThreads) void radiance_train32_kernel(RadTrainArgs a) {
  constexpr int CB = chunk_bytes(16 + KBS);
  __shared__ __attribute__((aligned(16))) char smem[kRing * CB];
  WStream<CB> ws{smem, nullptr, 0, 0, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const RadLayout& L = a.L;
  const char* W = a.packed;
  auto OP = [&](int i) { return W + L.op_off[i]; };
  auto OPB = [&](int i) { return (int)L.op_bytes[i]; };
  const float* head = (const float*)(W + L.head_off);  // [3][256] weights then [3] bias

  ws.start(OP(0), OPB(0), OP(0) + OPB(0), OPB(0));
  const int64_t Pn = a.P;
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < Pn; base += (int64_t)gridDim.x * kPointsPerWG) {
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < Pn;
    const int64_t p = base + wave * kTile + j;
    const bool valid = p < Pn;
    const int64_t pc = valid ? p : Pn - 1;
    float4 S[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * b + 4 * g + r;
        v[r] = (b < KBS && f < a.n_small) ? a.small[pc * a.ld_small + f] : 0.0f;
      }
      S[b] = make_float4(v[0], v[1], v[2], v[3]);
    }
    float4 X[16], Y[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) X[b] = *(const float4*)(a.feat + pc * 256 + 16 * b + 4 * g);
    auto store = [&](int l, const float4 (&H)[16]) {
      if (!valid) return;
      float* h = a.h[l] + p * 256 + 4 * g;
#pragma unroll
      for (int b = 0; b < 16; ++b) *(float4*)(h + 16 * b) = H[b];
    };
    gemm_fwd<NR_PREC_FP32, 16, KBS, 16, ACT_RELU>(ws, OP(0), OP(1), OPB(1), X, S, Y, nullptr, nullptr, false, lane);
    store(0, Y);
    gemm_fwd<NR_PREC_FP32, 16, 0, 16, ACT_RELU>(ws, OP(1), OP(2), OPB(2), Y, S, X, nullptr, nullptr, false, lane);
    store(1, X);
    gemm_fwd<NR_PREC_FP32, 16, 0, 16, ACT_RELU>(ws, OP(2), OP(3), OPB(3), X, S, Y, nullptr, nullptr, false, lane);
    store(2, Y);
    gemm_fwd<NR_PREC_FP32, 16, 0, 16, ACT_RELU>(ws, OP(3), has_next ? OP(0) : nullptr, OPB(0), Y, S, X, nullptr,
                                                nullptr, false, lane);
    store(3, X);
    // head: Linear(256 -> 3) + sigmoid (VALU dot products, as radiance_kernel)
    float r[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float part = 0.f;
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const float4 w = *(const float4*)(head + o * 256 + 16 * b + 4 * g);
        part = fmaf(X[b].x, w.x, part);
        part = fmaf(X[b].y, w.y, part);
        part = fmaf(X[b].z, w.z, part);
        part = fmaf(X[b].w, w.w, part);
      }
      r[o] = sigmoidf_ref(wave_sum4(part) + head[3 * 256 + o]);
    }
    if (valid && g == 0) {
      a.rgb[p * 3 + 0] = r[0];
      a.rgb[p * 3 + 1] = r[1];
      a.rgb[p * 3 + 2] = r[2];
    }
  }
  wait_vmcnt(0);
}

// =============================================================================================
// Radiance net on the v3 pipeline (rad4_kernel, f16x3, ReLU, D = 4): the sdf4_kernel structure
// (128-point tile, kNC-column waves, weight ring by LDS-DMA two chunks ahead, per-chunk operand
// split at a scale fixed from the op's pack-time bound, epilogue staged beside the next chunk's
// MFMAs) on cat([feature, x, embed_view(v), normals]) -> 3 x ReLU(256) -> ReLU(256) -> 3, with the
// Linear(256 -> 3) + sigmoid head folded into the last hidden op's epilogue as three running dot
// products (the lane's 8 outputs of each chunk; summed in the old kernel's order: block by block,
// then over the 4 lane groups).
// =============================================================================================
// ReLU op: out -> next operand (k-step c of oh/ol)
struct ReluEpi4 {
  f16x8 (&oh)[kNC][12];
  f16x8 (&ol)[kNC][12];
  const float (&sc)[kNC];
  float (&mrun)[kNC];
  float4 y[kNC][2];
  __device__ __forceinline__ void operator()(int c, const Z4& zz, int st) {
    const int q = st >> 2, k = st & 3;  // stages 4q..4q+3: column q
    if (q >= kNC) return;
    if (k < 2) {
      const float4 z = zz.z[q][k];
      y[q][k] = make_float4(fmaxf(z.x, 0.0f), fmaxf(z.y, 0.0f), fmaxf(z.z, 0.0f), fmaxf(z.w, 0.0f));
    } else if (k == 2) {
      mrun[q] = amax8(mrun[q], y[q][0], y[q][1]);
    } else {
      split8a(y[q][0], y[q][1], sc[q], oh[q][c], ol[q][c]);
    }
  }
};

// last hidden op: ReLU, then part[q][o] += sum_r y * head[o][row] over the lane's rows of the chunk
// (head [3][256] staged in LDS)
struct HeadEpi4 {
  const float* head;  // LDS
  float (&part)[kNC][3];
  int g;
  float4 y[kNC][2];
  __device__ __forceinline__ void operator()(int c, const Z4& zz, int st) {
    const int q = st >> 2, k = st & 3;
    if (q >= kNC) return;
    if (k < 2) {
      const float4 z = zz.z[q][k];
      y[q][k] = make_float4(fmaxf(z.x, 0.0f), fmaxf(z.y, 0.0f), fmaxf(z.z, 0.0f), fmaxf(z.w, 0.0f));
    } else {  // rows 0 (stage 2), 1 and 2 (stage 3)
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        if ((o == 0) != (k == 2)) continue;
        float p = part[q][o];
        // opaque lane offset: a hoisted address per (chunk, row, block) would pin 48 registers
        const uint32_t lo = opaque_lane(4 * g);
#pragma unroll
        for (int b = 0; b < 2; ++b) {  // block 2c + b, rows 16 (2c + b) + 4 g + r
          const float4 w = *(const float4*)(head + lo + o * 256 + 16 * (2 * c + b));
          p = fmaf(y[q][b].x, w.x, p);
          p = fmaf(y[q][b].y, w.y, p);
          p = fmaf(y[q][b].z, w.z, p);
          p = fmaf(y[q][b].w, w.w, p);
        }
        asm volatile("" : "+v"(p));  // computed here: sunk to the op's end, every chunk's y would stay live
        part[q][o] = p;
      }
    }
  }
};

// FOLD (NeuS render, nr_neus_fold_pack): a.feature holds u = (W0f W8f) h7 + (W0f b8f + b0), the
// geometry feature's share of layer 0 with its bias, written by sdf4_kernel's F8'.  Op 0 is R0'
// (a.r0_fold) over the small inputs alone, and u, kept in fp32 registers, is added in its epilogue.
struct FoldEpi4 {
  f16x8 (&oh)[kNC][12];
  f16x8 (&ol)[kNC][12];
  const float (&sc)[kNC];
  float (&mrun)[kNC];
  const float4 (&u)[kNC][16];
  float4 y[kNC][2];
  __device__ __forceinline__ void operator()(int c, const Z4& zz, int st) {
    const int q = st >> 2, k = st & 3;
    if (q >= kNC) return;
    if (k < 2) {
      const float4 z = zz.z[q][k], v = u[q][2 * c + k];
      y[q][k] = make_float4(fmaxf(z.x + v.x, 0.0f), fmaxf(z.y + v.y, 0.0f), fmaxf(z.z + v.z, 0.0f),
                            fmaxf(z.w + v.w, 0.0f));
    } else if (k == 2) {
      mrun[q] = amax8(mrun[q], y[q][0], y[q][1]);
    } else {
      split8a(y[q][0], y[q][1], sc[q], oh[q][c], ol[q][c]);
    }
  }
};

template <int KBS, bool FOLD>
__global__ __attribute__((amdgpu_flat_work_group_size(kT4, kT4), amdgpu_waves_per_eu(kWPE, kWPE)))
void rad4_kernel(std::conditional_t<FOLD, RadKArgsC, RadKArgs> a) {
  constexpr int KF = FOLD ? 0 : 16;  // op 0's input blocks: feature (16 unless folded), then the small inputs
  constexpr int K0 = KF + KBS;
  constexpr int C0 = chunk_bytes(K0), C16 = chunk_bytes(16);
  constexpr int CM = C0 > C16 ? C0 : C16;  // the ring's slot
  constexpr bool CLAIM = FOLD;  // tile claims (nr_mlp.h, a.claim): the render instances; the others keep their code
  __shared__ __attribute__((aligned(16))) char smem[kRing * CM + (3 * 256 + 4) * 4 + (CLAIM ? 16 : 0)];
  static_assert(kRing * CM + (3 * 256 + 4) * 4 + (CLAIM ? 16 : 0) <= 160 * 1024, "LDS budget");
  WStream4<CM> ws{smem, nullptr, 0, 0, 0};
  float* head = (float*)(smem + kRing * CM);  // [3][256] weights, then [3] bias
  int* const claim_lds = (int*)(head + 3 * 256 + 4);  // the claimed tile index (a.claim, as in sdf4_kernel)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const RadLayout& L = a.L;
  const char* W = a.packed;
  auto OP = [&](int i) {
    const char* w = FOLD && i == 0 ? a.r0_fold : W;
    asm volatile("" : "+s"(w));
    return FOLD && i == 0 ? w : w + L.op_off[i];
  };
  const bool view = L.view != 0;
  {
    const float* hsrc = (const float*)(W + L.head_off);
    for (int i = threadIdx.x; i < 3 * 256 + 4; i += kT4) head[i] = hsrc[i];
  }
  ws.template start<C0, C0>(OP(0), OP(0) + C0);  // its barrier also publishes the head
  Pend4 pd{};
  NoPre4 nopre;
  const int64_t Pn = a.P_dev ? min(a.P, (int64_t)*a.P_dev) : a.P;
  int* claim = nullptr;  // the counter; stays null in the instances that cannot claim (no new code there)
  if constexpr (CLAIM) claim = a.claim;
  int64_t next = 0;  // the next tile's first point (claimed)
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < Pn;
       base = claim ? next : base + (int64_t)gridDim.x * kPointsPerWG) {
    bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < Pn;
    // thread 0 draws the next tile ahead of the point loads and leaves it in LDS behind them; every wave
    // reads it before the last op, with the three ops' chunk barriers in between
    int claimed = 0;
    if (claim && threadIdx.x == 0) claimed = atomicAdd(claim, 1);
    const int64_t p0 = base + wave * 16 * kNC;
    f16x8 Uh[kNC][12], Ul[kNC][12], Vh[kNC][12], Vl[kNC][12];
    float m_in[kNC], xinv[kNC], mrun[kNC];
    float4 ufold[kNC][FOLD ? 16 : 1];  // FOLD: the point's u, rows 16 b + 4 g .. + 3 (the accumulator layout)
    float umax[kNC];                   // ... and its max |u| over the point's 256 rows
    bool valid[kNC];
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      const int64_t p = p0 + 16 * q + j;
      valid[q] = p < Pn;
      const int64_t pc = valid[q] ? p : Pn - 1;
      const int64_t pv = (pc / a.vdiv) % a.vmod;
      float xs[3], vs[3] = {0.f, 0.f, 0.f}, ns[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        xs[c] = a.x[pc * 3 + c];
        if (view) {
          vs[c] = a.vdir[pv * 3 + c];
          ns[c] = a.normals[pc * 3 + c];
        }
      }
      // the small inputs first: their embedding calls then see few live registers
      float4 X[K0];
      const int gq = (int)opaque_lane(g);  // not hoistable: the 4 KBS feature indices' tests stay in the tile
#pragma unroll
      for (int b = 0; b < KBS; ++b) {
        const int f = 16 * b + 4 * gq;
        X[KF + b] = make_float4(rad_small_feature(f, xs, vs, ns, a.nfreq_view, view),
                                rad_small_feature(f + 1, xs, vs, ns, a.nfreq_view, view),
                                rad_small_feature(f + 2, xs, vs, ns, a.nfreq_view, view),
                                rad_small_feature(f + 3, xs, vs, ns, a.nfreq_view, view));
      }
      if constexpr (FOLD) {
#pragma unroll
        for (int b = 0; b < 16; ++b) ufold[q][b] = *(const float4*)(a.feature + pc * 256 + 16 * b + 4 * g);
        float mu = 0.0f;
#pragma unroll
        for (int b = 0; b < 16; b += 2) mu = amax8(mu, ufold[q][b], ufold[q][b + 1]);
        umax[q] = max4_groups(mu);
      } else {
#pragma unroll
        for (int b = 0; b < 16; ++b) X[b] = *(const float4*)(a.feature + pc * 256 + 16 * b + 4 * g);
        umax[q] = 0.0f;
      }
      float m = 0.0f;
#pragma unroll
      for (int b = 0; b < K0; b += 2) m = amax8(m, X[b], X[b + 1]);
      m_in[q] = max4_groups(m);
      const float s = bound_scale(m_in[q]);  // exact-max scale of op 0's operand
#pragma unroll
      for (int k = 0; k < K0 / 2; ++k) split8a(X[2 * k], X[2 * k + 1], s, Uh[q][k], Ul[q][k]);
      xinv[q] = 1.0f / s;
      mrun[q] = 0.0f;
    }
    if (claim && threadIdx.x == 0) *claim_lds = claimed;
    auto next_scales = [&](int kb, float (&sc)[kNC]) {
      const float4 v = ws.buf()[2 * kb * 64 + 8];
#pragma unroll
      for (int q = 0; q < kNC; ++q) sc[q] = bound_scale(fmaf(v.y, m_in[q], v.z));
    };
    auto finish = [&](const float (&sc)[kNC]) {
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        m_in[q] = max4_groups(mrun[q]);
        mrun[q] = 0.0f;
        xinv[q] = 1.0f / sc[q];
      }
    };
    {
      float sc[kNC];
      if constexpr (FOLD) {  // |z + u| <= R m_small + B + max |u| (R0's bias is zero: b0 rides in u)
        const float4 v = ws.buf()[2 * K0 * 64 + 8];
#pragma unroll
        for (int q = 0; q < kNC; ++q) sc[q] = bound_scale(fmaf(v.y, m_in[q], v.z) + umax[q]);
        op4<K0, 16, C16, false, false>(ws, OP(0), OP(1), Uh, Ul, xinv, pd, nopre,
                                       FoldEpi4{Vh, Vl, sc, mrun, ufold}, lane);
      } else {
        next_scales(K0, sc);
        op4<K0, 16, C16, false, false>(ws, OP(0), OP(1), Uh, Ul, xinv, pd, nopre, ReluEpi4{Vh, Vl, sc, mrun}, lane);
      }
      finish(sc);
    }
    {
      float sc[kNC];
      next_scales(16, sc);
      op4<16, 16, C16, false, false>(ws, OP(1), OP(2), Vh, Vl, xinv, pd, nopre, ReluEpi4{Uh, Ul, sc, mrun}, lane);
      finish(sc);
    }
    {
      float sc[kNC];
      next_scales(16, sc);
      op4<16, 16, C16, false, false>(ws, OP(2), OP(3), Uh, Ul, xinv, pd, nopre, ReluEpi4{Vh, Vl, sc, mrun}, lane);
      finish(sc);
    }
    float part[kNC][3];
#pragma unroll
    for (int q = 0; q < kNC; ++q) part[q][0] = part[q][1] = part[q][2] = 0.0f;
    if (claim) {
      next = (int64_t)(gridDim.x + __builtin_amdgcn_readfirstlane(*claim_lds)) * kPointsPerWG;
      has_next = next < Pn;
    }
    op4<16, 16, C0, false, false>(ws, OP(3), has_next ? OP(0) : nullptr, Vh, Vl, xinv, pd, nopre,
                                  HeadEpi4{head, part, g}, lane);
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      float r[3];
#pragma unroll
      for (int o = 0; o < 3; ++o) r[o] = sigmoidf_ref(wave_sum4(part[q][o]) + head[3 * 256 + o]);
      if (valid[q] && g == 0) {
        const int64_t p = p0 + 16 * q + j;
        a.rgb[p * 3 + 0] = r[0];
        a.rgb[p * 3 + 1] = r[1];
        a.rgb[p * 3 + 2] = r[2];
      }
    }
  }
  pd.flush();
  wait_vmcnt(0);  // a block without tiles still has the prologue's second chunk in flight
}

// =============================================================================================
// NeRF++ background kernel (models/base.py:395-453, use_view_dirs=True, multires 10 on the 4-D
// inverted-sphere input [x/r, 1/r], multires_view 4).  Plain nn.Linear layers, ReLU.
// =============================================================================================
struct NerfKArgs {
  const char* packed;
  NerfLayout L;
  const float* x4;    // [P][4]
  const float* vdir;  // view direction of point p: vdir[((p / vdiv) % vmod) * 3]
  int64_t vdiv;
  int64_t vmod;
  int64_t P;
  float* sigma;       // [P]
  float* rgb;         // [P][3]
  const int* P_dev;   // optional device count: the first min(P, *P_dev) points are evaluated
};

// Embedder(input_dim=4, multires=10): [x, sin(x 2^0), cos(x 2^0), ..., sin(x 2^9), cos(x 2^9)]
__device__ __noinline__ float nerf_embed4(int f, float x0, float x1, float x2, float x3) {
  auto comp = [&](int c) { return c == 0 ? x0 : (c == 1 ? x1 : (c == 2 ? x2 : x3)); };
  if (f < 4) return comp(f);
  const int fp = f - 4;
  if (fp >= 80) return 0.0f;
  const int band = fp >> 3, m = fp & 7;
  const float v = fmul(comp(m & 3), (float)(1 << band));
  return m < 4 ? sinf(v) : cosf(v);
}

template <int P>
__global__ __launch_bounds__(kThreads) void nerf_kernel(NerfKArgs a) {
  constexpr int CB = chunk_bytes(22);  // N5: 16 + 6 input blocks
  __shared__ __attribute__((aligned(16))) char smem[kRing * CB];
  WStream<CB> ws{smem, nullptr, 0, 0, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const NerfLayout& L = a.L;
  const char* W = a.packed;
  auto OP = [&](int i) { return W + L.op_off[i]; };
  auto OPB = [&](int i) { return (int)L.op_bytes[i]; };
  const float* wa = (const float*)(W + L.alpha_off);
  const float* wr = (const float*)(W + L.rgb_off);

  ws.start(OP(N0), OPB(N0), OP(N0) + OPB(N0), OPB(N0));
  const int64_t Pn = a.P_dev ? min(a.P, (int64_t)*a.P_dev) : a.P;
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < Pn; base += (int64_t)gridDim.x * kPointsPerWG) {
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < Pn;
    const int64_t p = base + wave * kTile + j;
    const bool valid = p < Pn;
    const int64_t pc = valid ? p : Pn - 1;
    const float4 xin = *(const float4*)(a.x4 + pc * 4);
    const int64_t pv = (pc / a.vdiv) % a.vmod;
    const float v0 = a.vdir[pv * 3 + 0], v1 = a.vdir[pv * 3 + 1], v2 = a.vdir[pv * 3 + 2];
    float4 E[6], V[2];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      const int f = 16 * b + 4 * g;
      E[b] = make_float4(nerf_embed4(f + 0, xin.x, xin.y, xin.z, xin.w), nerf_embed4(f + 1, xin.x, xin.y, xin.z, xin.w),
                         nerf_embed4(f + 2, xin.x, xin.y, xin.z, xin.w), nerf_embed4(f + 3, xin.x, xin.y, xin.z, xin.w));
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int f = 16 * b + 4 * g;
      V[b] = make_float4(f + 0 < 27 ? embed_feature(f + 0, v0, v1, v2, 4) : 0.0f,
                         f + 1 < 27 ? embed_feature(f + 1, v0, v1, v2, 4) : 0.0f,
                         f + 2 < 27 ? embed_feature(f + 2, v0, v1, v2, 4) : 0.0f,
                         f + 3 < 27 ? embed_feature(f + 3, v0, v1, v2, 4) : 0.0f);
    }
    float4 X[16], Y[16];
    gemm_fwd<P, 0, 6, 16, ACT_RELU>(ws, OP(N0), OP(N1), OPB(N1), X, E, Y, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_RELU>(ws, OP(N1), OP(N2), OPB(N2), Y, E, X, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_RELU>(ws, OP(N2), OP(N3), OPB(N3), X, E, Y, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_RELU>(ws, OP(N3), OP(N4), OPB(N4), Y, E, X, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_RELU>(ws, OP(N4), OP(N5), OPB(N5), X, E, Y, nullptr, nullptr, false, lane);
    // skip: cat([input_pts, h]) (base.py:431-432); K blocks packed as [h ; embedding]
    gemm_fwd<P, 16, 6, 16, ACT_RELU>(ws, OP(N5), OP(N6), OPB(N6), Y, E, X, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_RELU>(ws, OP(N6), OP(N7), OPB(N7), X, E, Y, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 0, 16, ACT_RELU>(ws, OP(N7), OP(NF), OPB(NF), Y, E, X, nullptr, nullptr, false, lane);
    // sigma = alpha_linear(h) (no activation)
    float part = 0.f;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const float4 w = *(const float4*)(wa + 16 * b + 4 * g);
      part = fmaf(X[b].x, w.x, part);
      part = fmaf(X[b].y, w.y, part);
      part = fmaf(X[b].z, w.z, part);
      part = fmaf(X[b].w, w.w, part);
    }
    const float sigma = wave_sum4(part) + wa[256];
    // feature = feature_linear(h); h = relu(views_linears[0](cat([feature, embed_view(v)])))
    gemm_fwd<P, 16, 0, 16, ACT_NONE>(ws, OP(NF), OP(NV), OPB(NV), X, E, Y, nullptr, nullptr, false, lane);
    gemm_fwd<P, 16, 2, 8, ACT_RELU>(ws, OP(NV), has_next ? OP(N0) : nullptr, OPB(N0), Y, V, X, nullptr, nullptr,
                                    false, lane);
    float r[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float q = 0.f;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const float4 w = *(const float4*)(wr + o * 128 + 16 * b + 4 * g);
        q = fmaf(X[b].x, w.x, q);
        q = fmaf(X[b].y, w.y, q);
        q = fmaf(X[b].z, w.z, q);
        q = fmaf(X[b].w, w.w, q);
      }
      r[o] = sigmoidf_ref(wave_sum4(q) + wr[3 * 128 + o]);
    }
    if (valid && g == 0) {
      a.sigma[p] = sigma;
      a.rgb[p * 3 + 0] = r[0];
      a.rgb[p * 3 + 1] = r[1];
      a.rgb[p * 3 + 2] = r[2];
    }
  }
  wait_vmcnt(0);
}

// =============================================================================================
// NeRF++ background net in the training step (NeRFFn, models/base.py:426-453 with a graph), exact fp32
// products on v_mfma_f32_16x16x4_f32, the layer chain in registers (nerf_kernel<FP32>'s structure):
// * nerf_train32_fwd_kernel, over the fp32 render pack (nerf_layout): the embedded inputs read from the
//   training tensors (x_emb [P,84], v_emb [P,27], nr_nerf_train_input), every tensor the backward needs
//   stored -- the 8 ReLU outputs h_i [P,256], the feature [P,256], the view branch's ReLU output hv
//   [P,128] -- plus sigma [P] and rgb [P,3].  The ReLU decisions come from fp32 pre-activations, as the
//   reference's (the radiance net's note).
// * nerf_train32_bwd_kernel, over the training pack (nerf_bwd_layout: transposed ops): the data
//   gradients in one launch -- g3 = g_rgb sigmoid'(rgb) [P,3]; ghv = (g3 Wr) [hv > 0] [P,128];
//   g_feat = Wv[:, :256]^T ghv [P,256] (the view embedding takes no gradient); gz7 = (Wf^T g_feat +
//   g_sigma Wa) [h7 > 0]; gz_{i-1} = (W_i^T gz_i) [h_{i-1} > 0] for i = 7..1, W5^T restricted to the
//   h columns 84..339 of its input cat([x_emb, h4]) (base.py:431-432).  Each gz is stored for the
//   weight gradients (nr_wgrad).
// One launch each replaces 12 hipBLASLt GEMMs + 3 activation launches (forward) and 11 GEMMs + 10
// activation launches (backward).
// =============================================================================================
struct NerfTrainFwdArgs {
  const char* packed;
  NerfLayout L;
  const float* xe;  // [P][84]
  const float* ve;  // [P][27]
  int64_t P;
  float* h[8];      // [P][256]
  float* feat;      // [P][256]
  float* hv;        // [P][128]
  float* sigma;     // [P]
  float* rgb;       // [P][3]
};

__global__ __launch_bounds__(kThreads) void nerf_train32_fwd_kernel(NerfTrainFwdArgs a) {
  constexpr int CB = chunk_bytes(22);  // N5: 16 + 6 input blocks
  __shared__ __attribute__((aligned(16))) char smem[kRing * CB];
  WStream<CB> ws{smem, nullptr, 0, 0, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const NerfLayout& L = a.L;
  const char* W = a.packed;
  auto OP = [&](int i) { return W + L.op_off[i]; };
  auto OPB = [&](int i) { return (int)L.op_bytes[i]; };
  const float* wa = (const float*)(W + L.alpha_off);
  const float* wr = (const float*)(W + L.rgb_off);
  constexpr int F32 = NR_PREC_FP32;

  ws.start(OP(N0), OPB(N0), OP(N0) + OPB(N0), OPB(N0));
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < a.P; base += (int64_t)gridDim.x * kPointsPerWG) {
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < a.P;
    const int64_t p = base + wave * kTile + j;
    const bool valid = p < a.P;
    const int64_t pc = valid ? p : a.P - 1;
    float4 E[6], V[2];
#pragma unroll
    for (int b = 0; b < 6; ++b) {  // 84 = 21 float4s: feature f < 84 covers f .. f + 3
      const int f = 16 * b + 4 * g;
      E[b] = f < 84 ? *(const float4*)(a.xe + pc * 84 + f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int f = 16 * b + 4 * g;
      const float* v = a.ve + pc * 27;
      V[b] = make_float4(f + 0 < 27 ? v[f + 0] : 0.f, f + 1 < 27 ? v[f + 1] : 0.f, f + 2 < 27 ? v[f + 2] : 0.f,
                         f + 3 < 27 ? v[f + 3] : 0.f);
    }
    auto store = [&](float* dst, const float4 (&H)[16]) {  // [P][256] row p
      if (!valid) return;
      float* h = dst + p * 256 + 4 * g;
#pragma unroll
      for (int b = 0; b < 16; ++b) *(float4*)(h + 16 * b) = H[b];
    };
    float4 X[16], Y[16];
    gemm_fwd<F32, 0, 6, 16, ACT_RELU>(ws, OP(N0), OP(N1), OPB(N1), X, E, Y, nullptr, nullptr, false, lane);
    store(a.h[0], Y);
    gemm_fwd<F32, 16, 0, 16, ACT_RELU>(ws, OP(N1), OP(N2), OPB(N2), Y, E, X, nullptr, nullptr, false, lane);
    store(a.h[1], X);
    gemm_fwd<F32, 16, 0, 16, ACT_RELU>(ws, OP(N2), OP(N3), OPB(N3), X, E, Y, nullptr, nullptr, false, lane);
    store(a.h[2], Y);
    gemm_fwd<F32, 16, 0, 16, ACT_RELU>(ws, OP(N3), OP(N4), OPB(N4), Y, E, X, nullptr, nullptr, false, lane);
    store(a.h[3], X);
    gemm_fwd<F32, 16, 0, 16, ACT_RELU>(ws, OP(N4), OP(N5), OPB(N5), X, E, Y, nullptr, nullptr, false, lane);
    store(a.h[4], Y);
    // skip: cat([input_pts, h]) (base.py:431-432); K blocks packed as [h ; embedding]
    gemm_fwd<F32, 16, 6, 16, ACT_RELU>(ws, OP(N5), OP(N6), OPB(N6), Y, E, X, nullptr, nullptr, false, lane);
    store(a.h[5], X);
    gemm_fwd<F32, 16, 0, 16, ACT_RELU>(ws, OP(N6), OP(N7), OPB(N7), X, E, Y, nullptr, nullptr, false, lane);
    store(a.h[6], Y);
    gemm_fwd<F32, 16, 0, 16, ACT_RELU>(ws, OP(N7), OP(NF), OPB(NF), Y, E, X, nullptr, nullptr, false, lane);
    store(a.h[7], X);
    float part = 0.f;  // sigma = alpha_linear(h7)
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const float4 w = *(const float4*)(wa + 16 * b + 4 * g);
      part = fmaf(X[b].x, w.x, part);
      part = fmaf(X[b].y, w.y, part);
      part = fmaf(X[b].z, w.z, part);
      part = fmaf(X[b].w, w.w, part);
    }
    const float sigma = wave_sum4(part) + wa[256];
    // feature = feature_linear(h7), stored by the op's drain; hv = relu(views_linears[0](cat([feature, v])))
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NF), OP(NV), OPB(NV), X, E, Y, nullptr, a.feat + p * 256, valid, lane);
    gemm_fwd<F32, 16, 2, 8, ACT_RELU>(ws, OP(NV), has_next ? OP(N0) : nullptr, OPB(N0), Y, V, X, nullptr, nullptr,
                                      false, lane);
    if (valid) {
      float* hv = a.hv + p * 128 + 4 * g;
#pragma unroll
      for (int b = 0; b < 8; ++b) *(float4*)(hv + 16 * b) = X[b];
    }
    float r[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float q = 0.f;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const float4 w = *(const float4*)(wr + o * 128 + 16 * b + 4 * g);
        q = fmaf(X[b].x, w.x, q);
        q = fmaf(X[b].y, w.y, q);
        q = fmaf(X[b].z, w.z, q);
        q = fmaf(X[b].w, w.w, q);
      }
      r[o] = sigmoidf_ref(wave_sum4(q) + wr[3 * 128 + o]);
    }
    if (valid && g == 0) {
      a.sigma[p] = sigma;
      a.rgb[p * 3 + 0] = r[0];
      a.rgb[p * 3 + 1] = r[1];
      a.rgb[p * 3 + 2] = r[2];
    }
  }
  wait_vmcnt(0);
}

struct NerfTrainBwdArgs {
  const char* packed;
  NerfBwdLayout B;
  const float* rgb;      // [P][3]
  const float* hv;       // [P][128]
  const float* h[8];     // [P][256]
  const float* g_rgb;    // [P][3] or null (zero)
  const float* g_sigma;  // [P] or null (zero)
  int64_t P;
  float* g3;             // [P][3]
  float* ghv;            // [P][128]
  float* g_feat;         // [P][256]
  float* gz[8];          // [P][256]
};

template <int P>
__global__ __launch_bounds__(kThreads) void nerf_train32_bwd_kernel(NerfTrainBwdArgs a) {
  constexpr int CB = chunk_bytes(16);
  __shared__ __attribute__((aligned(16))) char smem[kRing * CB];
  WStream<CB> ws{smem, nullptr, 0, 0, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const NerfBwdLayout& L = a.B;
  const char* W = a.packed;
  auto OP = [&](int i) { return W + L.op_off[i]; };
  auto OPB = [&](int i) { return (int)L.op_bytes[i]; };
  const float* wr = (const float*)(W + L.wr_off);  // [3][128]
  const float* wa = (const float*)(W + L.wa_off);  // [256]
  constexpr int F32 = P;  // the products' precision (the name kept from the fp32-only kernel)
  const float4 E0[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};  // no second input segment

  ws.start(OP(NBV), OPB(NBV), OP(NBV) + OPB(NBV), OPB(NBV));
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < a.P; base += (int64_t)gridDim.x * kPointsPerWG) {
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < a.P;
    const int64_t p = base + wave * kTile + j;
    const bool valid = p < a.P;
    const int64_t pc = valid ? p : a.P - 1;
    // rgb = sigmoid(y): g3 = g_rgb y (1 - y) (act_kernel mode 3's arithmetic)
    float g3[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      const float y = a.rgb[pc * 3 + o];
      const float gy = a.g_rgb ? a.g_rgb[pc * 3 + o] : 0.0f;
      g3[o] = fmul(gy, fmul(y, fsub(1.0f, y)));
    }
    if (valid && g == 0) {
      a.g3[p * 3 + 0] = g3[0];
      a.g3[p * 3 + 1] = g3[1];
      a.g3[p * 3 + 2] = g3[2];
    }
    const float gs = a.g_sigma ? a.g_sigma[pc] : 0.0f;
    float4 X[16], Y[16];
    // ghv = (g3 Wr) where hv > 0 (views_linears' ReLU)
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int f = 16 * b + 4 * g;
      const float4 w0 = *(const float4*)(wr + f), w1 = *(const float4*)(wr + 128 + f),
                   w2 = *(const float4*)(wr + 256 + f);
      const float4 m = *(const float4*)(a.hv + pc * 128 + f);
      float4 v;
      v.x = m.x > 0.0f ? fmaf(g3[2], w2.x, fmaf(g3[1], w1.x, g3[0] * w0.x)) : 0.0f;
      v.y = m.y > 0.0f ? fmaf(g3[2], w2.y, fmaf(g3[1], w1.y, g3[0] * w0.y)) : 0.0f;
      v.z = m.z > 0.0f ? fmaf(g3[2], w2.z, fmaf(g3[1], w1.z, g3[0] * w0.z)) : 0.0f;
      v.w = m.w > 0.0f ? fmaf(g3[2], w2.w, fmaf(g3[1], w1.w, g3[0] * w0.w)) : 0.0f;
      X[b] = v;
      if (valid) *(float4*)(a.ghv + p * 128 + f) = v;
    }
#pragma unroll
    for (int b = 8; b < 16; ++b) X[b] = make_float4(0.f, 0.f, 0.f, 0.f);
    // (W_i^T gz)[h part] masked by h_{i-1} > 0, stored as gz_{i-1}
    auto mask_store = [&](float4 (&H)[16], const float* hprev, float* gz) {
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int f = 16 * b + 4 * g;
        const float4 m = *(const float4*)(hprev + pc * 256 + f);
        H[b] = make_float4(m.x > 0.0f ? H[b].x : 0.0f, m.y > 0.0f ? H[b].y : 0.0f, m.z > 0.0f ? H[b].z : 0.0f,
                           m.w > 0.0f ? H[b].w : 0.0f);
        if (valid) *(float4*)(gz + p * 256 + f) = H[b];
      }
    };
    // g_feat = Wv[:, :256]^T ghv, stored by the op's drain
    gemm_fwd<F32, 8, 0, 16, ACT_NONE>(ws, OP(NBV), OP(NBF), OPB(NBF), X, E0, Y, nullptr, a.g_feat + p * 256, valid,
                                      lane);
    // gz7 = (Wf^T g_feat + g_sigma Wa) where h7 > 0
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NBF), OP(NB7), OPB(NB7), Y, E0, X, nullptr, nullptr, false, lane);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const float4 w = *(const float4*)(wa + 16 * b + 4 * g);
      X[b] = make_float4(fmaf(gs, w.x, X[b].x), fmaf(gs, w.y, X[b].y), fmaf(gs, w.z, X[b].z), fmaf(gs, w.w, X[b].w));
    }
    mask_store(X, a.h[7], a.gz[7]);
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NB7), OP(NB6), OPB(NB6), X, E0, Y, nullptr, nullptr, false, lane);
    mask_store(Y, a.h[6], a.gz[6]);
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NB6), OP(NB5), OPB(NB5), Y, E0, X, nullptr, nullptr, false, lane);
    mask_store(X, a.h[5], a.gz[5]);
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NB5), OP(NB4), OPB(NB4), X, E0, Y, nullptr, nullptr, false, lane);
    mask_store(Y, a.h[4], a.gz[4]);
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NB4), OP(NB3), OPB(NB3), Y, E0, X, nullptr, nullptr, false, lane);
    mask_store(X, a.h[3], a.gz[3]);
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NB3), OP(NB2), OPB(NB2), X, E0, Y, nullptr, nullptr, false, lane);
    mask_store(Y, a.h[2], a.gz[2]);
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NB2), OP(NB1), OPB(NB1), Y, E0, X, nullptr, nullptr, false, lane);
    mask_store(X, a.h[1], a.gz[1]);
    gemm_fwd<F32, 16, 0, 16, ACT_NONE>(ws, OP(NB1), has_next ? OP(NBV) : nullptr, OPB(NBV), X, E0, Y, nullptr, nullptr,
                                       false, lane);
    mask_store(Y, a.h[0], a.gz[0]);
  }
  wait_vmcnt(0);
}

// =============================================================================================
// NeRF++ background net on the v3 pipeline (nerf4_kernel, f16x3): the rad4 / sdf4 structure
// (128-point tile, kNC-column waves, weight ring by LDS-DMA two chunks ahead, per-chunk operand split
// at a scale fixed from the op's pack-time bound, epilogues staged beside the next chunk's MFMAs) on
// models/base.py:426-453:
//   N0 (embed(x4): 84 -> 256) .. N4, ReLU;  N5 on cat([h4, embed(x4)]) (base.py:431-432);  N6, N7;
//   NF = [feature_linear; alpha_linear](h7): 256 feature rows (no activation) + sigma as row 0 of a
//   9th chunk (an alpha dot product riding N7's epilogue held 8 more registers and spilled);
//   NV on cat([feature, embed_view(v)]) -> 128, ReLU, with rgb_linear (128 -> 3) + sigmoid in its
//   epilogue.
// The 84-wide embedding stays in registers (fp32) from N0 until N5 re-splits it at N4's output scale;
// the view embedding is built just before NF and split at NF's output scale.
// =============================================================================================
// identity op (feature_linear, with alpha_linear's row as output block 16): chunks 0..7 -> next
// operand; chunk 8's row 0 is sigma (lane group 0, register 0 of the chunk's first block)
struct FeatSigmaEpi4 {
  f16x8 (&oh)[kNC][12];
  f16x8 (&ol)[kNC][12];
  const float (&sc)[kNC];
  float (&mrun)[kNC];
  float (&sigma)[kNC];
  __device__ __forceinline__ void operator()(int c, const Z4& zz, int st) {
    const int q = st >> 2, k = st & 3;
    if (q >= kNC) return;
    if (c == 8) {
      if (k == 3) sigma[q] = zz.z[q][0].x;
    } else if (k == 2) {
      mrun[q] = amax8(mrun[q], zz.z[q][0], zz.z[q][1]);
    } else if (k == 3) {
      split8a(zz.z[q][0], zz.z[q][1], sc[q], oh[q][c], ol[q][c]);
    }
  }
};

// last hidden op of a net with a [3][ROWS] head in LDS: ReLU, then part[q][o] += y . head[o] over the
// lane's rows of the chunk (rad4's HeadEpi4 with the head's row length as a parameter)
template <int ROWS>
struct HeadEpiN {
  const float* head;  // LDS
  float (&part)[kNC][3];
  int g;
  float4 y[kNC][2];
  __device__ __forceinline__ void operator()(int c, const Z4& zz, int st) {
    const int q = st >> 2, k = st & 3;
    if (q >= kNC) return;
    if (k < 2) {
      const float4 z = zz.z[q][k];
      y[q][k] = make_float4(fmaxf(z.x, 0.0f), fmaxf(z.y, 0.0f), fmaxf(z.z, 0.0f), fmaxf(z.w, 0.0f));
    } else {
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        if ((o == 0) != (k == 2)) continue;
        float p = part[q][o];
        const uint32_t lo = opaque_lane(4 * g);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float4 w = *(const float4*)(head + lo + o * ROWS + 16 * (2 * c + b));
          p = fmaf(y[q][b].x, w.x, p);
          p = fmaf(y[q][b].y, w.y, p);
          p = fmaf(y[q][b].z, w.z, p);
          p = fmaf(y[q][b].w, w.w, p);
        }
        asm volatile("" : "+v"(p));
        part[q][o] = p;
      }
    }
  }
};

__global__ __attribute__((amdgpu_flat_work_group_size(kT4, kT4), amdgpu_waves_per_eu(kWPE, kWPE)))
void nerf4_kernel(NerfKArgs a) {
  constexpr int C6 = chunk_bytes(6), C16 = chunk_bytes(16), C18 = chunk_bytes(18), C22 = chunk_bytes(22);
  constexpr int kHead = 3 * 128 + 4;  // rgb_linear [3][128], then [3] bias
  __shared__ __attribute__((aligned(16))) char smem[kRing * C22 + kHead * 4];
  static_assert(kRing * C22 + kHead * 4 <= 160 * 1024, "LDS budget");
  WStream4<C22> ws{smem, nullptr, 0, 0, 0};
  float* head = (float*)(smem + kRing * C22);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const NerfLayout& L = a.L;
  const char* W = a.packed;
  auto OP = [&](int i) {
    const char* w = W;
    asm volatile("" : "+s"(w));
    return w + L.op_off[i];
  };
  {
    const float* hsrc = (const float*)(W + L.rgb_off);
    for (int i = threadIdx.x; i < 3 * 128 + 3; i += kT4) head[i] = hsrc[i];
  }
  ws.template start<C6, C6>(OP(N0), OP(N0) + C6);  // its barrier also publishes the head
  Pend4 pd{};
  NoPre4 nopre;
  const int64_t Pn = a.P_dev ? min(a.P, (int64_t)*a.P_dev) : a.P;
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < Pn; base += (int64_t)gridDim.x * kPointsPerWG) {
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < Pn;
    const int64_t p0 = base + wave * 16 * kNC;
    f16x8 Uh[kNC][12], Ul[kNC][12], Vh[kNC][12], Vl[kNC][12];
    float4 E[kNC][6];
    float m_in[kNC], xinv[kNC], mrun[kNC], mE[kNC];
    bool valid[kNC];
    int64_t pcq[kNC];
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      const int64_t p = p0 + 16 * q + j;
      valid[q] = p < Pn;
      pcq[q] = valid[q] ? p : Pn - 1;
      const float4 xin = *(const float4*)(a.x4 + pcq[q] * 4);
      const int gq = (int)opaque_lane(g);
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const int f = 16 * b + 4 * gq;
        E[q][b] = make_float4(nerf_embed4(f + 0, xin.x, xin.y, xin.z, xin.w),
                              nerf_embed4(f + 1, xin.x, xin.y, xin.z, xin.w),
                              nerf_embed4(f + 2, xin.x, xin.y, xin.z, xin.w),
                              nerf_embed4(f + 3, xin.x, xin.y, xin.z, xin.w));
      }
      mE[q] = max4_groups(amax8(amax8(amax8(0.0f, E[q][0], E[q][1]), E[q][2], E[q][3]), E[q][4], E[q][5]));
      m_in[q] = mE[q];
      const float s = bound_scale(mE[q]);  // exact-max scale of N0's operand
#pragma unroll
      for (int k = 0; k < 3; ++k) split8a(E[q][2 * k], E[q][2 * k + 1], s, Uh[q][k], Ul[q][k]);
      xinv[q] = 1.0f / s;
      mrun[q] = 0.0f;
    }
    // output bound of the op about to run (its chunk 0 is the current ring slot): |relu(z)| <= |z| <=
    // R max|in| + B; floor: the largest value of an input concatenated to that output
    auto next_scales = [&](int kb, const float (&floor_max)[kNC], float (&sc)[kNC]) {
      const float4 v = ws.buf()[2 * kb * 64 + 8];
#pragma unroll
      for (int q = 0; q < kNC; ++q) sc[q] = bound_scale(fmaxf(fmaf(v.y, m_in[q], v.z), floor_max[q]));
    };
    auto finish = [&](const float (&sc)[kNC]) {
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        m_in[q] = max4_groups(mrun[q]);
        mrun[q] = 0.0f;
        xinv[q] = 1.0f / sc[q];
      }
    };
    float zero2[kNC];
#pragma unroll
    for (int q = 0; q < kNC; ++q) zero2[q] = 0.0f;
    {
      float sc[kNC];
      next_scales(6, zero2, sc);
      op4<6, 16, C16, false, false>(ws, OP(N0), OP(N1), Uh, Ul, xinv, pd, nopre, ReluEpi4{Vh, Vl, sc, mrun}, lane);
      finish(sc);
    }
    {
      float sc[kNC];
      next_scales(16, zero2, sc);
      op4<16, 16, C16, false, false>(ws, OP(N1), OP(N2), Vh, Vl, xinv, pd, nopre, ReluEpi4{Uh, Ul, sc, mrun}, lane);
      finish(sc);
    }
    {
      float sc[kNC];
      next_scales(16, zero2, sc);
      op4<16, 16, C16, false, false>(ws, OP(N2), OP(N3), Uh, Ul, xinv, pd, nopre, ReluEpi4{Vh, Vl, sc, mrun}, lane);
      finish(sc);
    }
    {
      float sc[kNC];
      next_scales(16, zero2, sc);
      op4<16, 16, C16, false, false>(ws, OP(N3), OP(N4), Vh, Vl, xinv, pd, nopre, ReluEpi4{Uh, Ul, sc, mrun}, lane);
      finish(sc);
    }
    {
      // N4's outputs (h4) and the embedding form N5's operand [h4 ; embed(x4)]: one scale per point
      float sc[kNC];
      next_scales(16, mE, sc);
      op4<16, 16, C22, false, false>(ws, OP(N4), OP(N5), Uh, Ul, xinv, pd, nopre, ReluEpi4{Vh, Vl, sc, mrun}, lane);
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        float4 Eq[6];  // the embedding again from the point (no 24 registers held across N0..N4)
        const float4 xin = *(const float4*)(a.x4 + pcq[q] * 4);
        const int gq = (int)opaque_lane(g);
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          const int f = 16 * b + 4 * gq;
          Eq[b] = make_float4(nerf_embed4(f + 0, xin.x, xin.y, xin.z, xin.w),
                              nerf_embed4(f + 1, xin.x, xin.y, xin.z, xin.w),
                              nerf_embed4(f + 2, xin.x, xin.y, xin.z, xin.w),
                              nerf_embed4(f + 3, xin.x, xin.y, xin.z, xin.w));
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) split8a(Eq[2 * k], Eq[2 * k + 1], sc[q], Vh[q][8 + k], Vl[q][8 + k]);
        mrun[q] = fmaxf(mrun[q], mE[q]);
      }
      finish(sc);
    }
    {
      float sc[kNC];
      next_scales(22, zero2, sc);
      op4<22, 16, C16, false, false>(ws, OP(N5), OP(N6), Vh, Vl, xinv, pd, nopre, ReluEpi4{Uh, Ul, sc, mrun}, lane);
      finish(sc);
    }
    {
      float sc[kNC];
      next_scales(16, zero2, sc);
      op4<16, 16, C16, false, false>(ws, OP(N6), OP(N7), Uh, Ul, xinv, pd, nopre, ReluEpi4{Vh, Vl, sc, mrun}, lane);
      finish(sc);
    }
    {
      float sc[kNC];
      next_scales(16, zero2, sc);
      op4<16, 16, C16, false, false>(ws, OP(N7), OP(NF), Vh, Vl, xinv, pd, nopre, ReluEpi4{Uh, Ul, sc, mrun}, lane);
      finish(sc);
    }
    float sig[kNC];
    // the view embedding (multires_view 4: 27 features in 2 blocks) joins the feature in NV's operand.
    // Its bound: |sin|, |cos| <= 1 and the raw components |v_i| (3 loads, no embedding held across NF)
    float mV[kNC];
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      const int64_t pv = (pcq[q] / a.vdiv) % a.vmod;
      mV[q] = fmaxf(1.0f, fmaxf(fabsf(a.vdir[pv * 3 + 0]), fmaxf(fabsf(a.vdir[pv * 3 + 1]), fabsf(a.vdir[pv * 3 + 2]))));
    }
    {
      float sc[kNC];
      next_scales(16, mV, sc);
      op4<16, 18, C18, false, false>(ws, OP(NF), OP(NV), Uh, Ul, xinv, pd, nopre,
                                     FeatSigmaEpi4{Vh, Vl, sc, mrun, sig}, lane);
#pragma unroll
      for (int q = 0; q < kNC; ++q) {
        const int64_t pv = (pcq[q] / a.vdiv) % a.vmod;
        const float v0 = a.vdir[pv * 3 + 0], v1 = a.vdir[pv * 3 + 1], v2 = a.vdir[pv * 3 + 2];
        const int gq = (int)opaque_lane(g);
        float4 Ve[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int f = 16 * b + 4 * gq;
          Ve[b] = make_float4(f + 0 < 27 ? embed_feature(f + 0, v0, v1, v2, 4) : 0.0f,
                              f + 1 < 27 ? embed_feature(f + 1, v0, v1, v2, 4) : 0.0f,
                              f + 2 < 27 ? embed_feature(f + 2, v0, v1, v2, 4) : 0.0f,
                              f + 3 < 27 ? embed_feature(f + 3, v0, v1, v2, 4) : 0.0f);
        }
        split8a(Ve[0], Ve[1], sc[q], Vh[q][8], Vl[q][8]);
        mrun[q] = fmaxf(mrun[q], mV[q]);
      }
      finish(sc);
    }
    float part[kNC][3];
#pragma unroll
    for (int q = 0; q < kNC; ++q) part[q][0] = part[q][1] = part[q][2] = 0.0f;
    op4<18, 8, C6, false, false>(ws, OP(NV), has_next ? OP(N0) : nullptr, Vh, Vl, xinv, pd, nopre,
                                 HeadEpiN<128>{head, part, g}, lane);
#pragma unroll
    for (int q = 0; q < kNC; ++q) {
      float r[3];
#pragma unroll
      for (int o = 0; o < 3; ++o) r[o] = sigmoidf_ref(wave_sum4(part[q][o]) + head[3 * 128 + o]);
      if (valid[q] && g == 0) {
        const int64_t p = p0 + 16 * q + j;
        a.sigma[p] = sig[q];
        a.rgb[p * 3 + 0] = r[0];
        a.rgb[p * 3 + 1] = r[1];
        a.rgb[p * 3 + 2] = r[2];
      }
    }
  }
  pd.flush();
  wait_vmcnt(0);  // a block without tiles still has the prologue's second chunk in flight
}

// =============================================================================================
// Training layer GEMM (tgemm_kernel, f16x3): one packed op of the render weight stream applied to a
// [P, K] fp32 activation matrix with the elementwise step that follows it in the training recipe
// fused into the epilogue (nr_train.hip header: primal, nabla chain, tangent and adjoint sweeps):
//   Y[p, o] = epi( sum_i X[p, i] M[o, i] (+ bias[o]) ),  M = the op's packed matrix (W or W^T)
// 128-point tiles (8 waves x 16 points), the input operand split at the exact per-point max and held
// in registers, the op's chunks streamed through the LDS ring by LDS-DMA two ahead.  Tensors the
// epilogue reads (softplus', g, zdot, saved activations) are fetched one chunk ahead by asm loads
// issued before the chunk's weight DMA, and waited for by count: a compiler-visible load would be
// waited on behind the in-flight DMA.  Every matrix is row-major with a row stride; the output
// column layout is the op's block layout (16-column blocks, padded rows computed from zero weights).
// =============================================================================================
enum TgMode { TG_NONE = 0, TG_SOFTPLUS = 1, TG_MUL = 3, TG_SPADJ = 4, TG_RELUMASK = 5 };  // 2: reserved

// float4 at byte offset off of a wave-uniform base, by asm (not waited on by the compiler)
__device__ __forceinline__ float4 tg_load(const float* base, uint32_t off) {
  f32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(v) : "v"(off), "s"(base) : "memory");
  return fromf(v);
}
// pin a loaded value behind the preceding s_waitcnt (uses cannot be scheduled above it)
__device__ __forceinline__ void tg_pin(float4& v) {
  f32x4 t = tof(v);
  asm volatile("" : "+v"(t));
  v = fromf(t);
}

// KB input blocks (the last KB2 from x2), NBO output blocks (the last NB2 to yb), epilogue MODE
// float4 store at byte offset off of a wave-uniform base, by asm: issued by every lane of the wave (clamped
// lanes rewrite the last row with that row's own values), so the store count of a chunk is exact for the
// counted waits (s_nop: the store-data hazard is not tracked through inline asm)
__device__ __forceinline__ void tg_store(float* base, uint32_t off, float4 v) {
  const f32x4 d = tof(v);
  asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(off), "v"(d), "s"(base) : "memory");
}

// float index of element (p, c) of a [P, ld] tensor, row-major or 16 x 16 blocked (NR_BLK_* in
// include/neurecon_hip.h: a 16-point x 16-column block is one contiguous 1 KB run, which is what one
// wave-instruction of the epilogue reads or writes; row-major it is 16 rows x 64 B).  c % 4 == 0 keeps
// c .. c + 3 inside one block in both layouts.
__device__ __forceinline__ uint32_t tg_elem(bool blk, uint32_t p, uint32_t ld, uint32_t c) {
  return blk ? (((p >> 4) * (ld >> 4) + (c >> 4)) << 8) + ((p & 15u) << 4) + (c & 15u) : p * ld + c;
}

// Next-tile prefetch: the next tile's input blocks are loaded during this tile's chunk loop (kPer per chunk, asm
// loads counted with the chunk's other VMEM), so a tile starts from registers instead of a chip-wide
// load burst (tools/tg_driver.py --stamps: the tile start was 27-37 % of the wave time)
template <int KB, int KB2, int NBO, int NB2, int MODE>
__global__ __attribute__((amdgpu_flat_work_group_size(kT4, kT4), amdgpu_waves_per_eu(kWPE, kWPE)))
void tgemm_kernel(TGemmArgs a) {
  constexpr int CB = chunk_bytes(KB);
  constexpr int NCH = NBO / 2, NS = KB / 2, KB1 = KB - KB2, NB1 = NBO - NB2;
  static_assert(NCH >= 2, "the 2-ahead stream needs >= 2 chunks");
  static_assert(NB1 % 2 == 0, "the output split falls between chunks");
  constexpr int TRING = 3;       // weight-ring slots
  constexpr int LA = TRING - 1;  // chunks issued ahead of the one being computed
  using WS = WStream4<CB, TRING>;
  __shared__ __attribute__((aligned(16))) char smem[TRING * CB];
  WS ws{smem, nullptr, 0, 0, 0, 0};
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  ws.template start<CB, CB>(uniform_ptr(a.op), uniform_ptr(a.op) + CB);
  // epilogue tensors by mode: TG_MUL / TG_RELUMASK read a; TG_SPADJ reads a (softplus'), g, zdot
  constexpr bool kA = MODE == TG_MUL || MODE == TG_SPADJ || MODE == TG_RELUMASK;
  constexpr bool kG = MODE == TG_SPADJ;
  constexpr int NA = kG ? 3 : (kA ? 1 : 0);
  // the g zdot term: g from a tensor, or the op's per-row vector (g_row: W8[0, :] for layer 7)
  const bool has_g = kG && (a.g != nullptr || a.g_row), g_tensor = kG && a.g != nullptr;
#ifdef NR_EXP_STAMPS  // stamps build: phases 0-3 of the chunk iterations as sdf4_kernel's, 4 = tile start
  if (lane == 0)
    for (int i = 0; i < kStampPh; ++i) stamp_lds()[wave * kStampPh + i] = 0;
#endif
  // next-tile prefetch: x1 blocks [0, NPF) (single-segment inputs; SPADJ holds 3 epilogue tensors in
  // registers and prefetches half)
  constexpr int kPer = 2;    // prefetched blocks issued per chunk iteration
  constexpr int kSpAdj = 8;  // blocks the adjoint GEMMs prefetch (their three epilogue tensors fill the registers)
  constexpr int NPF = KB2 == 0 ? ((MODE == TG_SPADJ ? kSpAdj : (KB1 < 2 * NCH ? KB1 : 2 * NCH)) & ~1) : 0;
  const bool blk1 = (a.blocked & NR_BLK_X1) != 0;
  const bool pf_ok = NPF > 0 && (blk1 || ((a.ld1 | (int64_t)((uintptr_t)a.x1 >> 2)) & 3) == 0);
  float4 Xn[NPF > 0 ? NPF : 1];
  bool have_pf = false;
  int nst_prev = 0;  // stores the previous tile's last flush issued (younger than its prefetch)
  for (int64_t base = (int64_t)blockIdx.x * kPointsPerWG; base < a.P; base += (int64_t)gridDim.x * kPointsPerWG) {
    NR_STAMP(ts0);
    const bool has_next = base + (int64_t)gridDim.x * kPointsPerWG < a.P;
    const int64_t p = base + wave * 16 + j;
    const bool valid = p < a.P;
    const uint32_t pc = (uint32_t)(valid ? p : a.P - 1);
    // this lane's row of the next tile (clamped: the last tile's rows are re-read, never stored)
    const uint32_t pcn = (uint32_t)min(p + (int64_t)gridDim.x * kPointsPerWG, a.P - 1);
    // ---- input operand: [x1 blocks ; x2 blocks], split at the exact per-point max ----
    f16x8 Uh[1][12], Ul[1][12];
    float xinv[1];
    {
      float4 X[KB];
      int b_first = 0;  // first x1 block loaded here (the ones before came with the previous tile)
      if constexpr (NPF > 0) {
        if (have_pf) {
          wait_vmcnt(nst_prev);  // the prefetch has landed; the final flush's stores may still fly
#pragma unroll
          for (int b = 0; b < NPF; ++b) {
            tg_pin(Xn[b]);
            const int col = 16 * b + 4 * g;  // columns past n1 read as zeros, as load_seg's
            X[b] = make_float4(col + 0 < a.n1 ? Xn[b].x : 0.f, col + 1 < a.n1 ? Xn[b].y : 0.f,
                               col + 2 < a.n1 ? Xn[b].z : 0.f, col + 3 < a.n1 ? Xn[b].w : 0.f);
          }
          b_first = NPF;
        }
      }
      auto load_seg = [&](const float* src, int64_t ld, int n, int b0, int nb, bool blk, int bs = 0) {
        const bool vec = blk || ((ld | (int64_t)((uintptr_t)src >> 2)) & 3) == 0;
#pragma unroll
        for (int b = 0; b < nb; ++b) {
          if (b < bs) continue;
          const int col = 16 * b + 4 * g;
          const float* e = src + tg_elem(blk, pc, (uint32_t)ld, (uint32_t)col);
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (vec && col + 3 < n) v = *(const float4*)e;
          else {
            if (col + 0 < n) v.x = e[0];
            if (col + 1 < n) v.y = e[1];
            if (col + 2 < n) v.z = e[2];
            if (col + 3 < n) v.w = e[3];
            // a compiler-visible vmcnt(0) on this (partial-block / unaligned) path: otherwise its loads
            // stay "maybe in flight" where the paths merge, and the compiler drains every load and store
            // in flight at each tile start of every launch (the previous tile's stores included)
            __builtin_amdgcn_s_waitcnt(0x0F70);
          }
          X[b0 + b] = v;
        }
      };
      if constexpr (NPF == KB1 && KB2 == 0) {
        // the prefetch covers every input block: the loads below run on the cold path only (the first
        // tile, or inputs the prefetch cannot take), which ends in its own compiler-visible vmcnt(0) --
        // so on the prefetched path the compiler has no load of its own to wait for before the split
        // (it waited vmcnt(0) there, draining the previous tile's epilogue stores at every tile start)
        if (!have_pf) {
          load_seg(a.x1, a.ld1, a.n1, 0, KB1, blk1, 0);
          __builtin_amdgcn_s_waitcnt(0x0F70);
        }
      } else {
        load_seg(a.x1, a.ld1, a.n1, 0, KB1, blk1, b_first);
        if constexpr (KB2 > 0) load_seg(a.x2, a.ld2, a.n2, KB1, KB2, (a.blocked & NR_BLK_X2) != 0);
      }
      float m = 0.0f;
#pragma unroll
      for (int b = 0; b < KB; b += 2) m = amax8(m, X[b], X[b + 1]);
      m = max4_groups(m);
      const float sc = bound_scale(m);
#pragma unroll
      for (int k = 0; k < NS; ++k) split8a(X[2 * k], X[2 * k + 1], sc, Uh[0][k], Ul[0][k]);
      xinv[0] = 1.0f / sc;
    }
    // epilogue tensors of chunk c (blocks 2c, 2c+1 < NB1), fetched one chunk ahead
    float4 aux[2][NA > 0 ? NA : 1][2];
    auto aux_issue = [&](int c, float4 (&dst)[NA > 0 ? NA : 1][2]) -> int {
      if constexpr (NA == 0) return 0;
      if (2 * c >= NB1) return 0;
      int n = 0;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const uint32_t col = (uint32_t)(16 * (2 * c + b) + 4 * g);
        dst[0][b] = tg_load(a.a, tg_elem(a.blocked & NR_BLK_A, pc, (uint32_t)a.lda, col) * 4u);
        ++n;
        if constexpr (kG) {
          if (g_tensor) {
            dst[1][b] = tg_load(a.g, tg_elem(a.blocked & NR_BLK_G, pc, (uint32_t)a.ldg, col) * 4u);
            ++n;
          }
          if (has_g) {
            dst[2][b] = tg_load(a.zd, tg_elem(a.blocked & NR_BLK_ZD, pc, (uint32_t)a.ldzd, col) * 4u);
            ++n;
          }
        }
      }
      return n;
    };
    aux_issue(0, aux[0]);
#ifdef NR_EXP_STAMPS
    stamp_add(4, stamp_now() - ts0);
#endif
    float dpart = 0.0f;
    // chunk c's outputs (y, y2, y3 per block) are stored at the start of iteration c+1, after that
    // iteration's loads and DMA: younger than everything its counted wait must see landed
    float4 pv[3][2];
    auto flush = [&](int c) -> int {
      const bool lo = 2 * c < NB1;
      float* dst = lo ? a.y : a.yb;
      int n = 0;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int B = 2 * c + b;
        const uint32_t col = (uint32_t)(16 * (lo ? B : B - NB1) + 4 * g);
        if (dst) {
          const bool blk = (a.blocked & (lo ? NR_BLK_Y : NR_BLK_YB)) != 0;
          tg_store(dst, tg_elem(blk, pc, (uint32_t)(lo ? a.ldy : a.ldyb), col) * 4u, pv[0][b]);
          ++n;
        }
        if constexpr (MODE == TG_SOFTPLUS || MODE == TG_MUL)
          if (lo && a.y2) {
            tg_store(a.y2, tg_elem(a.blocked & NR_BLK_Y2, pc, (uint32_t)a.ldy2, col) * 4u, pv[1][b]);
            ++n;
          }
        if constexpr (MODE == TG_SOFTPLUS)
          if (lo && a.y3) {
            tg_store(a.y3, tg_elem(a.blocked & NR_BLK_Y3, pc, (uint32_t)a.ldy3, col) * 4u, pv[2][b]);
            ++n;
          }
      }
      return n;
    };
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const char* opc = a.op;
      asm volatile("" : "+s"(opc));
      NR_STAMP(t0);
      int npend = 0;
      if (c + 1 < NCH) npend += aux_issue(c + 1, aux[(c + 1) & 1]);
      if (c + LA < NCH) {
        ws.template issue<CB>(opc + (c + LA) * CB);
        npend += WS::template npieces<CB>();
      } else if (has_next) {
        ws.template issue<CB>(opc + (c + LA - NCH) * CB);
        npend += WS::template npieces<CB>();
      }
      if (c > 0) npend += flush(c - 1);
      if constexpr (NPF > 0) {  // the next tile's x1 blocks 2c, 2c+1
        if (pf_ok && has_next && kPer * c < NPF) {
#pragma unroll
          for (int bb = 0; bb < kPer; ++bb) {
            const int b = kPer * c + bb;
            if (b < NPF) {
              Xn[b] = tg_load(a.x1, tg_elem(blk1, pcn, (uint32_t)a.ld1, (uint32_t)(16 * b + 4 * g)) * 4u);
              ++npend;
            }
          }
        }
      }
      NR_STAMP(t1);
      const float4* A = ws.buf();
      f32x4 acc[1][2] = {};
      mma4<NS>(A, Uh, Ul, acc, lane, [&](int) {});
      NR_STAMP(t2);
      const float inv = xinv[0] * A[2 * KB * 64 + 8].x;
      float4 z[2];
      if (a.use_bias) {
        z[0] = fma4s(acc[0][0], inv, A[2 * KB * 64 + g]);
        z[1] = fma4s(acc[0][1], inv, A[2 * KB * 64 + 4 + g]);
      } else {
        z[0] = fma4s(acc[0][0], inv, make_float4(0.f, 0.f, 0.f, 0.f));
        z[1] = fma4s(acc[0][1], inv, make_float4(0.f, 0.f, 0.f, 0.f));
      }
      // everything issued before this iteration has landed (this chunk's epilogue tensors, chunk c+1's
      // weights); pinning keeps every use of the asm-loaded registers behind the wait
      wait_vmcnt(npend);
      NR_STAMP(t3);
      if constexpr (NA > 0) {
#pragma unroll
        for (int t = 0; t < NA; ++t) { tg_pin(aux[c & 1][t][0]); tg_pin(aux[c & 1][t][1]); }
      }
      {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float zz[4] = {z[b].x, z[b].y, z[b].z, z[b].w};
          float o1[4], o2[4] = {0.f, 0.f, 0.f, 0.f};
          if constexpr (MODE == TG_SOFTPLUS) {  // torch softplus(beta=100, threshold=20) and softplus'
            const float4 rvv = A[2 * KB * 64 + 16 + 4 * b + g];  // the op's per-row vector (F7: W8[0, :])
            const float rv[4] = {rvv.x, rvv.y, rvv.z, rvv.w};
            float o3[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float t = zz[r] * 144.269504088896341f;  // 100 log2(e) z
              const float e = __builtin_amdgcn_exp2f(fminf(t, 126.0f));
              const float u = e + 1.0f;
              const bool lin = t > 28.8539008f;             // 100 z > 20
              o1[r] = lin ? zz[r] : __builtin_amdgcn_logf(u) * 0.0069314718055994531f;
              o2[r] = lin ? 1.0f : e * __builtin_amdgcn_rcpf(u);
              o3[r] = o2[r] * rv[r];
              dpart = fmaf(o1[r], rv[r], dpart);
            }
            pv[2][b] = make_float4(o3[0], o3[1], o3[2], o3[3]);
          } else if constexpr (MODE == TG_MUL) {
            const float av[4] = {aux[c & 1][0][b].x, aux[c & 1][0][b].y, aux[c & 1][0][b].z, aux[c & 1][0][b].w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float v = zz[r] * a.yscale;
              o1[r] = v;
              o2[r] = av[r] * v;
            }
          } else if constexpr (MODE == TG_SPADJ) {  // zbar = hbar s + g zdot 100 s (1 - s)
            const float av[4] = {aux[c & 1][0][b].x, aux[c & 1][0][b].y, aux[c & 1][0][b].z, aux[c & 1][0][b].w};
            const float gv[4] = {aux[c & 1][1][b].x, aux[c & 1][1][b].y, aux[c & 1][1][b].z, aux[c & 1][1][b].w};
            const float dv[4] = {aux[c & 1][2][b].x, aux[c & 1][2][b].y, aux[c & 1][2][b].z, aux[c & 1][2][b].w};
            const float4 rvv = A[2 * KB * 64 + 16 + 4 * b + g];
            const float rv[4] = {rvv.x, rvv.y, rvv.z, rvv.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float si = av[r];
              float w = fmul(zz[r] * a.yscale, si);
              if (has_g) {
                // s' = 100 s (1 - s); with g_scaled the tensor holds s g already
                const float d2 = a.g_scaled && !a.g_row ? fmul(fsub(1.0f, si), 100.0f)
                                                        : fmul(fmul(si, fsub(1.0f, si)), 100.0f);
                w = fadd(w, fmul(fmul(a.g_row ? rv[r] : gv[r], dv[r]), d2));
              }
              o1[r] = w;
            }
          } else if constexpr (MODE == TG_RELUMASK) {
            const float av[4] = {aux[c & 1][0][b].x, aux[c & 1][0][b].y, aux[c & 1][0][b].z, aux[c & 1][0][b].w};
#pragma unroll
            for (int r = 0; r < 4; ++r) o1[r] = av[r] > 0.0f ? zz[r] : 0.0f;
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) o1[r] = zz[r] * a.yscale;
          }
          pv[0][b] = make_float4(o1[0], o1[1], o1[2], o1[3]);
          pv[1][b] = make_float4(o2[0], o2[1], o2[2], o2[3]);
        }
      }
      NR_STAMP(t3e);
      // the counted wait above covered the next chunk's weights, so this iteration's DMA, stores and
      // prefetch stay in flight across the barrier (r05 with the prefetch: +0.8 % on the training step
      // alternated, against draining them here; a 4-slot ring gave +0.7 %)
      ws.flip_nowait();
#ifdef NR_EXP_STAMPS
      const uint64_t t4 = stamp_now();
      stamp_add(0, t1 - t0);   // VMEM issue: epilogue operands, weight DMA, previous chunk's stores
      stamp_add(1, t2 - t1);   // MFMA loop
      stamp_add(2, t3 - t2);   // bias + counted vmcnt wait
      stamp_add(5, t3e - t3);  // epilogue VALU
      stamp_add(3, t4 - t3e);  // barrier
#endif
    }
    nst_prev = flush(NCH - 1);
    if constexpr (MODE == TG_SOFTPLUS) {
      if (a.dot) {
        const float v = wave_sum4(dpart) + a.dot_bias;
        if (valid && g == 0) a.dot[p] = v;
      }
    }
    have_pf = pf_ok && has_next;
  }
  wait_vmcnt(0);
#ifdef NR_EXP_STAMPS
  if (lane == 0 && blockIdx.x < 2048)
    for (int i = 0; i < kStampPh; ++i)
      g_nr_stamps[(blockIdx.x * kW4 + wave) * kStampPh + i] = stamp_lds()[wave * kStampPh + i];
#endif
}

// (input blocks, output blocks, epilogue) instances the training path uses (neurecon_amd/training.py)
#define NR_TG_SHAPES(X)                                                                                  \
  X(4, 0, 16, 0, TG_SOFTPLUS) X(16, 0, 16, 0, TG_SOFTPLUS) X(16, 0, 14, 0, TG_SOFTPLUS)                   \
  X(18, 4, 16, 0, TG_SOFTPLUS)                                                                           \
  X(16, 0, 16, 0, TG_NONE) X(16, 0, 4, 0, TG_NONE) X(16, 0, 18, 2, TG_NONE) X(16, 0, 20, 4, TG_NONE)      \
  X(16, 0, 16, 0, TG_MUL) X(16, 0, 18, 4, TG_MUL) X(14, 0, 16, 0, TG_MUL) X(4, 0, 16, 0, TG_MUL)          \
  X(16, 0, 14, 0, TG_MUL) X(18, 4, 16, 0, TG_MUL)                                                        \
  X(18, 2, 16, 0, TG_SPADJ) X(16, 0, 16, 0, TG_SPADJ) X(16, 0, 18, 4, TG_SPADJ) X(14, 0, 16, 0, TG_SPADJ)  \
  X(2, 0, 16, 0, TG_RELUMASK) X(16, 0, 16, 0, TG_RELUMASK)

int launch_tgemm(const TGemmArgs& a, int KB, int KB2, int NBO, int NB2, hipStream_t stream) {
  if (a.P <= 0) return NR_OK;
  NR_REQUIRE(a.op && (a.y || a.yb || a.y2 || a.y3 || a.dot), NR_ERR_ARG, "tgemm: null op or no output");
  NR_REQUIRE(a.x1 && (KB2 == 0 || a.x2), NR_ERR_ARG, "tgemm: missing input segment");
  // 32-bit byte offsets of the asm loads and stores: the epilogue's tensors and the inputs (the next-tile
  // prefetch reads x1 at a 32-bit byte offset, load_seg forms a 32-bit float index); P * ld floats is the
  // extent of a tensor in both layouts (row-major and 16 x 16 blocked)
  const int64_t maxld = std::max({a.ld1, KB2 > 0 ? a.ld2 : (int64_t)0, a.lda, a.ldg, a.ldzd, a.ldy, a.ldyb, a.ldy2,
                                  a.ldy3});
  NR_REQUIRE(a.P * maxld * 4 < ((int64_t)1 << 31), NR_ERR_ARG, "tgemm: an input or epilogue operand exceeds 2 GB");
  if (a.blocked) {  // 16 x 16 blocked tensors: whole blocks of points and columns
    const int64_t lds[9] = {a.ld1, a.ld2, a.ldy, a.ldyb, a.ldy2, a.ldy3, a.lda, a.ldg, a.ldzd};
    bool ok = a.P % 16 == 0 && (a.blocked & ~0x1ff) == 0;
    for (int i = 0; i < 9; ++i) ok = ok && (!(a.blocked & (1 << i)) || (lds[i] > 0 && lds[i] % 16 == 0));
    NR_REQUIRE(ok, NR_ERR_ARG, "tgemm: a blocked tensor needs P and its leading dimension multiples of 16");
  }
  bool known = false;  // refused before any HIP call, as the argument errors above
#define NR_TG_KNOWN(kb, kb2, nbo, nb2, md) \
  known = known || (KB == kb && KB2 == kb2 && NBO == nbo && NB2 == nb2 && a.mode == md);
  NR_TG_SHAPES(NR_TG_KNOWN)
#undef NR_TG_KNOWN
  if (!known) {
    set_error("tgemm: unsupported (input blocks, output blocks) shape");
    return NR_ERR_UNSUPPORTED;
  }
  const int64_t tiles = (a.P + kPointsPerWG - 1) / kPointsPerWG;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const int grid = (int)std::min<int64_t>(tiles, cus);
  ProfScope prof("train_gemm", (double)a.P * KB * NBO * 256.0, stream);  // units: MACs (padded blocks)
#define NR_TG_CASE(kb, kb2, nbo, nb2, md)                                                      \
  if (KB == kb && KB2 == kb2 && NBO == nbo && NB2 == nb2 && a.mode == md) {                     \
    hipLaunchKernelGGL((tgemm_kernel<kb, kb2, nbo, nb2, md>), dim3(grid), dim3(kT4), 0, stream, a); \
    NR_HIP_CHECK(hipGetLastError());                                                            \
    return NR_OK;                                                                               \
  }
  NR_TG_SHAPES(NR_TG_CASE)
#undef NR_TG_CASE
  set_error("tgemm: unsupported (input blocks, output blocks) shape");
  return NR_ERR_UNSUPPORTED;
}

// =============================================================================================
// weight packing (device): effective W [rows][ld] -> chunk layout of one GEMM op
// =============================================================================================
// source element (W * scale) of A-element (ob, b, fi) of an op, or 0 for padding
__device__ __forceinline__ float pack_src(const PackOp& op, int ob, int i, int b, int fi) {
  int row = -1, col = -1;
  int ob_loc = ob;
  for (int s = 0; s < 2; ++s) {
    if (ob_loc < op.out[s].nblk) {
      const int rl = 16 * ob_loc + i;
      if (rl < op.out[s].nvalid) row = op.out[s].off + rl;
      break;
    }
    ob_loc -= op.out[s].nblk;
  }
  int b_loc = b;
  for (int s = 0; s < 2; ++s) {
    if (b_loc < op.in[s].nblk) {
      const int cl = 16 * b_loc + fi;
      if (cl < op.in[s].nvalid) col = op.in[s].off + cl;
      break;
    }
    b_loc -= op.in[s].nblk;
  }
  if (row < 0 || col < 0) return 0.0f;
  if (op.W2 && ob >= op.out[0].nblk) return op.W2[(int64_t)row * op.ld2 + col] * op.scale;  // out[1] rows of W2
  return (op.transpose ? op.W[(int64_t)col * op.ld + row] : op.W[(int64_t)row * op.ld + col]) * op.scale;
}

// bias of a row of output segment s (segment 1 reads bias2 when the op has a second matrix)
__device__ __forceinline__ float op_bias(const PackOp& op, int s, int row) {
  return (s == 1 && op.W2) ? op.bias2[row] : op.bias[row];
}

// weight scale 2^(13 - e) for max |W| = f 2^e (f16x3), 1 for fp32
__device__ __forceinline__ float wscale_of(int prec, float m) {
  if (prec != NR_PREC_F16X3) return 1.0f;
  if (!(m > 0.0f)) return 1.0f;
  return __builtin_ldexpf(1.0f, 13 - __builtin_amdgcn_frexp_expf(m));
}
__device__ __forceinline__ float wscale(const PackOp& op) {
  return wscale_of(op.prec, op.prec == NR_PREC_F16X3 ? *op.wmax : 0.0f);
}

// word e of a packed op
__device__ __forceinline__ void pack_word(const PackOp& op, uint32_t* __restrict__ dst, int64_t e) {
  const int KB = op.in[0].nblk + op.in[1].nblk;
  const int per_chunk = (2 * KB + 1) * 256;  // words
  const int c = (int)(e / per_chunk);
  const int w = (int)(e - (int64_t)c * per_chunk);
  if (w >= 2 * KB * 256) {  // bias slot: 2 blocks x 16 rows, [32] = 1 / weight scale
    const int idx = w - 2 * KB * 256;
    float v = 0.0f;
    if (idx < 32 && op.bias) {
      int ob_loc = 2 * c + idx / 16;
      for (int s = 0; s < 2; ++s) {
        if (ob_loc < op.out[s].nblk) {
          const int rl = 16 * ob_loc + (idx & 15);
          if (rl < op.out[s].nvalid) v = op_bias(op, s, op.out[s].off + rl);
          break;
        }
        ob_loc -= op.out[s].nblk;
      }
    } else if (idx == 32) {
      v = 1.0f / wscale(op);
    } else if ((idx == 33 || idx == 34) && op.bound) {
      v = op.bound[idx - 33];
    } else if (idx >= 96 && idx < 128 && op.bias) {  // bias * kT: op4's TS mode (softplus ops)
      int ob_loc = 2 * c + (idx - 96) / 16;
      for (int s = 0; s < 2; ++s) {
        if (ob_loc < op.out[s].nblk) {
          const int rl = 16 * ob_loc + (idx & 15);
          if (rl < op.out[s].nvalid) v = op_bias(op, s, op.out[s].off + rl) * kT;
          break;
        }
        ob_loc -= op.out[s].nblk;
      }
    } else if (idx >= 64 && idx < 96 && op.aux) {
      int ob_loc = 2 * c + (idx - 64) / 16;
      for (int s = 0; s < 2; ++s) {
        if (ob_loc < op.out[s].nblk) {
          const int rl = 16 * ob_loc + (idx & 15);
          if (rl < op.out[s].nvalid) v = op.aux[op.out[s].off + rl];
          break;
        }
        ob_loc -= op.out[s].nblk;
      }
    }
    dst[e] = __float_as_uint(v);
    return;
  }
  if (op.prec == NR_PREC_FP32) {  // [obl][b][lane][r] floats
    const int r = w & 3, lane = (w >> 2) & 63, t = w >> 8;
    const int b = t % KB, obl = t / KB;
    dst[e] = __float_as_uint(pack_src(op, 2 * c + obl, lane & 15, b, 4 * (lane >> 4) + r));
  } else {  // [obl][s][hl][lane][8 halves]; word = halves (2q, 2q+1)
    const int q = w & 3, lane = (w >> 2) & 63, hl = (w >> 8) & 1, t = w >> 9;
    const int NS = KB / 2, s = t % NS, obl = t / NS;
    const float sc = wscale(op);
    uint32_t word = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int el = 2 * q + h;
      const int b = 2 * s + (el >> 2), fi = 4 * (lane >> 4) + (el & 3);
      const float v = pack_src(op, 2 * c + obl, lane & 15, b, fi) * sc;
      const _Float16 hi = (_Float16)v;
      const _Float16 lo = (_Float16)(v - (float)hi);
      const _Float16 out = hl ? lo : hi;
      word |= (uint32_t)__builtin_bit_cast(uint16_t, out) << (16 * h);
    }
    dst[e] = word;
  }
}

// Packing runs every optimizer step in training (the no-grad sampler's render pack and the training
// pack follow the weights), for up to 17 ops per network: the ops of one pack call go in batches of
// kPackBatch through three launches -- pack_rows_kernel and pack_final_kernel (max |W * scale| for the
// f16x3 weight scale, and the op's bound) and pack_ops_kernel (one thread per packed word, blockIdx.y =
// op) -- instead of two memsets and three launches per op.
constexpr int kPackBatch = 20;  // a whole SDF pack (17 ops) in one batch: three launches per pack call
struct PackBatch {
  PackOp op[kPackBatch];
  uint32_t* dst[kPackBatch];
  int64_t n[kPackBatch];  // packed words of op i
};
static_assert(sizeof(PackBatch) <= 4096, "kernel argument size");

// one thread per 32-bit word of the packed op
__global__ void pack_ops_kernel(PackBatch pb) {
  const int o = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= pb.n[o]) return;
  pack_word(pb.op[o], pb.dst[o], e);
}

// The op's scales and bounds, in two launches over many workgroups (r06; r05 ran one 16-wave
// workgroup per op, ~60 us per batch of 8 ops: every optimizer step of training repacks 3-4 nets):
//   *wmax    = max |W * scale| (and of W2) -- f16x3 ops
//   bound[0] = max over packed output rows of sum_k |W * scale| (row L1 norm of the op's effective
//              matrix, x 1.0001: margin for the summation's rounding), bound[1] = max |bias|
// pack_rows_kernel (grid: row groups of 16 x ops): one wave per packed output row sums its KB x 16
// inputs (lanes strided over them, then wave-summed: the r05 kernel's order, so every op packs bit for
// bit as before), and each workgroup takes a slice of W (and W2) for the max; the partials go to words
// 128..255 of the op's packed bias slots, which pack_ops_kernel rewrites (to 0) afterwards.
// pack_final_kernel (one workgroup per op) reduces them: maxima are order-independent.
constexpr int kPackRowsPerWG = 16;
__device__ __forceinline__ uint32_t* pack_part(const PackBatch& pb, int o, int chunk, int word) {
  const PackOp& op = pb.op[o];
  const int KB = op.in[0].nblk + op.in[1].nblk;
  return pb.dst[o] + (int64_t)chunk * (2 * KB + 1) * 256 + 2 * KB * 256 + word;
}
__global__ __launch_bounds__(1024) void pack_rows_kernel(PackBatch pb) {
  const int o = blockIdx.y, grp = blockIdx.x;
  const PackOp& op = pb.op[o];
  const int NBO = op.out[0].nblk + op.out[1].nblk;
  const int R = NBO * 16, G = (R + kPackRowsPerWG - 1) / kPackRowsPerWG;
  if (grp >= G) return;
  __shared__ float red[2][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (op.bound) {
    const int r = grp * kPackRowsPerWG + wave;
    if (r < R) {
      const int KB = op.in[0].nblk + op.in[1].nblk;
      const int ob = r >> 4, i = r & 15;
      float sr = 0.0f;
      for (int e = lane; e < KB * 16; e += 64) sr += fabsf(pack_src(op, ob, i, e >> 4, e & 15));
      for (int off = 32; off > 0; off >>= 1) sr += __shfl_xor(sr, off);
      if (lane == 0) *pack_part(pb, o, r >> 5, 128 + (r & 31)) = __float_as_uint(sr * 1.0001f);
    }
  }
  if (op.prec == NR_PREC_F16X3) {  // this group's slice of W (and W2)
    float m = 0.0f, m2 = 0.0f;
    const int64_t a0 = op.wn * grp / G, a1 = op.wn * (grp + 1) / G;
    for (int64_t i = a0 + threadIdx.x; i < a1; i += 1024) m = fmaxf(m, fabsf(op.W[i] * op.scale));
    if (op.W2) {
      const int64_t b0 = op.wn2 * grp / G, b1 = op.wn2 * (grp + 1) / G;
      for (int64_t i = b0 + threadIdx.x; i < b1; i += 1024) m2 = fmaxf(m2, fabsf(op.W2[i] * op.scale));
    }
    for (int off = 32; off > 0; off >>= 1) {
      m = fmaxf(m, __shfl_xor(m, off));
      m2 = fmaxf(m2, __shfl_xor(m2, off));
    }
    if (lane == 0) {
      red[0][wave] = m;
      red[1][wave] = m2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float a = 0.0f, b = 0.0f;
      for (int w = 0; w < 16; ++w) {
        a = fmaxf(a, red[0][w]);
        b = fmaxf(b, red[1][w]);
      }
      // G <= 18 groups: chunk 0's words 192.. and 224..
      *pack_part(pb, o, 0, 192 + grp) = __float_as_uint(fmaxf(a, b));
    }
  }
}
__global__ __launch_bounds__(256) void pack_final_kernel(PackBatch pb) {
  const int o = blockIdx.x;
  const PackOp& op = pb.op[o];
  const int NBO = op.out[0].nblk + op.out[1].nblk;
  const int R = NBO * 16, G = (R + kPackRowsPerWG - 1) / kPackRowsPerWG;
  __shared__ float red[3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float best = 0.0f, bb = 0.0f, m = 0.0f;
  if (op.bound) {
    for (int r = threadIdx.x; r < R; r += 256) {
      best = fmaxf(best, __uint_as_float(*pack_part(pb, o, r >> 5, 128 + (r & 31))));
      if (op.bias) {
        const int ob = r >> 4, i = r & 15;
        int ob_loc = ob;
        for (int q = 0; q < 2; ++q) {
          if (ob_loc < op.out[q].nblk) {
            const int rl = 16 * ob_loc + i;
            if (rl < op.out[q].nvalid) bb = fmaxf(bb, fabsf(op_bias(op, q, op.out[q].off + rl)));
            break;
          }
          ob_loc -= op.out[q].nblk;
        }
      }
    }
  }
  if (op.prec == NR_PREC_F16X3 && threadIdx.x < G) m = __uint_as_float(*pack_part(pb, o, 0, 192 + threadIdx.x));
  for (int off = 32; off > 0; off >>= 1) {
    best = fmaxf(best, __shfl_xor(best, off));
    bb = fmaxf(bb, __shfl_xor(bb, off));
    m = fmaxf(m, __shfl_xor(m, off));
  }
  if (lane == 0) {
    red[0][wave] = m;
    red[1][wave] = best;
    red[2][wave] = bb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.0f, b = 0.0f, c = 0.0f;
    for (int w = 0; w < 4; ++w) {
      a = fmaxf(a, red[0][w]);
      b = fmaxf(b, red[1][w]);
      c = fmaxf(c, red[2][w]);
    }
    if (op.prec == NR_PREC_F16X3) *op.wmax = a;
    // the bias slot's word 32 once per op (sdf4_kernel's lean ops read it here, not from the chunks)
    if (op.winv) *op.winv = 1.0f / wscale_of(op.prec, a);
    if (op.bound) {
      op.bound[0] = b;
      op.bound[1] = c;
    }
  }
}

__global__ void pack_vec_kernel(const float* __restrict__ src, int off, int nvalid, int n, float* __restrict__ dst) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  dst[e] = e < nvalid ? src[off + e] : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int launch_pack_ops(const PackOp* ops, char* const* dst, int nops, hipStream_t stream) {
  for (int b0 = 0; b0 < nops; b0 += kPackBatch) {
    const int nb = std::min(kPackBatch, nops - b0);
    PackBatch pb{};
    int64_t nmax = 0;
    for (int i = 0; i < nb; ++i) {
      const PackOp& op = ops[b0 + i];
      NR_REQUIRE(op.prec != NR_PREC_F16X3 || op.wmax, NR_ERR_ARG, "pack: f16x3 needs a max-|W| word");
      const int KB = op.in[0].nblk + op.in[1].nblk;
      const int NBO = op.out[0].nblk + op.out[1].nblk;
      pb.op[i] = op;
      pb.dst[i] = (uint32_t*)dst[b0 + i];
      pb.n[i] = (int64_t)(NBO / 2) * (2 * KB + 1) * 256;
      nmax = std::max(nmax, pb.n[i]);
    }
    int gmax = 1;
    for (int i = 0; i < nb; ++i)
      gmax = std::max(gmax, ((pb.op[i].out[0].nblk + pb.op[i].out[1].nblk) * 16 + kPackRowsPerWG - 1) / kPackRowsPerWG);
    NR_REQUIRE(gmax <= 32, NR_ERR_UNSUPPORTED, "pack: more than 512 output rows in one op");
    hipLaunchKernelGGL(pack_rows_kernel, dim3(gmax, nb), dim3(1024), 0, stream, pb);
    NR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pack_final_kernel, dim3(nb), dim3(256), 0, stream, pb);
    NR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pack_ops_kernel, dim3((unsigned)((nmax + 255) / 256), nb), dim3(256), 0, stream, pb);
    NR_HIP_CHECK(hipGetLastError());
  }
  return NR_OK;
}

int launch_pack_op(const PackOp& op, char* dst, hipStream_t stream) { return launch_pack_ops(&op, &dst, 1, stream); }

int launch_pack_vec(const float* src, int off, int nvalid, int n, char* dst, hipStream_t stream) {
  hipLaunchKernelGGL(pack_vec_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, off, nvalid, n, (float*)dst);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

static int cu_count() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus;
}

static std::atomic<int> g_wg_cap{0};
void set_workgroup_cap(int n) { g_wg_cap = n; }

static int grid_for(int64_t P, int ppw = kPointsPerWG) {
  const int cap = g_wg_cap.load(), cus = cap > 0 ? std::min(cap, cu_count()) : cu_count();
  const int64_t need = (P + ppw - 1) / ppw;
  return (int)(need < cus ? (need > 0 ? need : 1) : cus);
}

int launch_sdf(const SdfLayout& L, const void* packed, const float* pts, int64_t P, float* sdf, float* nabla,
               float* feature, int nfreq, void* ws, size_t ws_bytes, hipStream_t stream, const int* P_dev,
               int P_mult, const void* f8_alt, int* claim) {
  if (P <= 0) return NR_OK;
  const int grid = grid_for(P);
  NR_REQUIRE(!f8_alt || (feature && L.prec == NR_PREC_F16X3 && !L.siren), NR_ERR_ARG,
             "sdf: an op in F8's place needs the f16x3 softplus net and a feature buffer");
  NR_REQUIRE(L.siren || L.prec != NR_PREC_F16X3 || nfreq == kEncBands, NR_ERR_UNSUPPORTED,
             "sdf: the f16x3 softplus net encodes 6 bands");
  SdfKArgs a{(const char*)packed, L, pts, P, sdf, nabla, feature, (float4*)ws, nfreq, P_dev, P_mult, nullptr, nullptr,
             nullptr, (const char*)f8_alt};
  const SdfKArgsC ac{a, claim};  // the instances that claim their tiles (kSdfClaim)
  ProfScope prof(nabla ? (feature ? "sdf_nabla_feat" : "sdf_nabla") : (feature ? "sdf_feat" : "sdf_fwd"), (double)P,
                 stream, P_dev, P_mult);
  if (L.siren) {
    if (nabla) {
      const size_t need = (size_t)grid * kScratchPerWG;
      NR_REQUIRE(ws && ws_bytes >= need, NR_ERR_WORKSPACE, "sdf nabla workspace too small");
      if (L.prec == NR_PREC_F16X3)
        hipLaunchKernelGGL((siren_sdf_kernel<NR_PREC_F16X3, true>), dim3(grid), dim3(kThreads), 0, stream, a);
      else hipLaunchKernelGGL((siren_sdf_kernel<NR_PREC_FP32, true>), dim3(grid), dim3(kThreads), 0, stream, a);
    } else {
      if (L.prec == NR_PREC_F16X3)
        hipLaunchKernelGGL((siren_sdf_kernel<NR_PREC_F16X3, false>), dim3(grid), dim3(kThreads), 0, stream, a);
      else hipLaunchKernelGGL((siren_sdf_kernel<NR_PREC_FP32, false>), dim3(grid), dim3(kThreads), 0, stream, a);
    }
    NR_HIP_CHECK(hipGetLastError());
    return NR_OK;
  }
  if (nabla) {
    const size_t need = (size_t)grid * kScratchPerWG;
    NR_REQUIRE(ws && ws_bytes >= need, NR_ERR_WORKSPACE, "sdf nabla workspace too small");
    if (L.prec == NR_PREC_F16X3) {
      if (feature) hipLaunchKernelGGL((sdf4_kernel<true, true, 0>), dim3(grid), dim3(kT4), 0, stream, ac);
      else hipLaunchKernelGGL((sdf4_kernel<true, false, 0>), dim3(grid), dim3(kT4), 0, stream, a);
    }
    else hipLaunchKernelGGL((sdf_kernel<NR_PREC_FP32, true>), dim3(grid), dim3(kThreads), 0, stream, a);
  } else {
    if (L.prec == NR_PREC_F16X3) {
      if (feature) hipLaunchKernelGGL((sdf4_kernel<false, true, 0>), dim3(grid), dim3(kT4), 0, stream, a);
      else if (P <= (int64_t)64 * cu_count())  // a few thousand points: 64-point tiles on all CUs
        hipLaunchKernelGGL((sdf4_kernel<false, false, 3>), dim3(grid_for(P, 64)), dim3(256), 0, stream, a);
      else hipLaunchKernelGGL((sdf4_kernel<false, false, 0>), dim3(grid), dim3(kT4), 0, stream, a);
    }
    else hipLaunchKernelGGL((sdf_kernel<NR_PREC_FP32, false>), dim3(grid), dim3(kThreads), 0, stream, a);
  }
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int launch_sdf_deferred(const SdfLayout& L, const void* packed, const float* pts, int64_t P, float* sdf, float* nabla,
                        int nfreq, float4* slabs, const int* tiles, const int* n_tiles, int stage, hipStream_t stream,
                        int* claim) {
  if (P <= 0) return NR_OK;
  NR_REQUIRE(L.prec == NR_PREC_F16X3 && !L.siren, NR_ERR_UNSUPPORTED, "deferred nablas: f16x3 softplus nets");
  NR_REQUIRE(nfreq == kEncBands, NR_ERR_UNSUPPORTED, "sdf: the f16x3 softplus net encodes 6 bands");
  SdfKArgs a{(const char*)packed, L, pts, P, sdf, nabla, nullptr, nullptr, nfreq, nullptr, 0, slabs, tiles, n_tiles};
  const SdfKArgsC ac{a, claim};  // stages 2 and 4 claim their tiles (kSdfClaim)
  if (stage == 1) {
    ProfScope prof("sdf_nabla_fwd", (double)P, stream);
    hipLaunchKernelGGL((sdf4_kernel<true, false, 1>), dim3(grid_for(P)), dim3(kT4), 0, stream, a);
  } else if (stage == 2) {
    ProfScope prof("sdf_nabla_bwd", (double)P, stream, n_tiles, 16);
    hipLaunchKernelGGL((sdf4_kernel<true, false, 2>), dim3(grid_for(P)), dim3(kT4), 0, stream, ac);
  } else {  // 4: `tiles` lists sample slots (neus_point_list); the units count its padding too
    NR_REQUIRE(stage == 4, NR_ERR_ARG, "deferred nablas: bad stage");
    ProfScope prof("sdf_nabla_bwd", (double)P, stream, n_tiles, 1);
    hipLaunchKernelGGL((sdf4_kernel<true, false, 4>), dim3(grid_for(P)), dim3(kT4), 0, stream, ac);
  }
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int launch_nerf(const NerfLayout& L, const void* packed, const float* x4, const float* vdir, int64_t vdiv,
                int64_t vmod, int64_t P, float* sigma, float* rgb, hipStream_t stream, const int* P_dev) {
  if (P <= 0) return NR_OK;
  const int grid = grid_for(P);
  NerfKArgs a{(const char*)packed, L, x4, vdir, vdiv, vmod, P, sigma, rgb, P_dev};
  ProfScope prof("nerf", (double)P, stream, P_dev, 1);
  if (L.prec == NR_PREC_F16X3) hipLaunchKernelGGL(nerf4_kernel, dim3(grid), dim3(kT4), 0, stream, a);  // v3 pipeline
  else hipLaunchKernelGGL((nerf_kernel<NR_PREC_FP32>), dim3(grid), dim3(kThreads), 0, stream, a);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int launch_nerf_train32_fwd(const NerfLayout& L, const void* packed, const float* xe, const float* ve, int64_t P,
                            float* const* h, float* feat, float* hv, float* sigma, float* rgb, hipStream_t stream) {
  if (P <= 0) return NR_OK;
  NR_REQUIRE(L.prec == NR_PREC_FP32, NR_ERR_ARG, "nerf train forward: needs the fp32 render pack");
  NerfTrainFwdArgs a{};
  a.packed = (const char*)packed;
  a.L = L;
  a.xe = xe;
  a.ve = ve;
  a.P = P;
  for (int i = 0; i < 8; ++i) a.h[i] = h[i];
  a.feat = feat;
  a.hv = hv;
  a.sigma = sigma;
  a.rgb = rgb;
  ProfScope prof("nerf_train32_fwd", (double)P, stream);
  hipLaunchKernelGGL(nerf_train32_fwd_kernel, dim3(grid_for(P)), dim3(kThreads), 0, stream, a);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int launch_nerf_train32_bwd(const NerfBwdLayout& B, const void* packed, const float* rgb, const float* hv,
                            const float* const* h, const float* g_rgb, const float* g_sigma, int64_t P, float* g3,
                            float* ghv, float* g_feat, float* const* gz, hipStream_t stream,
                            bool f16x3) {
  if (P <= 0) return NR_OK;
  NerfTrainBwdArgs a{};
  a.packed = (const char*)packed;
  a.B = B;
  a.rgb = rgb;
  a.hv = hv;
  for (int i = 0; i < 8; ++i) a.h[i] = h[i];
  a.g_rgb = g_rgb;
  a.g_sigma = g_sigma;
  a.P = P;
  a.g3 = g3;
  a.ghv = ghv;
  a.g_feat = g_feat;
  for (int i = 0; i < 8; ++i) a.gz[i] = gz[i];
  ProfScope prof("nerf_train32_bwd", (double)P, stream);
  if (f16x3) hipLaunchKernelGGL(nerf_train32_bwd_kernel<NR_PREC_F16X3>, dim3(grid_for(P)), dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL(nerf_train32_bwd_kernel<NR_PREC_FP32>, dim3(grid_for(P)), dim3(kThreads), 0, stream, a);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int launch_radiance_train32(const RadLayout& L, const void* packed, const float* feat, const float* small,
                            int64_t ld_small, int n_small, int64_t P, float* const* h, float* rgb, hipStream_t stream) {
  if (P <= 0) return NR_OK;
  if (L.prec != NR_PREC_FP32 || L.siren || L.D != 4 || (L.kbs != 2 && L.kbs != 4)) {
    set_error("nr_radiance_train_fwd32: needs the fp32 pack of a ReLU D=4 radiance net");
    return NR_ERR_UNSUPPORTED;
  }
  RadTrainArgs a{(const char*)packed, L, feat, small, ld_small, n_small, P, {h[0], h[1], h[2], h[3]}, rgb};
  ProfScope prof("radiance_train32", (double)P, stream);
  if (L.kbs == 2) hipLaunchKernelGGL((radiance_train32_kernel<2>), dim3(grid_for(P)), dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL((radiance_train32_kernel<4>), dim3(grid_for(P)), dim3(kThreads), 0, stream, a);
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

int launch_radiance(const RadLayout& L, const void* packed, const float* x, const float* vdir, int64_t vdiv,
                    int64_t vmod, const float* normals, const float* feature, int64_t P, float* rgb, int nfreq_view,
                    hipStream_t stream, const int* P_dev, const void* r0_fold, int* claim) {
  if (P <= 0) return NR_OK;
  const int grid = grid_for(P);
  NR_REQUIRE(!r0_fold || (L.prec == NR_PREC_F16X3 && !L.siren && L.D == 4), NR_ERR_ARG,
             "radiance: the folded layer 0 needs the f16x3 ReLU D=4 net");
  RadKArgs a{(const char*)packed, L, x, vdir, vdiv, vmod, normals, feature, P, rgb, nfreq_view, P_dev,
             (const char*)r0_fold};
  const RadKArgsC ac{a, claim};  // rad4_kernel<KBS, true>
  ProfScope prof("radiance", (double)P, stream, P_dev, 1);
  const bool h3 = L.prec == NR_PREC_F16X3;
  // (small-input blocks, activation, depth) variants
#define NR_RAD_LAUNCH(KBS, ACT, D)                                                                            \
  do {                                                                                                        \
    if (h3) hipLaunchKernelGGL((radiance_kernel<NR_PREC_F16X3, KBS, ACT, D>), dim3(grid), dim3(kThreads), 0, \
                               stream, a);                                                                    \
    else hipLaunchKernelGGL((radiance_kernel<NR_PREC_FP32, KBS, ACT, D>), dim3(grid), dim3(kThreads), 0,     \
                            stream, a);                                                                       \
  } while (0)
  if (L.kbs != 2 && L.kbs != 4) {
    set_error("radiance: unsupported small-input block count");
    return NR_ERR_UNSUPPORTED;
  }
  if (h3 && !L.siren && L.D == 4) {  // the v3 pipeline (rad4_kernel)
    if (r0_fold) {
      if (L.kbs == 2) hipLaunchKernelGGL((rad4_kernel<2, true>), dim3(grid), dim3(kT4), 0, stream, ac);
      else hipLaunchKernelGGL((rad4_kernel<4, true>), dim3(grid), dim3(kT4), 0, stream, ac);
    } else if (L.kbs == 2) hipLaunchKernelGGL((rad4_kernel<2, false>), dim3(grid), dim3(kT4), 0, stream, a);
    else hipLaunchKernelGGL((rad4_kernel<4, false>), dim3(grid), dim3(kT4), 0, stream, a);
  } else if (!L.siren && L.D == 4) {
    if (L.kbs == 2) NR_RAD_LAUNCH(2, ACT_RELU, 4); else NR_RAD_LAUNCH(4, ACT_RELU, 4);
  } else if (!L.siren && L.D == 5) {
    if (L.kbs == 2) NR_RAD_LAUNCH(2, ACT_RELU, 5); else NR_RAD_LAUNCH(4, ACT_RELU, 5);
  } else if (L.D == 4) {
    if (L.kbs == 2) NR_RAD_LAUNCH(2, ACT_SINE, 4); else NR_RAD_LAUNCH(4, ACT_SINE, 4);
  } else {
    if (L.kbs == 2) NR_RAD_LAUNCH(2, ACT_SINE, 5); else NR_RAD_LAUNCH(4, ACT_SINE, 5);
  }
#undef NR_RAD_LAUNCH
  NR_HIP_CHECK(hipGetLastError());
  return NR_OK;
}

}  // namespace nr

#ifdef NR_EXP_STAMPS
// per-wave phase totals of the last sdf4_kernel launch (stamps builds only)
extern "C" int nr_exp_stamps(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(nr::g_nr_stamps), sizeof(unsigned long long) * (size_t)n) == hipSuccess
             ? nr::kW4 * nr::kStampPh
             : -1;
}
// ... of the last sdf4_kernel launch with STAGE_ = stage (0..4)
extern "C" int nr_exp_stamps_stage(int stage, unsigned long long* out, int n) {
  if (stage < 0 || stage > 4 || n > nr::kStampSlot) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(nr::g_nr_stamps), sizeof(unsigned long long) * (size_t)n,
                             sizeof(unsigned long long) * (size_t)(1 + stage) * nr::kStampSlot) == hipSuccess
             ? nr::kW4 * nr::kStampPh
             : -1;
}
#endif
