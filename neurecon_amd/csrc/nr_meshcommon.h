// neurecon_amd — the building blocks the mesh kernels share (nr_mcubes, nr_meshops, nr_meshsample, nr_nn,
// nr_meshrender, nr_meshcull) and nr_surface's workspace plans: the workspace round-up, the face-index check, the
// workgroup prefix over wave totals and the one-workgroup scan of per-workgroup sums.  Exact fp32 / fp64
// arithmetic (f* / d*) and the launch helper are in nr_common.h.
#pragma once
#include "nr_common.h"

namespace nr {

// every workspace array starts on a 256-byte boundary
static inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

// a face may be dereferenced iff its three indices name vertices of [0, V)
__device__ __forceinline__ bool face_valid(int a, int b, int c, int64_t V) {
  return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

// Sum of `mine` (one value per wave, the same in all its lanes) over the workgroup's earlier waves; the total
// over all WG / 64 waves in `all`.  lds: WG / 64 ints.  Holds two barriers: EVERY thread of the workgroup must
// call it, so a call stands ahead of its kernel's early returns.
template <int WG>
__device__ __forceinline__ int wave_prefix(int mine, int* lds, int& all) {
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = mine;
  __syncthreads();
  int pre = 0;
  all = 0;
#pragma unroll
  for (int w = 0; w < WG / 64; ++w) {
    const int v = lds[w];
    pre += w < wave ? v : 0;
    all += v;
  }
  __syncthreads();
  return pre;
}

// Exclusive scan in place of nb items by ONE workgroup of WG threads: thread t owns the contiguous strip
// [t L, (t + 1) L), L = ceil(nb / WG), clipped to nb.  The strip sums go through a Hillis-Steele scan in LDS
// (s: WG accumulators), then every thread rewrites its strip with the bases.  get(q) reads item q as an Acc,
// put(q, base) stores the sum of the items before q.  Returns the total of all items, in every thread.  Acc is
// an integer type, or a struct of integers with += and -: the sums do not depend on their order.  Holds
// barriers: every thread of the workgroup must call it.
template <int WG, class Acc, class Get, class Put>
__device__ __forceinline__ Acc strip_scan(int64_t nb, Acc* s, Get get, Put put) {
  const int tid = threadIdx.x;
  const int64_t L = (nb + WG - 1) / WG;
  const int64_t lo = tid * L < nb ? tid * L : nb, hi = lo + L < nb ? lo + L : nb;
  Acc a{};
  for (int64_t q = lo; q < hi; ++q) a += get(q);
  s[tid] = a;
  __syncthreads();
  for (int off = 1; off < WG; off <<= 1) {
    Acc x{};
    if (tid >= off) x = s[tid - off];
    __syncthreads();
    s[tid] += x;
    __syncthreads();
  }
  Acc e = s[tid] - a;
  for (int64_t q = lo; q < hi; ++q) {
    const Acc c = get(q);
    put(q, e);
    e += c;
  }
  return s[WG - 1];
}

}  // namespace nr
