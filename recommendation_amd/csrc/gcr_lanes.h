// Lane-level reductions shared by the loss, dense, BPR and k-means units (gfx950; wave = 64 lanes).  gcr_common.h keeps the
// full-wave float sum / max; everything narrower or wider than that lives here, once.
#pragma once
#include "gcr_common.h"

__device__ __forceinline__ float gcr_dot4(const float4& a, const float4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// butterfly sum over aligned groups of LPR lanes (a power of two <= 64): every lane ends with its group's total
template <int LPR>
__device__ __forceinline__ float gcr_group_sum(float v) {
#pragma unroll
  for (int off = LPR / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, GCR_WAVE);
  return v;
}

// The same over groups of 16 lanes with the shuffles confined to the group (width 16).  gcr_group_sum<16> gives the same sums
// but other instructions in bpr_fwd_kernel and kmeans_finalize_kernel (EXPERIMENTS.md, "Loss, dense and BPR units: one copy
// ..."), so the callers that were written against this form keep it.
__device__ __forceinline__ float gcr_group16_sum(float v) {
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}

__device__ __forceinline__ double gcr_wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, GCR_WAVE);
  return v;
}

// Sum over `nblocks` per-workgroup partials of output k (part[b * elems + k]) by four lanes per output: lane q of the four
// adds its quarter of the partials in block order, loads eight deep, then the quarters are added in a fixed order — every
// lane of the four returns the total, bitwise reproducible.  All lanes call it; live = false contributes nothing.  (One
// thread per output walking all 1024 partials was a chain of 1024 dependent memory round trips: 229 us for a 64 x 64
// output, ten times the product that made the partials.)
__device__ __forceinline__ float gcr_fold_partials4(const float* __restrict__ part, int nblocks, int elems, int k, int q,
                                                    bool live) {
  float s = 0.f;
  if (live) {
    const int per = (nblocks + 3) / 4;
    const int b0 = q * per, b1 = min(nblocks, b0 + per);
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(b + u) * elems + k];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < b1; ++b) s += part[(int64_t)b * elems + k];
  }
  s += __shfl_xor(s, 1, 4);
  s += __shfl_xor(s, 2, 4);
  return s;
}
