// Fused batch-row gather + seeded element-wise dropout views (gfx950), forward and backward.
//
// ssl4rec.py:192-196 gathers the batch's item rows and pushes two `nn.Dropout` draws of them through the item tower:
// three [B, d] tensors, two mask tensors kept for the backward, and three index_put(accumulate) sorts behind them.  Here
// the clean rows and the V dropped views come out of ONE pass over the gathered rows, stacked [(1 + V) * n, d] so that
// the tower runs once over all of them, and the backward folds all 1 + V gradient blocks into one float atomic per
// table element.
//
// No mask is stored: bit e = i * d + c of view v is bit e of gcr_edge_mask_bits(n * d, p, seed + v) — the same Philox
// stream, counter block e >> 2, word e & 3, the same 24-bit grid and `keep = u >= p` — so the forward and the backward
// regenerate it from (seed, p).  With d % 4 == 0 a lane's four columns are one counter block: one Philox call per view.
// A recorded bitmap (keep_bits, [V, ceil(n * d / 32)] words in that bit order) replaces the draws when given.
#include "gcr_common.h"
#include "gcr_host.h"
#include "gcr_philox.h"

namespace {

constexpr uint32_t kStreamEdge = 0x45444745u;  // 'EDGE': gcr_rng.hip's mask stream
constexpr float kU24 = 5.9604644775390625e-8f;  // 2^-24

__device__ __forceinline__ U4 mask_block(uint64_t blk, uint64_t seed) {
  return philox4x32_10(U4{(uint32_t)blk, (uint32_t)(blk >> 32), 0u, kStreamEdge}, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// keep bits (bit t <-> element e0 + t) of the four elements of counter block e0 >> 2; e0 % 4 == 0
__device__ __forceinline__ uint32_t keep4(uint64_t e0, float p, uint64_t seed, const uint32_t* __restrict__ bits) {
  if (bits != nullptr) return (bits[e0 >> 5] >> (e0 & 31)) & 0xFu;
  const U4 r = mask_block(e0 >> 2, seed);
  return (uint32_t)((float)(r.x >> 8) * kU24 >= p) | (uint32_t)((float)(r.y >> 8) * kU24 >= p) << 1 |
         (uint32_t)((float)(r.z >> 8) * kU24 >= p) << 2 | (uint32_t)((float)(r.w >> 8) * kU24 >= p) << 3;
}

__device__ __forceinline__ bool keep1(uint64_t e, float p, uint64_t seed, const uint32_t* __restrict__ bits) {
  if (bits != nullptr) return (bits[e >> 5] >> (e & 31)) & 1u;
  const U4 r = mask_block(e >> 2, seed);
  const int w = (int)(e & 3);
  const uint32_t x = w == 0 ? r.x : (w == 1 ? r.y : (w == 2 ? r.z : r.w));
  return (float)(x >> 8) * kU24 >= p;
}

// one wave per batch row, 16 B per lane; block 0 of `out` is the gathered row, block 1 + v its view v
__global__ __launch_bounds__(256) void gather_dropout_vec4_kernel(const float4* __restrict__ table, const int64_t* __restrict__ idx,
                                                                  int64_t n, int d4, int64_t n_rows, float p, float scale,
                                                                  uint64_t seed, int n_views,
                                                                  const uint32_t* __restrict__ keep_bits, int64_t n_words,
                                                                  float4* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
    const int64_t r = idx[i];
    const bool ok = r >= 0 && r < n_rows;
    for (int q = lane; q < d4; q += 64) {
      const float4 x = ok ? table[r * d4 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
      out[i * d4 + q] = x;
      const uint64_t e0 = ((uint64_t)i * d4 + q) << 2;
      for (int v = 0; v < n_views; ++v) {
        const uint32_t m = keep4(e0, p, seed + v, keep_bits != nullptr ? keep_bits + v * n_words : nullptr);
        out[((int64_t)(1 + v) * n + i) * d4 + q] = make_float4((m & 1u) ? x.x * scale : 0.f, (m & 2u) ? x.y * scale : 0.f,
                                                              (m & 4u) ? x.z * scale : 0.f, (m & 8u) ? x.w * scale : 0.f);
      }
    }
  }
}

// any d (and unaligned pointers): one wave per batch row, one column per lane, one Philox call per element and view
__global__ __launch_bounds__(256) void gather_dropout_kernel(const float* __restrict__ table, const int64_t* __restrict__ idx,
                                                             int64_t n, int d, int64_t n_rows, float p, float scale,
                                                             uint64_t seed, int n_views, const uint32_t* __restrict__ keep_bits,
                                                             int64_t n_words, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
    const int64_t r = idx[i];
    const bool ok = r >= 0 && r < n_rows;
    for (int c = lane; c < d; c += 64) {
      const float x = ok ? table[r * d + c] : 0.f;
      out[i * d + c] = x;
      const uint64_t e = (uint64_t)i * d + c;
      for (int v = 0; v < n_views; ++v) {
        const bool k = keep1(e, p, seed + v, keep_bits != nullptr ? keep_bits + v * n_words : nullptr);
        out[((int64_t)(1 + v) * n + i) * d + c] = k ? x * scale : 0.f;
      }
    }
  }
}

// grad_table[idx[i], c] += g0[i, c] + scale * sum_v keep_v[i, c] * g_v[i, c].  The lanes read 16 B (one counter block)
// each, then the 256 sums of a 256-column chunk change hands inside the wave so that every atomic wave-instruction is
// 256 contiguous bytes of the destination row (the shape float atomics run fastest in), one atomic per element.
__global__ __launch_bounds__(256) void gather_dropout_bwd_vec4_kernel(const float4* __restrict__ g, const int64_t* __restrict__ idx,
                                                                      int64_t n, int d, int64_t n_rows, float p, float scale,
                                                                      uint64_t seed, int n_views,
                                                                      const uint32_t* __restrict__ keep_bits, int64_t n_words,
                                                                      float* __restrict__ grad_table) {
  const int lane = threadIdx.x & 63;
  const int d4 = d >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
    const int64_t r = idx[i];
    if (r < 0 || r >= n_rows) continue;          // wave-uniform
    float* __restrict__ dst = grad_table + r * d;
    for (int base = 0; base < d; base += 256) {
      const int q = (base >> 2) + lane;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < d4) {
        const float4 g0 = g[i * d4 + q];
        const uint64_t e0 = ((uint64_t)i * d4 + q) << 2;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int v = 0; v < n_views; ++v) {
          const uint32_t m = keep4(e0, p, seed + v, keep_bits != nullptr ? keep_bits + v * n_words : nullptr);
          const float4 gv = g[((int64_t)(1 + v) * n + i) * d4 + q];
          s.x += (m & 1u) ? gv.x : 0.f;
          s.y += (m & 2u) ? gv.y : 0.f;
          s.z += (m & 4u) ? gv.z : 0.f;
          s.w += (m & 8u) ? gv.w : 0.f;
        }
        acc = make_float4(fmaf(scale, s.x, g0.x), fmaf(scale, s.y, g0.y), fmaf(scale, s.z, g0.z), fmaf(scale, s.w, g0.w));
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (base + 64 * t >= d) break;           // wave-uniform
        const int src = 16 * t + (lane >> 2);    // column base + 64 t + lane is component lane & 3 of that lane's four
        const float a0 = __shfl(acc.x, src, GCR_WAVE), a1 = __shfl(acc.y, src, GCR_WAVE);
        const float a2 = __shfl(acc.z, src, GCR_WAVE), a3 = __shfl(acc.w, src, GCR_WAVE);
        const int w = lane & 3;
        const float val = w == 0 ? a0 : (w == 1 ? a1 : (w == 2 ? a2 : a3));
        const int c = base + 64 * t + lane;
        if (c < d) atomicAdd(dst + c, val);
      }
    }
  }
}

__global__ __launch_bounds__(256) void gather_dropout_bwd_kernel(const float* __restrict__ g, const int64_t* __restrict__ idx,
                                                                 int64_t n, int d, int64_t n_rows, float p, float scale,
                                                                 uint64_t seed, int n_views, const uint32_t* __restrict__ keep_bits,
                                                                 int64_t n_words, float* __restrict__ grad_table) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
    const int64_t r = idx[i];
    if (r < 0 || r >= n_rows) continue;
    for (int c = lane; c < d; c += 64) {
      const uint64_t e = (uint64_t)i * d + c;
      float s = 0.f;
      for (int v = 0; v < n_views; ++v) {
        const bool k = keep1(e, p, seed + v, keep_bits != nullptr ? keep_bits + v * n_words : nullptr);
        s += k ? g[((int64_t)(1 + v) * n + i) * d + c] : 0.f;
      }
      atomicAdd(grad_table + r * d + c, fmaf(scale, s, g[i * d + c]));
    }
  }
}

int dropout_grid(int64_t n) { return (int)gcr_grid((n + 3) / 4, 8192); }

}  // namespace

extern "C" int32_t gcr_gather_dropout_f32(const float* table, const int64_t* idx, int64_t n, int32_t d, int64_t n_rows,
                                          float p, uint64_t seed, int32_t n_views, const uint32_t* keep_bits, float* out,
                                          void* stream) {
  GCR_CHECK_ARG(n >= 0 && d >= 1 && n_rows >= 0 && n_views >= 1 && n_views <= 4 && p >= 0.f && p <= 1.f);
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(table && idx && out);
  const float scale = 1.0f / (1.0f - p);       // p == 1: inf, never multiplied (no element is kept)
  const int64_t n_words = (n * d + 31) / 32;
  if (d % 4 == 0 && aligned16(table, out))
    hipLaunchKernelGGL(gather_dropout_vec4_kernel, dim3(dropout_grid(n)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(table), idx, n, d / 4, n_rows, p, scale, seed, n_views, keep_bits,
                       n_words, reinterpret_cast<float4*>(out));
  else
    hipLaunchKernelGGL(gather_dropout_kernel, dim3(dropout_grid(n)), dim3(256), 0, (hipStream_t)stream, table, idx, n, d,
                       n_rows, p, scale, seed, n_views, keep_bits, n_words, out);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_gather_dropout_bwd_f32(const float* grad_out, const int64_t* idx, int64_t n, int32_t d, int64_t n_rows,
                                              float p, uint64_t seed, int32_t n_views, const uint32_t* keep_bits,
                                              float* grad_table, void* stream) {
  GCR_CHECK_ARG(n >= 0 && d >= 1 && n_rows >= 0 && n_views >= 1 && n_views <= 4 && p >= 0.f && p <= 1.f);
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(grad_out && idx && grad_table);
  const float scale = p < 1.f ? 1.0f / (1.0f - p) : 0.f;      // p == 1: every view is zero, only block 0 has a gradient
  const int64_t n_words = (n * d + 31) / 32;
  if (d % 4 == 0 && aligned16(grad_out))
    hipLaunchKernelGGL(gather_dropout_bwd_vec4_kernel, dim3(dropout_grid(n)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(grad_out), idx, n, d, n_rows, p, scale, seed, n_views, keep_bits,
                       n_words, grad_table);
  else
    hipLaunchKernelGGL(gather_dropout_bwd_kernel, dim3(dropout_grid(n)), dim3(256), 0, (hipStream_t)stream, grad_out, idx, n,
                       d, n_rows, p, scale, seed, n_views, keep_bits, n_words, grad_table);
  return GCR_LAUNCH_STATUS();
}
