// The f32 MFMA tile engine (v_mfma_f32_32x32x2_f32) under the InfoNCE / BCE kernels (gcr_pairs.h and its three units), the
// nearest-centroid search (gcr_kmeans.hip) and the ranking kernels (gcr_rank.hip), with the names its split-operand
// sibling (gcr_b3.h, the header of the split-operand engines EngB3 / EngH2) is written in.  Included at file scope; everything lives in an anonymous namespace.  The other
// MFMA sources (gcr_directau, gcr_buir, gcr_tri, gcr_dense) have loops of their own and take only the accumulator's
// type, its row layout and the tile height from here.
//
// Mapping.  The score tile is computed TRANSPOSED: MFMA "A" = 32 streamed table rows j, MFMA "B" = 32 stationary rows i,
// so in the 32x32 accumulator a lane owns ONE stationary row (column i = lane&31) and its 16 registers are 16 different
// table rows.  The K (= d) dimension is split between the two lane halves (half h covers features [h*d/2, (h+1)*d/2)), so
// each lane's operand slice is contiguous in memory: 16-byte global loads for the stationary rows, and conflict-free
// ds_read_b128 (row stride padded by 16 B) for the streamed tile.  gcr_infonce.hip's header has the whole picture.
#pragma once
#include "gcr_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileJ = 32;

template <int D>
struct Shape {
  static constexpr int KH = D / 2;                       // k-steps per 32x32 tile (2 k per MFMA)
  static constexpr int STRIDE = D + 4;                   // floats; +16 B pad -> conflict-free b128
  static constexpr int NT = D <= 128 ? 2 : 1;            // anchor tiles of 32 per wave
  static constexpr int NLD = (kTileJ * D / 4) / 256;     // float4 staged per thread and tile
  static constexpr int ANCHORS_PER_BLOCK = 4 * 32 * NT;
};

// C/D layout of the 32x32 accumulator: register r of lane (col = lane&31, h = lane>>5) is row
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Branch-free staging load (keeps the tile loop one scheduling region): rows past the table are
// clamped to the last row and multiplied by 0.
template <int D>
__device__ __forceinline__ void stage_load(const float* __restrict__ b, const float* __restrict__ b_scale,
                                           int64_t n_rows, int64_t j0, int tid, float4 (&regs)[Shape<D>::NLD],
                                           float mult = 1.0f) {
#pragma unroll
  for (int u = 0; u < Shape<D>::NLD; ++u) {
    const int idx = tid + 256 * u;
    const int row = idx / (D / 4), c4 = idx % (D / 4);
    const int64_t j = j0 + row;
    const int64_t jj = j < n_rows ? j : n_rows - 1;
    float4 v = *reinterpret_cast<const float4*>(b + jj * D + 4 * c4);
    float s = b_scale != nullptr ? b_scale[jj] * mult : mult;
    s = j < n_rows ? s : 0.f;
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    regs[u] = v;
  }
}

template <int D>
__device__ __forceinline__ void stage_store(float* __restrict__ tile, int tid, const float4 (&regs)[Shape<D>::NLD]) {
#pragma unroll
  for (int u = 0; u < Shape<D>::NLD; ++u) {
    const int idx = tid + 256 * u;
    const int row = idx / (D / 4), c4 = idx % (D / 4);
    *reinterpret_cast<float4*>(tile + row * Shape<D>::STRIDE + 4 * c4) = regs[u];
  }
}

// stationary operand: lane (i = lane&31, h) holds features [h*KH, (h+1)*KH) of its row, pre-scaled
template <int D>
__device__ __forceinline__ void load_stationary(const float* __restrict__ a, const float* __restrict__ a_scale,
                                                int64_t m_rows, int64_t row, int h, float mult,
                                                float (&frag)[Shape<D>::KH]) {
  const bool valid = row < m_rows;
  const float s = valid ? (a_scale != nullptr ? a_scale[row] : 1.0f) * mult : 0.f;
  const float* p = a + (valid ? row : 0) * D + h * Shape<D>::KH;
#pragma unroll
  for (int q = 0; q < Shape<D>::KH / 4; ++q) {
    float4 v = valid ? *reinterpret_cast<const float4*>(p + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    frag[4 * q + 0] = v.x * s;
    frag[4 * q + 1] = v.y * s;
    frag[4 * q + 2] = v.z * s;
    frag[4 * q + 3] = v.w * s;
  }
}

// S^T tile: acc[t][r] = log2-domain logit of (table row acc_row(r,h), anchor tile t / lane&31)
template <int D>
__device__ __forceinline__ void score_tile(const float* __restrict__ tile, int i32, int h,
                                           const float (&bfrag)[Shape<D>::NT][Shape<D>::KH],
                                           f32x16 (&acc)[Shape<D>::NT]) {
#pragma unroll
  for (int t = 0; t < Shape<D>::NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* base = tile + i32 * Shape<D>::STRIDE + h * Shape<D>::KH;
#pragma unroll
  for (int q = 0; q < Shape<D>::KH / 4; ++q) {
    const float4 av = *reinterpret_cast<const float4*>(base + 4 * q);
    const float ae[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < Shape<D>::NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae[e], bfrag[t][4 * q + e], acc[t], 0, 0, 0);
  }
}

// Which engine and which widths: shared by the InfoNCE / BCE launches and the k-means search.  The split-operand bf16
// engine (gcr_b3.h) serves d <= 128 unless the caller forces the f32 MFMA; gcr_pairs.h says why it is an argument.
bool use_b3(int d, bool force_f32 = false) { return d <= 128 && !force_f32; }
bool dim_supported(int d) { return d == 32 || d == 64 || d == 128 || d == 256; }

}  // namespace
