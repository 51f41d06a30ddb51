// The split-operand MFMA engines: the operand formats EngB3 (three bf16 planes) and EngH2 (two f16 planes) and the tile
// helpers templated on them (load_stationary_e, stage_store_e, score_tile_e), shared by the InfoNCE / BCE kernels (gcr_pairs.h,
// gcr_pairs_loop.h), the nearest-centroid search (gcr_kmeans.hip) and the fused ranking kernel (gcr_rank.hip).  Included at
// file scope like any other header, it brings gcr_tile.h's names with it and keeps its own in an anonymous namespace.
#pragma once
#include "gcr_tile.h"

namespace {

// ------------------------------------------------------------------------------------------
// Split-operand engine ("b3").  gfx950's bf16 MFMA (v_mfma_f32_32x32x16_bf16) runs at 16x the rate
// of the f32 MFMA and accumulates in f32.  Every f32 operand x is split ERROR-FREE into three
// bf16 planes x = x1 + x2 + x3 (+ <= 2^-27 |x|): x1 = bf16_rn(x), x2 = bf16_rn(x - x1),
// x3 = bf16_rn(x - x1 - x2), the subtractions being exact in f32; bf16 has the exponent range of
// f32, so this holds for any finite input.  A product x*y is then the six terms
//   x1y1 + (x1y2 + x2y1) + (x2y2 + x1y3 + x3y1),
// the dropped ones (x2y3, x3y2, x3y3) being <= 2^-26 |xy|, below the rounding of the f32
// accumulator that both engines share.  Six bf16 MFMAs of K = 16 replace eight f32 MFMAs of K = 2
// per 16 features: 2.67x fewer matrix-core cycles at f32 accuracy (the parity tests run on both
// engines with the same tolerances).  The split happens once per element: anchors when they are
// loaded, table rows on their way into LDS (three planes, 16-B padded rows, conflict-free b128).
// ------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){lo, hi}, bf16x2));   // v_cvt_pk_bf16_f32 (RNE)
}
__device__ __forceinline__ float bf16_lo(unsigned p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float bf16_hi(unsigned p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

// two f32 -> three packed bf16 pairs (planes 1..3)
__device__ __forceinline__ void split3(float a, float b, unsigned& p1, unsigned& p2, unsigned& p3) {
  p1 = pack_bf16(a, b);
  a -= bf16_lo(p1);
  b -= bf16_hi(p1);
  p2 = pack_bf16(a, b);
  a -= bf16_lo(p2);
  b -= bf16_hi(p2);
  p3 = pack_bf16(a, b);
}

template <int D>
struct ShapeB3 {
  static constexpr int KH = D / 2;                       // features per lane half
  static constexpr int KC = KH / 8;                      // MFMA k-chunks (8 bf16 per lane) per product term
  static constexpr int ROWB = 2 * D + 16;                // bytes per LDS row and plane (+16 B pad)
  static constexpr int PLANE = kTileJ * ROWB;            // bytes per plane
  static constexpr int NT = D <= 64 ? 2 : 1;             // anchor tiles of 32 per wave
  static constexpr int NLD = (kTileJ * D / 4) / 256;
  static constexpr int ANCHORS_PER_BLOCK = 4 * 32 * NT;
};

__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// deferred rescale of the flash forwards: the reference point of a row's running sums only moves when a tile's
// maximum exceeds it by more than 2^kDefer
constexpr float kDefer = 8.0f;

// ------------------------------------------------------------------------------------------
// The two operand formats of the split-operand kernels (forward, and the pipelined two-product loop).
//   EngB3  three bf16 planes, six product terms (above): any finite f32 operand, f32 accuracy.
//   EngH2  two f16 planes, THREE product terms: x = hi + lo with hi = f16(x), lo = f16(x - hi) (RNE,
//          v_cvt_pk_f16_f32) leaves <= 2^-22 |x|; hi*hi + hi*lo + lo*hi drops lo*lo (2^-22): half the matrix-core work of
//          EngB3 at an error of a few f32 roundings per product.  f16 has a 5-bit exponent, so the format is only used for
//          operands whose range is known — rows of at most unit norm (the caller's promise GCR_INFONCE_UNIT_ROWS; every
//          contrast loss of the reference normalises) and probabilities — each pre-scaled by a power of two that keeps its
//          largest value inside the f16 range and its typical values' residuals in the normal range:
//            stationary rows (<= inv_tau log2 e, inv_tau <= kH2MaxInvTau)   x 2^-2     (|.| <= 7.3)
//            streamed rows   (<= 1)                                          x 2^2
//            scores                                                          = the accumulator (product of the pre-scales 1)
//            P, MODE 1 (<= 2^kDefer = 2 relative to the lagging reference)   x 2^14
//            P, MODE 0 (w e^{s - lse} <= 2 max|w|)                           x 2^14 / 2^ceil(log2 max|w|) (max|w| from a
//                                                                            one-block pre-pass, h2_wscale_kernel)
//          Values below the f16 normal range (2^-14 after scaling: a row element under 2^-22, a probability 2^-28 under
//          the reference) go sub-normal, which v_cvt_pk_f16_f32 produces and v_mfma_f32_32x32x16_f16 honours
//          (scripts/exp/f16_denorm_probe.hip, run on the box): their absolute error stays <= 2^-25 of the scaled unit.
// ------------------------------------------------------------------------------------------
struct EngB3 {
  static constexpr int NPL = 3, NTERM = 6;
  static constexpr int kMinBlocks = 2;
  static constexpr float kSX = 1.0f, kSY = 1.0f;         // operand pre-scales
  static constexpr float kSInv = 1.0f;                   // accumulator -> log2-domain score
  static constexpr float kPExp = 0.0f;                   // log2 of the scale of P
  static constexpr float kDeferE = kDefer;
  static __host__ __device__ constexpr int ta(int t) { constexpr int v[6] = {2, 0, 1, 1, 0, 0}; return v[t]; }   // streamed-side
  static __host__ __device__ constexpr int tb(int t) { constexpr int v[6] = {0, 2, 1, 0, 1, 0}; return v[t]; }   // plane / other
  static __device__ __forceinline__ void split(float a, float b, unsigned (&p)[3]) { split3(a, b, p[0], p[1], p[2]); }
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) { return mfma_bf16(a, b, c); }
};

struct EngH2 {
  static constexpr int NPL = 2, NTERM = 3;
  static constexpr int kMinBlocks = 2;          // 3 would cap the kernel at 168 VGPRs: 11-52 spilled dwords, 4-12 % slower
  // Operand pre-scales whose PRODUCT is 1 (round 4; rounds 2-3 used 2^4 and 2^8 with an accumulator scale of 2^-12): the
  // accumulator then IS the log2-domain score and the `acc * 2^-12 - m` fma in front of every exp2 disappears — one vector
  // instruction per probability less in loops whose time is their count of vector instructions.  Emulated in
  // numpy over 20 000 row pairs per case (unit rows, near-duplicates, rows with a few large and many tiny elements; d = 32 /
  // 64; 1/tau = 2 / 10 / 20): worst |score error| 0.91e-6 / 1.90e-6 / 1.04e-6 at 1/tau = 10, against 0.89e-6 / 1.84e-6 /
  // 1.01e-6 with the old pre-scales — what matters for the f16 residual planes is that typical elements stay above 2^-3
  // (stationary rows carry the 1/tau log2 e factor: ~0.45-0.9 after x 2^-2; streamed unit rows ~0.5 after x 2^2), below it
  // a residual goes sub-normal with ABSOLUTE error <= 2^-25, which the dot product tolerates (tests/test_h2_format_cpu.py).
  static constexpr float kSX = 0.25f, kSY = 4.0f;
  static constexpr float kSInv = 1.0f;
  static constexpr float kPExp = 14.0f;
  static constexpr float kDeferE = 1.0f;
  static __host__ __device__ constexpr int ta(int t) { constexpr int v[3] = {1, 0, 0}; return v[t]; }
  static __host__ __device__ constexpr int tb(int t) { constexpr int v[3] = {0, 1, 0}; return v[t]; }
  // The lo plane = f16(x - hi): the residual comes out of ONE v_fma_mix_f32 per value, which reads the f16 half of `hi` in
  // place and subtracts it from the f32 value in f32 (exact: the difference of a value and its 11-bit rounding has <= 13
  // significant bits); a second convert rounds the pair to f16 (RNE, sub-normals kept): four instructions per pair.
  // Three forms of this split were measured on one box at 2048 x 1M x 64, all bit for bit the same planes: form 0 = convert,
  // two f16 -> f32 converts, two subtracts, convert (six instructions per pair); form 1 = this one; form 2 = the lo plane
  // straight out of v_fma_mixlo_f16 / v_fma_mixhi_f16 (three):
  //   MODE 1 (flash forward)        form 0: 1.81 ms   form 1: 1.70   form 2: same as form 1 within noise
  //   MODE 0 (table-side backward)  round 2 (175 vector instructions per tile): form 0: 1.78 ms, 1: 1.88, 2: 1.90;
  //                                 round 3 (110 per tile after the fold pre-pass): form 0: 1.39 ms, 1: 1.32, 2: 1.33
  //                                 (100K x 100K, 8 waves: 7.00 / 6.49 / 6.53; d = 32: 0.814 / 0.773 / 0.787)
  // Form 2 never beats form 1 although it is one instruction shorter per pair: the f16-destination mixed forms issue at
  // about twice the cost of a plain vector instruction.  Only form 1 is kept.
  static __device__ __forceinline__ void split(float a, float b, unsigned (&p)[2]) {
    const f16x2 hi = __builtin_convertvector((f32x2){a, b}, f16x2);                 // v_cvt_pk_f16_f32, RNE
    p[0] = __builtin_bit_cast(unsigned, hi);
    float ra, rb;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(p[0]), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(p[0]), "v"(b));
    p[1] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){ra, rb}, f16x2));
  }
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

// stationary operand planes of engine E: frag[p][c] = 8 consecutive features [h*KH + 8c, +8) of plane p
template <class E, int D>
__device__ __forceinline__ void load_stationary_e(const float* __restrict__ a, const float* __restrict__ a_scale,
                                                  int64_t m_rows, int64_t row, int h, float mult,
                                                  u32x4 (&frag)[E::NPL][ShapeB3<D>::KC]) {
  using S = ShapeB3<D>;
  const bool valid = row < m_rows;
  const float s = valid ? (a_scale != nullptr ? a_scale[row] : 1.0f) * mult : 0.f;
  const float* p = a + (valid ? row : 0) * D + h * S::KH;
#pragma unroll
  for (int c = 0; c < S::KC; ++c) {
    const float4 v0 = valid ? *reinterpret_cast<const float4*>(p + 8 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 v1 = valid ? *reinterpret_cast<const float4*>(p + 8 * c + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned q[4][E::NPL];
    E::split(v0.x * s, v0.y * s, q[0]);
    E::split(v0.z * s, v0.w * s, q[1]);
    E::split(v1.x * s, v1.y * s, q[2]);
    E::split(v1.z * s, v1.w * s, q[3]);
#pragma unroll
    for (int pl = 0; pl < E::NPL; ++pl) frag[pl][c] = (u32x4){q[0][pl], q[1][pl], q[2][pl], q[3][pl]};
  }
}

// one staged float4 of the streamed tile -> NPL row-major planes in LDS
template <class E, int D>
__device__ __forceinline__ void stage_store_e_one(unsigned char* __restrict__ tile, int tid, const float4& v, int u) {
  using S = ShapeB3<D>;
  const int idx = tid + 256 * u;
  const int row = idx / (D / 4), c4 = idx % (D / 4);
  unsigned qa[E::NPL], qb[E::NPL];
  E::split(v.x, v.y, qa);
  E::split(v.z, v.w, qb);
  unsigned char* p = tile + row * S::ROWB + c4 * 8;
#pragma unroll
  for (int pl = 0; pl < E::NPL; ++pl) *reinterpret_cast<uint2*>(p + pl * S::PLANE) = make_uint2(qa[pl], qb[pl]);
}

template <class E, int D>
__device__ __forceinline__ void stage_store_e(unsigned char* __restrict__ tile, int tid,
                                              const float4 (&regs)[ShapeB3<D>::NLD]) {
#pragma unroll
  for (int u = 0; u < ShapeB3<D>::NLD; ++u) stage_store_e_one<E, D>(tile, tid, regs[u], u);
}

// S^T tile (streamed rows x stationary rows) as in score_tile, NTERM products per k-chunk, smallest terms first
template <class E, int D, int NT>
__device__ __forceinline__ void score_tile_e(const unsigned char* __restrict__ tile, int i32, int h,
                                             const u32x4 (&bq)[NT][E::NPL][ShapeB3<D>::KC], f32x16 (&acc)[NT]) {
  using S = ShapeB3<D>;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const unsigned char* base = tile + i32 * S::ROWB + h * (S::KH * 2);
#pragma unroll
  for (int c = 0; c < S::KC; ++c) {
    u32x4 ap[E::NPL];
#pragma unroll
    for (int pl = 0; pl < E::NPL; ++pl) ap[pl] = *reinterpret_cast<const u32x4*>(base + pl * S::PLANE + 16 * c);
#pragma unroll
    for (int term = 0; term < E::NTERM; ++term)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = E::mfma(ap[E::ta(term)], bq[t][E::tb(term)][c], acc[t]);
  }
}

}  // namespace
