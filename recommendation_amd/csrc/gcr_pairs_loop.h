// The split-operand two-product kernels of the all-pairs losses: a score tile S = X Y^T is recomputed and, without leaving the register
// file, multiplied back into the streamed rows (P(S) Y) — the InfoNCE backward and flash-style forward (launched from
// gcr_infonce_flash.hip) and the BCE-with-logits forward / backward (gcr_bce.hip).  Kernel templates only: every
// instantiation is made by exactly one of those two units.  Shared pieces and launch plans: gcr_pairs.h.
#pragma once
#include "gcr_pairs.h"

namespace {

// ------------------------------------------------------------------------------------------
// Backward on the split-operand engine (d <= 64).  Same structure as infonce_bwd_kernel; the score
// tile is recomputed with exactly the forward's sequence of bf16 MFMAs (bitwise the forward's
// logits when the roles are the forward's, so sum_j P_ij = 1 to rounding), P is split into three
// bf16 planes in registers (an accumulator register pair -> one packed dword of each plane: the
// accumulator layout is already the B-operand layout of the 32x32x16 MFMA, k = the 8 + 8 streamed
// rows a lane holds per 16-row chunk), and the second product reads its A operand
// yhat[rows][feature] from a TRANSPOSED copy of the three planes in LDS ([feature][row] bf16,
// 72-B rows: conflict-free ds_read_b64), staged together with the row-major planes.
// ------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void stage_store_b3t_one(unsigned char* __restrict__ tile, int tid, const float4& v, int u) {
  using S = ShapeB3<D>;
  using B = BwdB3<D>;
  const int idx = tid + 256 * u;
  const int row = idx / (D / 4), c4 = idx % (D / 4);
  unsigned a1, a2, a3, b1, b2, b3;
  split3(v.x, v.y, a1, a2, a3);
  split3(v.z, v.w, b1, b2, b3);
  unsigned char* p = tile + row * S::ROWB + c4 * 8;
  *reinterpret_cast<uint2*>(p) = make_uint2(a1, b1);
  *reinterpret_cast<uint2*>(p + S::PLANE) = make_uint2(a2, b2);
  *reinterpret_cast<uint2*>(p + 2 * S::PLANE) = make_uint2(a3, b3);
  unsigned short* q = reinterpret_cast<unsigned short*>(tile + 3 * S::PLANE + (4 * c4) * B::RT + row * 2);
  const unsigned pa[3] = {a1, a2, a3}, pb[3] = {b1, b2, b3};
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    unsigned short* qq = q + pl * (B::TPLANE / 2);
    qq[0] = (unsigned short)(pa[pl] & 0xffffu);
    qq[B::RT / 2] = (unsigned short)(pa[pl] >> 16);
    qq[2 * (B::RT / 2)] = (unsigned short)(pb[pl] & 0xffffu);
    qq[3 * (B::RT / 2)] = (unsigned short)(pb[pl] >> 16);
  }
}

// SIDES: which softmax terms of P are live — 0 both, 1 only the stationary rows' (w_x, lse_x), 2 only the
// streamed rows' (w_y, lse_y): a dead term costs an exp2 and an FMA per score in the exposed part of the loop.
template <int D, bool EXD = false, int SIDES = 0>
__global__ __launch_bounds__(256, 2) void infonce_bwd_b3_kernel(
    const float* __restrict__ x, const float* __restrict__ x_scale, int64_t mx, const float* __restrict__ y,
    const float* __restrict__ y_scale, int64_t ny, float scale2, float out_scale, const float* __restrict__ lse_x,
    const float* __restrict__ w_x, const float* __restrict__ lse_y, const float* __restrict__ w_y, int nsplit,
    int64_t tiles_per_split, float* __restrict__ gpart) {
  using S = ShapeB3<D>;
  using B = BwdB3<D>;
  // d = 128: one tile is 54 KB (row-major + transposed planes): a single LDS buffer (two barriers per tile,
  // two blocks per CU cover each other) instead of the double buffer of d <= 64
  constexpr int NBUF = D <= 64 ? 2 : 1;
  __shared__ __align__(16) unsigned char lds[NBUF][B::TILE_BYTES];
  __shared__ __align__(16) float st_lse[2][kTileJ];
  __shared__ __align__(16) float st_w[2][kTileJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t mblk = blockIdx.x / nsplit;
  const int split = blockIdx.x % nsplit;
  const int64_t row_i = (mblk * 4 + wave) * 32 + i32;

  u32x4 bq[1][3][S::KC];
  load_stationary_e<EngB3, D>(x, x_scale, mx, row_i, h, scale2, bq[0]);
  const bool on_x = row_i < mx && w_x != nullptr;
  const float wl = on_x ? w_x[row_i] : 0.f;
  const float lse2l = on_x ? lse_x[row_i] * kLog2e : 1.0e30f;    // disabled term: exp2(-huge) = 0, never 0 * inf
  f32x16 gacc[B::CT];
#pragma unroll
  for (int c = 0; c < B::CT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[c][r] = 0.f;

  const int64_t total_tiles = (ny + kTileJ - 1) / kTileJ;
  const int64_t tile0 = (int64_t)split * tiles_per_split;
  const int64_t tile1 = min(total_tiles, tile0 + tiles_per_split);
  float4 regs[S::NLD];
  float s_lse = 0.f, s_w = 0.f;
  auto load_stats = [&](int64_t j0) {
    if (tid < kTileJ) {
      const int64_t j = j0 + tid;
      const bool on = j < ny && w_y != nullptr;
      s_w = on ? w_y[j] : 0.f;
      s_lse = on ? lse_y[j] * kLog2e : 1.0e30f;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int u = 0; u < S::NLD; ++u) stage_store_b3t_one<D>(lds[buf % NBUF], tid, regs[u], u);
    if (tid < kTileJ) {
      st_lse[buf][tid] = s_lse;
      st_w[buf][tid] = s_w;
    }
  };
  {
    if (tile0 < tile1) {
      stage_load<D>(y, y_scale, ny, tile0 * kTileJ, tid, regs);
      load_stats(tile0 * kTileJ);
      store_tile(0);
    }
    __syncthreads();
    for (int64_t tt = tile0; tt < tile1; ++tt) {
      const int cur = (int)((tt - tile0) & 1);
      const bool more = tt + 1 < tile1;
      if (more) {
        stage_load<D>(y, y_scale, ny, (tt + 1) * kTileJ, tid, regs);
        load_stats((tt + 1) * kTileJ);
      }
      f32x16 acc[1];
      score_tile_e<EngB3, D, 1>(lds[cur % NBUF], i32, h, bq, acc);
      const int64_t j0 = tt * kTileJ;
      const bool ragged = j0 + kTileJ > ny;
      const int xr = EXD ? diag_offset(row_i, j0, h) : -1;
      // P in place of the scores
  #pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 lr = *reinterpret_cast<const float4*>(&st_lse[cur][8 * g + 4 * h]);
        const float4 wr = *reinterpret_cast<const float4*>(&st_w[cur][8 * g + 4 * h]);
        const float lre[4] = {lr.x, lr.y, lr.z, lr.w};
        const float wre[4] = {wr.x, wr.y, wr.z, wr.w};
  #pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const bool dead = (ragged && (j0 + acc_row(r, h) >= ny)) || (EXD && xr == e + 8 * g);
          const float sc = dead ? -INFINITY : acc[0][r];
          if (SIDES == 1) acc[0][r] = wl * __builtin_amdgcn_exp2f(sc - lse2l);
          else if (SIDES == 2) acc[0][r] = wre[e] * __builtin_amdgcn_exp2f(sc - lre[e]);
          else acc[0][r] = wl * __builtin_amdgcn_exp2f(sc - lse2l) + wre[e] * __builtin_amdgcn_exp2f(sc - lre[e]);
        }
      }
      // G^T[c][i] += yhat[j][c] * P[j][i], 16 streamed rows per k-chunk, six bf16 terms
      const unsigned char* tbase = lds[cur % NBUF] + 3 * S::PLANE + i32 * B::RT + 8 * h;
  #pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        u32x4 pp[3];
        {
          unsigned q[3][4];
  #pragma unroll
          for (int e = 0; e < 4; ++e) split3(acc[0][8 * kc + 2 * e], acc[0][8 * kc + 2 * e + 1], q[0][e], q[1][e], q[2][e]);
  #pragma unroll
          for (int pl = 0; pl < 3; ++pl) pp[pl] = (u32x4){q[pl][0], q[pl][1], q[pl][2], q[pl][3]};
        }
  #pragma unroll
        for (int c = 0; c < B::CT; ++c) {
          u32x4 ya[3];
  #pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
            const unsigned char* p = tbase + pl * B::TPLANE + (32 * c) * B::RT + 32 * kc;
            const uint2 lo = *reinterpret_cast<const uint2*>(p);
            const uint2 hi = *reinterpret_cast<const uint2*>(p + 16);
            ya[pl] = (u32x4){lo.x, lo.y, hi.x, hi.y};
          }
          gacc[c] = mfma_bf16(ya[2], pp[0], gacc[c]);
          gacc[c] = mfma_bf16(ya[0], pp[2], gacc[c]);
          gacc[c] = mfma_bf16(ya[1], pp[1], gacc[c]);
          gacc[c] = mfma_bf16(ya[1], pp[0], gacc[c]);
          gacc[c] = mfma_bf16(ya[0], pp[1], gacc[c]);
          gacc[c] = mfma_bf16(ya[0], pp[0], gacc[c]);
        }
      }
      if (NBUF == 1) __syncthreads();          // every wave is done reading the only buffer
      if (more) store_tile(cur ^ 1);
      __syncthreads();
    }
  }

  // gacc[c] register rr of lane (i, h) is column 32*c + acc_row(rr, h) of row i
  float* gout = gpart + (int64_t)split * mx * D;
  if (row_i < mx) {
#pragma unroll
    for (int c = 0; c < B::CT; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 v = make_float4(gacc[c][4 * g + 0] * out_scale, gacc[c][4 * g + 1] * out_scale,
                               gacc[c][4 * g + 2] * out_scale, gacc[c][4 * g + 3] * out_scale);
        *reinterpret_cast<float4*>(gout + row_i * D + 32 * c + 8 * g + 4 * h) = v;
      }
  }
}

// ------------------------------------------------------------------------------------------
// Forward WITH the softmax-weighted row sum ("fwd_o", flash-attention forward):
//   lse[i] = log sum_j exp(s_ij),   o[i, :] = sum_j softmax_j(s_i.)_j * yhat_j
// in one pass over the streamed rows (online max, deferred rescale).  For a row-softmax loss the
// gradient w.r.t. the stationary side is then  dL/dxhat_i = dL/dlse_i * inv_tau * o[i, :]  — no
// backward pass over the M x N tile for that side; the backward recomputes the score tile ONCE
// (streamed-side gradient) instead of twice.  Same tile engine as infonce_bwd_b3_kernel: score
// MFMAs in the forward's order (bitwise the forward's logits), P split in registers, second product
// against the transposed planes.  The two lane halves of a stationary row hold different streamed
// rows of the same k-chunk, so they share one running maximum (one cross-half shuffle per tile).
// Rescaling the accumulators is deferred while no logit exceeds the reference point by more than
// 2^kDefer (wave-uniform branch): after the first tiles it almost never runs.
// ------------------------------------------------------------------------------------------

template <int D, bool EXD = false>
__global__ __launch_bounds__(256, 2) void infonce_fwdo_b3_kernel(
    const float* __restrict__ x, const float* __restrict__ x_scale, int64_t mx, const float* __restrict__ y,
    const float* __restrict__ y_scale, int64_t ny, float scale2, int nsplit, int64_t tiles_per_split,
    float2* __restrict__ part, float* __restrict__ opart) {
  using S = ShapeB3<D>;
  using B = BwdB3<D>;
  constexpr int NBUF = D <= 64 ? 2 : 1;
  __shared__ __align__(16) unsigned char lds[NBUF][B::TILE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t mblk = blockIdx.x / nsplit;
  const int split = blockIdx.x % nsplit;
  const int64_t row_i = (mblk * 4 + wave) * 32 + i32;

  u32x4 bq[1][3][S::KC];
  load_stationary_e<EngB3, D>(x, x_scale, mx, row_i, h, scale2, bq[0]);
  float m_run = kNegBig, l_run = 0.f;
  f32x16 gacc[B::CT];
#pragma unroll
  for (int c = 0; c < B::CT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[c][r] = 0.f;

  const int64_t total_tiles = (ny + kTileJ - 1) / kTileJ;
  const int64_t tile0 = (int64_t)split * tiles_per_split;
  const int64_t tile1 = min(total_tiles, tile0 + tiles_per_split);

  // scores (log2 domain) -> un-normalised probabilities relative to the running reference point
  auto softmax_p = [&](f32x16& acc, int64_t tt) {
    const int64_t j0 = tt * kTileJ;
    if (EXD || j0 + kTileJ > ny) {                       // wave-uniform: ragged last tile / excluded diagonal
      const int xr = EXD ? diag_offset(row_i, j0, h) : -1;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const bool dead = (j0 + acc_row(r, h) >= ny) || (EXD && xr == e + 8 * g);
          acc[r] = dead ? -INFINITY : acc[r];
        }
    }
    float tmax = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
#pragma unroll
    for (int g = 1; g < 4; ++g)
      tmax = fmaxf(tmax, fmaxf(fmaxf(acc[4 * g], acc[4 * g + 1]), fmaxf(acc[4 * g + 2], acc[4 * g + 3])));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));        // both halves of a stationary row agree
    if (__any(tmax > m_run + kDefer)) {
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int c = 0; c < B::CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) gacc[c][r] *= alpha;
      m_run = m_new;
    }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[r] = __builtin_amdgcn_exp2f(acc[r] - m_run);
      sum += acc[r];
    }
    l_run += sum;
  };

  {
    float4 regs[S::NLD];
    if (tile0 < tile1) {
      stage_load<D>(y, y_scale, ny, tile0 * kTileJ, tid, regs);
#pragma unroll
      for (int u = 0; u < S::NLD; ++u) stage_store_b3t_one<D>(lds[0], tid, regs[u], u);
    }
    __syncthreads();
    for (int64_t tt = tile0; tt < tile1; ++tt) {
      const int cur = (int)((tt - tile0) & 1);
      const bool more = tt + 1 < tile1;
      if (more) stage_load<D>(y, y_scale, ny, (tt + 1) * kTileJ, tid, regs);
      f32x16 acc[1];
      score_tile_e<EngB3, D, 1>(lds[cur % NBUF], i32, h, bq, acc);
      softmax_p(acc[0], tt);
      const unsigned char* tbase = lds[cur % NBUF] + 3 * S::PLANE + i32 * B::RT + 8 * h;
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        u32x4 pp[3];
        {
          unsigned q[3][4];
#pragma unroll
          for (int e = 0; e < 4; ++e) split3(acc[0][8 * kc + 2 * e], acc[0][8 * kc + 2 * e + 1], q[0][e], q[1][e], q[2][e]);
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) pp[pl] = (u32x4){q[pl][0], q[pl][1], q[pl][2], q[pl][3]};
        }
#pragma unroll
        for (int c = 0; c < B::CT; ++c) {
          u32x4 ya[3];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
            const unsigned char* p = tbase + pl * B::TPLANE + (32 * c) * B::RT + 32 * kc;
            const uint2 lo = *reinterpret_cast<const uint2*>(p);
            const uint2 hi = *reinterpret_cast<const uint2*>(p + 16);
            ya[pl] = (u32x4){lo.x, lo.y, hi.x, hi.y};
          }
          gacc[c] = mfma_bf16(ya[2], pp[0], gacc[c]);
          gacc[c] = mfma_bf16(ya[0], pp[2], gacc[c]);
          gacc[c] = mfma_bf16(ya[1], pp[1], gacc[c]);
          gacc[c] = mfma_bf16(ya[1], pp[0], gacc[c]);
          gacc[c] = mfma_bf16(ya[0], pp[1], gacc[c]);
          gacc[c] = mfma_bf16(ya[0], pp[0], gacc[c]);
        }
      }
      if (NBUF == 1) __syncthreads();          // every wave is done reading the only buffer
      if (more) {
#pragma unroll
        for (int u = 0; u < S::NLD; ++u) stage_store_b3t_one<D>(lds[(cur ^ 1) % NBUF], tid, regs[u], u);
      }
      __syncthreads();
    }
  }

  // per-split partial: (reference point, sum of both halves) and the un-normalised O rows
  const float l_o = __shfl_xor(l_run, 32, 64);
  if (h == 0 && row_i < mx) part[(int64_t)split * mx + row_i] = make_float2(m_run, l_run + l_o);
  float* gout = opart + (int64_t)split * mx * D;
  if (row_i < mx) {
#pragma unroll
    for (int c = 0; c < B::CT; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 v = make_float4(gacc[c][4 * g + 0], gacc[c][4 * g + 1], gacc[c][4 * g + 2], gacc[c][4 * g + 3]);
        *reinterpret_cast<float4*>(gout + row_i * D + 32 * c + 8 * g + 4 * h) = v;
      }
  }
}

// ------------------------------------------------------------------------------------------
// Two-product tile loop, software-pipelined ACROSS tiles (d <= 64): the exposed part of the loops above is
// the VALU work between the two MFMA phases (P from the scores + its bf16 split: ~150 instructions per
// tile against ~1500 cycles of MFMA, ~50 % MFMA-busy measured).  Here step t runs
//     phase A   score MFMAs of tile t+1          ||  operand split + LDS stores of tile t+2 (staging)
//     phase B   second-product MFMAs of tile t   ||  P(t+1) from the finished scores + its bf16 split
// so every VALU instruction sits in an MFMA shadow; one barrier per step.  LDS: ONE row-major image of the
// three bf16 planes per tile serves both products — `ds_read_b128` rows for the score operand, the
// transposing `ds_read_b64_tr_b16` for the second product's operand (the 2-byte stores of a transposed copy
// were 8-way bank-conflicted and made the loop LDS-bound) — in a ring of three tiles (t read in B, t+1 read in
// A, t+2 being written in A): 3 x 13.5 KB = 40.5 KB.
//   MODE 0  backward: P = w_x e^{s - lse_x} + w_y e^{s - lse_y}   (infonce_bwd_b3_kernel's arithmetic)
//   MODE 1  forward with the weighted row sum (infonce_fwdo_b3_kernel's arithmetic): online reference point,
//           the rare rescale of the accumulators happens between two B phases.
//   MODE 2  BCE-with-logits forward (lightgcn.py:109-113): row sums of softplus(s) and o_i = sum_j sigmoid(s_ij) y_j
//           (sigmoid <= 1: no reference point, no rescale); MODE 3 its backward, P = (w_x[i] + w_y[j]) sigmoid(s_ij)
//           (SIDES 1 / 2: the weights sit on the stationary / the streamed rows).
// ------------------------------------------------------------------------------------------
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 lds_read_tr16(const unsigned char* p) {      // ds_read_b64_tr_b16; EXEC must be all ones
  return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p));
}

// max |w| over both weight vectors -> hw[0] = 2^14 / 2^ceil(log2 max|w|) (what the weights are multiplied by before
// they meet e^{s - lse} <= 1, so that P stays in f16 range), hw[1] = 1 / (hw[0] * 2^8) (undoes it, and the streamed
// operand's 2^8, on the way out).  One block.
__global__ __launch_bounds__(1024) void h2_wscale_kernel(const float* __restrict__ w_x, int64_t mx,
                                                         const float* __restrict__ w_y, int64_t ny, float* __restrict__ hw) {
  __shared__ float red[16];
  float m = 0.f;
  if (w_x != nullptr)
    for (int64_t i = threadIdx.x; i < mx; i += 1024) m = fmaxf(m, fabsf(w_x[i]));
  if (w_y != nullptr)
    for (int64_t i = threadIdx.x; i < ny; i += 1024) m = fmaxf(m, fabsf(w_y[i]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) m = fmaxf(m, red[k]);
    int e = 0;
    if (m > 0.f && m < INFINITY) (void)frexpf(m, &e);                 // m = f * 2^e, f in [0.5, 1): |w| 2^-e < 1
    e = min(max(e, -100), 100);
    hw[0] = ldexpf(1.0f, 14 - e);
    hw[1] = 1.0f / (hw[0] * EngH2::kSY);
  }
}

// Pre-pass of the two-f16-plane backward loop (MODE 0): a scaled, zero-padded image of the STREAMED rows and of their
// statistics, so that the loop stages a tile with two plain loads per lane — no scale loads, multiplies, end-of-array
// clamps or selects per tile.  The loop's time is its count of vector instructions, and the streamed side of
// a backward launch is read once per row block: mx / 128 times.
//   FOLDW = false:  l_j = lse_j log2 e,  w'_j = w_j hw[0] 2^-l_j,  yhat_j = y_scale_j kSY y_j   (padding: 1e30, 0, zero row)
//   FOLDW = true (statistics on the streamed rows only, SIDES = 2): the weight of row j moves INTO the exponent and its
//   sign into the row,
//     P_ij y_j = w_j e^{s_ij - lse_j} y_j = 2^(c_j s'_ij + e_j) (sgn_j y_j),   s'_ij = x_i . (sgn_j y_j) the score the loop sees,
//     e_j = log2(|w_j| hw[0]) - lse_j log2 e,   c_j = sgn_j kSInv,   yhat_j = sgn_j y_scale_j kSY y_j,
//   so that a probability costs one fma and one exp2 in the loop instead of fma, exp2 and a multiply.  w_j = 0 gives
//   e_j = -inf, i.e. P = 0, like the padding rows (e = -1e30, zero row).
// Layout of `img`: l or e [rows], w' or c [rows], yhat[rows][D], rows = fold_rows(ny).
template <int D, bool FOLDW>
__global__ __launch_bounds__(256) void h2_prestage_kernel(const float* __restrict__ y, const float* __restrict__ y_scale,
                                                          const float* __restrict__ w_y, const float* __restrict__ lse_y,
                                                          int64_t ny, const float* __restrict__ hw, float* __restrict__ img,
                                                          bool write_stats) {
  const int64_t rows = fold_rows(ny);
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= rows * (D / 4)) return;
  const int64_t j = k / (D / 4);
  const int c4 = (int)(k % (D / 4));
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  float s0 = FOLDW ? -1.0e30f : 1.0e30f, s1 = FOLDW ? EngH2::kSInv : 0.f;
  if (j < ny) {
    float sgn = 1.0f;
    if (w_y != nullptr) {
      const float w = w_y[j] * hw[0];
      if (FOLDW) {
        sgn = w < 0.f ? -1.0f : 1.0f;
        s0 = fmaf(-lse_y[j], kLog2e, __log2f(fabsf(w)));
        s1 = sgn * EngH2::kSInv;
      } else {
        // statistics on BOTH sides (the only user of this form): the loop factors the common 2^s out of
        //   w_i 2^(s - l_i) + w_j 2^(s - l_j) = 2^s (w_i 2^-l_i + w_j 2^-l_j),
        // so the streamed row's weight arrives multiplied by its 2^-l (l >= every score of the row: no overflow)
        s0 = lse_y[j] * kLog2e;
        s1 = w * __builtin_amdgcn_exp2f(-s0);
      }
    }
    const float sc = sgn * EngH2::kSY * (y_scale != nullptr ? y_scale[j] : 1.0f);
    v = *reinterpret_cast<const float4*>(y + j * D + 4 * c4);
    v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
  }
  *reinterpret_cast<float4*>(img + 2 * rows + j * D + 4 * c4) = v;
  if (c4 == 0 && write_stats) {                            // (w_y == nullptr: every row like the padding)
    img[j] = s0;
    img[rows + j] = s1;
  }
}

// (LDS rows of 36 dwords: the 16 rows of every ds_read_b128 lane group start in 16 different bank quads, but rows q
// and q + 2 of the four that one ds_read_b64_tr_b16 gathers share 8 banks — every transposing read takes two passes,
// 22-28 % of the loop's LDS cycles are conflicts (SQ_LDS_BANK_CONFLICT).  Placing tile row 16kc + 8g + 4h + q in LDS row
// 16kc + 4q + 2g + h removes them and was measured: no change in time (the LDS is 22-27 % busy), so the plain order stays.)
// NW = 8: a 512-thread workgroup of 256 stationary rows.  Its waves 4..7 run the same stream ONE barrier interval behind
// waves 0..3 (two barriers per step: after the score phase and after the P phase), so that on every SIMD one wave is in
// its MFMA-heavy score phase while its partner is in its VALU-heavy P phase, and both halves share one staged tile
// (each lane stages one float4 of it in its own score phase): half the staging work per MFMA.  Ring of four tiles.
template <class E, int D, int MODE, bool EXD, int SIDES, int NW = 4>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 1 : E::kMinBlocks) void infonce_pipe_kernel(
    const float* __restrict__ x, const float* __restrict__ x_scale, int64_t mx, const float* __restrict__ y,
    const float* __restrict__ y_scale, int64_t ny, float scale2, float out_scale, const float* __restrict__ lse_x,
    const float* __restrict__ w_x, const float* __restrict__ lse_y, const float* __restrict__ w_y, int nsplit,
    int64_t tiles_per_split, float* __restrict__ gpart, float2* __restrict__ part, const float* __restrict__ hw) {
  using S = ShapeB3<D>;
  using B = BwdB3<D>;
  static_assert(D <= 64 || (D == 128 && std::is_same<E, EngH2>::value), "d = 128: two planes only (registers)");
  constexpr int NPL = E::NPL, NTERM = E::NTERM;
  constexpr int RM = NPL * S::PLANE;
  constexpr int THREADS = 64 * NW;
  constexpr int F4T = kTileJ * D / 4;                        // float4s per streamed tile
  constexpr int NLDW = (F4T + THREADS - 1) / THREADS;        // ... per thread
  constexpr int RING = NW == 8 ? 4 : 3;
  static_assert(NW == 4 || NW == 8, "four or eight waves");
  // PRE (h2_prestage_kernel ran in front): y = the scaled rows, lse_y / w_y = the streamed rows' statistics in the loop's
  // units, all padded to whole tiles; FOLD: the statistics are (e, c), the weights live in the exponent
  constexpr bool PRE = MODE == 0 && std::is_same<E, EngH2>::value;
  constexpr bool FOLD = PRE && SIDES == 2;
  constexpr bool BWD = MODE == 0 || MODE == 3;               // per-row weights (MODE 0: and lse) ride with the tiles
  constexpr bool FWD = MODE == 1 || MODE == 2;               // running row sums + the o accumulators
  constexpr bool NOO = MODE == 2 && SIDES == 1;              // BCE row sums only (no gradient wanted): no second product
  // UNS: BCE on two f16 planes.  Its rows are not unit rows, so the launch scales both sides to unit norm (x_scale /
  // y_scale = 1 / |row|) and every score is UN-SCALED by the two norms before the softplus / sigmoid: lse_x / lse_y carry
  // the norms, w_y the streamed rows' factor of the second product (norm x weight, pre-scaled into f16 range by hw[0]).
  constexpr bool UNS = MODE >= 2 && std::is_same<E, EngH2>::value;
  constexpr bool STATS = (BWD && SIDES != 1) || UNS;         // per-row values of the streamed rows ride with the tiles
  // UNSREF (UNS with a second product): the probabilities sigmoid x (norm x weight) go into f16 planes, whose floor would
  // flush a row whose sigmoids are ALL tiny.  Every stationary row therefore carries a running power-of-two reference 2^q,
  // q ~ log2 of the largest sigmoid seen so far (min(s_max, 0): within one bit of it), the planes hold sigmoid 2^-q x
  // (norm x weight) <= 2^15, the accumulators are rescaled when a tile raises q by more than one (the flash forward's
  // deferred rescale, rare after the first tiles) and the result is multiplied by 2^q on the way out.
  constexpr bool UNSREF = UNS && !NOO;
  static_assert(MODE < 2 || (!EXD && NW == 4), "BCE modes: four waves");
  static_assert(MODE != 3 || SIDES == 1 || SIDES == 2, "BCE backward: weights on one side");
  static_assert(!(UNS && MODE == 3 && SIDES == 1), "two-plane BCE backward: the weights sit on the streamed rows");
  __shared__ __align__(16) unsigned char lds_rm[RING][RM];   // ring: tile t (B, transposed reads), t+1 (A), t+2 (staging)
  __shared__ __align__(16) float st_lse[RING][kTileJ];
  __shared__ __align__(16) float st_w[RING][kTileJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t mblk = blockIdx.x / nsplit;
  const int split = blockIdx.x % nsplit;
  const int64_t row_i = (mblk * NW + wave) * 32 + i32;

  // MODE 0 on EngH2: weights pre-scaled into f16 range (h2_wscale_kernel); hw == nullptr otherwise
  const float w_mul = hw != nullptr ? hw[0] : 1.0f;
  const bool on_x = BWD && row_i < mx && w_x != nullptr;
  const float wl = on_x ? w_x[row_i] * w_mul : 0.f;
  const float lse2l = (MODE == 0 && on_x) ? lse_x[row_i] * kLog2e : 1.0e30f;
  const float rs = (UNS && row_i < mx) ? lse_x[row_i] : 1.0f;   // UNS: the stationary row's norm
  // BOTHF (two planes, statistics on both sides): one exp2 per probability — the unit rows bound the score (|s| <= 28.9
  // in log2 units), so 2^s is taken once and multiplied by w_i 2^-l_i + w_j 2^-l_j (the streamed half premultiplied by
  // h2_prestage_kernel): exp2 + add + multiply instead of two fused multiply-adds, two exp2, two multiplies and an add
  constexpr bool BOTHF = PRE && SIDES == 0;
  const float ax = BOTHF ? wl * __builtin_amdgcn_exp2f(-lse2l) : 0.f;
  // FOLDX (statistics on the stationary rows only): the same move as FOLD inside the kernel — |w_i| into the exponent,
  // sgn w_i into the stationary operand (the scores flip with it, hence c_x) and back out of the gradient row at the end:
  //   P_ij = w_i e^{s_ij - lse_i} = sgn_i 2^(c_x s'_ij + e_x)
  constexpr bool FOLDX = MODE == 0 && SIDES == 1;
  const float sgn_x = FOLDX && wl < 0.f ? -1.0f : 1.0f;
  const float c_x = sgn_x * E::kSInv;
  const float e_x = (MODE == 0 && on_x) ? fmaf(-lse_x[row_i], kLog2e, __log2f(fabsf(wl))) : -1.0e30f;
  u32x4 bq[1][NPL][S::KC];
  load_stationary_e<E, D>(x, x_scale, mx, row_i, h, scale2 * E::kSX * sgn_x, bq[0]);
  float m_run = UNSREF ? -100.0f : kNegBig, l_run = 0.f;   // MODE 1: reference point of the row; UNSREF: q
  f32x16 gacc[B::CT];
#pragma unroll
  for (int c = 0; c < B::CT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[c][r] = 0.f;

  const int64_t total_tiles = (ny + kTileJ - 1) / kTileJ;
  const int64_t tile0 = (int64_t)split * tiles_per_split;
  const int64_t tile1 = min(total_tiles, tile0 + tiles_per_split);
  if (tile0 < tile1) {
    constexpr int NP = 3 * NLDW, NS1 = NTERM * S::KC, NG = B::CT * 2 * NTERM;
    const int64_t last = tile1 - 1;
    StagedRows<NLDW> ra, rb;                                // (raw rows + their scales: multiplied where they are staged)
    float sla = 0.f, swa = 0.f, slb = 0.f, swb = 0.f;
    auto load_tile = [&](int64_t t, StagedRows<NLDW>& r, float& sl, float& sw) {
      const int64_t j0 = min(t, last) * kTileJ;
      // wave-uniform tile base + 32-bit per-thread offsets (a ragged last tile clamps its rows to the last valid
      // one and zeroes their scale): no 64-bit vector arithmetic in the loop
      const int rem = (int)min((int64_t)kTileJ, ny - j0);
      const float* tb = y + j0 * D;
      const float* sp = y_scale != nullptr ? y_scale + j0 : y;               // (no scale: a dummy word through a zero stride)
      const int sstride = y_scale != nullptr ? 1 : 0;
      if (PRE) {                                             // scaled and padded already: uniform base + a constant offset per lane
#pragma unroll
        for (int u = 0; u < NLDW; ++u)
          r.v[u] = *reinterpret_cast<const float4*>(tb + 4u * (unsigned)min(tid + THREADS * u, F4T - 1));
        if (SIDES != 1 && tid < kTileJ) {
          sw = w_y[j0 + tid];
          sl = lse_y[j0 + tid];
        }
        return;
      }
#pragma unroll
      for (int u = 0; u < NLDW; ++u) {
        const int idx = min(tid + THREADS * u, F4T - 1);     // (more threads than float4s: the surplus reloads the last one)
        const int row = idx / (D / 4), c4 = idx % (D / 4);
        const unsigned rr = (unsigned)min(row, rem - 1) & (kTileJ - 1);   // (masked: a provably small offset folds into the load)
        // loads only: the scale is multiplied in where the row is staged, two steps from here (doing it on the spot put
        // a `s_waitcnt vmcnt(0)` behind the loads — a memory round trip in front of every step's first MFMA)
        r.v[u] = *reinterpret_cast<const float4*>(tb + (rr * D + 4u * c4));   // uniform base + 32-bit lane offset
        r.s[u] = sp[rr * (unsigned)sstride];
        r.live[u] = row < rem;
      }
      if ((BWD || UNS) && tid < kTileJ) {
        const int64_t j = j0 + tid;
        const bool on = j < ny && w_y != nullptr;
        sw = on ? w_y[j] * w_mul : 0.f;
        if (UNS) sl = j < ny ? lse_y[j] : 1.0f;             // the streamed row's norm (a masked row: -inf x 1)
        else sl = (MODE == 0 && on) ? lse_y[j] * kLog2e : 1.0e30f;
      }
    };
    // one third of the staging of one float4: split (x, y), split (z, w), row-major plane stores
    auto stage_part = [&](int pi, const StagedRows<NLDW>& st, float4 (&tm)[NLDW], unsigned (&sa)[NLDW][NPL],
                          unsigned (&sb)[NLDW][NPL], unsigned char* rm, int sbuf, float sl, float sw) {
      const int u = pi / 3, k = pi % 3;
      const int idx = tid + THREADS * u;
      const int row = idx / (D / 4), c4 = idx % (D / 4);
      if (k == 0) {
        tm[u] = st.v[u];
        if (!PRE) {
          const float sc = st.live[u] ? (y_scale != nullptr ? st.s[u] * E::kSY : E::kSY) : 0.f;
          tm[u].x *= sc; tm[u].y *= sc; tm[u].z *= sc; tm[u].w *= sc;
        }
        E::split(tm[u].x, tm[u].y, sa[u]);
      } else if (k == 1) {
        E::split(tm[u].z, tm[u].w, sb[u]);
      } else {
        unsigned char* p = rm + row * S::ROWB + c4 * 8;
        if (THREADS * NLDW == F4T || idx < F4T) {
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) *reinterpret_cast<uint2*>(p + pl * S::PLANE) = make_uint2(sa[u][pl], sb[u][pl]);
        }
        if ((BWD || UNS) && u == 0 && tid < kTileJ) {
          st_lse[sbuf][tid] = sl;
          st_w[sbuf][tid] = sw;
        }
      }
    };
    auto stage_all = [&](const StagedRows<NLDW>& st, unsigned char* rm, int sbuf, float sl, float sw) {
      unsigned sa[NLDW][NPL], sb[NLDW][NPL];
      float4 tm[NLDW];
#pragma unroll
      for (int pi = 0; pi < NP; ++pi) stage_part(pi, st, tm, sa, sb, rm, sbuf, sl, sw);
    };
    // micro-unit m of P(t) from the finished scores of tile t: MODE 0: 0..15 one register each, 16..23 one split3
    // each; MODE 1: the same after `prepare` fixed the reference point.
    float m_use = kNegBig, alpha = 1.0f, psum = 0.f, p_off = 0.f;
    bool rescale = false;
    auto prepare = [&](f32x16& acc, int64_t t, int sbuf) {   // masks (ragged tile / excluded diagonal); MODE 1: reference point
      const int64_t j0 = t * kTileJ;
      const int lim = (int)min((int64_t)kTileJ, ny - j0);   // rows of this tile that exist (wave-uniform)
      // (statistics on the streamed rows only, MODE 0 / SIDES 2: no end-of-array mask — rows behind the end carry w' = 0
      // or e = -1e30, P = 0 whatever their score.  Everywhere else they need it: such a row is staged as a zero row, score
      // 0, and against real scores that are all far below 0 its stationary-side "probability" e^{0 - lse_i} overflows
      // the f16 planes — inf times the zero row.  Under FOLDX the masked score is -inf / c_x: +inf for a negative weight.)
      if (EXD || (lim < kTileJ && !(MODE == 0 && SIDES == 2))) {
        // a real (scalar) branch: if-converted, the 16 selects with their compares would run for every tile
        if (!EXD) asm volatile("" ::: "memory");
        const int xr = EXD ? diag_offset(row_i, j0, h) : -1;
        const float dead_score = FOLDX ? -INFINITY * sgn_x : -INFINITY;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            const bool dead = (acc_row(r, h) >= lim) || (EXD && xr == e + 8 * g);
            acc[r] = dead ? dead_score : acc[r];
          }
      }
      if (MODE == 1) {
        float tmax = acc[0];                              // chained: one v_max3_f32 per pair of scores
#pragma unroll
        for (int r = 1; r < 16; r += 2) tmax = fmaxf(fmaxf(tmax, acc[r]), acc[r + 1 < 16 ? r + 1 : r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * E::kSInv;
        rescale = __any(tmax > m_run + E::kDeferE);
        m_use = rescale ? fmaxf(m_run, tmax) : m_run;
        alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        psum = 0.f;
        p_off = E::kPExp - m_use;
      }
      if (MODE == 2) psum = 0.f;
      if (UNSREF) {
        // scores un-scaled here (so that their maximum is known before the first probability), q from the largest one
        float smax = -INFINITY;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 l4 = *reinterpret_cast<const float4*>(&st_lse[sbuf][8 * g + 4 * h]);
          acc[4 * g + 0] *= rs * l4.x; acc[4 * g + 1] *= rs * l4.y; acc[4 * g + 2] *= rs * l4.z; acc[4 * g + 3] *= rs * l4.w;
          smax = fmaxf(fmaxf(fmaxf(fmaxf(smax, acc[4 * g]), acc[4 * g + 1]), acc[4 * g + 2]), acc[4 * g + 3]);
        }
        smax = fmaxf(smax, __shfl_xor(smax, 32, 64));       // both lane halves feed the same output row
        const float q_tile = fmaxf(fminf(smax, 0.f), -100.0f);
        rescale = __any(q_tile > m_run + 1.0f);
        m_use = rescale ? fmaxf(m_run, q_tile) : m_run;
        alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        p_off = __builtin_amdgcn_exp2f(-m_use);             // 2^-q: what a probability is multiplied by
      }
    };
    // streamed rows' statistics (MODE 0, SIDES != 1): accumulator register r = 4 g + e of lane half h is tile row
    // 8 g + 4 h + e, so ONE ds_read_b128 per array serves four consecutive P units; group g + 1 is fetched while group g
    // is being used (16 registers).  Per-unit ds_read_b32 pairs were 32 LDS instructions per tile: 9 % of the backward
    // (timing-only build with constants: 1.82 -> 1.66 ms).
    float4 sl4[2], sw4[2];
    auto stats_begin = [&](int sbuf) {
      if (STATS) {
        sl4[0] = *reinterpret_cast<const float4*>(&st_lse[sbuf][4 * h]);
        sw4[0] = *reinterpret_cast<const float4*>(&st_w[sbuf][4 * h]);
      }
    };
    auto p_unit = [&](int m, f32x16& acc, int sbuf, unsigned (&pq)[2][NPL][4]) {
      if (m < 16) {
        const int r = m;
        float lre = 0.f, wre = 0.f;
        if (STATS) {
          const int g = r >> 2, e = r & 3;
          if (e == 0 && g < 3) {
            sl4[(g + 1) & 1] = *reinterpret_cast<const float4*>(&st_lse[sbuf][8 * (g + 1) + 4 * h]);
            sw4[(g + 1) & 1] = *reinterpret_cast<const float4*>(&st_w[sbuf][8 * (g + 1) + 4 * h]);
          }
          const float4 l4 = sl4[g & 1], w4 = sw4[g & 1];
          lre = e == 0 ? l4.x : (e == 1 ? l4.y : (e == 2 ? l4.z : l4.w));
          wre = e == 0 ? w4.x : (e == 1 ? w4.y : (e == 2 ? w4.z : w4.w));
        }
        const float unscale = UNSREF ? 1.0f : (UNS ? rs * lre : E::kSInv);   // accumulator -> log2-domain score (UNSREF: done in `prepare`)
        if (MODE == 1) {
          acc[r] = __builtin_amdgcn_exp2f(fmaf(acc[r], E::kSInv, p_off));
          psum += acc[r];
        } else if (MODE == 2) {
          float sp, sg;
          bce_terms(acc[r] * unscale, sp, sg);
          psum += sp;
          acc[r] = UNSREF ? sg * (wre * p_off) : (UNS ? sg * wre : sg);
        } else {
          const float sc = acc[r];
          if (MODE == 3) {
            acc[r] = (SIDES == 1 ? wl : (UNSREF ? wre * p_off : wre)) * bce_sigmoid(sc * unscale);
          } else if (SIDES == 1) acc[r] = __builtin_amdgcn_exp2f(fmaf(sc, c_x, e_x));
          else if (FOLD) acc[r] = __builtin_amdgcn_exp2f(fmaf(sc, wre, lre));
          else if (SIDES == 2) acc[r] = wre * __builtin_amdgcn_exp2f(fmaf(sc, E::kSInv, -lre));
          else if (BOTHF) acc[r] = __builtin_amdgcn_exp2f(sc * E::kSInv) * (ax + wre);
          else acc[r] = wl * __builtin_amdgcn_exp2f(fmaf(sc, E::kSInv, -lse2l)) + wre * __builtin_amdgcn_exp2f(fmaf(sc, E::kSInv, -lre));
        }
      } else {
        if (NOO) return;                                 // (no second product: nothing to split)
        const int e = m - 16;                            // pair (2e, 2e + 1): k-chunk e / 4, dword e % 4
        unsigned q[NPL];
        E::split(acc[2 * e], acc[2 * e + 1], q);
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) pq[e >> 2][pl][e & 3] = q[pl];
      }
    };
    auto finish_p = [&]() {                               // MODE 1: between two B phases
      if (MODE == 1) {
        if (rescale) {
          l_run *= alpha;
#pragma unroll
          for (int c = 0; c < B::CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) gacc[c][r] *= alpha;
          m_run = m_use;
        }
        l_run += psum;
      }
      if (MODE == 2) l_run += psum;
      if (UNSREF && rescale) {
#pragma unroll
        for (int c = 0; c < B::CT; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) gacc[c][r] *= alpha;
        m_run = m_use;
      }
    };
    auto score_plain = [&](const unsigned char* rm, f32x16& acc) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const unsigned char* base = rm + i32 * S::ROWB + h * (S::KH * 2);
#pragma unroll
      for (int c = 0; c < S::KC; ++c) {
        u32x4 ap[NPL];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) ap[pl] = *reinterpret_cast<const u32x4*>(base + pl * S::PLANE + 16 * c);
#pragma unroll
        for (int term = 0; term < NTERM; ++term) acc = E::mfma(ap[E::ta(term)], bq[0][E::tb(term)][c], acc);
      }
    };

    // ---- prologue: tiles 0 and 1 staged, P(tile0) ready, tile 2 in registers, tile 3 loading
    unsigned pqa[2][NPL][4], pqb[2][NPL][4];
    f32x16 acc;
    load_tile(tile0, ra, sla, swa);
    stage_all(ra, lds_rm[0], 0, sla, swa);
    load_tile(tile0 + 1, ra, sla, swa);
    stage_all(ra, lds_rm[1], 1, sla, swa);
    load_tile(tile0 + 2, ra, sla, swa);
    __syncthreads();
    score_plain(lds_rm[0], acc);
    prepare(acc, tile0, 0);
    stats_begin(0);
#pragma unroll
    for (int m = 0; m < 24; ++m) p_unit(m, acc, 0, pqa);
    finish_p();
    __syncthreads();

    // step t: tile t's P planes in `pc`, tile t+2 in `st` registers; produces P(t+1) in `pn`, loads tile t+3 to `ld`
    auto step = [&](auto next_c, int64_t t, int k3, unsigned (&pc)[2][NPL][4], unsigned (&pn)[2][NPL][4],
                    const StagedRows<NLDW>& st, float st_l, float st_w_v, StagedRows<NLDW>& ld, float& ld_l, float& ld_w) {
      constexpr bool real_next = decltype(next_c)::value;    // false only for the split's last tile (compile time:
                                                             // no branch may sit between the MFMAs of a phase)
      load_tile(t + 3, ld, ld_l, ld_w);
      // tile t in ring slot k3, t+1 in k3 + 1, t+2 goes to k3 + 2 (planes and per-tile statistics alike)
      const int slot1 = (k3 + 1) % RING, slot2 = (k3 + 2) % RING;
      unsigned char* rm_out = lds_rm[slot2];
      unsigned sa[NLDW][NPL], sb[NLDW][NPL];
      float4 tm[NLDW];
      // phase A: S^T of tile t+1 || staging of tile t+2
      {
        const unsigned char* base = lds_rm[slot1] + i32 * S::ROWB + h * (S::KH * 2);
        u32x4 ap[2][NPL];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) ap[0][pl] = *reinterpret_cast<const u32x4*>(base + pl * S::PLANE);
#pragma unroll
        for (int c = 0; c < S::KC; ++c) {
          if (c + 1 < S::KC) {
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl)
              ap[(c + 1) & 1][pl] = *reinterpret_cast<const u32x4*>(base + pl * S::PLANE + 16 * (c + 1));
          }
#pragma unroll
          for (int term = 0; term < NTERM; ++term) {
            const int slot = c * NTERM + term;
            f32x16 cin = acc;
            if (slot == 0) {
#pragma unroll
              for (int r = 0; r < 16; ++r) cin[r] = 0.f;
            }
            acc = E::mfma(ap[c & 1][E::ta(term)], bq[0][E::tb(term)][c], cin);
#pragma unroll
            for (int pi = slot * NP / NS1; pi < (slot + 1) * NP / NS1; ++pi)
              stage_part(pi, st, tm, sa, sb, rm_out, slot2, st_l, st_w_v);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      if (NW == 8) __syncthreads();                      // interval boundary: the partner group moves on to its score phase
      if (BWD || real_next) prepare(acc, t + 1, slot1);
      stats_begin(slot1);
      __builtin_amdgcn_sched_barrier(0);
      // phase B: second product of tile t || P(t+1)
      // A operand yhat^T[feature][tile row] straight from the ROW-MAJOR planes with the transposing LDS read
      // (ds_read_b64_tr_b16: per 16-lane group a 4-row x 16-column block, lane 4q + p supplies the address of
      // (row q, columns 4p..4p+3) and receives column `lane & 15`, rows 0..3): no transposed copy of the tile, no
      // 2-byte stores.  Fragment element j of lane half h is tile row 16 kc + 8 (j >> 2) + 4 h + (j & 3), the
      // k order of the accumulator-as-operand P planes.
      const unsigned char* tbase = lds_rm[k3] + (4 * h + ((lane & 15) >> 2)) * S::ROWB + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
      auto load_ya = [&](int grp, u32x4 (&ya)[NPL]) {     // grp = kc * CT + c
        const int kc = grp / B::CT, c = grp % B::CT;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
          const unsigned char* p = tbase + pl * S::PLANE + (16 * kc) * S::ROWB + 64 * c;
          const uint2 lo = lds_read_tr16(p);
          const uint2 hi = lds_read_tr16(p + 8 * S::ROWB);
          ya[pl] = (u32x4){lo.x, lo.y, hi.x, hi.y};
        }
      };
      u32x4 ya[2][NPL];
      if (!NOO) load_ya(0, ya[0]);
#pragma unroll
      for (int grp = 0; grp < 2 * B::CT; ++grp) {
        const int kc = grp / B::CT, c = grp % B::CT;
        if (!NOO && grp + 1 < 2 * B::CT) load_ya(grp + 1, ya[(grp + 1) & 1]);
        u32x4 pp[NPL];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) pp[pl] = (u32x4){pc[kc][pl][0], pc[kc][pl][1], pc[kc][pl][2], pc[kc][pl][3]};
#pragma unroll
        for (int term = 0; term < NTERM; ++term) {
          if (!NOO) gacc[c] = E::mfma(ya[grp & 1][E::ta(term)], pp[E::tb(term)], gacc[c]);
          const int slot = grp * NTERM + term;
          if (BWD || real_next) {
#pragma unroll
            for (int m = slot * 24 / NG; m < (slot + 1) * 24 / NG; ++m) p_unit(m, acc, slot1, pn);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (BWD || real_next) finish_p();
      __syncthreads();
    };
    // NW = 8: waves 4..7 take one barrier more before the loop and waves 0..3 one more after it: the same number for
    // all, the second group one interval behind
    // (the group test on a scalar: a barrier inside a vector-divergent branch could be executed with an empty EXEC mask)
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    if (NW == 8 && wave_s >= 4) __syncthreads();
    int k3 = 0;
    int64_t tt = tile0;
    for (; tt + 2 < tile1; tt += 2) {
      step(std::true_type{}, tt, k3, pqa, pqb, ra, sla, swa, rb, slb, swb);
      k3 = (k3 + 1) % RING;
      step(std::true_type{}, tt + 1, k3, pqb, pqa, rb, slb, swb, ra, sla, swa);
      k3 = (k3 + 1) % RING;
    }
    if (tt + 1 < tile1) {                                  // two tiles left
      step(std::true_type{}, tt, k3, pqa, pqb, ra, sla, swa, rb, slb, swb);
      k3 = (k3 + 1) % RING;
      step(std::false_type{}, tt + 1, k3, pqb, pqa, rb, slb, swb, ra, sla, swa);
    } else {                                               // one tile left
      step(std::false_type{}, tt, k3, pqa, pqb, ra, sla, swa, rb, slb, swb);
    }
    if (NW == 8 && wave_s < 4) __syncthreads();
  }

  float* gout = gpart + (int64_t)split * mx * D;
  if (FWD) {
    const float l_o = __shfl_xor(l_run, 32, 64);
    // the sum carries the scale of P (2^kPExp), the rows P's and the streamed operand's; MODE 2: plain log2-domain sum
    if (h == 0 && row_i < mx)
      part[(int64_t)split * mx + row_i] =
          MODE == 2 ? make_float2(0.f, l_run + l_o) : make_float2(m_run, (l_run + l_o) * __builtin_amdgcn_exp2f(-E::kPExp));
  }
  const float o_mul = out_scale * (hw != nullptr ? hw[1] : 1.0f) * sgn_x * (UNSREF ? __builtin_amdgcn_exp2f(m_run) : 1.0f);
  if (!NOO && row_i < mx) {
#pragma unroll
    for (int c = 0; c < B::CT; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 v = make_float4(gacc[c][4 * g + 0] * o_mul, gacc[c][4 * g + 1] * o_mul,
                               gacc[c][4 * g + 2] * o_mul, gacc[c][4 * g + 3] * o_mul);
        *reinterpret_cast<float4*>(gout + row_i * D + 32 * c + 8 * g + 4 * h) = v;
      }
  }
}

}  // namespace
