// Shared pieces of the all-pairs kernels — InfoNCE (gcr_infonce.hip: lse-only forward and row ops; gcr_infonce_flash.hip:
// flash forward and backward) and BCE-with-logits (gcr_bce.hip): the softmax / softplus epilogues, the two f32-engine
// kernels (forward and backward), engine selection, the column split (FwdPlan), the merge and reduce kernels, the width
// dispatch and one launch plan per family (PairsPlan).  The split-operand two-product kernels: gcr_pairs_loop.h; the MFMA
// engines: gcr_tile.h (f32), gcr_b3.h (split operands).
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "gcr_b3.h"
#include "gcr_host.h"   // dispatch_value, dispatch_bool, gcr_align

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kNegBig = -1.0e30f;

// online-softmax update with one finished score tile; `rem` = table rows left from this lane's
// first accumulator row (n_rows - j0 - 4h): rows at or past it are masked out (ragged last tile).
// EXD: additionally the row whose in-tile offset (acc_row without the 4h) equals xr[t] is left out of
// anchor tile t's sums (the excluded diagonal pair; xr[t] < 0: none in this tile).
template <int NT, bool MASK, bool EXD = false>
__device__ __forceinline__ void lse_update(const f32x16 (&acc)[NT], int rem, float (&m_run)[NT], float (&l_run)[NT],
                                           const int* xr = nullptr) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rc = (r & 3) + 8 * (r >> 2);
      const bool keep = (!MASK || rc < rem) && !(EXD && rc == xr[t]);
      v[r] = keep ? acc[t][r] : -INFINITY;
    }
    float tmax = v[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, v[r]);
    const float m_new = fmaxf(m_run[t], tmax);
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(v[r] - m_new);
    l_run[t] = l_run[t] * __builtin_amdgcn_exp2f(m_run[t] - m_new) + sum;
    m_run[t] = m_new;
  }
}

// log2-domain pieces of the BCE-with-logits element (lightgcn.py:109-113): for the log2-domain score s2 = s log2 e
//   softplus(s) = ln2 * (max(s2, 0) + log2(1 + u)),  sigmoid(s) = s2 >= 0 ? 1 / (1 + u) : u / (1 + u),  u = 2^-|s2|.
// log2(1 + u) is compensated for the rounding of v = 1 + u (e = u - (v - 1) exactly; log2(v + e) = log2 v + (e / v) log2 e),
// so a strongly negative score keeps its ~2^s2 instead of 0.  The correction is taken as e log2 e: leaving the 1 / v out
// changes it by e u / v log2 e <= 2^-24 u log2 e, i.e. 2^-23 of log2(1 + u) at most — and the row-sum launch, which needs
// no sigmoid, then needs no reciprocal either (one quarter-rate instruction and a multiply per score less).
// A masked score (-inf) gives softplus = 0 and sigmoid = 0.
__device__ __forceinline__ void bce_terms(float s2, float& softplus2, float& sig) {
  const float u = __builtin_amdgcn_exp2f(-fabsf(s2));
  const float v = 1.0f + u;
  const float e = u - (v - 1.0f);
  softplus2 = fmaxf(s2, 0.f) + fmaf(e, kLog2e, __builtin_amdgcn_logf(v));
  const float rc = __builtin_amdgcn_rcpf(v);
  sig = s2 >= 0.f ? rc : u * rc;
}

// sigmoid alone (the backward's probability): 1 / (1 + 2^-s2) holds for either sign — 2^-s2 = inf gives 0, a masked score
// (-inf) gives 0, and 1 + 2^-s2 rounds at 2^-24 of itself whatever its size — three instructions instead of six.
__device__ __forceinline__ float bce_sigmoid(float s2) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-s2));
}

// BCE forward on the f32 engine: l_run += sum over the tile's live rows of softplus2
template <int NT, bool MASK>
__device__ __forceinline__ void bce_update(const f32x16 (&acc)[NT], int rem, float (&l_run)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rc = (r & 3) + 8 * (r >> 2);
      float sp, sg;
      bce_terms((!MASK || rc < rem) ? acc[t][r] : -INFINITY, sp, sg);
      sum += sp;
    }
    l_run[t] += sum;
  }
}

// in-tile offset of table row `i` for lane half h of the tile starting at j0 (matches (r&3)+8(r>>2) of
// the register that holds it), or -1 when the row is not one of this lane's 16
__device__ __forceinline__ int diag_offset(int64_t i, int64_t j0, int h) {
  const int64_t d = i - j0 - 4 * h;
  return (d >= 0 && d < 28) ? (int)d : -1;
}

__device__ __forceinline__ int rows_left(int64_t n_rows, int64_t j0, int h) {
  const int64_t rem = n_rows - j0 - 4 * h;
  return (int)(rem > 64 ? 64 : (rem < 0 ? 0 : rem));
}

// d <= 64 runs 3 blocks per CU: two symmetric waves on one SIMD fall into lock-step (their MFMA
// phases and exp2 phases coincide, scripts/exp_infonce.hip), a third wave breaks it (109 -> 126 TF
// on the bare tile loop); needs VGPRs <= 168.  (Folding a logit bound into the MFMA C operand to
// drop the running max was tried: not faster, and it costs ~1e-5 of the lse - pos difference.)
//
// COLSUM (gcl.py:34, the `sim.T` cross-entropy): the same pass also accumulates, for every table row
// j, sum_i exp2(t_ij - col_bound2) over the anchors: 32 extra exp2 per tile, a 5-step DPP row
// reduction per accumulator register (lane 31 / 63 end up with the two half-wave sums) and one
// float atomic per (wave, table row).  It needs a known logit bound (unit-norm rows: |t| <= scale2),
// and replaces a whole second pass with the roles swapped.
__device__ __forceinline__ float half_wave_sum_to_last_lane(float v) {
  // inclusive DPP scan inside each row of 16, then row 0 -> row 1 and row 2 -> row 3 broadcast-add:
  // lane 31 = sum(lanes 0..31), lane 63 = sum(lanes 32..63)
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, true));
  return v;
}

// one tile's share of a lane between its global load and its LDS store (infonce_fwd_e_kernel, infonce_pipe_kernel)
template <int N>
struct StagedRows {
  float4 v[N];
  float s[N];
  bool live[N];
};

template <int D, bool COLSUM, bool EXD = false, bool BCE = false>
__global__ __launch_bounds__(256, (D <= 64 ? 3 : 2)) void infonce_fwd_kernel(const float* __restrict__ a,
                                                             const float* __restrict__ a_scale, int64_t m_rows,
                                                             const float* __restrict__ b,
                                                             const float* __restrict__ b_scale, int64_t n_rows,
                                                             float scale2, int nsplit, int64_t tiles_per_split,
                                                             float2* __restrict__ part, float* __restrict__ col_sum,
                                                             float col_bound2) {
  using S = Shape<D>;
  __shared__ __align__(16) float lds[2][kTileJ * S::STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t mblk = blockIdx.x / nsplit;
  const int split = blockIdx.x % nsplit;
  const int64_t i0 = (mblk * 4 + wave) * (32 * S::NT);

  float bfrag[S::NT][S::KH];
#pragma unroll
  for (int t = 0; t < S::NT; ++t) load_stationary<D>(a, a_scale, m_rows, i0 + 32 * t + i32, h, scale2, bfrag[t]);

  float m_run[S::NT], l_run[S::NT], a_valid[S::NT];
#pragma unroll
  for (int t = 0; t < S::NT; ++t) {
    m_run[t] = kNegBig;
    l_run[t] = 0.f;
    a_valid[t] = (i0 + 32 * t + i32 < m_rows) ? 1.0f : 0.f;   // padding anchors add nothing to a column
  }

  const int64_t total_tiles = (n_rows + kTileJ - 1) / kTileJ;
  const int64_t tile0 = (int64_t)split * tiles_per_split;
  const int64_t tile1 = min(total_tiles, tile0 + tiles_per_split);
  float4 regs[S::NLD];
  if (tile0 < tile1) {
    stage_load<D>(b, b_scale, n_rows, tile0 * kTileJ, tid, regs);
    stage_store<D>(lds[0], tid, regs);
  }
  __syncthreads();
  for (int64_t tt = tile0; tt < tile1; ++tt) {
    const int cur = (int)((tt - tile0) & 1);
    // always stage a tile (the last iteration re-stages its own): keeps the loop body branch-free
    const int64_t nxt = tt + 1 < tile1 ? tt + 1 : tt;
    stage_load<D>(b, b_scale, n_rows, nxt * kTileJ, tid, regs);
    f32x16 acc[S::NT];
    score_tile<D>(lds[cur], i32, h, bfrag, acc);
    if (BCE) {                                      // sum of softplus instead of the online logsumexp
      if ((tt + 1) * kTileJ > n_rows)
        bce_update<S::NT, true>(acc, rows_left(n_rows, tt * kTileJ, h), l_run);
      else
        bce_update<S::NT, false>(acc, 64, l_run);
    } else if (EXD) {                               // diagonal pair (i, j = i) left out of the sums
      int xr[S::NT];
#pragma unroll
      for (int t = 0; t < S::NT; ++t) xr[t] = diag_offset(i0 + 32 * t + i32, tt * kTileJ, h);
      lse_update<S::NT, true, true>(acc, rows_left(n_rows, tt * kTileJ, h), m_run, l_run, xr);
    } else if ((tt + 1) * kTileJ > n_rows)   // only the table's ragged last tile pays for the row mask
      lse_update<S::NT, true>(acc, rows_left(n_rows, tt * kTileJ, h), m_run, l_run);
    else
      lse_update<S::NT, false>(acc, 64, m_run, l_run);
    if (COLSUM) {
      const int64_t j0 = tt * kTileJ;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float e = 0.f;
#pragma unroll
        for (int t = 0; t < S::NT; ++t) e += a_valid[t] * __builtin_amdgcn_exp2f(acc[t][r] - col_bound2);
        e = half_wave_sum_to_last_lane(e);
        const int64_t j = j0 + acc_row(r, h);
        if (i32 == 31 && j < n_rows) atomicAdd(col_sum + j, e);
      }
    }
    stage_store<D>(lds[cur ^ 1], tid, regs);
    __syncthreads();
  }

#pragma unroll
  for (int t = 0; t < S::NT; ++t) {
    const float m_o = __shfl_xor(m_run[t], 32, 64), l_o = __shfl_xor(l_run[t], 32, 64);
    const float m = fmaxf(m_run[t], m_o);
    const float l = l_run[t] * __builtin_amdgcn_exp2f(m_run[t] - m) + l_o * __builtin_amdgcn_exp2f(m_o - m);
    const int64_t row = i0 + 32 * t + i32;
    if (h == 0 && row < m_rows) part[(int64_t)split * m_rows + row] = BCE ? make_float2(0.f, l_run[t] + l_o) : make_float2(m, l);
  }
}

// Engine selection (use_b3, gcr_tile.h).  Default: the split-operand bf16 engine for d <= 128, where forward AND
// backward have it; d = 256 stays on the f32 MFMA (its three operand planes would not fit the registers).  The flag
// GCR_INFONCE_ENGINE_F32 of the _ex entry points forces the f32 MFMA.  The choice is an ARGUMENT, never
// read from the environment: the host wrapper resolves it once per forward and hands the same flag to
// the backward (which must recompute the forward's logits with the forward's engine, or sum_j P_ij = 1
// only holds to ~1e-6 and near-cancelling gradients lose digits).
//
// The two-plane f16 format of the pipelined two-product loop (EngH2, gcr_b3.h): rows of at most unit norm (the caller's
// promise), d <= 64, 1/tau within the pre-scale's head-room
// (1/tau <= 20 covers every call site of the reference — tau in 0.07 .. 0.5 — and keeps the format's logit error,
// 3 * 2^-22 * inv_tau * log2 e in the worst case, an order below the 1e-5 of the parity tests; at 1/tau = 40 .. 60 the
// two formats differ by up to 1.3e-5 in the gradients, scripts/stress_infonce_formats.py)
constexpr float kH2MaxInvTau = 20.0f;
bool use_h2(int d, float inv_tau, bool unit_rows, bool force_f32) {
  return use_b3(d, force_f32) && unit_rows && d <= 64 && inv_tau > 0.f && inv_tau <= kH2MaxInvTau;
}
// ... and the two-product loop (flash forward, backward) also at d = 128: two planes of 128 features fit the pipelined
// loop's registers (12-99 spilled dwords at 256), three do not (infonce_fwdo_b3_kernel / infonce_bwd_b3_kernel)
bool use_h2_loop(int d, float inv_tau, bool unit_rows, bool force_f32) {
  return use_b3(d, force_f32) && unit_rows && d <= 128 && inv_tau > 0.f && inv_tau <= kH2MaxInvTau;
}

struct FwdPlan {
  int nsplit;
  int64_t tiles_per_split;
  int64_t m_blocks;
};

// Column split.  `resident` = blocks the chip holds at once (256 CUs x blocks/CU of the kernel).
//  * few row blocks: ONE wave of blocks, nsplit = floor(resident / m_blocks): a grid slightly larger
//    than the resident set (784 vs 768) costs a whole extra round (2.15 -> 3.0 ms measured);
//  * many row blocks: several rounds are unavoidable, so make them short: <= 320 tiles per block and
//    >= 3 rounds (100K x 100K: 95 TF at 782 blocks, 119 TF at 3128; scripts/perf_infonce_ab.py);
//  * never fewer than 16 tiles per block (anchor prologue + partial merge dominate below that).
FwdPlan plan_fwd(int64_t m, int64_t n, int anchors_per_block, int64_t resident) {
  FwdPlan p;
  p.m_blocks = (m + anchors_per_block - 1) / anchors_per_block;
  const int64_t total_tiles = (n + kTileJ - 1) / kTileJ;
  int64_t nsplit;
  if (p.m_blocks * 2 <= resident) {
    nsplit = resident / p.m_blocks;
  } else {
    nsplit = (total_tiles + 319) / 320;
    if (p.m_blocks * nsplit < 3 * resident) nsplit = (3 * resident + p.m_blocks - 1) / p.m_blocks;
  }
  const int64_t max_split = total_tiles / 16 > 0 ? total_tiles / 16 : 1;
  if (nsplit > max_split) nsplit = max_split;
  if (nsplit > total_tiles) nsplit = total_tiles;
  if (nsplit < 1) nsplit = 1;
  p.tiles_per_split = (total_tiles + nsplit - 1) / nsplit;
  p.nsplit = (int)((total_tiles + p.tiles_per_split - 1) / p.tiles_per_split);
  if (p.nsplit < 1) p.nsplit = 1;
  return p;
}

// ------------------------------------------------------------------------------------------
// Backward (flash-style recompute).  For stationary rows x_i and streamed rows y_j:
//   P_ij = w_x[i] * exp(s_ij - lse_x[i]) + w_y[j] * exp(s_ij - lse_y[j]),  s = logits (1/tau scaled)
//   G[i, :] = inv_tau * sum_j P_ij * yhat_j                  (gradient w.r.t. the scaled row xhat_i)
// The score tile is recomputed exactly as in the forward; because its accumulator already has the
// stationary row on the lane and the streamed rows in the registers, register r IS the MFMA
// B-operand of k-step r of the second product G^T[c][i] += yhat[j_r][c] * P[j_r][i] (no LDS round
// trip for P); the A operand yhat[j_r(h)][c] is a conflict-free ds_read_b32 from the same tile.
// w_x/lse_x are the "lane side" statistics (row-softmax of the stationary rows), w_y/lse_y the
// "register side" ones (softmax over the stationary index for every streamed row): calling the
// kernel twice with the roles swapped yields both input gradients of the symmetric loss.
// ------------------------------------------------------------------------------------------
template <int D>
struct BwdShape {
  static constexpr int NT = D <= 64 ? 2 : 1;
  static constexpr int CT = D / 32 > 4 ? 4 : D / 32;     // column tiles of 32 handled per launch
  static constexpr int PASSES = (D / 32) / CT;
  static constexpr int ROWS_PER_BLOCK = 4 * 32 * NT;
};

template <int D, bool EXD = false, bool BCE = false>
__global__ __launch_bounds__(256, 2) void infonce_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ x_scale, int64_t mx, const float* __restrict__ y,
    const float* __restrict__ y_scale, int64_t ny, float scale2, float out_scale, const float* __restrict__ lse_x,
    const float* __restrict__ w_x, const float* __restrict__ lse_y, const float* __restrict__ w_y, int ct0, int nsplit,
    int64_t tiles_per_split, float* __restrict__ gpart) {
  using S = Shape<D>;
  using B = BwdShape<D>;
  __shared__ __align__(16) float lds[2][kTileJ * S::STRIDE];
  __shared__ __align__(16) float st_lse[2][kTileJ];
  __shared__ __align__(16) float st_w[2][kTileJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t mblk = blockIdx.x / nsplit;
  const int split = blockIdx.x % nsplit;
  const int64_t i0 = (mblk * 4 + wave) * (32 * B::NT);

  float bfrag[B::NT][S::KH];
  float lse2l[B::NT], wl[B::NT];
#pragma unroll
  for (int t = 0; t < B::NT; ++t) {
    const int64_t row = i0 + 32 * t + i32;
    load_stationary<D>(x, x_scale, mx, row, h, scale2, bfrag[t]);
    const bool on = row < mx && w_x != nullptr;
    wl[t] = on ? w_x[row] : 0.f;
    lse2l[t] = (on && !BCE) ? lse_x[row] * kLog2e : 1.0e30f;  // disabled term: exp2(-huge) = 0, never 0 * inf
  }
  f32x16 gacc[B::NT][B::CT];
#pragma unroll
  for (int t = 0; t < B::NT; ++t)
#pragma unroll
    for (int c = 0; c < B::CT; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) gacc[t][c][r] = 0.f;

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
      s_lse = (on && !BCE) ? lse_y[j] * kLog2e : 1.0e30f;
    }
  };
  auto store_stats = [&](int buf) {
    if (tid < kTileJ) {
      st_lse[buf][tid] = s_lse;
      st_w[buf][tid] = s_w;
    }
  };
  if (tile0 < tile1) {
    stage_load<D>(y, y_scale, ny, tile0 * kTileJ, tid, regs);
    load_stats(tile0 * kTileJ);
    stage_store<D>(lds[0], tid, regs);
    store_stats(0);
  }
  __syncthreads();
  for (int64_t tt = tile0; tt < tile1; ++tt) {
    const int cur = (int)((tt - tile0) & 1);
    const bool more = tt + 1 < tile1;
    if (more) {
      stage_load<D>(y, y_scale, ny, (tt + 1) * kTileJ, tid, regs);
      load_stats((tt + 1) * kTileJ);
    }
    f32x16 acc[B::NT];
    {
#pragma unroll
      for (int t = 0; t < B::NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      const float* base = lds[cur] + i32 * S::STRIDE + h * S::KH;
#pragma unroll
      for (int q = 0; q < S::KH / 4; ++q) {
        const float4 av = *reinterpret_cast<const float4*>(base + 4 * q);
        const float ae[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = 0; t < B::NT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae[e], bfrag[t][4 * q + e], acc[t], 0, 0, 0);
      }
    }
    const int64_t j0 = tt * kTileJ;
    const bool ragged = j0 + kTileJ > ny;
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
        const bool dead_j = ragged && (j0 + acc_row(r, h) >= ny);
#pragma unroll
        for (int t = 0; t < B::NT; ++t) {
          // EXD: the diagonal pair (stationary row i, streamed row j = i) carries no probability
          const bool dead = dead_j || (EXD && diag_offset(i0 + 32 * t + i32, j0, h) == e + 8 * g);
          const float sc = dead ? -INFINITY : acc[t][r];
          if (BCE) {                                // P = (w_x[i] + w_y[j]) sigmoid(s_ij)
            acc[t][r] = (wl[t] + wre[e]) * bce_sigmoid(sc);
          } else
            acc[t][r] = wl[t] * __builtin_amdgcn_exp2f(sc - lse2l[t]) + wre[e] * __builtin_amdgcn_exp2f(sc - lre[e]);
        }
      }
    }
    // G^T[c][i] += yhat[j_r][c] * P[j_r][i]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* yrow = lds[cur] + acc_row(r, h) * S::STRIDE + 32 * ct0 + i32;
#pragma unroll
      for (int c = 0; c < B::CT; ++c) {
        const float yv = yrow[32 * c];
#pragma unroll
        for (int t = 0; t < B::NT; ++t)
          gacc[t][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(yv, acc[t][r], gacc[t][c], 0, 0, 0);
      }
    }
    if (more) {
      stage_store<D>(lds[cur ^ 1], tid, regs);
      store_stats(cur ^ 1);
    }
    __syncthreads();
  }

  // gacc[t][c] register rr of lane (i, h) is column 32*(ct0+c) + acc_row(rr, h) of row i
  float* gout = gpart + (int64_t)split * mx * D;
#pragma unroll
  for (int t = 0; t < B::NT; ++t) {
    const int64_t row = i0 + 32 * t + i32;
    if (row < mx) {
#pragma unroll
      for (int c = 0; c < B::CT; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 v = make_float4(gacc[t][c][4 * g + 0] * out_scale, gacc[t][c][4 * g + 1] * out_scale,
                                 gacc[t][c][4 * g + 2] * out_scale, gacc[t][c][4 * g + 3] * out_scale);
          *reinterpret_cast<float4*>(gout + row * D + 32 * (ct0 + c) + 8 * g + 4 * h) = v;
        }
    }
  }
}

// workgroup shape of the split-operand two-product kernels (gcr_pairs_loop.h)
template <int D>
struct BwdB3 {
  static constexpr int CT = D / 32;                    // feature tiles of 32, all in one launch
  static constexpr int RT = 72;                        // bytes per feature of a transposed plane
  static constexpr int TPLANE = D * RT;
  static constexpr int ROWS_PER_BLOCK = 128;           // one tile of 32 stationary rows per wave
  static constexpr int TILE_BYTES = 3 * ShapeB3<D>::PLANE + 3 * TPLANE;
};

// natural-log LSE of the scaled logits from the per-split (max2, sum2) partials
__global__ void infonce_merge_kernel(const float2* __restrict__ part, int nsplit, int64_t m_rows,
                                     float* __restrict__ lse) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m_rows) return;
  float m = kNegBig;
  for (int s = 0; s < nsplit; ++s) m = fmaxf(m, part[(int64_t)s * m_rows + i].x);
  float l = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float2 p = part[(int64_t)s * m_rows + i];
    l += p.y * __builtin_amdgcn_exp2f(p.x - m);
  }
  lse[i] = (m + __log2f(l)) * kLn2;
}

// lse and o from the per-split partials: o = sum_s O_s 2^(m_s - m) / sum_s l_s 2^(m_s - m)
__global__ __launch_bounds__(256) void infonce_merge_o_kernel(const float2* __restrict__ part, const float* __restrict__ opart,
                                                              int nsplit, int64_t m_rows, int d, float* __restrict__ lse,
                                                              float* __restrict__ o) {
  const int d4 = d / 4;
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m_rows * d4) return;
  const int64_t i = k / d4;
  const int c = (int)(k % d4);
  float m = kNegBig;
  for (int s = 0; s < nsplit; ++s) m = fmaxf(m, part[(int64_t)s * m_rows + i].x);
  float l = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < nsplit; ++s) {
    const float2 p = part[(int64_t)s * m_rows + i];
    const float w = __builtin_amdgcn_exp2f(p.x - m);
    l += p.y * w;
    const float4 v = reinterpret_cast<const float4*>(opart)[((int64_t)s * m_rows + i) * d4 + c];
    acc.x += v.x * w; acc.y += v.y * w; acc.z += v.z * w; acc.w += v.w * w;
  }
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  reinterpret_cast<float4*>(o)[i * d4 + c] = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
  if (c == 0) lse[i] = (m + __log2f(l)) * kLn2;
}

// g[i, :] = sum over splits (fixed order) of the partial gradients
__global__ __launch_bounds__(256) void bwd_reduce_kernel(const float* __restrict__ gpart, int nsplit, int64_t n4,
                                                         float* __restrict__ g) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n4; k += (int64_t)gridDim.x * blockDim.x) {
    float4 s = reinterpret_cast<const float4*>(gpart)[k];
    for (int p = 1; p < nsplit; ++p) {
      const float4 v = reinterpret_cast<const float4*>(gpart)[(int64_t)p * n4 + k];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    reinterpret_cast<float4*>(g)[k] = s;
  }
}

// ... for the two-product launches (flash forward, backward, BCE loop)
FwdPlan plan_bwd_rows(int64_t mx, int64_t ny, int d, int rows_per_block, int64_t resident) {
  FwdPlan p = plan_fwd(mx, ny, rows_per_block, resident);
  // every split keeps an [mx, D] fp32 partial: with many stationary rows the row blocks alone fill
  // the chip, and the partials must stay small (cap 1 GiB)
  const int64_t total_tiles = (ny + kTileJ - 1) / kTileJ;
  while (p.nsplit > 1 && (p.m_blocks >= 3 * resident || (int64_t)p.nsplit * mx * d * 4 > (1ll << 30))) {
    p.tiles_per_split *= 2;
    p.nsplit = (int)((total_tiles + p.tiles_per_split - 1) / p.tiles_per_split);
  }
  return p;
}

// `resident` of a kernel that runs `per_cu` workgroups per CU: 3 for the f32 forward at d <= 64 (its launch bounds), 2 for
// every other 256-thread kernel, 1 for the 512-thread forms
constexpr int64_t kCUs = 256;
constexpr int64_t resident_blocks(int per_cu) { return kCUs * per_cu; }

// The 512-thread forms (NW = 8 of infonce_fwd_e_kernel and infonce_pipe_kernel: twice the rows per workgroup, one
// workgroup per CU) share each staged tile between two wave groups, which pays at d = 64 with long tile loops: measured
// against the 256-thread form of the flash forward on one box — 2048 x 1M 1.73 -> 1.60 ms, 100K x 100K 7.93 -> 7.73 ms;
// d = 32 (nothing to share: 256 lanes already stage a whole tile) 4-14 % slower.  (The backward used it too in round 2 —
// 100K x 100K 9.20 -> 8.94 ms — until its staging moved into a pre-pass: launch_bwd.)
constexpr int64_t kEightWaveTiles = 256;
bool h2_eight_waves(int d, const FwdPlan& p8) { return d == 64 && p8.tiles_per_split >= kEightWaveTiles; }

bool bce_pipe(int d, bool force_f32) { return d <= 64 && use_b3(d, force_f32); }

// ------------------------------------------------------------------------------------------
// Dispatch over the four widths of the all-pairs kernels (gcr_host.h: dispatch_value, dispatch_bool).
// ------------------------------------------------------------------------------------------
template <class F>
auto dispatch_dim(int d, F&& f) { return dispatch_value<32, 64, 128, 256>(d, std::forward<F>(f)); }
// the lse forward's (COLSUM, EXD): plain, column sums or excluded diagonal — the last two never meet
template <class F>
void dispatch_lse_mode(bool exd, bool colsum, F&& f) {
  if (exd) f(std::false_type{}, std::true_type{});
  else if (colsum) f(std::true_type{}, std::false_type{});
  else f(std::false_type{}, std::false_type{});
}

// ------------------------------------------------------------------------------------------
// One plan per launch family: the paths its launcher can take for (m, n, d) — engine and workgroup form — with the column
// split of each and the byte offsets of its regions of the workspace.  The launcher picks one path and takes every pointer
// from it; the _workspace_bytes export is the largest `bytes` of the same enumeration (the query has no flags: it covers
// every engine).  Rows per workgroup come from the kernels' shape structs: a retuned shape moves launch and query together.
// ------------------------------------------------------------------------------------------
struct PairsPath {
  bool open = false;        // the launcher can take this path at this width
  FwdPlan p{};
  // byte offsets into the workspace (0 where the path has no such region)
  int64_t hw = 0;           // h2_wscale_kernel's two floats
  int64_t image = 0;        // h2_prestage_kernel's image of the streamed rows
  int64_t part = 0;         // per-split (max, sum) pairs, or the per-split partial gradients
  int64_t opart = 0;        // per-split o rows
  int64_t scales = 0;       // bce_row_scales_kernel: inv, nrm of both sides and f of the streamed side
  int64_t bytes = 0;        // what the path needs of the workspace
};

template <int N>
struct PairsPlan {
  PairsPath path[N];
  PairsPath& open(int k, const FwdPlan& p) { return path[k] = PairsPath{true, p}; }
  int64_t bytes() const {
    int64_t b = 0;
    for (const PairsPath& q : path) b = q.open && q.bytes > b ? q.bytes : b;
    return b;
  }
};

template <class T>
T* ws_at(void* workspace, int64_t offset) { return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset); }

// lse-only forward: (max, sum) pairs per split and anchor
enum { kLseF32, kLseSplit, kLseSplit8, kLsePaths };
PairsPlan<kLsePaths> plan_lse_fwd(int64_t m, int64_t n, int d) {
  PairsPlan<kLsePaths> pl;
  auto open = [&](int k, const FwdPlan& p) { pl.open(k, p).bytes = p.nsplit * m * (int64_t)sizeof(float2); };
  dispatch_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    open(kLseF32, plan_fwd(m, n, Shape<D>::ANCHORS_PER_BLOCK, resident_blocks(D <= 64 ? 3 : 2)));
    if constexpr (D <= 128) open(kLseSplit, plan_fwd(m, n, ShapeB3<D>::ANCHORS_PER_BLOCK, resident_blocks(2)));
    if constexpr (D == 64) open(kLseSplit8, plan_fwd(m, n, 2 * ShapeB3<D>::ANCHORS_PER_BLOCK, resident_blocks(1)));
  });
  return pl;
}

// flash forward (d <= 128): the (reference point, sum) pairs, the un-normalised o rows behind them
enum { kFlashRows4, kFlashRows8, kFlashPaths };
PairsPlan<kFlashPaths> plan_flash_fwd(int64_t m, int64_t n, int d) {
  PairsPlan<kFlashPaths> pl;
  auto open = [&](int k, const FwdPlan& p) {
    PairsPath& q = pl.open(k, p);
    q.opart = p.nsplit * m * (int64_t)sizeof(float2);
    q.bytes = q.opart + p.nsplit * m * d * (int64_t)sizeof(float);
  };
  dispatch_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    if constexpr (D <= 128) open(kFlashRows4, plan_bwd_rows(m, n, D, BwdB3<D>::ROWS_PER_BLOCK, resident_blocks(2)));
    // (d = 32 never takes the 512-thread form — h2_eight_waves — but the size query has counted it for every d <= 64 since
    // the form exists, and the sizes callers see stay what they were)
    if constexpr (D <= 64) open(kFlashRows8, plan_bwd_rows(m, n, D, 2 * BwdB3<D>::ROWS_PER_BLOCK, resident_blocks(1)));
  });
  return pl;
}

// InfoNCE backward: d <= 128 starts with the two floats of h2_wscale_kernel, followed at kBwdHeader by
// h2_prestage_kernel's image of the streamed rows (two per-row arrays and the scaled rows themselves, padded to whole
// tiles), rounded to 256 B; the per-split partial gradients start behind them (a single split writes g itself)
constexpr int64_t kBwdHeader = 256;
constexpr int64_t fold_rows(int64_t ny) { return (ny + kTileJ - 1) / kTileJ * kTileJ; }
constexpr int64_t bwd_header_bytes(int64_t ny, int d) {
  return d <= 128 ? kBwdHeader + gcr_align(fold_rows(ny) * (2 + d) * (int64_t)sizeof(float), 256) : 0;
}
enum { kBwdF32, kBwdSplit, kBwdPaths };
PairsPlan<kBwdPaths> plan_infonce_bwd(int64_t mx, int64_t ny, int d) {
  PairsPlan<kBwdPaths> pl;
  auto open = [&](int k, const FwdPlan& p) {
    PairsPath& q = pl.open(k, p);
    q.image = kBwdHeader;
    q.part = bwd_header_bytes(ny, d);
    q.bytes = q.part + (p.nsplit > 1 ? p.nsplit * mx * d * (int64_t)sizeof(float) : 0);
  };
  dispatch_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    open(kBwdF32, plan_bwd_rows(mx, ny, D, BwdShape<D>::ROWS_PER_BLOCK, resident_blocks(2)));
    if constexpr (D <= 128) open(kBwdSplit, plan_bwd_rows(mx, ny, D, BwdB3<D>::ROWS_PER_BLOCK, resident_blocks(2)));
  });
  return pl;
}

// BCE: behind the partials of whichever path runs (rounded to 256 B, at ONE offset for both paths) the scratch of the
// two-plane format (d <= 64): inv / nrm of both sides, f of the streamed side, hw[2]
enum { kBceLoop, kBceF32, kBcePaths };
void bce_scratch_behind(PairsPlan<kBcePaths>& pl, int64_t m, int64_t n, int d) {
  const int64_t core = gcr_align(pl.bytes(), 256);
  for (PairsPath& q : pl.path) {
    q.scales = core;
    q.hw = core + (2 * m + 3 * n) * (int64_t)sizeof(float);
    q.bytes = core + (d <= 64 ? gcr_align((2 * m + 3 * n + 8) * (int64_t)sizeof(float), 256) : 0);
  }
}

// BCE forward: row sums of softplus per split (as float2, like the lse partials), at d <= 64 the o rows behind them (the
// f32 path has no o, but its partials are sized like the loop's)
PairsPlan<kBcePaths> plan_bce_fwd(int64_t m, int64_t n, int d) {
  PairsPlan<kBcePaths> pl;
  auto open = [&](int k, const FwdPlan& p) {
    PairsPath& q = pl.open(k, p);
    q.opart = p.nsplit * m * (int64_t)sizeof(float2);
    q.bytes = q.opart + (d <= 64 ? p.nsplit * m * d * (int64_t)sizeof(float) : 0);
  };
  dispatch_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    if constexpr (D <= 64) open(kBceLoop, plan_bwd_rows(m, n, D, BwdB3<D>::ROWS_PER_BLOCK, resident_blocks(2)));
    open(kBceF32, plan_fwd(m, n, Shape<D>::ANCHORS_PER_BLOCK, resident_blocks(D <= 64 ? 3 : 2)));
  });
  bce_scratch_behind(pl, m, n, d);
  return pl;
}

// BCE backward: the per-split partial gradients (a single split writes g itself)
PairsPlan<kBcePaths> plan_bce_bwd(int64_t mx, int64_t ny, int d) {
  PairsPlan<kBcePaths> pl;
  auto open = [&](int k, const FwdPlan& p) {
    pl.open(k, p).bytes = p.nsplit > 1 ? p.nsplit * mx * d * (int64_t)sizeof(float) : 0;
  };
  dispatch_dim(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    if constexpr (D <= 64) open(kBceLoop, plan_bwd_rows(mx, ny, D, BwdB3<D>::ROWS_PER_BLOCK, resident_blocks(2)));
    open(kBceF32, plan_bwd_rows(mx, ny, D, BwdShape<D>::ROWS_PER_BLOCK, resident_blocks(2)));
  });
  bce_scratch_behind(pl, mx, ny, d);
  return pl;
}

int32_t reduce_splits(const FwdPlan& p, const float* gpart, int64_t mx, int d, float* g, hipStream_t s) {
  if (p.nsplit <= 1) return GCR_OK;
  const int64_t n4 = mx * d / 4;
  const int64_t want = (n4 + 255) / 256;
  hipLaunchKernelGGL(bwd_reduce_kernel, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(256), 0, s, gpart, p.nsplit,
                     n4, g);
  return GCR_LAUNCH_STATUS();
}

}  // namespace

// One pass of the InfoNCE backward on the f32 engine: launched by gcr_infonce_flash.hip, instantiated in gcr_infonce.hip
// beside the f32 forward — the two kernels share the internal staging helpers of gcr_tile.h, and compiled in different units
// the forward comes out as other machine code at d >= 64 (EXPERIMENTS.md).  Takes no type of the anonymous namespace.
__attribute__((visibility("hidden"))) void gcr_infonce_bwd_f32_launch(
    int d, bool exd, dim3 grid, hipStream_t s, const float* x, const float* x_scale, int64_t mx, const float* y,
    const float* y_scale, int64_t ny, float scale2, float out_scale, const float* lse_x, const float* w_x, const float* lse_y,
    const float* w_y, int ct0, int nsplit, int64_t tiles_per_split, float* gpart);
