// InfoNCE / prototype-contrast logits with fused temperature scale and row logsumexp on the
// fp32 MFMA of gfx950 (v_mfma_f32_32x32x2_f32: exact f32, 64 FLOP/clk/SIMD, ~155 TF dense).
//
// Replaces the materialised score matrices of
//   InfoNCE            ncl.py:125-130, ssl4rec.py:19-23   (view1 @ view2.T / t -> log_softmax diag)
//   info_nce_loss      gcl.py:28-35                       (sim, sim.T cross-entropies)
//   ssl_layer_loss     ncl.py:358-367                     (B anchors x ALL layer-0 rows, exp-sum)
//   ProtoNCE_loss      ncl.py:369-375, batch_softmax_loss ssl4rec.py:25-30
// The M x N logits never leave the register file.
//
// Mapping.  The score tile is computed TRANSPOSED: MFMA "A" = 32 streamed table rows j, MFMA "B" =
// 32 stationary anchors i, so in the 32x32 accumulator a lane owns ONE anchor (column i = lane&31)
// and its 16 registers are 16 different table rows: the online max / exp2-sum over j is in-lane
// work, no cross-lane traffic until one final lane<->lane+32 merge.  The K (= d) dimension is
// split between the two lane halves (half h covers features [h*d/2, (h+1)*d/2)), so each lane's
// operand slice is contiguous in memory: 16-byte global loads for the stationary anchors, and
// conflict-free ds_read_b128 (row stride padded by 16 B) for the streamed tile.
// A wave keeps NT x 32 anchors (pre-multiplied by 1/||a|| * 1/tau * log2(e)) in registers and walks
// a column range of the table; table tiles of 32 rows are staged global -> registers -> LDS
// (normalised on the way) one tile ahead of the MFMAs (double buffer, one barrier per tile).
// Grid = anchor blocks x column splits; split partials (max, sum) are merged by a second kernel.
//
// This file holds the lse-only forward and the row ops (row norms, positive logit and its gradient, the gradient through
// F.normalize).  The flash forward and the backward are in gcr_infonce_flash.hip, the BCE-with-logits launches, which
// instantiate the same kernel templates with another epilogue, in gcr_bce.hip; what the three share is gcr_pairs.h, the
// two-product kernels gcr_pairs_loop.h.  The f32 engine they are built on is gcr_tile.h, the split-operand engines (EngB3,
// EngH2) gcr_b3.h; the nearest-centroid search of the k-means E-step, a third user of both, is in gcr_kmeans.hip.
#include "gcr_pairs.h"

namespace {

// staging with a workgroup of THREADS lanes (the 512-thread form of infonce_fwd_e_kernel: one float4 per lane at d = 64)
// The loads only: the row AND its scale go to registers untouched, the multiply happens where the tile is staged
// (stage_store_t_one), most of a tile loop iteration later.  (Multiplying here — and loading the scale inside an
// `if (b_scale)` — made every iteration open with `global_load ...; s_waitcnt vmcnt(0)`: a whole memory round trip in
// front of the first MFMA of every tile, for all waves of the workgroup at once.)  `b_scale == nullptr` loads a dummy
// word of `b` through a zero stride instead of branching (the value is replaced by 1 where it is used; both pointers are
// global, so the load stays a global_load — a generic-address load would tie vmcnt to lgkmcnt).
template <int D, int THREADS>
__device__ __forceinline__ void stage_load_t(const float* __restrict__ b, const float* __restrict__ b_scale, int64_t n_rows,
                                             int64_t j0, int tid, StagedRows<(kTileJ * D / 4) / THREADS>& g) {
  const float* __restrict__ sp = b_scale != nullptr ? b_scale + j0 : b;          // wave-uniform bases + small 32-bit lane offsets
  const float* __restrict__ tb = b + j0 * D;
  const unsigned stride = b_scale != nullptr ? 1u : 0u;
  const int rem = (int)min((int64_t)kTileJ, n_rows - j0);  // rows of this tile that exist (>= 1)
#pragma unroll
  for (int u = 0; u < (kTileJ * D / 4) / THREADS; ++u) {
    const int idx = tid + THREADS * u;
    const int row = idx / (D / 4), c4 = idx % (D / 4);
    const unsigned rr = (unsigned)min(row, rem - 1) & (kTileJ - 1);   // rows behind the end repeat the last one ...
    g.v[u] = *reinterpret_cast<const float4*>(tb + (rr * D + 4u * c4));
    g.s[u] = sp[rr * stride];
    g.live[u] = row < rem;                                   // ... with scale 0, applied with the multiply
  }
}

template <class E, int D, int THREADS>
__device__ __forceinline__ void stage_store_t_one(unsigned char* __restrict__ tile, int tid, const float4& v, float sc,
                                                  bool live, bool has_scale, int u) {
  using S = ShapeB3<D>;
  const int idx = tid + THREADS * u;
  const int row = idx / (D / 4), c4 = idx % (D / 4);
  unsigned qa[E::NPL], qb[E::NPL];
  sc = live ? (has_scale ? sc * E::kSY : E::kSY) : 0.f;
  E::split(v.x * sc, v.y * sc, qa);
  E::split(v.z * sc, v.w * sc, qb);
  unsigned char* p = tile + row * S::ROWB + c4 * 8;
#pragma unroll
  for (int pl = 0; pl < E::NPL; ++pl) *reinterpret_cast<uint2*>(p + pl * S::PLANE) = make_uint2(qa[pl], qb[pl]);
}

// NW = 8: a 512-thread workgroup of 512 anchors shares each staged table tile — half the staging (operand split + LDS
// stores) per MFMA of the 256-thread form; chosen for long splits at d = 64 (launch_fwd).
template <class E, int D, bool COLSUM, bool EXD = false, int NW = 4>
__global__ __launch_bounds__(64 * NW, 2) void infonce_fwd_e_kernel(const float* __restrict__ a,
                                                                const float* __restrict__ a_scale, int64_t m_rows,
                                                                const float* __restrict__ b,
                                                                const float* __restrict__ b_scale, int64_t n_rows,
                                                                float scale2, int nsplit, int64_t tiles_per_split,
                                                                float2* __restrict__ part, float* __restrict__ col_sum,
                                                                float col_bound2) {
  using S = ShapeB3<D>;
  constexpr int NPL = E::NPL, NTERM = E::NTERM;
  constexpr int THREADS = 64 * NW, NLD = (kTileJ * D / 4) / THREADS;
  static_assert(NLD >= 1, "more lanes than float4s in a tile");
  __shared__ __align__(16) unsigned char lds[2][NPL * S::PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t mblk = blockIdx.x / nsplit;
  const int split = blockIdx.x % nsplit;
  const int64_t i0 = (mblk * NW + wave) * (32 * S::NT);

  u32x4 bq[S::NT][NPL][S::KC];
#pragma unroll
  for (int t = 0; t < S::NT; ++t)
    load_stationary_e<E, D>(a, a_scale, m_rows, i0 + 32 * t + i32, h, scale2 * E::kSX, bq[t]);

  // Two-plane format = rows of at most unit norm (the caller's promise): every log2-domain logit is <= scale2, so the
  // running sums take that bound as a FIXED reference point (terms >= 2^(-2 scale2) >= 2^-58 at 1/tau <= 20): no row
  // maximum, no rescale — 14 of ~100 vector instructions per 32 x 32 tile less
  constexpr bool FIXREF = E::NPL == 2;
  // ... and that fixed point is ZERO: a term is 2^s with |s| <= scale2 <= 29, the sum over up to 2^40 rows stays below 2^70
  // — no reference needed for range, none for precision (f32 is scale-invariant) — so with E::kSInv == 1 a probability is
  // exp2 of the accumulator register itself
  const float m_fix = 0.f;
  float m_run[S::NT], l_run[S::NT], a_valid[S::NT];
#pragma unroll
  for (int t = 0; t < S::NT; ++t) {
    m_run[t] = FIXREF ? m_fix : kNegBig;
    l_run[t] = 0.f;
    a_valid[t] = (i0 + 32 * t + i32 < m_rows) ? 1.0f : 0.f;
  }

  const int64_t total_tiles = (n_rows + kTileJ - 1) / kTileJ;
  const int64_t tile0 = (int64_t)split * tiles_per_split;
  const int64_t tile1 = min(total_tiles, tile0 + tiles_per_split);
  StagedRows<NLD> ga, gb;                                  // two tiles in flight: loaded in one step, staged in the next
  auto colsum = [&](const f32x16 (&acc)[S::NT], int64_t tt) {
    const int64_t j0 = tt * kTileJ;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float e = 0.f;
#pragma unroll
      for (int t = 0; t < S::NT; ++t) e += a_valid[t] * __builtin_amdgcn_exp2f(acc[t][r] - col_bound2);   // acc already scaled
      e = half_wave_sum_to_last_lane(e);
      const int64_t j = j0 + acc_row(r, h);
      if (i32 == 31 && j < n_rows) atomicAdd(col_sum + j, e);
    }
  };
  // the table's last tile is the only one that can be ragged
  auto epilogue_any = [&](f32x16 (&acc)[S::NT], int64_t tt) {
    if (E::kSInv != 1.0f) {                               // accumulator -> log2-domain scores
#pragma unroll
      for (int t = 0; t < S::NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] *= E::kSInv;
    }
    if (EXD) {
      int xr[S::NT];
#pragma unroll
      for (int t = 0; t < S::NT; ++t) xr[t] = diag_offset(i0 + 32 * t + i32, tt * kTileJ, h);
      lse_update<S::NT, true, true>(acc, rows_left(n_rows, tt * kTileJ, h), m_run, l_run, xr);
    } else if ((tt + 1) * kTileJ > n_rows)
      lse_update<S::NT, true>(acc, rows_left(n_rows, tt * kTileJ, h), m_run, l_run);
    else
      lse_update<S::NT, false>(acc, 64, m_run, l_run);
    if (COLSUM) colsum(acc, tt);
  };
  if (tile0 >= tile1) {
    // empty split (plan_fwd never makes one): fall through to the (kNegBig, 0) partial
  } else {
    // Software pipeline, interleaved by hand: the MFMAs of tile tt+1 alternate in program order with
    // the softmax VALU work of tile tt (branch-free: every tile before the split's last one is full)
    // and with the operand split of tile tt+2, one share of VALU "units" per MFMA slot, pinned by
    // sched_barrier.  A wave issues in order, so this is what lets ONE wave keep the matrix pipe busy
    // under its own exp2 / max / add stream (two waves of a SIMD otherwise fall into lock-step and
    // serialise: measured 48 % MFMA utilisation before, scripts/perf_infonce_engine_ab.py).
    constexpr int NS = NTERM * S::KC * S::NT;                     // MFMA slots per step
    constexpr int NU = 22 * S::NT + NLD + (COLSUM ? 16 : 0);      // VALU micro-units per step
    const int64_t last = tile1 - 1;
    f32x16 acc_a[S::NT], acc_b[S::NT];
    auto store_all = [&](unsigned char* tile, const StagedRows<NLD>& g) {
#pragma unroll
      for (int u = 0; u < NLD; ++u) stage_store_t_one<E, D, THREADS>(tile, tid, g.v[u], g.s[u], g.live[u], b_scale != nullptr, u);
    };
    stage_load_t<D, THREADS>(b, b_scale, n_rows, tile0 * kTileJ, tid, ga);
    stage_load_t<D, THREADS>(b, b_scale, n_rows, min(tile0 + 1, last) * kTileJ, tid, gb);
    store_all(lds[0], ga);
    stage_load_t<D, THREADS>(b, b_scale, n_rows, min(tile0 + 2, last) * kTileJ, tid, ga);
    __syncthreads();
    score_tile_e<E, D, S::NT>(lds[0], i32, h, bq, acc_a);
    store_all(lds[1], gb);
    __syncthreads();
    // step tt: scores of tile tt + 1 (in lds[nb]) || softmax of tile tt || staging of tile tt + 2 (loaded one step
    // earlier, in `st`) into the other buffer || the loads of tile tt + 3 into `ld`: a load has a whole step to land — it
    // used to be issued at the top of the step that staged it, with its scale multiplied in on the spot, i.e. behind a
    // `s_waitcnt vmcnt(0)` that every wave of the workgroup sat out in front of the step's first MFMA
    auto step = [&](f32x16 (&cur)[S::NT], f32x16 (&nxt)[S::NT], int64_t tt, int nb, StagedRows<NLD>& ld,
                    const StagedRows<NLD>& st) {
      stage_load_t<D, THREADS>(b, b_scale, n_rows, min(tt + 3, last) * kTileJ, tid, ld);
      const unsigned char* base = lds[nb] + i32 * S::ROWB + h * (S::KH * 2);
      unsigned char* out = lds[nb ^ 1];
      float tmax[S::NT], m_new[S::NT], sum[S::NT];
      int xr[S::NT];
      if (EXD) {
#pragma unroll
        for (int t = 0; t < S::NT; ++t) xr[t] = diag_offset(i0 + 32 * t + i32, tt * kTileJ, h);
      }
      // micro-unit m of the step's VALU work: m < 22*NT -> softmax unit m / NT of anchor tile m % NT
      // (0-3 partial max, 4 new max, 5-20 exp2-add of one register, 21 fold into the running sum);
      // then the operand split + LDS store of one staged float4; then (COLSUM) one register's column sums
      auto micro = [&](int m) {
        const int u = m / S::NT, t = m % S::NT;
        if (m >= 22 * S::NT + NLD) {
          if (COLSUM) {
            const int r = m - 22 * S::NT - NLD;
            float e = 0.f;
#pragma unroll
            for (int q = 0; q < S::NT; ++q) e += a_valid[q] * __builtin_amdgcn_exp2f(fmaf(cur[q][r], E::kSInv, -col_bound2));
            e = half_wave_sum_to_last_lane(e);
            const int64_t j = tt * kTileJ + acc_row(r, h);
            if (i32 == 31 && j < n_rows) atomicAdd(col_sum + j, e);
          }
        } else if (m >= 22 * S::NT) {
          stage_store_t_one<E, D, THREADS>(out, tid, st.v[m - 22 * S::NT], st.s[m - 22 * S::NT], st.live[m - 22 * S::NT],
                                           b_scale != nullptr, m - 22 * S::NT);
        } else if (u < 4) {
          if (EXD) {                                    // excluded diagonal pair: -inf before it is seen by max / exp2
#pragma unroll
            for (int e = 0; e < 4; ++e) cur[t][4 * u + e] = (xr[t] == e + 8 * u) ? -INFINITY : cur[t][4 * u + e];
          }
          if (!FIXREF) {
            // chained so that each pair of scores costs one v_max3_f32
            const float x0 = u == 0 ? cur[t][0] : tmax[t];
            tmax[t] = fmaxf(fmaxf(fmaxf(fmaxf(x0, cur[t][4 * u]), cur[t][4 * u + 1]), cur[t][4 * u + 2]), cur[t][4 * u + 3]);
          }
        } else if (u == 4) {
          m_new[t] = FIXREF ? m_fix : fmaxf(m_run[t], tmax[t] * E::kSInv);
          sum[t] = 0.f;
        } else if (u < 21) {
          if (FIXREF && E::kSInv == 1.0f) sum[t] += __builtin_amdgcn_exp2f(cur[t][u - 5]);
          else sum[t] += __builtin_amdgcn_exp2f(fmaf(cur[t][u - 5], E::kSInv, -m_new[t]));
        } else if (FIXREF) {
          l_run[t] += sum[t];
        } else {
          l_run[t] = l_run[t] * __builtin_amdgcn_exp2f(m_run[t] - m_new[t]) + sum[t];
          m_run[t] = m_new[t];
        }
      };
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
#pragma unroll
          for (int t = 0; t < S::NT; ++t) {
            const int slot = (c * NTERM + term) * S::NT + t;
            f32x16 cin = nxt[t];
            if (c == 0 && term == 0) {
#pragma unroll
              for (int r = 0; r < 16; ++r) cin[r] = 0.f;
            }
            nxt[t] = E::mfma(ap[c & 1][E::ta(term)], bq[t][E::tb(term)][c], cin);
#pragma unroll
            for (int u = slot * NU / NS; u < (slot + 1) * NU / NS; ++u) micro(u);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      // pin the running statistics here: without it the compiler sinks this step's softmax work past
      // the barrier into the next step, in front of its MFMAs
#pragma unroll
      for (int t = 0; t < S::NT; ++t) asm volatile("" : "+v"(m_run[t]), "+v"(l_run[t]));
      __syncthreads();
    };
    int64_t tt = tile0;
    for (; tt + 2 <= last; tt += 2) {
      step(acc_a, acc_b, tt, 1, gb, ga);
      step(acc_b, acc_a, tt + 1, 0, ga, gb);
    }
    if (tt < last) {
      step(acc_a, acc_b, tt, 1, gb, ga);
      epilogue_any(acc_b, last);
    } else {
      epilogue_any(acc_a, last);
    }
  }

#pragma unroll
  for (int t = 0; t < S::NT; ++t) {
    const float m_o = __shfl_xor(m_run[t], 32, 64), l_o = __shfl_xor(l_run[t], 32, 64);
    const float m = fmaxf(m_run[t], m_o);
    const float l = l_run[t] * __builtin_amdgcn_exp2f(m_run[t] - m) + l_o * __builtin_amdgcn_exp2f(m_o - m);
    const int64_t row = i0 + 32 * t + i32;
    if (h == 0 && row < m_rows) part[(int64_t)split * m_rows + row] = make_float2(m, l);
  }
}

__device__ __forceinline__ float group16_sum(float v) {
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}

// out[r] = 1 / max(||x_r||_2, eps)   (F.normalize's denominator, ncl.py:127, gcl.py:29-30)
__global__ __launch_bounds__(256) void row_inv_norm_kernel(const float* __restrict__ x, int64_t n, int d, float eps,
                                                           float* __restrict__ out) {
  const int l16 = threadIdx.x & 15;
  for (int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); r < n; r += (int64_t)gridDim.x * 16) {
    float ss = 0.f;
    if ((d & 3) == 0) {
      for (int c = l16 * 4; c < d; c += 64) {
        const float4 v = *reinterpret_cast<const float4*>(x + r * d + c);
        ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      }
    } else {
      for (int c = l16; c < d; c += 16) ss += x[r * d + c] * x[r * d + c];
    }
    ss = group16_sum(ss);
    if (l16 == 0) out[r] = 1.0f / fmaxf(sqrtf(ss), eps);
  }
}

// out[i] = scale * a_scale[i] * b_scale[p] * <a_i, b_p>,  p = pos[i] (or i): the positive logit
__global__ __launch_bounds__(256) void pos_logit_kernel(const float* __restrict__ a, const float* __restrict__ a_scale,
                                                        const float* __restrict__ b, const float* __restrict__ b_scale,
                                                        const int64_t* __restrict__ pos, int64_t m, int64_t n, int d,
                                                        float scale, float* __restrict__ out) {
  const int l16 = threadIdx.x & 15;
  for (int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); i < m; i += (int64_t)gridDim.x * 16) {
    const int64_t p = pos != nullptr ? pos[i] : i;
    float dot = 0.f;
    const bool ok = p >= 0 && p < n;
    if (ok) {
      if ((d & 3) == 0) {
        for (int c = l16 * 4; c < d; c += 64) {
          const float4 u = *reinterpret_cast<const float4*>(a + i * d + c);
          const float4 v = *reinterpret_cast<const float4*>(b + p * d + c);
          dot += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
        }
      } else {
        for (int c = l16; c < d; c += 16) dot += a[i * d + c] * b[p * d + c];
      }
    }
    dot = group16_sum(dot);
    if (l16 == 0) {
      const float sa = a_scale != nullptr ? a_scale[i] : 1.0f;
      const float sb = (ok && b_scale != nullptr) ? b_scale[p] : 1.0f;
      out[i] = ok ? scale * sa * sb * dot : __builtin_nanf("");
    }
  }
}

// positive-logit term: gx[i] += c_i * inv_tau * yhat[p_i] (row-exclusive), gy[p_i] += c_i * inv_tau * xhat[i] (atomic)
__global__ __launch_bounds__(256) void pos_bwd_kernel(const float* __restrict__ x, const float* __restrict__ x_scale,
                                                      const float* __restrict__ y, const float* __restrict__ y_scale,
                                                      const int64_t* __restrict__ pos, const float* __restrict__ coef,
                                                      int64_t mx, int64_t ny, int d, float inv_tau, float* gx,
                                                      float* gy) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < mx; i += (int64_t)gridDim.x * 4) {
    const int64_t p = pos != nullptr ? pos[i] : i;
    if (p < 0 || p >= ny) continue;
    const float c = coef[i] * inv_tau;
    const float sx = x_scale != nullptr ? x_scale[i] : 1.0f;
    const float sy = y_scale != nullptr ? y_scale[p] : 1.0f;
    for (int col = lane; col < d; col += 64) {
      if (gx != nullptr) gx[i * d + col] += c * sy * y[p * d + col];
      if (gy != nullptr) atomicAdd(gy + p * d + col, c * sx * x[i * d + col]);
    }
  }
}

// through F.normalize: out = inv * (ghat - xhat <xhat, ghat>), xhat = x * inv  (out may alias ghat)
__global__ __launch_bounds__(256) void normalize_bwd_kernel(const float* __restrict__ x, const float* __restrict__ inv,
                                                            const float* ghat, int64_t n, int d, float* out) {
  const int l16 = threadIdx.x & 15;
  for (int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); r < n; r += (int64_t)gridDim.x * 16) {
    const float s = inv[r];
    float dot = 0.f;
    for (int c = l16; c < d; c += 16) dot += x[r * d + c] * s * ghat[r * d + c];
    dot = group16_sum(dot);
    for (int c = l16; c < d; c += 16) out[r * d + c] = s * (ghat[r * d + c] - x[r * d + c] * s * dot);
  }
}

template <int D>
int32_t launch_fwd(const float* a, const float* a_scale, int64_t m, const float* b, const float* b_scale, int64_t n,
                   float inv_tau, float* lse, float* col_sum, float col_bound, void* workspace, bool exd, bool force_f32,
                   bool unit_rows, hipStream_t s) {
  if (col_sum != nullptr) {
    hipError_t err = hipMemsetAsync(col_sum, 0, sizeof(float) * (size_t)n, s);
    if (err != hipSuccess) return gcr_hip_status(err);
  }
  const auto pl = plan_lse_fwd(m, n, D);
  const bool h2 = use_h2(D, inv_tau, unit_rows, force_f32);
  // 512 anchors per workgroup, one workgroup per CU: each staged table tile feeds twice the MFMAs
  const PairsPath& q8 = pl.path[kLseSplit8];
  const bool eight = h2 && q8.open && !exd && col_sum == nullptr && m >= 2 * ShapeB3<D>::ANCHORS_PER_BLOCK &&
                     h2_eight_waves(D, q8.p);
  const PairsPath& q = pl.path[eight ? kLseSplit8 : (use_b3(D, force_f32) ? kLseSplit : kLseF32)];
  const FwdPlan& p = q.p;
  float2* part = ws_at<float2>(workspace, q.part);
  const dim3 grid((unsigned)(p.m_blocks * p.nsplit));
  const float scale2 = inv_tau * kLog2e, cb2 = col_sum != nullptr ? col_bound * kLog2e : 0.f;
  auto split_fwd = [&](auto eng) {                        // the 256-thread split-operand kernel on engine E
    using E = decltype(eng);
    dispatch_lse_mode(exd, col_sum != nullptr, [&](auto colsum, auto ex) {
      hipLaunchKernelGGL((infonce_fwd_e_kernel<E, D, decltype(colsum)::value, decltype(ex)::value>), grid, dim3(256), 0, s, a,
                         a_scale, m, b, b_scale, n, scale2, p.nsplit, p.tiles_per_split, part, col_sum, cb2);
    });
  };
  if (!use_b3(D, force_f32)) {
    dispatch_lse_mode(exd, col_sum != nullptr, [&](auto colsum, auto ex) {
      hipLaunchKernelGGL((infonce_fwd_kernel<D, decltype(colsum)::value, decltype(ex)::value>), grid, dim3(256), 0, s, a,
                         a_scale, m, b, b_scale, n, scale2, p.nsplit, p.tiles_per_split, part, col_sum, cb2);
    });
  } else if constexpr (D <= 128) {
    if (!h2) split_fwd(EngB3{});
    else if constexpr (D <= 64) {
      if (!eight) split_fwd(EngH2{});
      else if constexpr (D == 64)
        hipLaunchKernelGGL((infonce_fwd_e_kernel<EngH2, D, false, false, 8>), grid, dim3(512), 0, s, a, a_scale, m, b, b_scale,
                           n, scale2, p.nsplit, p.tiles_per_split, part, col_sum, cb2);
    }
  }
  int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  hipLaunchKernelGGL(infonce_merge_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, part, p.nsplit, m, lse);
  return GCR_LAUNCH_STATUS();
}

}  // namespace

void gcr_infonce_bwd_f32_launch(int d, bool exd, dim3 grid, hipStream_t s, const float* x, const float* x_scale, int64_t mx,
                                const float* y, const float* y_scale, int64_t ny, float scale2, float out_scale,
                                const float* lse_x, const float* w_x, const float* lse_y, const float* w_y, int ct0, int nsplit,
                                int64_t tiles_per_split, float* gpart) {
  dispatch_dim(d, [&](auto dc) {
    dispatch_bool(exd, [&](auto ex) {
      hipLaunchKernelGGL((infonce_bwd_kernel<decltype(dc)::value, decltype(ex)::value>), grid, dim3(256), 0, s, x, x_scale, mx,
                         y, y_scale, ny, scale2, out_scale, lse_x, w_x, lse_y, w_y, ct0, nsplit, tiles_per_split, gpart);
    });
  });
}

extern "C" int32_t gcr_infonce_engine(int32_t d) { return dim_supported(d) && use_b3(d) ? 1 : 0; }

extern "C" int64_t gcr_infonce_fwd_workspace_bytes(int64_t m, int64_t n, int32_t d) {
  if (m <= 0 || n <= 0 || !dim_supported(d)) return 0;
  return plan_lse_fwd(m, n, d).bytes();
}

extern "C" int32_t gcr_infonce_fwd_ex_f32(const float* a, const float* a_scale, int64_t m, const float* b,
                                          const float* b_scale, int64_t n, int32_t d, float inv_tau, float* lse,
                                          float* col_sum, float col_bound, void* workspace, uint32_t flags,
                                          void* stream) {
  GCR_CHECK_ARG(m >= 0 && n >= 1);
  GCR_CHECK_ARG((flags & ~(uint32_t)(GCR_INFONCE_EXCLUDE_DIAGONAL | GCR_INFONCE_ENGINE_F32 | GCR_INFONCE_UNIT_ROWS)) == 0);
  const bool exd = (flags & GCR_INFONCE_EXCLUDE_DIAGONAL) != 0;
  const bool force_f32 = (flags & GCR_INFONCE_ENGINE_F32) != 0;
  const bool unit = (flags & GCR_INFONCE_UNIT_ROWS) != 0;
  GCR_CHECK_ARG(!(exd && col_sum != nullptr));
  if (!dim_supported(d)) return GCR_EUNSUPPORTED;
  if (m == 0) return GCR_OK;
  GCR_CHECK_ARG(a != nullptr && b != nullptr && lse != nullptr && workspace != nullptr);
  GCR_CHECK_ARG(m < (1ll << 40) && n < (1ll << 40));
  return dispatch_dim(d, [&](auto dc) {
    return launch_fwd<decltype(dc)::value>(a, a_scale, m, b, b_scale, n, inv_tau, lse, col_sum, col_bound, workspace, exd,
                                           force_f32, unit, (hipStream_t)stream);
  });
}

extern "C" int32_t gcr_infonce_fwd_f32(const float* a, const float* a_scale, int64_t m, const float* b,
                                       const float* b_scale, int64_t n, int32_t d, float inv_tau, float* lse,
                                       float* col_sum, float col_bound, void* workspace, void* stream) {
  return gcr_infonce_fwd_ex_f32(a, a_scale, m, b, b_scale, n, d, inv_tau, lse, col_sum, col_bound, workspace, 0u, stream);
}

extern "C" int32_t gcr_row_inv_norm_f32(const float* x, int64_t n, int32_t d, float eps, float* out, void* stream) {
  GCR_CHECK_ARG(n >= 0 && d >= 1);
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(x != nullptr && out != nullptr);
  const int64_t want = (n + 15) / 16;
  hipLaunchKernelGGL(row_inv_norm_kernel, dim3((unsigned)(want > 8192 ? 8192 : want)), dim3(256), 0,
                     (hipStream_t)stream, x, n, d, eps, out);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_pos_logit_f32(const float* a, const float* a_scale, const float* b, const float* b_scale,
                                     const int64_t* pos, int64_t m, int64_t n, int32_t d, float scale, float* out,
                                     void* stream) {
  GCR_CHECK_ARG(m >= 0 && n >= 0 && d >= 1);
  if (m == 0) return GCR_OK;
  GCR_CHECK_ARG(a != nullptr && b != nullptr && out != nullptr);
  const int64_t want = (m + 15) / 16;
  hipLaunchKernelGGL(pos_logit_kernel, dim3((unsigned)(want > 8192 ? 8192 : want)), dim3(256), 0, (hipStream_t)stream,
                     a, a_scale, b, b_scale, pos, m, n, d, scale, out);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_infonce_pos_bwd_f32(const float* x, const float* x_scale, const float* y, const float* y_scale,
                                           const int64_t* pos, const float* coef, int64_t mx, int64_t ny, int32_t d,
                                           float inv_tau, float* gx, float* gy, void* stream) {
  GCR_CHECK_ARG(mx >= 0 && ny >= 0 && d >= 1);
  if (mx == 0) return GCR_OK;
  GCR_CHECK_ARG(x != nullptr && y != nullptr && coef != nullptr && (gx != nullptr || gy != nullptr));
  const int64_t want = (mx + 3) / 4;
  hipLaunchKernelGGL(pos_bwd_kernel, dim3((unsigned)(want > 8192 ? 8192 : want)), dim3(256), 0, (hipStream_t)stream, x,
                     x_scale, y, y_scale, pos, coef, mx, ny, d, inv_tau, gx, gy);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_normalize_bwd_f32(const float* x, const float* inv_norm, const float* ghat, int64_t n,
                                         int32_t d, float* out, void* stream) {
  GCR_CHECK_ARG(n >= 0 && d >= 1);
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(x != nullptr && inv_norm != nullptr && ghat != nullptr && out != nullptr);
  const int64_t want = (n + 15) / 16;
  hipLaunchKernelGGL(normalize_bwd_kernel, dim3((unsigned)(want > 8192 ? 8192 : want)), dim3(256), 0,
                     (hipStream_t)stream, x, inv_norm, ghat, n, d, out);
  return GCR_LAUNCH_STATUS();
}
