// SEPT's tri-training block — pseudo-label selection + neighbour discrimination for three views (gfx950).
//
// Replaces, per batch, univariate/sept_social.py:394-420,447-457: label_prediction x3 (unique, two gathers, two
// F.normalize, an M x M matmul, a softmax), generate_pesudo_labels x3 (add, topk) and neighbor_discrimination x3 (the
// gathers and normalisations again, a second M x M matmul, exp, sums) over the M distinct users `uniq` of the batch.
// With e_v[i] = X_v[uniq[i]] / max(|.|, 1e-12), a[j] = A[uniq[j]] / max(|.|, 1e-12), S_v[i, j] = <e_v[i], a[j]>:
//
//   prepare   one wave per (table, i): the normalised rows x^ [4, M, d] and 1 / max(|x|, 1e-12).
//   sweep     grid (32-row tiles, column splits), three waves per workgroup, wave v = view v.  A wave keeps its 32 rows
//             of e_v in registers, loads one 32-row tile of a per step, and forms S_v^T on the f32 MFMA
//             (v_mfma_f32_32x32x2_f32): lane (l32, h) then holds row i = l32 at the 16 columns acc_row(r, h).
//             sweep 0: row sums of exp(S_v).  sweep 1: P_v = exp(S_v) / Z_v goes through the LDS so that wave v reads the
//             two OTHER views' tiles, c_v = P_a + P_b, and keeps a sorted k-candidate list per lane in the LDS (a later
//             candidate of a lane always has the larger column, so `>` alone gives ties to the smaller column); the same
//             sweep sums exp((S_v - 1) / t), in double: the backward subtracts the reciprocals of this sum and of the sum
//             over the positives, two numbers that agree to 1 / (M - k) when nearly every column is a positive.
//             |S| <= 1: no running maximum anywhere.
//   finish    one wave per (view, row): merges the 2 x splits candidate lists by rank (value descending, then column
//             ascending: gcr_topk_masked_f32's rule), writes `positive`, sets the row's membership bits, recomputes the k
//             positive scores on the MFMA in the sweep's operand order (bitwise the sweep's S), sums their exponentials in
//             double like the sweep, and writes 1 / sum_j e and 1 / sum_j e - 1 / sum_{pos} e, the cancelling difference of
//             the two sums formed in double.
//   reduce    the three losses from the per-row terms, summed in double in a fixed order.
//
// Backward: prepare again, then two sweeps that recompute the score tiles, form
//   w_v[i, j] = (g_v / t) exp((S - 1) / t) (1 / sum_j e - [j in pos_v[i]] / sum_{pos} e)      (the forward's two numbers)
// (membership read from the forward's bitmap: no scatter) and feed w straight back into the MFMA as the B operand of
// w^T a (rows) or w e_v (columns) — the accumulator layout of the first product IS the B layout of the second, as in
// gcr_directau.hip.  Per-split partials are added in split (and view) order by the last kernel, which applies the
// normalisation backward and writes row uniq[i] of each gradient table: one writer per row, no float atomics, bitwise
// reproducible.
#include "gcr_host.h"
#include "gcr_lanes.h"
#include "gcr_tile.h"   // f32x16, acc_row, kTileJ = 32 rows of a tile

namespace {

constexpr int kViews = 3;
constexpr int kMaxSplits = 8;
constexpr int kMaxK = 32;
constexpr float kNormEps = 1e-12f;   // F.normalize's eps
constexpr int kNoCol = 0x7fffffff;
constexpr float kMaxInvT = 40.f;    // e = exp((S - 1) / t) >= exp(-2 / t) stays a normal f32

struct TriTabs {
  const float* tab[4];     // friend, sharing, rec, augmented
};
struct TriGrads {
  float* tab[4];
};

// xhat [4, m, D], inv_norm [4, m]; an id outside [0, n_rows) is a zero row
template <int D>
__global__ __launch_bounds__(256) void tri_prepare_kernel(TriTabs T, const int64_t* __restrict__ uniq, int64_t m,
                                                          int64_t n_rows, float* __restrict__ xhat,
                                                          float* __restrict__ inv_norm) {
  constexpr int NV = (D + 63) / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < 4 * m; w += (int64_t)gridDim.x * 4) {
    const int s = (int)(w / m);
    const int64_t i = w - (int64_t)s * m;
    const int64_t row = uniq[i];
    const bool ok = row >= 0 && row < n_rows;
    float x[NV], ss = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = lane + 64 * v;
      x[v] = (ok && c < D) ? T.tab[s][row * D + c] : 0.f;
      ss += x[v] * x[v];
    }
    ss = gcr_wave_sum(ss);
    const float inv = 1.0f / fmaxf(sqrtf(ss), kNormEps);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = lane + 64 * v;
      if (c < D) xhat[((int64_t)s * m + i) * D + c] = x[v] * inv;
    }
    if (lane == 0) inv_norm[(int64_t)s * m + i] = inv;
  }
}

// this lane's half of the k index of row `row`: columns [h D/2, (h + 1) D/2)
template <int D>
__device__ __forceinline__ void load_half_row(const float* __restrict__ tab, int64_t row, bool ok, int h, float* out) {
  const float4* p = reinterpret_cast<const float4*>(tab + row * D + h * (D / 2));
#pragma unroll
  for (int q = 0; q < D / 8; ++q) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) v = p[q];
    out[4 * q] = v.x; out[4 * q + 1] = v.y; out[4 * q + 2] = v.z; out[4 * q + 3] = v.w;
  }
}

// MODE 0: part_z[split, v, i] = sum_j exp(S_v[i, j]) over the split's columns (float: a softmax denominator)
// MODE 1: the same sums of exp((S_v - 1) inv_t), float terms added in double (double)    (replay: no selection)
// MODE 2: MODE 1 + the candidate lists, from z1 = the MODE 0 partials
template <int MODE>
struct TriSum {                      // the type of a MODE's partial sums
  typedef double type;
};
template <>
struct TriSum<0> {
  typedef float type;
};

template <int D, int MODE>
__global__ __launch_bounds__(192) void tri_sweep_kernel(const float* __restrict__ xhat, int64_t m, int n_tiles, int n_splits,
                                                        int k, float inv_t, const float* __restrict__ z1,
                                                        typename TriSum<MODE>::type* __restrict__ part_z,
                                                        float* __restrict__ cand_val, int* __restrict__ cand_col) {
  typedef typename TriSum<MODE>::type sum_t;
  extern __shared__ float tri_lds[];
  float* ptile = tri_lds;                                        // [3][16][64]
  float* lval = tri_lds + kViews * 16 * 64;                      // [3][k][64]
  int* lcol = reinterpret_cast<int*>(lval + kViews * k * 64);    // [3][k][64]
  const int tid = threadIdx.x, lane = tid & 63, v = tid >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int split = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kTileJ + l32;
  const bool row_ok = i < m;
  const float* E = xhat + (int64_t)v * m * D;
  const float* A = xhat + (int64_t)3 * m * D;
  float xr[D / 2];
  load_half_row<D>(E, i, row_ok, h, xr);
  float inv_z = 0.f;
  float* my_val = lval + (v * k) * 64 + lane;
  int* my_col = lcol + (v * k) * 64 + lane;
  float thr = -INFINITY;
  if (MODE == 2) {
    float z = 0.f;
    if (row_ok)
      for (int s = 0; s < n_splits; ++s) z += z1[((int64_t)s * kViews + v) * m + i];      // split order
    inv_z = row_ok ? 1.0f / z : 0.f;
    for (int q = 0; q < k; ++q) {
      my_val[q * 64] = -INFINITY;
      my_col[q * 64] = kNoCol;
    }
  }
  sum_t run = 0;
  for (int jt = split; jt < n_tiles; jt += n_splits) {
    const int64_t b0 = (int64_t)jt * kTileJ;
    float xc[D / 2];
    load_half_row<D>(A, b0 + l32, b0 + l32 < m, h, xc);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < D / 2; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[q], xr[q], acc, 0, 0, 0);
    // acc[r] = S_v[i][b0 + acc_row(r, h)]
    sum_t part = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool live = row_ok && b0 + acc_row(r, h) < m;
      if (MODE == 0) {
        part += live ? expf(acc[r]) : 0.f;
      } else {
        part += (sum_t)(live ? expf((acc[r] - 1.0f) * inv_t) : 0.f);
        if (MODE == 2) ptile[(v * 16 + r) * 64 + lane] = live ? expf(acc[r]) * inv_z : 0.f;
      }
    }
    run += part;
    if (MODE == 2) {
      __syncthreads();
      const int va = (v + 1) % kViews, vb = (v + 2) % kViews;
      float c[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pa = ptile[(va * 16 + r) * 64 + lane], pb = ptile[(vb * 16 + r) * 64 + lane];
        c[r] = v == 1 ? pb + pa : pa + pb;                       // P_s + P_r | P_f + P_r | P_f + P_s
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t j = b0 + acc_row(r, h);
        if (row_ok && j < m && c[r] > thr) {
          int p = k - 1;
          while (p > 0 && my_val[(p - 1) * 64] < c[r]) {
            my_val[p * 64] = my_val[(p - 1) * 64];
            my_col[p * 64] = my_col[(p - 1) * 64];
            --p;
          }
          my_val[p * 64] = c[r];
          my_col[p * 64] = (int)j;
          thr = my_val[(k - 1) * 64];
        }
      }
    }
  }
  run += __shfl_xor(run, 32, GCR_WAVE);
  if (h == 0 && row_ok) part_z[((int64_t)split * kViews + v) * m + i] = run;
  if (MODE == 2 && row_ok) {
    const int64_t base = (((int64_t)v * m + i) * (2 * n_splits) + split * 2 + h) * k;
    for (int q = 0; q < k; ++q) {
      cand_val[base + q] = my_val[q * 64];
      cand_col[base + q] = my_col[q * 64];
    }
  }
}

// one wave per (view, row).  rsum [2, 3, m] = (1 / sum_j e, 1 / sum_j e - 1 / sum_{pos} e) with e = exp((S - 1) / t);
// row_loss [3, m].  The reciprocals keep f32's RELATIVE precision; a log-sum of size ~1/t stored in f32 carries an absolute
// error of ulp(1/t) ~ 1e-6 into every softmax the backward rebuilds from it.  The second number is what a positive's weight
// multiplies: with M - k columns outside the label set the two reciprocals agree to 1 / (M - k), and one ulp of either
// (of a float sum, of a reciprocal rounded to float) is M - k ulps of their difference.  Both sums add the same float terms
// in double and the difference is (sum_{pos} e - sum_j e) / sum_j e / sum_{pos} e, the numerator formed in double.
template <int D>
__global__ __launch_bounds__(256) void tri_finish_kernel(const float* __restrict__ xhat, int64_t m, int n_tiles, int n_splits,
                                                         int k, float inv_t, int replay, const double* __restrict__ part_zt,
                                                         const float* __restrict__ cand_val, const int* __restrict__ cand_col,
                                                         int64_t* __restrict__ positive, float* __restrict__ rsum,
                                                         float* __restrict__ row_loss, uint32_t* __restrict__ member) {
  __shared__ float cv[4][2 * kMaxSplits * kMaxK];
  __shared__ int cc[4][2 * kMaxSplits * kMaxK];
  __shared__ int sel[4][kMaxK];
  __shared__ float sc[4][kTileJ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* A = xhat + (int64_t)3 * m * D;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < kViews * m; w += (int64_t)gridDim.x * 4) {
    const int v = (int)(w / m);
    const int64_t i = w - (int64_t)v * m;
    if (lane < k) sel[wave][lane] = -1;
    if (!replay) {
      const int n_cand = 2 * n_splits * k;
      const int64_t base = ((int64_t)v * m + i) * n_cand;
      for (int c = lane; c < n_cand; c += 64) {
        cv[wave][c] = cand_val[base + c];
        cc[wave][c] = cand_col[base + c];
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      for (int c = lane; c < n_cand; c += 64) {
        const float val = cv[wave][c];
        const int col = cc[wave][c];
        if (col == kNoCol) continue;
        int rank = 0;
        for (int o = 0; o < n_cand; ++o) {
          const float ov = cv[wave][o];
          const int oc = cc[wave][o];
          rank += (ov > val || (ov == val && oc < col)) ? 1 : 0;
        }
        if (rank < k) {
          sel[wave][rank] = col;
          positive[((int64_t)v * m + i) * k + rank] = col;
        }
      }
    } else if (lane < k) {
      const int64_t j = positive[((int64_t)v * m + i) * k + lane];
      sel[wave][lane] = (j >= 0 && j < m) ? (int)j : -1;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < k && sel[wave][lane] >= 0) {
      const int j = sel[wave][lane];
      atomicOr(member + ((int64_t)v * m + i) * n_tiles + (j >> 5), 1u << (j & 31));
    }
    // the k positive scores on the MFMA with the sweep's operand order: bitwise the S the sweeps saw, so a row whose
    // positives are all its columns sums the very same terms twice
    const int l32 = lane & 31, h = lane >> 5;
    const int jsel = l32 < k ? sel[wave][l32] : -1;
    float xa[D / 2], xb[D / 2];
    load_half_row<D>(A, jsel, jsel >= 0, h, xa);
    load_half_row<D>(xhat + (int64_t)v * m * D, i, true, h, xb);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < D / 2; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[q], xb[q], acc, 0, 0, 0);
    if (l32 == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[wave][acc_row(r, h)] = acc[r];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double ps = 0.0;
    for (int q = 0; q < k; ++q)
      if (sel[wave][q] >= 0) ps += (double)expf((sc[wave][q] - 1.0f) * inv_t);
    double zt = 0.0;
    for (int s = 0; s < n_splits; ++s) zt += part_zt[((int64_t)s * kViews + v) * m + i];
    if (lane == 0) {
      const float zf = (float)zt, pf = (float)ps;
      rsum[(int64_t)v * m + i] = 1.0f / zf;
      // 1 / zt - 1 / ps, the cancellation in double.  Two quotients, not one by zf * pf: e >= exp(-2 kMaxInvT) = 1.8e-35 keeps
      // either sum a normal float, their product it does not; the first quotient lies in [-1, 0], the second within 1 / pf
      rsum[((int64_t)kViews + v) * m + i] = (float)(ps - zt) / zf / pf;
      row_loss[(int64_t)v * m + i] = -logf(pf / zf);                 // :419 forms the ratio first, too
    }
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ __launch_bounds__(192) void tri_reduce_kernel(const float* __restrict__ row_loss, int64_t m, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, v = threadIdx.x >> 6;
  double s = 0.0;
  for (int64_t i = lane; i < m; i += 64) s += (double)row_loss[(int64_t)v * m + i];
  s = gcr_wave_sum_f64(s);
  if (lane == 0) loss[v] = (float)s;
}

// COLSIDE false: fixed = 32 rows i of e_v, swept = tiles of a;  part[split, v, i, :]  = sum_j w_v[i, j] a[j]
// COLSIDE true:  fixed = 32 columns j of a, swept = tiles of e_v; part[split, v, j, :] = sum_i w_v[i, j] e_v[i]
template <int D, bool COLSIDE>
__global__ __launch_bounds__(192) void tri_bwd_sweep_kernel(const float* __restrict__ xhat, int64_t m, int n_tiles, int n_splits,
                                                            float inv_t, const float* __restrict__ rsum,
                                                            const uint32_t* __restrict__ member, const float* __restrict__ g,
                                                            float* __restrict__ part) {
  constexpr int kStride = D + 1;
  __shared__ float swt[kViews][kTileJ * kStride];
  const int tid = threadIdx.x, lane = tid & 63, v = tid >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int split = blockIdx.y;
  const int64_t f = (int64_t)blockIdx.x * kTileJ + l32;
  const bool f_ok = f < m;
  const float* F = xhat + (int64_t)(COLSIDE ? 3 : v) * m * D;
  const float* S = xhat + (int64_t)(COLSIDE ? v : 3) * m * D;
  const float* iz_v = rsum + (int64_t)v * m;
  const float* id_v = rsum + ((int64_t)kViews + v) * m;          // 1 / sum_j e - 1 / sum_{pos} e
  const uint32_t* mem_v = member + (int64_t)v * m * n_tiles;
  float xr[D / 2];
  load_half_row<D>(F, f, f_ok, h, xr);
  const float gt = g[v] * inv_t;
  const float iz_f = (!COLSIDE && f_ok) ? iz_v[f] : 0.f;
  const float id_f = (!COLSIDE && f_ok) ? id_v[f] : 0.f;
  f32x16 oacc[D / 32];
#pragma unroll
  for (int ch = 0; ch < D / 32; ++ch)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[ch][r] = 0.f;
  float* mine = swt[v];
  for (int st = split; st < n_tiles; st += n_splits) {
    const int64_t s0 = (int64_t)st * kTileJ;
    __syncthreads();
    for (int idx = lane; idx < kTileJ * D; idx += 64) {
      const int row = idx / D, c = idx - row * D;
      mine[row * kStride + c] = s0 + row < m ? S[(s0 + row) * D + c] : 0.f;
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* ap = mine + l32 * kStride + h * (D / 2);
#pragma unroll
    for (int q = 0; q < D / 2; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[q], xr[q], acc, 0, 0, 0);
    // acc[r] = <swept row s0 + acc_row(r, h), fixed row f>
    const uint32_t word_f = (!COLSIDE && f_ok) ? mem_v[f * n_tiles + st] : 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ar = acc_row(r, h);
      const int64_t sw = s0 + ar;
      const bool live = f_ok && sw < m;
      float iz = iz_f, id = id_f;
      bool bit = (word_f >> ar) & 1u;
      if (COLSIDE) {
        iz = live ? iz_v[sw] : 0.f;
        id = live ? id_v[sw] : 0.f;
        bit = live ? ((mem_v[sw * n_tiles + blockIdx.x] >> l32) & 1u) : false;
      }
      const float w = gt * expf((acc[r] - 1.0f) * inv_t) * (bit ? id : iz);
      acc[r] = live ? w : 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < D / 32; ++ch) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float xv = mine[acc_row(r, h) * kStride + ch * 32 + l32];
        oacc[ch] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, acc[r], oacc[ch], 0, 0, 0);
      }
    }
  }
  if (f_ok) {
    float* out = part + (((int64_t)split * kViews + v) * m + f) * D;
#pragma unroll
    for (int ch = 0; ch < D / 32; ++ch)
#pragma unroll
      for (int r = 0; r < 16; ++r) out[ch * 32 + acc_row(r, h)] = oacc[ch][r];
  }
}

// one wave per (table, i): the partials in split (and, for the augmented table, view) order, then the normalize backward
template <int D>
__global__ __launch_bounds__(256) void tri_bwd_rows_kernel(const float* __restrict__ xhat, const float* __restrict__ inv_norm,
                                                           const int64_t* __restrict__ uniq, int64_t m, int64_t n_rows,
                                                           int n_splits, const float* __restrict__ part_e,
                                                           const float* __restrict__ part_a, TriGrads G) {
  constexpr int NV = (D + 63) / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < 4 * m; w += (int64_t)gridDim.x * 4) {
    const int s = (int)(w / m);
    const int64_t i = w - (int64_t)s * m;
    const int64_t row = uniq[i];
    if (row < 0 || row >= n_rows) continue;                      // wave-uniform
    float gh[NV], xh[NV], dot = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int c = lane + 64 * q;
      float a = 0.f;
      if (c < D) {
        if (s < 3) {
          for (int sp = 0; sp < n_splits; ++sp) a += part_e[(((int64_t)sp * kViews + s) * m + i) * D + c];
        } else {
          for (int sp = 0; sp < n_splits; ++sp)
            for (int v = 0; v < kViews; ++v) a += part_a[(((int64_t)sp * kViews + v) * m + i) * D + c];
        }
      }
      gh[q] = a;
      xh[q] = c < D ? xhat[((int64_t)s * m + i) * D + c] : 0.f;
      dot += xh[q] * a;
    }
    dot = gcr_wave_sum(dot);
    const float inv = inv_norm[(int64_t)s * m + i];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int c = lane + 64 * q;
      if (c < D) G.tab[s][row * D + c] = inv * (gh[q] - xh[q] * dot);
    }
  }
}

int splits_for(int64_t n_tiles) {
  int64_t want = (256 + n_tiles - 1) / n_tiles;
  if (want > kMaxSplits) want = kMaxSplits;
  if (want > n_tiles) want = n_tiles;
  return (int)(want < 1 ? 1 : want);
}

struct TriWorkspace {
  int64_t xhat, inv_norm, z1, zt, row_loss, cand_val, cand_col, part_e, part_a, total;      // offsets in 4-byte words
};

TriWorkspace tri_layout(int64_t m, int d, int k) {
  TriWorkspace w;
  WsCarve c;
  const int64_t n_tiles = (m + kTileJ - 1) / kTileJ;
  const int ns = splits_for(n_tiles < 1 ? 1 : n_tiles);
  w.xhat = c.take(4 * m * d);
  w.inv_norm = c.take(4 * m);
  w.z1 = c.take((int64_t)ns * kViews * m);
  w.zt = c.take(2 * (int64_t)ns * kViews * m);                                               // doubles
  w.row_loss = c.take(kViews * m);
  w.cand_val = c.take((int64_t)kViews * m * 2 * ns * k);
  w.cand_col = c.take((int64_t)kViews * m * 2 * ns * k);
  w.part_e = c.take((int64_t)ns * kViews * m * d);
  w.part_a = c.take((int64_t)ns * kViews * m * d);
  w.total = c.at;
  return w;
}

TriTabs tri_tabs(const float* x_f, const float* x_s, const float* x_r, const float* aug) {
  TriTabs T;
  T.tab[0] = x_f; T.tab[1] = x_s; T.tab[2] = x_r; T.tab[3] = aug;
  return T;
}

bool tri_args_ok(int64_t n_rows, int64_t m, int32_t k) {
  return n_rows >= 0 && n_rows < (1ll << 31) && m >= 0 && m < (1ll << 22) && k >= 1 && k <= kMaxK;
}

unsigned row_blocks(int64_t waves) { return (unsigned)gcr_grid((waves + 3) / 4, 8192); }

}  // namespace

extern "C" int32_t gcr_tri_supported(int32_t d, int32_t k) {
  return (d == 32 || d == 64 || d == 128) && k >= 1 && k <= kMaxK;
}

extern "C" int64_t gcr_tri_workspace_bytes(int64_t m, int32_t d, int32_t k) {
  if (m < 1 || !gcr_tri_supported(d, k)) return 0;
  return tri_layout(m, d, k).total * (int64_t)sizeof(float);
}

extern "C" int64_t gcr_tri_member_words(int64_t m) {
  return m < 1 ? 0 : kViews * m * ((m + kTileJ - 1) / kTileJ);
}

extern "C" int32_t gcr_tri_fwd_f32(const float* x_f, const float* x_s, const float* x_r, const float* aug, int64_t n_rows,
                                   int32_t d, const int64_t* uniq, int64_t m, int32_t k, float inv_t, int32_t replay,
                                   float* loss, int64_t* positive, float* rsum, float* inv_norm, uint32_t* member,
                                   void* workspace, void* stream) {
  if (!gcr_tri_supported(d, k)) return GCR_EUNSUPPORTED;
  GCR_CHECK_ARG(tri_args_ok(n_rows, m, k) && inv_t > 0.f && inv_t <= kMaxInvT && loss);
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) return GCR_OK;
  GCR_CHECK_ARG(m >= k);
  GCR_CHECK_ARG(x_f && x_s && x_r && aug && uniq && positive && rsum && inv_norm && member && workspace);
  const TriWorkspace w = tri_layout(m, d, k);
  float* ws = reinterpret_cast<float*>(workspace);
  const int n_tiles = (int)((m + kTileJ - 1) / kTileJ);
  const int ns = splits_for(n_tiles);
  const TriTabs T = tri_tabs(x_f, x_s, x_r, aug);
  int32_t st = gcr_hip_status(hipMemsetAsync(member, 0, (size_t)gcr_tri_member_words(m) * sizeof(uint32_t), s));
  if (st != GCR_OK) return st;
  const dim3 grid((unsigned)n_tiles, (unsigned)ns);
  const size_t lds_sel = (size_t)(kViews * 16 * 64 + 2 * kViews * k * 64) * sizeof(float);
  int* cand_col = reinterpret_cast<int*>(ws + w.cand_col);
  double* zt = reinterpret_cast<double*>(ws + w.zt);             // every offset is a multiple of 64 words
  dispatch_value<32, 64, 128>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    hipLaunchKernelGGL((tri_prepare_kernel<D>), dim3(row_blocks(4 * m)), dim3(256), 0, s, T, uniq, m, n_rows, ws + w.xhat,
                       inv_norm);
    if (replay) {
      hipLaunchKernelGGL((tri_sweep_kernel<D, 1>), grid, dim3(192), 0, s, ws + w.xhat, m, n_tiles, ns, (int)k, inv_t,
                         (const float*)nullptr, zt, (float*)nullptr, (int*)nullptr);
    } else {
      hipLaunchKernelGGL((tri_sweep_kernel<D, 0>), grid, dim3(192), 0, s, ws + w.xhat, m, n_tiles, ns, (int)k, inv_t,
                         (const float*)nullptr, ws + w.z1, (float*)nullptr, (int*)nullptr);
      hipLaunchKernelGGL((tri_sweep_kernel<D, 2>), grid, dim3(192), lds_sel, s, ws + w.xhat, m, n_tiles, ns, (int)k, inv_t,
                         ws + w.z1, zt, ws + w.cand_val, cand_col);
    }
    hipLaunchKernelGGL((tri_finish_kernel<D>), dim3(row_blocks(kViews * m)), dim3(256), 0, s, ws + w.xhat, m, n_tiles, ns,
                       (int)k, inv_t, (int)replay, zt, ws + w.cand_val, cand_col, positive, rsum, ws + w.row_loss, member);
  });
  hipLaunchKernelGGL(tri_reduce_kernel, dim3(1), dim3(192), 0, s, ws + w.row_loss, m, loss);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_tri_bwd_f32(const float* x_f, const float* x_s, const float* x_r, const float* aug, int64_t n_rows,
                                   int32_t d, const int64_t* uniq, int64_t m, int32_t k, float inv_t, const float* rsum,
                                   const uint32_t* member, const float* g, float* d_f, float* d_s, float* d_r, float* d_aug,
                                   void* workspace, void* stream) {
  if (!gcr_tri_supported(d, k)) return GCR_EUNSUPPORTED;
  GCR_CHECK_ARG(tri_args_ok(n_rows, m, k) && inv_t > 0.f && inv_t <= kMaxInvT);
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) return GCR_OK;
  GCR_CHECK_ARG(x_f && x_s && x_r && aug && uniq && rsum && member && g && d_f && d_s && d_r && d_aug && workspace);
  const TriWorkspace w = tri_layout(m, d, k);
  float* ws = reinterpret_cast<float*>(workspace);
  const int n_tiles = (int)((m + kTileJ - 1) / kTileJ);
  const int ns = splits_for(n_tiles);
  const TriTabs T = tri_tabs(x_f, x_s, x_r, aug);
  TriGrads G;
  G.tab[0] = d_f; G.tab[1] = d_s; G.tab[2] = d_r; G.tab[3] = d_aug;
  const dim3 grid((unsigned)n_tiles, (unsigned)ns);
  dispatch_value<32, 64, 128>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    hipLaunchKernelGGL((tri_prepare_kernel<D>), dim3(row_blocks(4 * m)), dim3(256), 0, s, T, uniq, m, n_rows, ws + w.xhat,
                       ws + w.inv_norm);
    hipLaunchKernelGGL((tri_bwd_sweep_kernel<D, false>), grid, dim3(192), 0, s, ws + w.xhat, m, n_tiles, ns, inv_t, rsum,
                       member, g, ws + w.part_e);
    hipLaunchKernelGGL((tri_bwd_sweep_kernel<D, true>), grid, dim3(192), 0, s, ws + w.xhat, m, n_tiles, ns, inv_t, rsum,
                       member, g, ws + w.part_a);
    hipLaunchKernelGGL((tri_bwd_rows_kernel<D>), dim3(row_blocks(4 * m)), dim3(256), 0, s, ws + w.xhat, ws + w.inv_norm,
                       uniq, m, n_rows, ns, ws + w.part_e, ws + w.part_a, G);
  });
  return GCR_LAUNCH_STATUS();
}
