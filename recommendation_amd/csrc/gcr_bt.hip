// Barlow Twins (redundancy reduction) over two full-batch views h1, h2 [n, d]: univariate/gbt.py:203-228, 386-395.
//
//   col_stats   column mean and unbiased std of a row-major [n, d] array.  Every thread runs Welford's update over the
//               SHIFTED values x - k of its rows, k = the first row it sees (a provisional mean: the running mean stays
//               of the size of the spread, not of the offset, so its rounding does too); the (count, mean, M2) partials
//               are merged by Chan's rule in a fixed order, inside the workgroup, then over the workgroups.  One launch
//               over the rows and one small one.  (Plain sums of (x - k) and (x - k)^2 lost 1.1e-6 of the std at 256
//               rows per thread when k lay two deviations off the mean.)
//   product     c = z1^T z2 / n on v_mfma_f32_32x32x2_f32, rows split over the chip as in gcr_dense.hip's tall-skinny
//               x^T g; z = (h - mean) / (std + eps) is applied to the operands as they are loaded and never written.
//               d = 256 runs as four 128 x 128 quadrants (blockIdx.y), each re-reading half of either view.
//   reduce      the workgroups' partials summed in a fixed order, scaled by 1 / n, and the loss terms of the 64 outputs
//               of a workgroup summed; a last one-workgroup launch adds those <= 1024 numbers.
//   prep        from c and the upstream scalar: G = dL/dc, G^T, t1 = rowsum(G c), t2 = colsum(G c) and per column the
//               two coefficients of the backward (include/gcr.h has the formulas).  One workgroup per row of c.
//   bwd         one launch over the rows; blockIdx.y picks the gradient.  A wave keeps 32 rows of G (or G^T) in
//               registers, the OTHER view's row tile is standardised into LDS, one 32 x 32 output tile per wave and
//               tile on the MFMA, the own view's (h - mean) term added in the epilogue.
// No float atomics, no host read-back; every sum has one order: outputs are bitwise reproducible.
#include "gcr_host.h"
#include "gcr_lanes.h"
#include "gcr_tile.h"   // f32x16, acc_row

namespace {

constexpr int kBtLossParts = 1024;                           // d * d / 64 <= 1024 reduce workgroups

int stat_blocks(int64_t n) { return (int)gcr_grid((n + 255) / 256, 1024); }      // >= 256 rows per workgroup

bool bt_dim_ok(int d) { return d == 32 || d == 64 || d == 96 || d == 128 || d == 256; }

// product launch: workgroups along the rows (times four quadrants at d = 256) and rows per workgroup (even: a row pair
// never straddles two workgroups)
int bt_blocks(int64_t n, int d) { return (int)gcr_grid((n + 255) / 256, d == 256 ? 256 : 1024); }
int64_t bt_rows(int64_t n, int nb) {
  const int64_t per = ((n + nb - 1) / nb + 1) & ~(int64_t)1;
  return per < 256 ? 256 : per;                              // below the cap: whole chunks of 256, the last one short
}
int64_t stat_rows(int64_t n, int nb) {
  const int64_t per = (n + nb - 1) / nb;
  return per < 256 ? 256 : per;
}

// Chan's merge of (count, mean, M2) b into a; an empty side leaves the other unchanged
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
  const float tot = na + nb;
  const float w = tot > 0.f ? nb / tot : 0.f;
  const float delta = mb - ma;
  ma += delta * w;
  qa += qb + delta * delta * (na * w);
  na = tot;
}

// Welford's update of (mean m, M2 q) of the SHIFTED values y = v - k by the cnt-th row (inv = 1 / cnt)
__device__ __forceinline__ void welford_add(const float4& v, const float4& k, float inv, float4& m, float4& q) {
  const float a = v.x - k.x, b = v.y - k.y, c = v.z - k.z, e = v.w - k.w;
  const float da = a - m.x, db = b - m.y, dc = c - m.z, de = e - m.w;
  m.x += da * inv; m.y += db * inv; m.z += dc * inv; m.w += de * inv;
  q.x += da * (a - m.x); q.y += db * (b - m.y); q.z += dc * (c - m.z); q.w += de * (e - m.w);
}

// part[view][block][0 / 1][d] = mean / M2 of the block's rows (the count follows from the geometry).  Thread t owns the
// column quad t % (d / 4) of every (256 / (d / 4))-th row; blockIdx.y picks the view.
__global__ __launch_bounds__(256) void col_stats_part_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                             int64_t n, int d, int64_t rows_per_block,
                                                             float* __restrict__ part) {
  __shared__ float4 s_mean[256], s_m2[256];
  __shared__ int s_cnt[256];
  const float* __restrict__ x = blockIdx.y ? xb : xa;
  const int nq = d >> 2, step = 256 / nq;
  const int q = threadIdx.x % nq, lr = threadIdx.x / nq;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(n, r0 + rows_per_block);
  float4 k = make_float4(0.f, 0.f, 0.f, 0.f), m = k, m2 = k;
  int cnt = 0;
  if (lr < step && r0 + lr < r1) {
    int64_t r = r0 + lr;
    const float* p = x + 4 * q;
    k = *reinterpret_cast<const float4*>(p + r * d);
    for (; r + 3 * (int64_t)step < r1; r += 4 * step) {
      const float4 v0 = *reinterpret_cast<const float4*>(p + r * d);
      const float4 v1 = *reinterpret_cast<const float4*>(p + (r + step) * d);
      const float4 v2 = *reinterpret_cast<const float4*>(p + (r + 2 * step) * d);
      const float4 v3 = *reinterpret_cast<const float4*>(p + (r + 3 * step) * d);
      welford_add(v0, k, 1.0f / (float)(cnt + 1), m, m2);
      welford_add(v1, k, 1.0f / (float)(cnt + 2), m, m2);
      welford_add(v2, k, 1.0f / (float)(cnt + 3), m, m2);
      welford_add(v3, k, 1.0f / (float)(cnt + 4), m, m2);
      cnt += 4;
    }
    for (; r < r1; r += step) welford_add(*reinterpret_cast<const float4*>(p + r * d), k, 1.0f / (float)(++cnt), m, m2);
  }
  s_mean[threadIdx.x] = make_float4(k.x + m.x, k.y + m.y, k.z + m.z, k.w + m.w);
  s_m2[threadIdx.x] = m2;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x < nq) {
    float4 m = s_mean[threadIdx.x], m2 = s_m2[threadIdx.x];
    float c0 = (float)s_cnt[threadIdx.x], c1 = c0, c2 = c0, c3 = c0;
    for (int g = 1; g < step; ++g) {
      const int o = threadIdx.x + g * nq;
      const float4 bm = s_mean[o], bq = s_m2[o];
      const float bc = (float)s_cnt[o];
      chan_merge(c0, m.x, m2.x, bc, bm.x, bq.x);
      chan_merge(c1, m.y, m2.y, bc, bm.y, bq.y);
      chan_merge(c2, m.z, m2.z, bc, bm.z, bq.z);
      chan_merge(c3, m.w, m2.w, bc, bm.w, bq.w);
    }
    float* dst = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * d + 4 * threadIdx.x;
    *reinterpret_cast<float4*>(dst) = m;
    *reinterpret_cast<float4*>(dst + d) = m2;
  }
}

// The workgroups' partials merged in block order: four lanes per column, each a quarter of the blocks (loads four deep),
// then the four quarters in order.  64 columns per workgroup; blockIdx.y picks the view.
__global__ __launch_bounds__(256) void col_stats_combine_kernel(const float* __restrict__ part, int nblocks, int64_t n,
                                                                int64_t rows_per_block, int d, float* __restrict__ mean_a,
                                                                float* __restrict__ std_a, float* __restrict__ mean_b,
                                                                float* __restrict__ std_b) {
  __shared__ float s_n[256], s_m[256], s_q[256];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
  const float* __restrict__ src = part + (int64_t)blockIdx.y * nblocks * 2 * d + col;
  const int per = (nblocks + 3) / 4;
  const int b0 = sub * per, b1 = min(nblocks, b0 + per);
  float na = 0.f, ma = 0.f, qa = 0.f;
  if (col < d) {
    int b = b0;
    for (; b + 4 <= b1; b += 4) {
      float m[4], q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        m[u] = src[(int64_t)(b + u) * 2 * d];
        q[u] = src[(int64_t)(b + u) * 2 * d + d];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t left = n - (int64_t)(b + u) * rows_per_block;
        chan_merge(na, ma, qa, (float)(left < 0 ? 0 : (left > rows_per_block ? rows_per_block : left)), m[u], q[u]);
      }
    }
    for (; b < b1; ++b) {
      const int64_t left = n - (int64_t)b * rows_per_block;
      chan_merge(na, ma, qa, (float)(left < 0 ? 0 : (left > rows_per_block ? rows_per_block : left)),
                 src[(int64_t)b * 2 * d], src[(int64_t)b * 2 * d + d]);
    }
  }
  s_n[threadIdx.x] = na;
  s_m[threadIdx.x] = ma;
  s_q[threadIdx.x] = qa;
  __syncthreads();
  if (sub == 0 && col < d) {
    for (int g = 1; g < 4; ++g) chan_merge(na, ma, qa, s_n[threadIdx.x + 64 * g], s_m[threadIdx.x + 64 * g], s_q[threadIdx.x + 64 * g]);
    (blockIdx.y ? mean_b : mean_a)[col] = ma;
    (blockIdx.y ? std_b : std_a)[col] = sqrtf(qa / (float)(n - 1));
  }
}

// gcr_dense.hip's tall-skinny X^T G with the operands standardised as they are loaded: four waves over one chunk of rows,
// wave w owns the 32 x 32 output tiles w, w + 4, ... of a (32 TX) x (32 TG) block of c whose corner blockIdx.y picks
// (d = 256: four 128 x 128 quadrants; otherwise the whole of c).  stats NULL: raw operands.  32 rows of either view at a
// time go through LDS (16-B coalesced loads, standardised on the way in; the next tile's loads are in flight during the
// products): with k = the row pair, lane (column, k) reads its MFMA operand as one conflict-free 4-B LDS word.  (Each lane
// loading its own 4-B operands from global memory, as gram_tn_kernel does, ran 3.7 ms at n = 1.1M, d = 128 — sixteen
// times the MFMA time — and 14.8 ms for the four quadrants of d = 256.)
template <int TX, int TG>
__global__ __launch_bounds__(256) void bt_product_kernel(const float* __restrict__ h1, const float* __restrict__ h2, int64_t n,
                                                         int d, int64_t rows_per_block, const float* __restrict__ stats,
                                                         float eps, float* __restrict__ part) {
  constexpr int NTILE = TX * TG, PER_WAVE = (NTILE + 3) / 4, R = 32;
  constexpr int CX = 32 * TX, CG = 32 * TG;
  // row strides: the two lane halves read rows 2 s and 2 s + 1 of one column; + 32 floats where the rows would share banks
  constexpr int SX = CX % 64 == 0 ? CX + 32 : CX, SG = CG % 64 == 0 ? CG + 32 : CG;
  constexpr int QX = CX / 4, QG = CG / 4, NLX = R * QX / 256, NLG = R * QG / 256;
  static_assert((R * QX) % 256 == 0 && (R * QG) % 256 == 0, "tile does not divide over the threads");
  __shared__ __attribute__((aligned(16))) float t1[R * SX], t2[R * SG];
  __shared__ __attribute__((aligned(16))) float s_m1[CX], s_i1[CX], s_m2[CG], s_i2[CG];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, h = lane >> 5;
  const int x0 = (blockIdx.y >> 1) * 128, g0 = (blockIdx.y & 1) * 128;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(n, r0 + rows_per_block);
  for (int c = threadIdx.x; c < CX; c += 256) {
    s_m1[c] = stats != nullptr ? stats[x0 + c] : 0.f;
    s_i1[c] = stats != nullptr ? 1.0f / (stats[d + x0 + c] + eps) : 1.0f;
  }
  for (int c = threadIdx.x; c < CG; c += 256) {
    s_m2[c] = stats != nullptr ? stats[2 * d + g0 + c] : 0.f;
    s_i2[c] = stats != nullptr ? 1.0f / (stats[3 * d + g0 + c] + eps) : 1.0f;
  }
  f32x16 acc[PER_WAVE];
  int oa[PER_WAVE], ob[PER_WAVE];
#pragma unroll
  for (int t = 0; t < PER_WAVE; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int tile = min(wave + 4 * t, NTILE - 1);
    oa[t] = 32 * (tile / TG) + c32;
    ob[t] = 32 * (tile % TG) + c32;
  }
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 rx[NLX], rg[NLG];
  auto load = [&](int64_t rb) {
#pragma unroll
    for (int u = 0; u < NLX; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int64_t row = rb + idx / QX;
      rx[u] = row < r1 ? *reinterpret_cast<const float4*>(h1 + row * d + x0 + 4 * (idx % QX)) : zero4;
    }
#pragma unroll
    for (int u = 0; u < NLG; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int64_t row = rb + idx / QG;
      rg[u] = row < r1 ? *reinterpret_cast<const float4*>(h2 + row * d + g0 + 4 * (idx % QG)) : zero4;
    }
  };
  if (r0 < r1) load(r0);
  for (int64_t rb = r0; rb < r1; rb += R) {
    __syncthreads();                                         // the statistics are in LDS; the previous tile has been read
#pragma unroll
    for (int u = 0; u < NLX; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int row = idx / QX, c4 = idx % QX;
      const float4 m = *reinterpret_cast<const float4*>(s_m1 + 4 * c4), i = *reinterpret_cast<const float4*>(s_i1 + 4 * c4);
      const float4 v = rx[u];
      *reinterpret_cast<float4*>(t1 + row * SX + 4 * c4) =
          rb + row < r1 ? make_float4((v.x - m.x) * i.x, (v.y - m.y) * i.y, (v.z - m.z) * i.z, (v.w - m.w) * i.w) : zero4;
    }
#pragma unroll
    for (int u = 0; u < NLG; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int row = idx / QG, c4 = idx % QG;
      const float4 m = *reinterpret_cast<const float4*>(s_m2 + 4 * c4), i = *reinterpret_cast<const float4*>(s_i2 + 4 * c4);
      const float4 v = rg[u];
      *reinterpret_cast<float4*>(t2 + row * SG + 4 * c4) =
          rb + row < r1 ? make_float4((v.x - m.x) * i.x, (v.y - m.y) * i.y, (v.z - m.z) * i.z, (v.w - m.w) * i.w) : zero4;
    }
    __syncthreads();
    if (rb + R < r1) load(rb + R);                           // in flight during the products
#pragma unroll
    for (int s = 0; s < R / 2; ++s) {
      float av[PER_WAVE], bv[PER_WAVE];
#pragma unroll
      for (int t = 0; t < PER_WAVE; ++t) {
        av[t] = t1[(2 * s + h) * SX + oa[t]];
        bv[t] = t2[(2 * s + h) * SG + ob[t]];
      }
#pragma unroll
      for (int t = 0; t < PER_WAVE; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc[t], 0, 0, 0);
    }
  }
  float* dst = part + (int64_t)blockIdx.x * d * d;
#pragma unroll
  for (int t = 0; t < PER_WAVE; ++t) {
    if (wave + 4 * t < NTILE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(x0 + oa[t] - c32 + acc_row(r, h)) * d + g0 + ob[t]] = acc[t][r];
    }
  }
}

// c[e] = (sum over the workgroups' partials) / n, four lanes per output (gcr_lanes.h: gcr_fold_partials4), and
// loss_part[block] = the loss terms of the block's 64 outputs: (1 - c)^2 on the diagonal, lambda c^2 off it.
__global__ __launch_bounds__(256) void bt_reduce_kernel(const float* __restrict__ part, int nblocks, int d, float inv_n,
                                                        float lambda, float* __restrict__ c, float* __restrict__ loss_part) {
  __shared__ float s_w[4];
  const int elems = d * d;
  const int k = blockIdx.x * 64 + (threadIdx.x >> 2);
  const int q = threadIdx.x & 3;
  const float s = gcr_fold_partials4(part, nblocks, elems, k, q, k < elems);
  float term = 0.f;
  if (k < elems && q == 0) {
    const float cv = s * inv_n;
    c[k] = cv;
    term = (k / d == k % d) ? (1.0f - cv) * (1.0f - cv) : lambda * cv * cv;
  }
  term = gcr_wave_sum(term);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = term;
  __syncthreads();
  if (threadIdx.x == 0) loss_part[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

__global__ __launch_bounds__(256) void bt_loss_kernel(const float* __restrict__ loss_part, int nparts, float* __restrict__ loss) {
  __shared__ float s_w[4];
  float s = 0.f;
  for (int k = threadIdx.x; k < nparts; k += 256) s += loss_part[k];
  s = gcr_wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// Workgroup b: row b of G and of G^T (gmat = G then G^T, d x d each), t1[b] = sum_k G[b,k] c[b,k], t2[b] = sum_j G[j,b] c[j,b]
// and coef = A1, B1, A2, B2 ([d] each): g_h = A (z_other G-product) - B (h - mean).  A column of zero std gets A = B = 0.
__global__ __launch_bounds__(256) void bt_prep_kernel(const float* __restrict__ c, int d, int64_t n, float lambda, float eps,
                                                      int batch_norm, const float* __restrict__ stats,
                                                      const float* __restrict__ g_loss, float* __restrict__ gmat,
                                                      float* __restrict__ coef) {
  __shared__ float s_r[4], s_c[4];
  const int b = blockIdx.x;
  const float gl = g_loss[0];
  float sr = 0.f, sc = 0.f;
  for (int k = threadIdx.x; k < d; k += 256) {
    const float cr = c[b * d + k], cc = c[k * d + b];
    const float gr = gl * (k == b ? -2.0f * (1.0f - cr) : 2.0f * lambda * cr);
    const float gc = gl * (k == b ? -2.0f * (1.0f - cc) : 2.0f * lambda * cc);
    gmat[b * d + k] = gr;
    gmat[d * d + b * d + k] = gc;
    sr += gr * cr;
    sc += gc * cc;
  }
  sr = gcr_wave_sum(sr);
  sc = gcr_wave_sum(sc);
  if ((threadIdx.x & 63) == 0) {
    s_r[threadIdx.x >> 6] = sr;
    s_c[threadIdx.x >> 6] = sc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t1 = (s_r[0] + s_r[1]) + (s_r[2] + s_r[3]), t2 = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
    const float fn = (float)n;
    if (batch_norm) {
      const float s1 = stats[d + b], s2 = stats[3 * d + b];
      coef[b] = s1 > 0.f ? 1.0f / (fn * (s1 + eps)) : 0.f;
      coef[d + b] = s1 > 0.f ? t1 / ((s1 + eps) * (fn - 1.0f) * s1) : 0.f;
      coef[2 * d + b] = s2 > 0.f ? 1.0f / (fn * (s2 + eps)) : 0.f;
      coef[3 * d + b] = s2 > 0.f ? t2 / ((s2 + eps) * (fn - 1.0f) * s2) : 0.f;
    } else {
      coef[b] = coef[2 * d + b] = 1.0f / fn;
      coef[d + b] = coef[3 * d + b] = 0.f;
    }
  }
}

// blockIdx.y = 0: g_h1 = A1 (z2 G^T) - B1 (h1 - m1);  1: g_h2 = A2 (z1 G) - B2 (h2 - m2).  NW waves; wave w owns output
// columns [32 (w % NJ), +32) of the row sub-tile w / NJ and keeps its 32 rows of G (side 0) or G^T (side 1) in registers,
// the reduction index split between the lane halves (half h: [h D/2, (h + 1) D/2), contiguous per lane as in gcr_tile.h).
// A tile of the other view (32 RT rows) is standardised into LDS (row stride + 16 B: conflict-free 16-B reads), the next
// tile's loads are in flight during the products.
template <int D, int NW>
__global__ __launch_bounds__(64 * NW) void bt_bwd_kernel(const float* __restrict__ h1, const float* __restrict__ h2, int64_t n,
                                                         const float* __restrict__ stats, float eps, int batch_norm,
                                                         const float* __restrict__ gmat, const float* __restrict__ coef,
                                                         float* __restrict__ g_h1, float* __restrict__ g_h2) {
  constexpr int NJ = D / 32, RT = NW / NJ, ROWS = 32 * RT, KH = D / 2, STRIDE = D + 4, NT = 64 * NW, NQ = D / 4;
  constexpr int NLD = ROWS * NQ / NT, RSTEP = NT / NQ;
  static_assert(NW % NJ == 0 && NT % NQ == 0 && (ROWS * NQ) % NT == 0, "tile does not divide over the threads");
  __shared__ __attribute__((aligned(16))) float tile[ROWS * STRIDE];
  const int side = blockIdx.y;
  float* __restrict__ out = side ? g_h2 : g_h1;
  if (out == nullptr) return;
  const float* __restrict__ other = side ? h1 : h2;
  const float* __restrict__ own = side ? h2 : h1;
  const float* __restrict__ o_stats = stats + (side ? 0 : 2 * D);
  const float* __restrict__ w_stats = stats + (side ? 2 * D : 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, h = lane >> 5;
  const int jt = wave % NJ, rt = wave / NJ;
  const int j = 32 * jt + c32;

  float bfrag[KH];
  {
    const float* p = gmat + (int64_t)side * D * D + j * D + h * KH;
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(p + 4 * q);
      bfrag[4 * q + 0] = v.x;
      bfrag[4 * q + 1] = v.y;
      bfrag[4 * q + 2] = v.z;
      bfrag[4 * q + 3] = v.w;
    }
  }
  const int c4 = threadIdx.x % NQ, srow = threadIdx.x / NQ;
  float4 sm = make_float4(0.f, 0.f, 0.f, 0.f), si = make_float4(1.f, 1.f, 1.f, 1.f);
  float ca = coef[side * 2 * D + j], cb = 0.f, wm = 0.f;
  if (batch_norm) {
    sm = *reinterpret_cast<const float4*>(o_stats + 4 * c4);
    const float4 sd = *reinterpret_cast<const float4*>(o_stats + D + 4 * c4);
    si = make_float4(1.0f / (sd.x + eps), 1.0f / (sd.y + eps), 1.0f / (sd.z + eps), 1.0f / (sd.w + eps));
    cb = coef[side * 2 * D + D + j];
    wm = w_stats[j];
  }
  const int64_t ntiles = (n + ROWS - 1) / ROWS;
  float4 regs[NLD];
  int64_t t = blockIdx.x;
  if (t < ntiles) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int64_t row = t * ROWS + srow + RSTEP * u;
      regs[u] = row < n ? *reinterpret_cast<const float4*>(other + row * D + 4 * c4) : sm;
    }
  }
  for (; t < ntiles; t += gridDim.x) {
    __syncthreads();                                         // the previous tile's products have read the LDS tile
#pragma unroll
    for (int u = 0; u < NLD; ++u) {                          // a row past n holds the mean: z = 0
      const float4 v = regs[u];
      *reinterpret_cast<float4*>(tile + (srow + RSTEP * u) * STRIDE + 4 * c4) =
          make_float4((v.x - sm.x) * si.x, (v.y - sm.y) * si.y, (v.z - sm.z) * si.z, (v.w - sm.w) * si.w);
    }
    __syncthreads();
    const int64_t tn = t + gridDim.x;
    if (tn < ntiles) {
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const int64_t row = tn * ROWS + srow + RSTEP * u;
        regs[u] = row < n ? *reinterpret_cast<const float4*>(other + row * D + 4 * c4) : sm;
      }
    }
    const int64_t rbase = t * ROWS + 32 * rt;
    float ownv[16];
    if (batch_norm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = rbase + acc_row(r, h);
        ownv[r] = row < n ? own[row * D + j] : wm;
      }
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* base = tile + (32 * rt + c32) * STRIDE + h * KH;
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(base + 4 * q);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bfrag[4 * q + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bfrag[4 * q + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bfrag[4 * q + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bfrag[4 * q + 3], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = rbase + acc_row(r, h);
      if (row < n) out[row * D + j] = batch_norm ? acc[r] * ca - cb * (ownv[r] - wm) : acc[r] * ca;
    }
  }
}

int32_t launch_col_stats(const float* xa, const float* xb, int64_t n, int d, float* mean_a, float* std_a, float* mean_b,
                         float* std_b, float* part, hipStream_t s) {
  const int nb = stat_blocks(n), views = xb != nullptr ? 2 : 1;
  const int64_t per = stat_rows(n, nb);
  hipLaunchKernelGGL(col_stats_part_kernel, dim3((unsigned)nb, (unsigned)views), dim3(256), 0, s, xa, xb, n, d, per, part);
  int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  hipLaunchKernelGGL(col_stats_combine_kernel, dim3((unsigned)((d + 63) / 64), (unsigned)views), dim3(256), 0, s, part, nb, n,
                     per, d, mean_a, std_a, mean_b, std_b);
  return GCR_LAUNCH_STATUS();
}

int64_t stats_part_floats(int64_t n, int d, int views) { return (int64_t)views * stat_blocks(n) * 2 * d; }

// one workspace for both calls, offsets in floats; nothing is padded: the regions are multiples of four floats
struct BtWorkspace {
  int64_t part;        // product partials [bt_blocks][d, d]
  int64_t stat_part;   // column-statistics partials of both views
  int64_t loss_part;   // kBtLossParts loss terms
  int64_t gmat;        // G, G^T [2][d, d]
  int64_t coef;        // A1, B1, A2, B2 [4][d]
  int64_t total;
};

BtWorkspace bt_layout(int64_t n, int d) {
  BtWorkspace w;
  WsCarve c;
  const int64_t dd = (int64_t)d * d;
  w.part = c.take(bt_blocks(n, d) * dd, 1);
  w.stat_part = c.take(stats_part_floats(n, d, 2), 1);
  w.loss_part = c.take(kBtLossParts, 1);
  w.gmat = c.take(2 * dd, 1);
  w.coef = c.take(4 * d, 1);
  w.total = c.at;
  return w;
}

}  // namespace

extern "C" int64_t gcr_col_stats_workspace_bytes(int64_t n, int32_t d) {
  if (n < 2 || d < 4 || d > 1024 || (d & 3) != 0) return 0;
  return stats_part_floats(n, d, 1) * (int64_t)sizeof(float);
}

extern "C" int32_t gcr_col_stats_f32(const float* x, int64_t n, int32_t d, float* mean, float* std, void* workspace,
                                     void* stream) {
  GCR_CHECK_ARG(n >= 2);
  if (d < 4 || d > 1024 || (d & 3) != 0) return GCR_EUNSUPPORTED;
  GCR_CHECK_ARG(x != nullptr && mean != nullptr && std != nullptr && workspace != nullptr);
  return launch_col_stats(x, nullptr, n, d, mean, std, nullptr, nullptr, reinterpret_cast<float*>(workspace),
                          (hipStream_t)stream);
}

extern "C" int32_t gcr_bt_supported(int32_t d) { return bt_dim_ok(d); }

extern "C" int64_t gcr_bt_workspace_bytes(int64_t n, int32_t d) {
  if (n < 1 || !bt_dim_ok(d)) return 0;
  return bt_layout(n, d).total * (int64_t)sizeof(float);
}

extern "C" int32_t gcr_bt_fwd_f32(const float* h1, const float* h2, int64_t n, int32_t d, float lambda, float eps,
                                  int32_t batch_norm, float* stats, float* c, float* loss, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= (batch_norm ? 2 : 1));
  if (!bt_dim_ok(d)) return GCR_EUNSUPPORTED;
  GCR_CHECK_ARG(h1 != nullptr && h2 != nullptr && c != nullptr && loss != nullptr && workspace != nullptr);
  GCR_CHECK_ARG(!batch_norm || stats != nullptr);
  hipStream_t s = (hipStream_t)stream;
  const int nb = bt_blocks(n, d);
  const int64_t per = bt_rows(n, nb), dd = (int64_t)d * d;
  const BtWorkspace w = bt_layout(n, d);
  float* ws = reinterpret_cast<float*>(workspace);
  float *part = ws + w.part, *stat_part = ws + w.stat_part, *loss_part = ws + w.loss_part;
  int32_t st;
  if (batch_norm) {
    st = launch_col_stats(h1, h2, n, d, stats, stats + d, stats + 2 * d, stats + 3 * d, stat_part, s);
    if (st != GCR_OK) return st;
  }
  const float* sp = batch_norm ? stats : nullptr;
  dispatch_value<32, 64, 96, 128, 256>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value, T = D == 256 ? 4 : D / 32;      // d = 256: four quadrants of 128 x 128
    hipLaunchKernelGGL((bt_product_kernel<T, T>), dim3((unsigned)nb, D == 256 ? 4 : 1), dim3(256), 0, s, h1, h2, n, (int)d, per,
                       sp, eps, part);
  });
  st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  const int nred = (int)((dd + 63) / 64);
  hipLaunchKernelGGL(bt_reduce_kernel, dim3((unsigned)nred), dim3(256), 0, s, part, nb, (int)d, 1.0f / (float)n, lambda, c,
                     loss_part);
  st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  hipLaunchKernelGGL(bt_loss_kernel, dim3(1), dim3(256), 0, s, loss_part, nred, loss);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_bt_bwd_f32(const float* h1, const float* h2, int64_t n, int32_t d, float lambda, float eps,
                                  int32_t batch_norm, const float* stats, const float* c, const float* g_loss, float* g_h1,
                                  float* g_h2, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= (batch_norm ? 2 : 1));
  if (!bt_dim_ok(d)) return GCR_EUNSUPPORTED;
  if (g_h1 == nullptr && g_h2 == nullptr) return GCR_OK;
  GCR_CHECK_ARG(h1 != nullptr && h2 != nullptr && c != nullptr && g_loss != nullptr && workspace != nullptr);
  GCR_CHECK_ARG(!batch_norm || stats != nullptr);
  hipStream_t s = (hipStream_t)stream;
  const BtWorkspace w = bt_layout(n, d);
  float *gmat = reinterpret_cast<float*>(workspace) + w.gmat, *coef = reinterpret_cast<float*>(workspace) + w.coef;
  hipLaunchKernelGGL(bt_prep_kernel, dim3((unsigned)d), dim3(256), 0, s, c, (int)d, n, lambda, eps, (int)batch_norm, stats,
                     g_loss, gmat, coef);
  int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  const float* sp = batch_norm ? stats : gmat;               // never read without batch_norm
  dispatch_value<32, 64, 96, 128, 256>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value, NW = D == 96 ? 3 : (D == 256 ? 8 : 4), ROWS = 32 * (NW / (D / 32));
    const unsigned tiles = (unsigned)gcr_grid((n + ROWS - 1) / ROWS, D == 256 ? 512 : 1024);
    hipLaunchKernelGGL((bt_bwd_kernel<D, NW>), dim3(tiles, 2), dim3(64 * NW), 0, s, h1, h2, n, sp, eps, (int)batch_norm, gmat,
                       coef, g_h1, g_h2);
  });
  return GCR_LAUNCH_STATUS();
}
