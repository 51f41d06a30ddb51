// BUIR's bootstrap loss (predictor + two cosines per pair) and its row-wise target update (gfx950).
//
// Replaces, per batch, univariate/buir.py:260-262, 269-277, 323-325: four advanced-index gathers, nn.Linear twice, four
// F.normalize, the products, the sums and the mean — and, for the update, buir.py:254-257.  With side 0 = (x = on_user[u],
// t = tg_item[i]) and side 1 = (x = on_item[i], t = tg_user[u]), p = W x + bias and c = <p, t> / max(|p|, eps) / max(|t|, eps):
//
//   forward   rows     grid (32-position tiles, 2 sides), four waves.  A wave forms 32 positions x 32 outputs of p on the f32
//                      MFMA (v_mfma_f32_32x32x2_f32; A = 32 rows of W, B = the 32 gathered rows, both read from global a
//                      half row per lane, no LDS staging: W is at most 1 MiB and stays in L2) for every fourth 32-output
//                      chunk and sums |p|^2, <p, t>, |t|^2 of its chunks; the four waves' sums meet in the LDS in wave
//                      order.  Saves stats [2, 3, B] = (|p|, |t|, c) and nothing of width d.
//             reduce   loss = (1 / B) sum_b (2 - 2 c_0[b]) + (2 - 2 c_1[b]), summed in double in a fixed order.
//   backward  dp       grid (tiles, sides, output chunks), one wave: p again (the forward's product, bit for bit), then
//                      dp = -(2 g / B) (t / max(|t|, eps) - c p / |p|) / |p|   (|p| < eps: torch's clamp branch, no
//                      projection and 1 / eps) into dp [2, B, d].
//             grad     one grid, one wave per block: blocks of the first range form dx = W^T dp per (tile, side, 32 columns)
//                      into dx [2, B, d]; the others form a [32, 32] tile of sum_b dp x^T over one split of the 2 B
//                      positions (side 0 first) into dW_part [S, d, d], and those of column chunk 0 the column sums of dp
//                      into db_part [S, d].
//             finish   waves of the first range: one per sorted position; the head of a run of equal ids adds the run's dx
//                      rows in sorted (= position) order and WRITES the row.  The others add the S partials in split order.
// One writer per word, fixed orders, no float atomics: every output is bitwise reproducible.
#include "gcr_host.h"
#include "gcr_tile.h"   // f32x16, acc_row, kTileJ = 32 rows of a tile

namespace {

constexpr int kMaxD = 512;
constexpr int kMaxSplits = 32;
constexpr float kNormEps = 1e-12f;   // F.normalize's eps

__device__ __forceinline__ float4 ld4(const float* p) {
  return p ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// C[acc_row(r, h)][l32] = <a_row of lane l32, b_row of lane l32> over d columns; lane (l32, h) feeds columns
// [h d / 2, (h + 1) d / 2) of both.  A NULL row is a zero row.
__device__ __forceinline__ f32x16 rows_dot_tile(const float* a_row, const float* b_row, int d, int h) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int half = d >> 1;
  const float* pa = a_row ? a_row + h * half : nullptr;
  const float* pb = b_row ? b_row + h * half : nullptr;
  for (int q = 0; q < half; q += 4) {
    const float4 a = ld4(pa ? pa + q : nullptr), b = ld4(pb ? pb + q : nullptr);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
  return acc;
}

struct BuirArgs {
  const float* on[2];      // on_user, on_item
  const float* tg[2];      // tg_user, tg_item
  const int64_t* idx[2];   // u_idx, i_idx
  int64_t n[2];            // n_users, n_items
  int64_t batch;
  int d;
  const float* w;
  const float* bias;
};

// row of side s's table for position b: x = on[s][idx[s][b]], t = tg[1 - s][idx[1 - s][b]]; NULL outside the table
__device__ __forceinline__ const float* row_of(const float* tab, const int64_t* idx, int64_t n_rows, int64_t b, int64_t batch,
                                               int d) {
  if (b >= batch) return nullptr;
  const int64_t id = idx[b];
  return (id >= 0 && id < n_rows) ? tab + id * d : nullptr;
}

__global__ __launch_bounds__(256) void buir_fwd_rows_kernel(BuirArgs A, float* __restrict__ stats) {
  __shared__ float red[3][4][kTileJ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
  const int side = blockIdx.y, d = A.d;
  const int64_t b = (int64_t)blockIdx.x * kTileJ + l32;
  const float* x_row = row_of(A.on[side], A.idx[side], A.n[side], b, A.batch, d);
  const float* t_row = row_of(A.tg[1 - side], A.idx[1 - side], A.n[1 - side], b, A.batch, d);
  const int n_chunks = (d + 31) >> 5;
  float pp = 0.f, pt = 0.f, tt = 0.f;
  for (int chunk = wave; chunk < n_chunks; chunk += 4) {
    const int o0 = chunk * 32, o = o0 + l32;
    const f32x16 acc = rows_dot_tile(o < d ? A.w + (int64_t)o * d : nullptr, x_row, d, h);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ob = o0 + 8 * g + 4 * h;              // d % 16 == 0: a group of four outputs is inside d or outside
      if (ob < d) {
        const float4 bi = ld4(A.bias + ob), tv = ld4(t_row ? t_row + ob : nullptr);
        const float p0 = acc[4 * g] + bi.x, p1 = acc[4 * g + 1] + bi.y, p2 = acc[4 * g + 2] + bi.z, p3 = acc[4 * g + 3] + bi.w;
        pp += p0 * p0; pp += p1 * p1; pp += p2 * p2; pp += p3 * p3;
        pt += p0 * tv.x; pt += p1 * tv.y; pt += p2 * tv.z; pt += p3 * tv.w;
        tt += tv.x * tv.x; tt += tv.y * tv.y; tt += tv.z * tv.z; tt += tv.w * tv.w;
      }
    }
  }
  pp += __shfl_xor(pp, 32, GCR_WAVE);
  pt += __shfl_xor(pt, 32, GCR_WAVE);
  tt += __shfl_xor(tt, 32, GCR_WAVE);
  if (h == 0) {
    red[0][wave][l32] = pp;
    red[1][wave][l32] = pt;
    red[2][wave][l32] = tt;
  }
  __syncthreads();
  if (threadIdx.x < kTileJ && b < A.batch) {
    float s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = ((red[k][0][l32] + red[k][1][l32]) + red[k][2][l32]) + red[k][3][l32];
    const float np = sqrtf(s[0]), nt = sqrtf(s[2]);
    float* st = stats + (int64_t)side * 3 * A.batch;
    st[b] = np;
    st[A.batch + b] = nt;
    st[2 * A.batch + b] = s[1] / fmaxf(np, kNormEps) / fmaxf(nt, kNormEps);
  }
}

__global__ __launch_bounds__(256) void buir_loss_kernel(const float* __restrict__ stats, int64_t batch, float* __restrict__ loss) {
  __shared__ double part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* c0 = stats + 2 * batch;
  const float* c1 = stats + 5 * batch;
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < batch; b += 256) s += (double)((2.0f - 2.0f * c0[b]) + (2.0f - 2.0f * c1[b]));
  // gcr_lanes.h's gcr_wave_sum_f64, written out: through the call the compiler orders two instructions of this kernel the
  // other way round, and the units of this family are held to their instructions
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, GCR_WAVE);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((((part[0] + part[1]) + part[2]) + part[3]) / (double)batch);
}

// dp [2, B, d]
__global__ __launch_bounds__(64) void buir_dp_kernel(BuirArgs A, const float* __restrict__ stats, const float* __restrict__ g,
                                                     float* __restrict__ dp) {
  const int lane = threadIdx.x, l32 = lane & 31, h = lane >> 5;
  const int side = blockIdx.y, d = A.d, o0 = blockIdx.z * 32, o = o0 + l32;
  const int64_t b = (int64_t)blockIdx.x * kTileJ + l32;
  const bool live = b < A.batch;
  const float* x_row = row_of(A.on[side], A.idx[side], A.n[side], b, A.batch, d);
  const float* t_row = row_of(A.tg[1 - side], A.idx[1 - side], A.n[1 - side], b, A.batch, d);
  const f32x16 acc = rows_dot_tile(o < d ? A.w + (int64_t)o * d : nullptr, x_row, d, h);
  if (!live) return;
  const float* st = stats + (int64_t)side * 3 * A.batch;
  const float np = st[b], nt = st[A.batch + b], c = st[2 * A.batch + b];
  const float inv_p = 1.0f / fmaxf(np, kNormEps), inv_t = 1.0f / fmaxf(nt, kNormEps);
  const float cp = np >= kNormEps ? c * inv_p : 0.f;           // below the clamp the norm is a constant: no projection
  const float coef = -2.0f * g[0] / (float)A.batch * inv_p;
  float* out = dp + ((int64_t)side * A.batch + b) * d;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ob = o0 + 8 * q + 4 * h;
    if (ob < d) {
      const float4 bi = ld4(A.bias + ob), tv = ld4(t_row ? t_row + ob : nullptr);
      float4 r;
      r.x = coef * (tv.x * inv_t - cp * (acc[4 * q] + bi.x));
      r.y = coef * (tv.y * inv_t - cp * (acc[4 * q + 1] + bi.y));
      r.z = coef * (tv.z * inv_t - cp * (acc[4 * q + 2] + bi.z));
      r.w = coef * (tv.w * inv_t - cp * (acc[4 * q + 3] + bi.w));
      *reinterpret_cast<float4*>(out + ob) = r;
    }
  }
}

// blocks [0, n_dx): dx[s, b, k0 + ..] = sum_o W[o, k] dp[s, b, o] for (tile, side, column chunk);
// the others: dW_part[split, o0 + .., k0 + ..] = sum over the split's positions of dp[v, o] x[v, k], and db_part
__global__ __launch_bounds__(64) void buir_grad_kernel(BuirArgs A, const float* __restrict__ dp, int n_tiles, int n_chunks,
                                                       int n_dx, int n_splits, int split_len, float* __restrict__ dx,
                                                       float* __restrict__ dw_part, float* __restrict__ db_part) {
  const int lane = threadIdx.x, l32 = lane & 31, h = lane >> 5, d = A.d;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  int blk = blockIdx.x;
  if (blk < n_dx) {
    const int kc = blk % n_chunks;
    blk /= n_chunks;
    const int side = blk & 1, tile = blk >> 1;
    const int k = kc * 32 + l32;
    const int64_t b = (int64_t)tile * kTileJ + l32;
    const bool live = b < A.batch;
    const float* drow = live ? dp + ((int64_t)side * A.batch + b) * d : nullptr;
    const float* wcol = k < d ? A.w + k : nullptr;
    const int half = d >> 1, obase = h * half;
    for (int q = 0; q < half; q += 4) {
      const float4 bv = ld4(drow ? drow + obase + q : nullptr);
      float a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = wcol ? wcol[(int64_t)(obase + q + j) * d] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], bv.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], bv.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], bv.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], bv.w, acc, 0, 0, 0);
    }
    if (!live) return;
    float* out = dx + ((int64_t)side * A.batch + b) * d;      // acc[r] = dx[b][kc * 32 + acc_row(r, h)]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kb = kc * 32 + 8 * q + 4 * h;
      if (kb < d) *reinterpret_cast<float4*>(out + kb) = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
    }
    return;
  }
  blk -= n_dx;
  const int kc = blk % n_chunks;
  blk /= n_chunks;
  const int oc = blk % n_chunks, split = blk / n_chunks;
  const int o = oc * 32 + l32, k = kc * 32 + l32;
  const int64_t total = 2 * A.batch;
  const int64_t v0 = (int64_t)split * split_len;
  const int64_t v1 = v0 + split_len < total ? v0 + split_len : total;
  float bsum = 0.f;
  for (int64_t vb = v0; vb < v1; vb += 8) {                    // split_len % 8 == 0: lane half h takes vb + 2 j + h
    float a[4], x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t v = vb + 2 * j + h;
      a[j] = 0.f;
      x[j] = 0.f;
      if (v < v1) {
        const int side = v >= A.batch ? 1 : 0;
        const int64_t id = A.idx[side][v - side * A.batch];
        if (o < d) a[j] = dp[v * d + o];
        if (k < d && id >= 0 && id < A.n[side]) x[j] = A.on[side][id * d + k];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x[j], acc, 0, 0, 0);
      bsum += a[j];
    }
  }
  if (k < d) {                                                  // acc[r] = dW[oc * 32 + acc_row(r, h)][k]
    float* out = dw_part + (int64_t)split * d * d;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int orow = oc * 32 + acc_row(r, h);
      if (orow < d) out[(int64_t)orow * d + k] = acc[r];
    }
  }
  if (kc == 0) {
    bsum += __shfl_xor(bsum, 32, GCR_WAVE);
    if (h == 0 && o < d) db_part[(int64_t)split * d + o] = bsum;
  }
}

struct BuirOrder {
  const uint32_t* keys[2];
  const int32_t* perm[2];
  float* grad[2];
};

__global__ __launch_bounds__(256) void buir_finish_kernel(BuirOrder O, const float* __restrict__ dx, int64_t batch, int d,
                                                          int64_t n_users, int64_t n_items, int n_seg_blocks, int n_splits,
                                                          const float* __restrict__ dw_part, const float* __restrict__ db_part,
                                                          float* __restrict__ g_w, float* __restrict__ g_bias) {
  if ((int)blockIdx.x >= n_seg_blocks) {
    const int64_t e = (int64_t)(blockIdx.x - n_seg_blocks) * 256 + threadIdx.x;
    const int64_t nw = (int64_t)d * d;
    if (e < nw) {
      float s = 0.f;
      for (int sp = 0; sp < n_splits; ++sp) s += dw_part[sp * nw + e];
      g_w[e] = s;
    } else if (e < nw + d) {
      float s = 0.f;
      for (int sp = 0; sp < n_splits; ++sp) s += db_part[(int64_t)sp * d + (e - nw)];
      g_bias[e - nw] = s;
    }
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  if (w >= 2 * batch) return;
  const int side = w >= batch ? 1 : 0;
  const int64_t j = w - side * batch;
  const uint32_t* keys = O.keys[side];
  const uint32_t key = keys[j];
  if ((int64_t)key >= (side ? n_items : n_users)) return;       // ids outside the table sort last with the key n_keys
  if (j > 0 && keys[j - 1] == key) return;                      // not the head of its run
  constexpr int NV = kMaxD / 64;
  float s[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) s[q] = 0.f;
  const float* src = dx + (int64_t)side * batch * d;
  for (int64_t jj = j; jj < batch && keys[jj] == key; ++jj) {
    const float* row = src + (int64_t)O.perm[side][jj] * d;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int c = lane + 64 * q;
      if (c < d) s[q] += row[c];
    }
  }
  float* out = O.grad[side] + (int64_t)key * d;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int c = lane + 64 * q;
    if (c < d) out[c] = s[q];
  }
}

// one wave per position; the wave that sets the row's claim bit first does the row's one update
__global__ __launch_bounds__(256) void ema_rows_kernel(float* __restrict__ target, const float* __restrict__ online,
                                                       const int64_t* __restrict__ idx, int64_t n, int d, int64_t n_rows,
                                                       float m, float one_minus_m, uint32_t* __restrict__ claim) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n; i += (int64_t)gridDim.x * 4) {
    const int64_t r = idx[i];
    if (r < 0 || r >= n_rows) continue;                         // wave-uniform
    uint32_t old = 0;
    if (lane == 0) old = atomicOr(claim + (r >> 5), 1u << (r & 31));
    old = (uint32_t)gcr_readlane_i((int)old, 0);
    if ((old >> (r & 31)) & 1u) continue;
    float* t = target + r * d;
    const float* o = online + r * d;
    for (int c = lane; c < d; c += 64) t[c] = __fadd_rn(__fmul_rn(t[c], m), __fmul_rn(o[c], one_minus_m));
  }
}

struct BuirWorkspace {
  int64_t dp, dx, dw_part, db_part, total;      // offsets in floats
  int n_splits, split_len;
};

BuirWorkspace buir_layout(int64_t batch, int d) {
  BuirWorkspace w;
  const int n_chunks = (d + 31) / 32;
  int64_t s = 512 / (n_chunks * n_chunks);
  if (s > kMaxSplits) s = kMaxSplits;
  const int64_t most = (2 * batch + 7) / 8;                     // at least eight positions per split
  if (s > most) s = most;
  if (s < 1) s = 1;
  int64_t len = (2 * batch + s - 1) / s;
  len = (len + 7) & ~(int64_t)7;
  w.n_splits = (int)((2 * batch + len - 1) / len);
  if (w.n_splits < 1) w.n_splits = 1;
  w.split_len = (int)len;
  WsCarve c;
  w.dp = c.take(2 * batch * d);
  w.dx = c.take(2 * batch * d);
  w.dw_part = c.take((int64_t)w.n_splits * d * d);
  w.db_part = c.take((int64_t)w.n_splits * d);
  w.total = c.at;
  return w;
}

BuirArgs buir_args(const float* on_user, const float* on_item, const float* tg_user, const float* tg_item, int64_t n_users,
                   int64_t n_items, int d, const int64_t* u_idx, const int64_t* i_idx, int64_t batch, const float* w,
                   const float* bias) {
  BuirArgs A;
  A.on[0] = on_user; A.on[1] = on_item; A.tg[0] = tg_user; A.tg[1] = tg_item;
  A.idx[0] = u_idx; A.idx[1] = i_idx; A.n[0] = n_users; A.n[1] = n_items;
  A.batch = batch; A.d = d; A.w = w; A.bias = bias;
  return A;
}

bool buir_args_ok(int64_t n_users, int64_t n_items, int64_t batch) {
  return n_users >= 0 && n_users < (1ll << 31) && n_items >= 0 && n_items < (1ll << 31) && batch >= 0 && batch < (1ll << 24);
}

}  // namespace

extern "C" int32_t gcr_buir_supported(int32_t d) { return d >= 16 && d <= kMaxD && d % 16 == 0; }

extern "C" int64_t gcr_buir_workspace_bytes(int64_t batch, int32_t d) {
  if (batch < 1 || batch >= (1ll << 24) || !gcr_buir_supported(d)) return 0;
  return buir_layout(batch, d).total * (int64_t)sizeof(float);
}

extern "C" int32_t gcr_buir_fwd_f32(const float* on_user, const float* on_item, const float* tg_user, const float* tg_item,
                                    int64_t n_users, int64_t n_items, int32_t d, const int64_t* u_idx, const int64_t* i_idx,
                                    int64_t batch, const float* w, const float* bias, float* loss, float* stats,
                                    void* stream) {
  if (!gcr_buir_supported(d)) return GCR_EUNSUPPORTED;
  GCR_CHECK_ARG(buir_args_ok(n_users, n_items, batch));
  if (batch == 0) return GCR_OK;
  GCR_CHECK_ARG(on_user && on_item && tg_user && tg_item && u_idx && i_idx && w && bias && loss && stats);
  GCR_CHECK_ARG(aligned16(on_user, on_item, tg_user, tg_item, w, bias));
  hipStream_t s = (hipStream_t)stream;
  const BuirArgs A = buir_args(on_user, on_item, tg_user, tg_item, n_users, n_items, d, u_idx, i_idx, batch, w, bias);
  const unsigned n_tiles = (unsigned)((batch + kTileJ - 1) / kTileJ);
  hipLaunchKernelGGL(buir_fwd_rows_kernel, dim3(n_tiles, 2), dim3(256), 0, s, A, stats);
  hipLaunchKernelGGL(buir_loss_kernel, dim3(1), dim3(256), 0, s, stats, batch, loss);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_buir_bwd_f32(const float* on_user, const float* on_item, const float* tg_user, const float* tg_item,
                                    int64_t n_users, int64_t n_items, int32_t d, const int64_t* u_idx, const int64_t* i_idx,
                                    int64_t batch, const float* w, const float* bias, const float* stats, const float* g,
                                    const uint32_t* keys_u, const int32_t* perm_u, const uint32_t* keys_i,
                                    const int32_t* perm_i, float* g_on_user, float* g_on_item, float* g_w, float* g_bias,
                                    void* workspace, void* stream) {
  if (!gcr_buir_supported(d)) return GCR_EUNSUPPORTED;
  GCR_CHECK_ARG(buir_args_ok(n_users, n_items, batch));
  if (batch == 0) return GCR_OK;
  GCR_CHECK_ARG(on_user && on_item && tg_user && tg_item && u_idx && i_idx && w && bias && stats && g && keys_u && perm_u &&
                keys_i && perm_i && g_on_user && g_on_item && g_w && g_bias && workspace);
  GCR_CHECK_ARG(aligned16(on_user, on_item, tg_user, tg_item, w, bias, workspace));
  hipStream_t s = (hipStream_t)stream;
  const BuirArgs A = buir_args(on_user, on_item, tg_user, tg_item, n_users, n_items, d, u_idx, i_idx, batch, w, bias);
  BuirOrder O;
  O.keys[0] = keys_u; O.keys[1] = keys_i; O.perm[0] = perm_u; O.perm[1] = perm_i;
  O.grad[0] = g_on_user; O.grad[1] = g_on_item;
  const BuirWorkspace L = buir_layout(batch, d);
  float* ws = reinterpret_cast<float*>(workspace);
  const int n_tiles = (int)((batch + kTileJ - 1) / kTileJ), n_chunks = (d + 31) / 32;
  hipLaunchKernelGGL(buir_dp_kernel, dim3((unsigned)n_tiles, 2, (unsigned)n_chunks), dim3(64), 0, s, A, stats, g, ws + L.dp);
  const int n_dx = n_tiles * 2 * n_chunks, n_dw = n_chunks * n_chunks * L.n_splits;
  hipLaunchKernelGGL(buir_grad_kernel, dim3((unsigned)(n_dx + n_dw)), dim3(64), 0, s, A, ws + L.dp, n_tiles, n_chunks, n_dx,
                     L.n_splits, L.split_len, ws + L.dx, ws + L.dw_part, ws + L.db_part);
  const int n_seg_blocks = (int)((2 * batch + 3) / 4);
  const int n_w_blocks = (int)(((int64_t)d * d + d + 255) / 256);
  hipLaunchKernelGGL(buir_finish_kernel, dim3((unsigned)(n_seg_blocks + n_w_blocks)), dim3(256), 0, s, O, ws + L.dx, batch,
                     (int)d, n_users, n_items, n_seg_blocks, L.n_splits, ws + L.dw_part, ws + L.db_part, g_w, g_bias);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_ema_rows_f32(float* target, const float* online, const int64_t* idx, int64_t n, int32_t d,
                                    int64_t n_rows, double momentum, uint32_t* claim_bits, void* stream) {
  GCR_CHECK_ARG(n >= 0 && d >= 1 && n_rows >= 0 && n_rows < (1ll << 40));
  if (n == 0 || n_rows == 0) return GCR_OK;
  GCR_CHECK_ARG(target && online && idx && claim_bits);
  hipStream_t s = (hipStream_t)stream;
  const int32_t st = gcr_hip_status(hipMemsetAsync(claim_bits, 0, (size_t)((n_rows + 31) / 32) * sizeof(uint32_t), s));
  if (st != GCR_OK) return st;
  hipLaunchKernelGGL(ema_rows_kernel, dim3((unsigned)gcr_grid((n + 3) / 4, 8192)), dim3(256), 0, s, target, online, idx, n,
                     (int)d, n_rows, (float)momentum, (float)(1.0 - momentum), claim_bits);
  return GCR_LAUNCH_STATUS();
}
