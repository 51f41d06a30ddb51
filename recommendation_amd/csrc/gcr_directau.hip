// DirectAU's loss family — alignment + uniformity over gathered, L2-normalised batch rows (gfx950).
//
// Replaces, for the three row sets u = user_emb[user_idx], p = item_emb[pos_idx], n = item_emb[neg_idx] of
// directau.py:222-226, the gathers, F.normalize x3, the alignment means (directau.py:245-246), torch.pdist + exp + mean
// of uniformity (directau.py:248-251) and the Frobenius norms of l2_reg_loss (directau.py:35-36) by two launches:
//
//   prepare   one wave per batch position: gathers the (up to) three rows, writes the normalised rows x^ and
//             1 / max(|x|, 1e-12), and per-block partials of A_pos, A_neg, Q_u, Q_p, Q_n.
//   tile      one workgroup per (32-row tile, set, 64-column slice of d): its four waves walk the column tiles
//             w, w + 4, ... of the SAME set; per tile  T[b][a] = x^_b . x^_a  on the f32 MFMA (v_mfma_f32_32x32x2_f32),
//             e = exp(-t (|x^_a|^2 + |x^_b|^2 - 2 T)) with the position a = b and the ragged edge masked, g[a] += sum_b e,
//             and — flash style, so that the backward never sees a pair again —  o[a, :] += sum_b e x^_b[:]  as a second
//             MFMA product whose B operand is the accumulator of the first (T is computed TRANSPOSED for that: the C
//             layout of T^T is the B layout of the second product, no shuffle).  The four waves' partial r / o are added
//             in wave order, G_s = 1/2 sum_a g_s[a] from per-tile partials in tile order by the last workgroup to
//             finish (an integer ticket; no float atomics): r, o and all eight sums are bitwise reproducible.
//
// Two positions that hold the SAME table row are an ordinary pair for G (e = 1 exactly), but their share of the gradient,
// e (x^_a - x^_b), is exactly 0: they are left out of r and o.  Kept in, a row that recurs k times would carry k x^_a in
// both r x^_a and o_a, and the backward would have to recover the other pairs' contribution (which at t = 3 is a
// hundredth of that) from the difference of two rounded numbers.
// |x^_a|^2 is carried instead of assuming 1, so a zero row (x^ = 0, as F.normalize gives) is at distance 1 from a unit
// row and 0 from another zero row.  d wider than 64 is walked in 64-column
// chunks through the LDS (41 KB static for any d); the o slices of one row tile are separate workgroups that each redo
// the first product (the problem is latency-bound at the reference's batch sizes, not matrix-core-bound).
//
// Backward: one launch, one wave per batch position.  From r, o, inv_norm and the table rows it forms the gradient with
// respect to x^ of every set, applies the normalize backward and the 2 g_Q x term, and adds the row into the table
// gradient with one float atomic per element (duplicate ids collide, as in gcr_scatter_add_rows_f32).
#include "gcr_host.h"
#include "gcr_lanes.h"
#include "gcr_tile.h"   // f32x16, acc_row, kTileJ = 32: rows of a tile (the MFMA's M and N)

namespace {

constexpr int kKC = 64;             // feature columns staged per chunk = width of an o slice
constexpr int kStride = kKC + 1;     // LDS row stride: odd, so 32 rows of one column fall into 32 banks
constexpr int kWaves = 4;
constexpr int kMaxPrepBlocks = 256;
constexpr int kPrepVals = 5;         // A_pos, A_neg, Q_u, Q_p, Q_n
constexpr float kNormEps = 1e-12f;   // F.normalize's eps

struct AuSets {
  const float* tab[3];
  const int64_t* idx[3];
  int64_t n_rows[3];
};

// row of set s at batch position b: idx NULL = the table's own row b; -1 for an id out of range (a zero row)
__device__ __forceinline__ int64_t au_row(const AuSets& S, int s, int64_t b) {
  const int64_t row = S.idx[s] != nullptr ? S.idx[s][b] : b;
  return (row >= 0 && row < S.n_rows[s]) ? row : -1;
}

template <int NV>
__global__ __launch_bounds__(256) void au_prepare_kernel(AuSets S, int d, int64_t batch, int n_sets, float* __restrict__ xhat,
                                                         float* __restrict__ inv_norm, float* __restrict__ sqn,
                                                         int32_t* __restrict__ row_id, float* __restrict__ part,
                                                         unsigned* __restrict__ ticket) {
  __shared__ float red[kWaves][kPrepVals];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0u;     // the tile launch's completion count
  float acc[kPrepVals];
#pragma unroll
  for (int k = 0; k < kPrepVals; ++k) acc[k] = 0.f;
  for (int64_t b = (int64_t)blockIdx.x * kWaves + wave; b < batch; b += (int64_t)gridDim.x * kWaves) {
    float xh[3][NV];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
#pragma unroll
      for (int v = 0; v < NV; ++v) xh[s][v] = 0.f;
      if (s >= n_sets) continue;
      const int64_t row = au_row(S, s, b);
      float x[NV], ss = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = lane + 64 * v;
        x[v] = (row >= 0 && c < d) ? S.tab[s][row * d + c] : 0.f;
        ss += x[v] * x[v];
      }
      ss = gcr_wave_sum(ss);
      const float inv = 1.0f / fmaxf(sqrtf(ss), kNormEps);
      float hh = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = lane + 64 * v;
        xh[s][v] = x[v] * inv;
        hh += xh[s][v] * xh[s][v];
        if (c < d) xhat[((int64_t)s * batch + b) * d + c] = xh[s][v];
      }
      hh = gcr_wave_sum(hh);
      if (lane == 0) {
        inv_norm[(int64_t)s * batch + b] = inv;
        sqn[(int64_t)s * batch + b] = hh;
        row_id[(int64_t)s * batch + b] = (int32_t)row;        // -1: out of range (all such rows are the same zero row)
      }
      acc[2 + s] += ss;
    }
#pragma unroll
    for (int s = 1; s < 3; ++s) {
      if (s >= n_sets) continue;
      float dp = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float df = xh[0][v] - xh[s][v];
        dp += df * df;
      }
      acc[s - 1] += gcr_wave_sum(dp);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kPrepVals; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kPrepVals) {
    float s = 0.f;
    for (int w = 0; w < kWaves; ++w) s += red[w][threadIdx.x];   // fixed order
    part[(int64_t)blockIdx.x * kPrepVals + threadIdx.x] = s;
  }
}

// grid = (row tiles, sets, o slices).  WANT_O = false: the sums only (one slice, no r / o written).
template <bool WANT_O>
__global__ __launch_bounds__(256) void au_tile_kernel(const float* __restrict__ xhat, const float* __restrict__ sqn,
                                                      const int32_t* __restrict__ row_id, int d, int64_t batch, int n_sets,
                                                      float t, float* __restrict__ r_out, float* __restrict__ o_out,
                                                      float* __restrict__ r_part,
                                                      const float* __restrict__ prep_part, int prep_blocks,
                                                      unsigned* __restrict__ ticket, float* __restrict__ sums) {
  __shared__ float rowt[kTileJ * kStride];
  __shared__ float colt[kWaves][kTileJ * kStride];
  __shared__ float red_r[kWaves][kTileJ];      // sum_b e over the pairs that carry a gradient
  __shared__ float red_g[kWaves][kTileJ];      // sum_b e over all pairs (G)
  __shared__ int is_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int s = blockIdx.y, z = blockIdx.z;
  const int64_t a0 = (int64_t)blockIdx.x * kTileJ;
  const int64_t n_tiles = (batch + kTileJ - 1) / kTileJ;
  const int n_chunks = (d + kKC - 1) / kKC;
  const float* X = xhat + (int64_t)s * batch * d;
  const float* N2 = sqn + (int64_t)s * batch;
  const int32_t* ID = row_id + (int64_t)s * batch;
  const int64_t a = a0 + l32;
  const float na = a < batch ? N2[a] : 0.f;
  const int32_t ida = a < batch ? ID[a] : -2;
  const int kw_z = min(kKC, d - z * kKC);                    // columns of this workgroup's o slice

  auto load_row_chunk = [&](int kc) {                        // all 256 threads: rows a0.. of chunk kc
    const int kw = min(kKC, d - kc * kKC);
    for (int i = tid; i < kTileJ * kw; i += 256) {
      const int row = i / kw, c = i - row * kw;
      const int64_t ar = a0 + row;
      rowt[row * kStride + c] = ar < batch ? X[ar * d + kc * kKC + c] : 0.f;
    }
  };
  if (n_chunks == 1) load_row_chunk(0);                      // stays resident

  f32x16 oacc[2];
#pragma unroll
  for (int ch = 0; ch < 2; ++ch)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[ch][r] = 0.f;
  float r_run = 0.f, g_run = 0.f;

  const int64_t n_iter = (n_tiles + kWaves - 1) / kWaves;
  for (int64_t it = 0; it < n_iter; ++it) {
    const int64_t jt = it * kWaves + wave;
    const bool active = jt < n_tiles;
    const int64_t b0 = jt * kTileJ;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int q = 0; q < n_chunks; ++q) {
      const int kc = (z + 1 + q) % n_chunks;                 // this slice's own chunk comes last and stays in colt
      const int kw = min(kKC, d - kc * kKC);
      __syncthreads();                                       // everyone is done with the previous chunk
      if (n_chunks > 1) load_row_chunk(kc);
      for (int i = lane; i < kTileJ * kw; i += 64) {
        const int row = i / kw, c = i - row * kw;
        const int64_t br = b0 + row;
        colt[wave][row * kStride + c] = (active && br < batch) ? X[br * d + kc * kKC + c] : 0.f;
      }
      __syncthreads();
      const float* ap = &colt[wave][l32 * kStride + h];
      const float* bp = &rowt[l32 * kStride + h];
      for (int k = 0; k < kw; k += 2)                        // T^T: M = column-tile row b, N = row-tile row a
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], bp[k], acc, 0, 0, 0);
    }
    // e for the 16 pairs of this lane: (a = a0 + l32, b = b0 + acc_row(r, h))
    float rsum = 0.f, gsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t b = b0 + acc_row(r, h);
      const bool live = active && b < batch && a < batch && a != b;
      const float nb = live ? N2[b] : 0.f;
      const bool same = live && ID[b] == ida;              // one table row at two positions: distance 0, no gradient
      const float dist2 = na + nb - 2.0f * acc[r];
      const float e = live ? (same ? 1.0f : expf(-t * dist2)) : 0.f;
      gsum += e;
      acc[r] = same ? 0.f : e;
      rsum += acc[r];
    }
    r_run += rsum;
    g_run += gsum;
    if (WANT_O) {
      // o^T[c][a] += sum_b x^[b][c] e[b][a]: k-step r of the product takes b = acc_row(r, h) — exactly the rows this
      // lane's accumulator register r holds — so acc[r] IS the B operand
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) {
        if (ch * 32 < kw_z) {
          const int c = ch * 32 + l32;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float xv = c < kw_z ? colt[wave][acc_row(r, h) * kStride + c] : 0.f;
            oacc[ch] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, acc[r], oacc[ch], 0, 0, 0);
          }
        }
      }
    }
  }

  // the four waves' partials, added in wave order
  r_run += __shfl_xor(r_run, 32, GCR_WAVE);
  g_run += __shfl_xor(g_run, 32, GCR_WAVE);
  if (h == 0) {
    red_r[wave][l32] = r_run;
    red_g[wave][l32] = g_run;
  }
  __syncthreads();                                           // also: every wave is done reading colt
  if (z == 0 && wave == 0) {
    float gt = 0.f;
    if (h == 0 && a < batch) {
      gt = ((red_g[0][l32] + red_g[1][l32]) + red_g[2][l32]) + red_g[3][l32];
      if (WANT_O) r_out[(int64_t)s * batch + a] = ((red_r[0][l32] + red_r[1][l32]) + red_r[2][l32]) + red_r[3][l32];
    }
    const float tile_sum = gcr_wave_sum(gt);
    if (lane == 0) r_part[(int64_t)s * n_tiles + blockIdx.x] = tile_sum;
  }
  if (WANT_O) {
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      if (ch * 32 < kw_z) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = ch * 32 + acc_row(r, h);
          if (c < kw_z) colt[wave][l32 * kStride + c] = oacc[ch][r];
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < kTileJ * kw_z; i += 256) {
      const int row = i / kw_z, c = i - row * kw_z;
      const int o = row * kStride + c;
      const float v = ((colt[0][o] + colt[1][o]) + colt[2][o]) + colt[3][o];
      const int64_t ar = a0 + row;
      if (ar < batch) o_out[((int64_t)s * batch + ar) * d + z * kKC + c] = v;
    }
  }

  // the last workgroup to finish folds the partials into the eight sums, in a fixed order
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const unsigned total = gridDim.x * gridDim.y * gridDim.z;
    is_last = atomicAdd(ticket, 1u) == total - 1u;
  }
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  for (int k = wave; k < 8; k += kWaves) {
    double sum = 0.0;
    if (k >= 2 && k < 5) {                                   // G_s = 1/2 sum_a sum_{b != a} e_ab
      const int gs = k - 2;
      if (gs < n_sets)
        for (int64_t i = lane; i < n_tiles; i += 64)
          sum += (double)__hip_atomic_load(r_part + (int64_t)gs * n_tiles + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sum *= 0.5;
    } else {
      const int col = k < 2 ? k : k - 3;                     // A_pos, A_neg | Q_u, Q_p, Q_n
      for (int i = lane; i < prep_blocks; i += 64) sum += (double)prep_part[(int64_t)i * kPrepVals + col];
    }
    sum = gcr_wave_sum_f64(sum);
    if (lane == 0) sums[k] = (float)sum;
  }
}

template <int NV>
__global__ __launch_bounds__(256) void au_bwd_kernel(AuSets S, int d, int64_t batch, int n_sets, float t,
                                                     const float* __restrict__ inv_norm, const float* __restrict__ r_in,
                                                     const float* __restrict__ o_in, const float* __restrict__ g_sums,
                                                     float* __restrict__ g_user, float* __restrict__ g_item) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float g_a[3] = {0.f, 2.f * g_sums[0], 2.f * g_sums[1]};                          // d |x^_u - x^_s|^2 = 2 (..)
  const float g_g[3] = {-2.f * t * g_sums[2], -2.f * t * g_sums[3], -2.f * t * g_sums[4]};
  const float g_q[3] = {2.f * g_sums[5], 2.f * g_sums[6], 2.f * g_sums[7]};
  for (int64_t b = (int64_t)blockIdx.x * kWaves + wave; b < batch; b += (int64_t)gridDim.x * kWaves) {
    float x[3][NV], xh[3][NV], inv[3];
    int64_t row[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      row[s] = s < n_sets ? au_row(S, s, b) : -1;
      inv[s] = s < n_sets ? inv_norm[(int64_t)s * batch + b] : 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = lane + 64 * v;
        x[s][v] = (row[s] >= 0 && c < d) ? S.tab[s][row[s] * d + c] : 0.f;
        xh[s][v] = x[s][v] * inv[s];
      }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (s >= n_sets || row[s] < 0) continue;              // wave-uniform
      const float rr = r_in[(int64_t)s * batch + b];
      float gh[NV], dot = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = lane + 64 * v;
        const float ov = c < d ? o_in[((int64_t)s * batch + b) * d + c] : 0.f;
        float g = g_g[s] * (rr * xh[s][v] - ov);
        if (s == 0) {
          if (n_sets >= 2) g += g_a[1] * (xh[0][v] - xh[1][v]);
          if (n_sets >= 3) g += g_a[2] * (xh[0][v] - xh[2][v]);
        } else {
          g += g_a[s] * (xh[s][v] - xh[0][v]);
        }
        gh[v] = g;
        dot += xh[s][v] * g;
      }
      dot = gcr_wave_sum(dot);
      float* out = s == 0 ? g_user : g_item;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = lane + 64 * v;
        if (c < d) atomicAdd(out + row[s] * d + c, inv[s] * (gh[v] - xh[s][v] * dot) + g_q[s] * x[s][v]);
      }
    }
  }
}

int prep_blocks_for(int64_t batch) { return (int)gcr_grid((batch + kWaves - 1) / kWaves, kMaxPrepBlocks); }

struct AuWorkspace {
  int64_t xhat, sqn, row_id, prep_part, r_part, ticket, total;      // offsets in floats (4-byte words)
};

AuWorkspace au_layout(int64_t batch, int d) {
  AuWorkspace w;
  WsCarve c;
  const int64_t n_tiles = (batch + kTileJ - 1) / kTileJ;
  w.xhat = c.take(3 * batch * d);
  w.sqn = c.take(3 * batch);
  w.row_id = c.take(3 * batch);
  w.prep_part = c.take((int64_t)kMaxPrepBlocks * kPrepVals);
  w.r_part = c.take(3 * n_tiles);
  w.ticket = c.take(64);
  w.total = c.at;
  return w;
}

AuSets au_sets(const float* user_tab, const float* item_tab, const int64_t* u_idx, const int64_t* i_idx, const int64_t* j_idx,
               int64_t n_users, int64_t n_items) {
  AuSets S;
  S.tab[0] = user_tab; S.tab[1] = item_tab; S.tab[2] = item_tab;
  S.idx[0] = u_idx; S.idx[1] = i_idx; S.idx[2] = j_idx;
  S.n_rows[0] = n_users; S.n_rows[1] = n_items; S.n_rows[2] = n_items;
  return S;
}

bool au_args_ok(int32_t d, int64_t batch, int32_t n_sets, int64_t n_users, int64_t n_items) {
  return d >= 2 && d <= 512 && d % 2 == 0 && batch >= 1 && batch < (1ll << 24) && n_sets >= 1 && n_sets <= 3 && n_users >= 0 &&
         n_items >= 0 && n_users < (1ll << 31) && n_items < (1ll << 31);
}

}  // namespace

extern "C" int64_t gcr_directau_workspace_bytes(int64_t batch, int32_t d) {
  if (batch < 1 || d < 1) return 0;
  return au_layout(batch, d).total * (int64_t)sizeof(float);
}

extern "C" int32_t gcr_directau_fwd_f32(const float* user_tab, const float* item_tab, int32_t d, const int64_t* u_idx,
                                        const int64_t* i_idx, const int64_t* j_idx, int64_t batch, int32_t n_sets,
                                        int64_t n_users, int64_t n_items, float t, float* sums, float* inv_norm, float* r,
                                        float* o, void* workspace, void* stream) {
  GCR_CHECK_ARG(au_args_ok(d, batch, n_sets, n_users, n_items));
  GCR_CHECK_ARG(user_tab && sums && inv_norm && workspace && (n_sets == 1 || item_tab));
  GCR_CHECK_ARG((r != nullptr) == (o != nullptr));
  // an absent index vector addresses rows 0..batch-1 of its table
  GCR_CHECK_ARG(u_idx || n_users >= batch);
  GCR_CHECK_ARG(n_sets < 2 || i_idx || n_items >= batch);
  GCR_CHECK_ARG(n_sets < 3 || j_idx || n_items >= batch);
  hipStream_t s = (hipStream_t)stream;
  const AuWorkspace w = au_layout(batch, d);
  float* ws = reinterpret_cast<float*>(workspace);
  unsigned* ticket = reinterpret_cast<unsigned*>(ws + w.ticket);
  const AuSets S = au_sets(user_tab, item_tab, u_idx, i_idx, j_idx, n_users, n_items);
  const int pb = prep_blocks_for(batch);
  int32_t* row_id = reinterpret_cast<int32_t*>(ws + w.row_id);
  dispatch_columns<1, 2, 4, 8>(d, [&](auto nv) {
    hipLaunchKernelGGL((au_prepare_kernel<decltype(nv)::value>), dim3(pb), dim3(256), 0, s, S, (int)d, batch, (int)n_sets,
                       ws + w.xhat, inv_norm, ws + w.sqn, row_id, ws + w.prep_part, ticket);
  });
  int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  const unsigned n_tiles = (unsigned)((batch + kTileJ - 1) / kTileJ);
  if (o != nullptr) {
    const unsigned n_slices = (unsigned)((d + kKC - 1) / kKC);
    hipLaunchKernelGGL((au_tile_kernel<true>), dim3(n_tiles, (unsigned)n_sets, n_slices), dim3(256), 0, s, ws + w.xhat,
                       ws + w.sqn, row_id, (int)d, batch, (int)n_sets, t, r, o, ws + w.r_part, ws + w.prep_part, pb, ticket, sums);
  } else {
    hipLaunchKernelGGL((au_tile_kernel<false>), dim3(n_tiles, (unsigned)n_sets, 1), dim3(256), 0, s, ws + w.xhat,
                       ws + w.sqn, row_id, (int)d, batch, (int)n_sets, t, (float*)nullptr, (float*)nullptr, ws + w.r_part,
                       ws + w.prep_part, pb, ticket, sums);
  }
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_directau_bwd_f32(const float* user_tab, const float* item_tab, int32_t d, const int64_t* u_idx,
                                        const int64_t* i_idx, const int64_t* j_idx, int64_t batch, int32_t n_sets,
                                        int64_t n_users, int64_t n_items, float t, const float* inv_norm, const float* r,
                                        const float* o, const float* g_sums, float* g_user_tab, float* g_item_tab,
                                        void* stream) {
  GCR_CHECK_ARG(au_args_ok(d, batch, n_sets, n_users, n_items));
  GCR_CHECK_ARG(user_tab && inv_norm && r && o && g_sums && g_user_tab && (n_sets == 1 || (item_tab && g_item_tab)));
  GCR_CHECK_ARG(u_idx || n_users >= batch);
  GCR_CHECK_ARG(n_sets < 2 || i_idx || n_items >= batch);
  GCR_CHECK_ARG(n_sets < 3 || j_idx || n_items >= batch);
  const AuSets S = au_sets(user_tab, item_tab, u_idx, i_idx, j_idx, n_users, n_items);
  const unsigned blocks = (unsigned)gcr_grid((batch + kWaves - 1) / kWaves, 8192);
  dispatch_columns<1, 2, 4, 8>(d, [&](auto nv) {
    hipLaunchKernelGGL((au_bwd_kernel<decltype(nv)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, S, (int)d, batch,
                       (int)n_sets, t, inv_norm, r, o, g_sums, g_user_tab, g_item_tab);
  });
  return GCR_LAUNCH_STATUS();
}
