// One GIN layer of BGRL's encoder (torch_geometric's GINConv over Sequential(Linear, ReLU, Linear), then ReLU and F.dropout:
// bgrl_g2l.py:500-505, 525-529) behind the sum aggregation, as one kernel forward and one backward:
//     t = relu(s w1^T + b1),   h = keep * keep_scale * relu(t w2^T + b2),   s = (1 + eps) x + A x from the caller (the tuned SpMM)
// which composed in torch is two GEMMs, two bias adds, two ReLUs and a dropout over all n nodes, with the hidden activation,
// both pre-activations and a mask kept for autograd.  gcr_sage.hip's layer with a second product chained behind the first:
// a workgroup of four waves walks tiles of ROWS rows;
//   phase 1  copies the s rows into an LDS tile S [ROWS][DIN] (coalesced);
//   phase 2  the f32 MFMA (v_mfma_f32_32x32x2_f32, exact f32 products; gcr_tile.h's accumulator layout) multiplies S by
//            w1^T [DIN, DOUT], adds b1, applies the ReLU and leaves t in a second LDS tile T [ROWS][DOUT]: t never reaches
//            memory;
//   phase 3  multiplies T by w2^T [DOUT, DOUT]; the epilogue adds b2, applies the ReLU and the keep bit and writes h.
// Both weights are transposed once per call into the workspace, so that the B operand's reads are coalesced.
// The backward rebuilds S, recomputes T with the forward's own loop (`hidden_tile`: the same products in the same order,
// so the inner ReLU's mask is the forward's, bit for bit), builds M [ROWS][DOUT] = g * keep_scale where h > 0 (a dropped
// element has h == 0 and gets no gradient either way) and gives
//   U = (M w2) where t > 0  (a third tile),   ds = U w1  (the host finishes dx = (1 + eps) ds + A^T ds with the SpMM; skipped
//   when nobody wants it),   dw2 += M^T T,  db2 += column sums of M,   dw1 += U^T S,  db1 += column sums of U
// with the 32 x 32 accumulators of dw1 and dw2 and the bias sums held across the workgroup's tiles, written once per
// workgroup and folded in workgroup order by gcr_fold_partials4: no atomics, bitwise reproducible.
// LDS rows are padded by two words (gcr_diffuse.hip's bank rule).  LDS budget (of a CU's 160 KB), forward / backward:
//   tiles: forward ROWS = 64 for dout <= 64 and 32 for dout = 128 (every wave owns a 32 x 32 tile of the second product from
//          dout = 64 on): (ROWS (DIN + DOUT + 4)) words, 17 - 50 KB;  backward ROWS = 32, four tiles: 32 (DIN + 3 DOUT + 8)
//          words, 17 - 66 KB;
//   weights: w1^T and w2^T (backward: w1^T and w2) sit in LDS beside the tiles when (DIN + DOUT) DOUT <= 8192 words (32 KB:
//          every pair with dout = 32, and (32, 64), (64, 64)), so that two workgroups still share a CU; the other pairs
//          ((128, 64): 48 KB, dout = 128: 80 - 128 KB) read them through the caches, as gcr_sage.hip does from 64 KB on: both
//          weights beside the tiles would leave one workgroup per CU and every phase's latency exposed.
#include "gcr_host.h"
#include "gcr_lanes.h"
#include "gcr_tile.h"   // f32x16, acc_row

namespace {

// Workgroups of a launch, at most (gcr_sage.hip's reasoning: the phases of a tile are serial inside a workgroup, the CU
// overlaps them across workgroups).  The backward holds up to 128 accumulator registers and 66 KB of LDS, so two workgroups
// per CU are resident: 512.
constexpr int FWD_CAP = 1024;
constexpr int BWD_CAP = 512;      // also the number of partials of dw1, db1, dw2, db2 (at most 129 KB each)
constexpr int BWD_ROWS = 32;

__host__ __device__ constexpr int fwd_rows(int dout) { return dout <= 64 ? 64 : 32; }
__host__ __device__ constexpr bool w_in_lds(int din, int dout) { return (din + dout) * dout <= 8192; }

// position of element [k][n] in the LDS copy of a [rows, COLS] matrix (gcr_diffuse.hip): from 64 columns on, rows of odd k
// swap their 32-column halves, so that the B operand's two half-waves (k, k + 1) read 64 distinct banks
template <int COLS>
__device__ __forceinline__ int w_at(int k, int n) {
  return k * COLS + (COLS >= 64 ? (n ^ ((k & 1) << 5)) : n);
}

// bit (r, c) of the keep bitmap, bit index r * dout + c in int64
__device__ __forceinline__ bool kept(const uint32_t* __restrict__ keep, int64_t r, int dout, int c) {
  const int64_t at = r * dout + c;
  return (keep[at >> 5] >> (at & 31)) & 1u;
}

// S[lr][0 .. DIN) = s's row row0 + lr; rows past n are zero.  G = min(64, DIN) lanes per row, NV = DIN / G consecutive
// columns per lane; at DIN = 32 the half-waves take one row each.  Every load is issued before the first LDS store
// (gcr_sage.hip's fill_tile).
template <int DIN, int ROWS, int STRIDE>
__device__ __forceinline__ void fill_rows(float* __restrict__ S, const float* __restrict__ s, int64_t row0, int64_t n) {
  constexpr int G = DIN >= 64 ? 64 : 32, NV = DIN / G, RPW = 64 / G, IT = ROWS / (4 * RPW);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane % G, c0 = gl * NV, lr0 = wave * RPW + lane / G;
  float sv[IT][NV];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int64_t r = row0 + lr0 + it * 4 * RPW;
#pragma unroll
    for (int j = 0; j < NV; ++j) sv[it][j] = 0.f;
    if (r < n) {
#pragma unroll
      for (int j = 0; j < NV; ++j) sv[it][j] = s[r * DIN + c0 + j];
    }
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int lr = lr0 + it * 4 * RPW;
#pragma unroll
    for (int j = 0; j < NV; ++j) S[lr * STRIDE + c0 + j] = sv[it][j];
  }
}

// the 32 x 32 tile  A[32 rows][K] B[K][32 columns]:  a_row = A's row of this lane's column index (c32) plus hh in LDS,
// B [K][BCOLS] in LDS (bl, w_at's layout) or in memory (bg, row-major), col = this lane's column of B
template <int K, int BCOLS, bool B_LDS>
__device__ __forceinline__ f32x16 tile_ab(const float* __restrict__ a_row, const float* __restrict__ bl,
                                          const float* __restrict__ bg, int col, int hh) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
  for (int k = 0; k < K; k += 2) {
    const float a = a_row[k];
    const float b = B_LDS ? bl[w_at<BCOLS>(k + hh, col)] : bg[(k + hh) * BCOLS + col];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc += A^T B over the 32 rows of two LDS tiles: A's 32 columns from a_col, B's from b_col (each plus c32)
template <int AS, int BS>
__device__ __forceinline__ void tile_tn(f32x16& acc, const float* __restrict__ A, const float* __restrict__ B, int a_col,
                                        int b_col, int hh) {
#pragma unroll 8
  for (int r = 0; r < BWD_ROWS; r += 2) {
    const float a = A[(r + hh) * AS + a_col];
    const float b = B[(r + hh) * BS + b_col];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
}

// T = relu(S w1^T + b1) for a tile of ROWS rows, LDS to LDS: the one loop of the forward and of the backward's
// recomputation, so that both give every t the same bits whatever ROWS is (an element's k order does not depend on it)
template <int DIN, int DOUT, int ROWS, bool W_LDS>
__device__ __forceinline__ void hidden_tile(const float* __restrict__ S, const float* __restrict__ w1l,
                                            const float* __restrict__ w1g, const float* __restrict__ b1,
                                            float* __restrict__ T) {
  constexpr int SS = DIN + 2, TS = DOUT + 2, TN = DOUT / 32, NT = (ROWS / 32) * TN, PER_WAVE = (NT + 3) / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int t = 0; t < PER_WAVE; ++t) {
    const int ot = wave + 4 * t;
    if (ot < NT) {
      const int tm = ot / TN, tn = ot % TN, cc = 32 * tn + c32;
      const f32x16 acc = tile_ab<DIN, DOUT, W_LDS>(S + (32 * tm + c32) * SS + hh, w1l, w1g, cc, hh);
      const float bv = b1[cc];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[r] + bv;
        T[(32 * tm + acc_row(r, hh)) * TS + cc] = v < 0.f ? 0.f : v;
      }
    }
  }
}

// wt = [w1^T [din, dout]; w2^T [dout, dout]]: the B operands of the two chained products, coalesced
__global__ __launch_bounds__(256) void gin_wt_kernel(const float* __restrict__ w1, const float* __restrict__ w2, int din,
                                                     int dout, float* __restrict__ wt) {
  const int i = blockIdx.x * 256 + threadIdx.x;           // index into wt
  if (i < (din + dout) * dout) {
    const int k = i / dout, c = i % dout;
    wt[i] = k < din ? w1[c * din + k] : w2[c * dout + k - din];
  }
}

template <int DIN, int DOUT, bool W_LDS>
__global__ __launch_bounds__(256) void gin_fwd_kernel(int64_t n, const float* __restrict__ s, const float* __restrict__ wt,
                                                      const float* __restrict__ b1, const float* __restrict__ b2,
                                                      const uint32_t* __restrict__ keep, float keep_scale,
                                                      float* __restrict__ h) {
  constexpr int ROWS = fwd_rows(DOUT), SS = DIN + 2, TS = DOUT + 2, TN = DOUT / 32, NT = (ROWS / 32) * TN, PER_WAVE = (NT + 3) / 4;
  __shared__ float S[ROWS * SS];
  __shared__ float T[ROWS * TS];
  __shared__ float Wl[W_LDS ? (DIN + DOUT) * DOUT : 1];   // w1^T, then w2^T
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, hh = lane >> 5;
  if (W_LDS) {
    for (int i = threadIdx.x; i < DIN * DOUT; i += 256) Wl[w_at<DOUT>(i / DOUT, i % DOUT)] = wt[i];
    for (int i = threadIdx.x; i < DOUT * DOUT; i += 256) Wl[DIN * DOUT + w_at<DOUT>(i / DOUT, i % DOUT)] = wt[DIN * DOUT + i];
  }
  const int64_t ntiles = (n + ROWS - 1) / ROWS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * ROWS;
    // S is read by hidden_tile alone and T by the second product alone, each between two barriers of this trip, so the
    // next trip's fill (S) and hidden_tile (T, behind the fill's barrier) need no barrier at the loop's end
    fill_rows<DIN, ROWS, SS>(S, s, row0, n);
    __syncthreads();
    hidden_tile<DIN, DOUT, ROWS, W_LDS>(S, Wl, wt, b1, T);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PER_WAVE; ++t) {
      const int ot = wave + 4 * t;
      if (ot < NT) {
        const int tm = ot / TN, tn = ot % TN, cc = 32 * tn + c32;
        const f32x16 acc = tile_ab<DOUT, DOUT, W_LDS>(T + (32 * tm + c32) * TS + hh, Wl + DIN * DOUT, wt + DIN * DOUT, cc, hh);
        const float bv = b2[cc];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = row0 + 32 * tm + acc_row(r, hh);
          if (row < n) {
            float v = acc[r] + bv;
            v = v < 0.f ? 0.f : v;
            const bool on = keep == nullptr || kept(keep, row, DOUT, cc);
            h[row * DOUT + cc] = on ? v * keep_scale : 0.f;
          }
        }
      }
    }
  }
}

template <int DIN, int DOUT, bool W_LDS>
__global__ __launch_bounds__(256) void gin_bwd_kernel(int64_t n, const float* __restrict__ s, const float* __restrict__ w1,
                                                      const float* __restrict__ w2, const float* __restrict__ wt,
                                                      const float* __restrict__ b1, const float* __restrict__ h,
                                                      const float* __restrict__ g, float keep_scale, float* __restrict__ ds,
                                                      float* __restrict__ part) {
  constexpr int ROWS = BWD_ROWS, SS = DIN + 2, TS = DOUT + 2;
  constexpr int TN = DOUT / 32, KN = DIN / 32;
  constexpr int U_PER = (TN + 3) / 4, DS_PER = (KN + 3) / 4;            // U and ds: one row of 32 x 32 tiles each
  constexpr int DW2_NT = TN * TN, DW2_PER = (DW2_NT + 3) / 4;           // dw2 [DOUT][DOUT]
  constexpr int DW1_NT = TN * KN, DW1_PER = (DW1_NT + 3) / 4;           // dw1 [DOUT][DIN]
  constexpr int M_IT = ROWS * DOUT / 256, M_CHUNK = M_IT < 8 ? M_IT : 8;
  __shared__ float S[ROWS * SS];
  __shared__ float T[ROWS * TS];
  __shared__ float M[ROWS * TS];
  __shared__ float U[ROWS * TS];
  __shared__ float Wl[W_LDS ? (DIN + DOUT) * DOUT : 1];                 // w1^T [DIN][DOUT], then w2 [DOUT][DOUT]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, hh = lane >> 5;
  if (W_LDS) {
    for (int i = threadIdx.x; i < DIN * DOUT; i += 256) Wl[w_at<DOUT>(i / DOUT, i % DOUT)] = wt[i];
    for (int i = threadIdx.x; i < DOUT * DOUT; i += 256) Wl[DIN * DOUT + w_at<DOUT>(i / DOUT, i % DOUT)] = w2[i];
  }
  f32x16 dw2[DW2_PER], dw1[DW1_PER];
#pragma unroll
  for (int t = 0; t < DW2_PER; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dw2[t][r] = 0.f;
#pragma unroll
  for (int t = 0; t < DW1_PER; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dw1[t][r] = 0.f;
  float db2 = 0.f, db1 = 0.f;                                           // column threadIdx.x, threads below DOUT
  const int64_t ntiles = (n + ROWS - 1) / ROWS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * ROWS;
    fill_rows<DIN, ROWS, SS>(S, s, row0, n);
    {                                                                   // M = g keep_scale where h > 0; loads first
#pragma unroll 1
      for (int it0 = 0; it0 < M_IT; it0 += M_CHUNK) {
        float gv[M_CHUNK], hv[M_CHUNK];
#pragma unroll
        for (int it = 0; it < M_CHUNK; ++it) {
          const int i = threadIdx.x + 256 * (it0 + it);
          const int64_t r = row0 + i / DOUT;
          gv[it] = hv[it] = 0.f;
          if (r < n) {
            const int64_t at = r * DOUT + i % DOUT;
            gv[it] = g[at];
            hv[it] = h[at];
          }
        }
#pragma unroll
        for (int it = 0; it < M_CHUNK; ++it) {
          const int i = threadIdx.x + 256 * (it0 + it);
          M[(i / DOUT) * TS + i % DOUT] = hv[it] > 0.f ? gv[it] * keep_scale : 0.f;      // 0 in the rows past n
        }
      }
    }
    __syncthreads();
    hidden_tile<DIN, DOUT, ROWS, W_LDS>(S, Wl, wt, b1, T);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < U_PER; ++t) {                                   // U = (M w2) where t > 0
      const int tn = wave + 4 * t;
      if (tn < TN) {
        const int cc = 32 * tn + c32;
        const f32x16 acc = tile_ab<DOUT, DOUT, W_LDS>(M + c32 * TS + hh, Wl + DIN * DOUT, w2, cc, hh);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int at = acc_row(r, hh) * TS + cc;
          U[at] = T[at] > 0.f ? acc[r] : 0.f;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < DW2_PER; ++t) {                                 // dw2 += M^T T
      const int ot = wave + 4 * t;
      if (ot < DW2_NT) tile_tn<TS, TS>(dw2[t], M, T, 32 * (ot / TN) + c32, 32 * (ot % TN) + c32, hh);
    }
    if (threadIdx.x < DOUT) {
#pragma unroll 8
      for (int r = 0; r < ROWS; ++r) db2 += M[r * TS + threadIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < DW1_PER; ++t) {                                 // dw1 += U^T S
      const int ot = wave + 4 * t;
      if (ot < DW1_NT) tile_tn<TS, SS>(dw1[t], U, S, 32 * (ot / KN) + c32, 32 * (ot % KN) + c32, hh);
    }
    if (threadIdx.x < DOUT) {
#pragma unroll 8
      for (int r = 0; r < ROWS; ++r) db1 += U[r * TS + threadIdx.x];
    }
    if (ds != nullptr) {                                                // ds = U w1, w1 [DOUT][DIN] through the caches
#pragma unroll
      for (int t = 0; t < DS_PER; ++t) {
        const int tn = wave + 4 * t;
        if (tn < KN) {
          const int cc = 32 * tn + c32;
          const f32x16 acc = tile_ab<DOUT, DIN, false>(U + c32 * TS + hh, nullptr, w1, cc, hh);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + acc_row(r, hh);
            if (row < n) ds[row * DIN + cc] = acc[r];
          }
        }
      }
    }
    __syncthreads();                                                    // the next trip's fills write S and M
  }
  // one partial per workgroup: dw1 [DOUT][DIN], db1 [DOUT], dw2 [DOUT][DOUT], db2 [DOUT]
  float* dst = part + (int64_t)blockIdx.x * (DOUT * DIN + DOUT * DOUT + 2 * DOUT);
#pragma unroll
  for (int t = 0; t < DW1_PER; ++t) {
    const int ot = wave + 4 * t;
    if (ot < DW1_NT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(32 * (ot / KN) + acc_row(r, hh)) * DIN + 32 * (ot % KN) + c32] = dw1[t][r];
    }
  }
  float* dst2 = dst + DOUT * DIN + DOUT;
#pragma unroll
  for (int t = 0; t < DW2_PER; ++t) {
    const int ot = wave + 4 * t;
    if (ot < DW2_NT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) dst2[(32 * (ot / TN) + acc_row(r, hh)) * DOUT + 32 * (ot % TN) + c32] = dw2[t][r];
    }
  }
  if (threadIdx.x < DOUT) {
    dst[DOUT * DIN + threadIdx.x] = db1;
    dst2[DOUT * DOUT + threadIdx.x] = db2;
  }
}

// the workgroups' partials summed in workgroup order, four lanes per output
__global__ __launch_bounds__(256) void gin_reduce_kernel(const float* __restrict__ part, int nblocks, int din, int dout,
                                                         float* __restrict__ dw1, float* __restrict__ db1,
                                                         float* __restrict__ dw2, float* __restrict__ db2) {
  const int elems = dout * din + dout * dout + 2 * dout;
  const int k = blockIdx.x * 64 + (threadIdx.x >> 2);
  const int qd = threadIdx.x & 3;
  const float v = gcr_fold_partials4(part, nblocks, elems, k, qd, k < elems);
  if (k < elems && qd == 0) {
    int o = k;
    if (o < dout * din) dw1[o] = v;
    else if ((o -= dout * din) < dout) db1[o] = v;
    else if ((o -= dout) < dout * dout) dw2[o] = v;
    else db2[o - dout * dout] = v;
  }
}

int fwd_blocks(int64_t n, int dout) { return (int)gcr_grid((n + fwd_rows(dout) - 1) / fwd_rows(dout), FWD_CAP); }
int bwd_blocks(int64_t n) { return (int)gcr_grid((n + BWD_ROWS - 1) / BWD_ROWS, BWD_CAP); }
bool width_ok(int d) { return d == 32 || d == 64 || d == 128; }

// f(DIN, DOUT as integral constants) for a supported pair
template <class F>
void dispatch_pair(int din, int dout, F&& f) {
  dispatch_value<32, 64, 128>(din, [&](auto a) { dispatch_value<32, 64, 128>(dout, [&](auto b) { f(a, b); }); });
}

int32_t launch_wt(const float* w1, const float* w2, int din, int dout, float* wt, hipStream_t s) {
  const int elems = (din + dout) * dout;
  hipLaunchKernelGGL(gin_wt_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, w1, w2, din, dout, wt);
  return GCR_LAUNCH_STATUS();
}

}  // namespace

extern "C" int32_t gcr_gin_supported(int32_t din, int32_t dout) { return width_ok(din) && width_ok(dout); }

extern "C" int64_t gcr_gin_workspace_bytes(int64_t n, int32_t din, int32_t dout) {
  if (n <= 0 || !gcr_gin_supported(din, dout)) return 0;
  const int64_t w = ((int64_t)din + dout) * dout;                       // [w1^T; w2^T], then the partials
  return (w + (int64_t)bwd_blocks(n) * (w + 2 * dout)) * (int64_t)sizeof(float);
}

extern "C" int32_t gcr_gin_fwd_f32(int64_t n, const float* s, const float* w1, const float* b1, const float* w2,
                                   const float* b2, int32_t din, int32_t dout, const uint32_t* keep_bits, float keep_scale,
                                   float* h, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0 && gcr_gin_supported(din, dout));
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(s != nullptr && w1 != nullptr && b1 != nullptr && w2 != nullptr && b2 != nullptr && h != nullptr &&
                workspace != nullptr && h != s && aligned16(s, w1, b1, w2, b2, h, workspace) && aligned16(keep_bits));
  hipStream_t st = (hipStream_t)stream;
  float* wt = reinterpret_cast<float*>(workspace);
  const int32_t rc = launch_wt(w1, w2, din, dout, wt, st);
  if (rc != GCR_OK) return rc;
  const dim3 grid((unsigned)fwd_blocks(n, dout));
  dispatch_pair(din, dout, [&](auto a, auto b) {
    constexpr int DIN = decltype(a)::value, DOUT = decltype(b)::value;
    hipLaunchKernelGGL((gin_fwd_kernel<DIN, DOUT, w_in_lds(DIN, DOUT)>), grid, dim3(256), 0, st, n, s, (const float*)wt, b1, b2,
                       keep_bits, keep_scale, h);
  });
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_gin_bwd_f32(int64_t n, const float* s, const float* w1, const float* b1, const float* w2,
                                   const float* h, const float* g, int32_t din, int32_t dout, float keep_scale, float* ds,
                                   float* dw1, float* db1, float* dw2, float* db2, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0 && gcr_gin_supported(din, dout));
  GCR_CHECK_ARG(dw1 != nullptr && db1 != nullptr && dw2 != nullptr && db2 != nullptr && aligned16(dw1, db1, dw2, db2));
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    const size_t f = sizeof(float);
    int32_t rc = gcr_hip_status(hipMemsetAsync(dw1, 0, f * (size_t)din * (size_t)dout, st));
    if (rc == GCR_OK) rc = gcr_hip_status(hipMemsetAsync(db1, 0, f * (size_t)dout, st));
    if (rc == GCR_OK) rc = gcr_hip_status(hipMemsetAsync(dw2, 0, f * (size_t)dout * (size_t)dout, st));
    if (rc == GCR_OK) rc = gcr_hip_status(hipMemsetAsync(db2, 0, f * (size_t)dout, st));
    return rc;
  }
  GCR_CHECK_ARG(s != nullptr && w1 != nullptr && b1 != nullptr && w2 != nullptr && h != nullptr && g != nullptr &&
                workspace != nullptr && aligned16(s, w1, b1, w2, h, g, workspace) && aligned16(ds));
  GCR_CHECK_ARG(ds != s && ds != h && ds != g);
  float* wt = reinterpret_cast<float*>(workspace);
  float* part = wt + ((int64_t)din + dout) * dout;
  int32_t rc = launch_wt(w1, w2, din, dout, wt, st);
  if (rc != GCR_OK) return rc;
  const int nb = bwd_blocks(n);
  dispatch_pair(din, dout, [&](auto a, auto b) {
    constexpr int DIN = decltype(a)::value, DOUT = decltype(b)::value;
    hipLaunchKernelGGL((gin_bwd_kernel<DIN, DOUT, w_in_lds(DIN, DOUT)>), dim3((unsigned)nb), dim3(256), 0, st, n, s, w1, w2,
                       (const float*)wt, b1, h, g, keep_scale, ds, part);
  });
  rc = GCR_LAUNCH_STATUS();
  if (rc != GCR_OK) return rc;
  const int elems = (din + dout) * dout + 2 * dout;
  hipLaunchKernelGGL(gin_reduce_kernel, dim3((unsigned)((elems + 63) / 64)), dim3(256), 0, st, (const float*)part, nb, (int)din,
                     (int)dout, dw1, db1, dw2, db2);
  return GCR_LAUNCH_STATUS();
}
