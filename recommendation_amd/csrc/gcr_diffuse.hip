// DiffNet's social-diffusion layer (univariate/diffnet.py:1127-1130) as one kernel forward and one backward:
//     Z = S x;  h = relu([Z | x] W),  W = [W_top; W_bot] [2d, d]
// which the reference runs as sparse.mm, cat, matmul and relu over ALL users on every batch (about ten [U, d] passes
// through HBM per layer and a [U, 2d] tensor kept for autograd).  Here a workgroup of four waves walks tiles of ROWS rows:
//   phase 1  each wave sums its rows of S x (the row's entries in stored order, eight gathers in flight) into an LDS tile
//            T [ROWS][2d] next to the coalesced x rows (or copies a precomputed z there);
//   phase 2  the f32 MFMA (v_mfma_f32_32x32x2_f32, exact f32 products; operand layout as gcr_dense.hip's gram comment)
//            multiplies the tile by W and the epilogue writes relu.
// The backward rebuilds T the same way (Z is never saved), masks g by h > 0 into a second tile M [ROWS][d], and gives
//   [p | q] = M W^T   (the host finishes dx = S^T p + q with the SpMM),   dw += T^T M
// with dw's 32 x 32 accumulators held across the workgroup's tiles, written once per workgroup and folded in workgroup
// order by gcr_fold_partials4: no atomics, bitwise reproducible.
// LDS rows are padded by two words: the A operand's reads (32 rows of one column, the k pair in the half-waves) then
// fall on 64 distinct banks.  W sits in LDS for d <= 64 (8 / 32 KB, `w_at`) and is read through the caches at d = 128
// (128 KB does not fit next to the tile).
#include "gcr_host.h"
#include "gcr_lanes.h"
#include "gcr_tile.h"   // f32x16

namespace {

constexpr int FWD_CAP = 512;      // workgroups of a launch, at most (two per CU)

__host__ __device__ constexpr int fwd_rows(int d) { return d <= 64 ? 64 : 32; }
constexpr int BWD_ROWS = 32;
__host__ __device__ constexpr int bwd_cap(int d) { return d <= 64 ? 512 : 256; }

// position of element [k][n] in the LDS copy of a [rows, COLS] matrix: from 64 columns on, rows of odd k swap their 32-column
// halves, so that the B operand's two half-waves (k, k + 1) read 64 distinct banks (32 columns alternate by themselves)
template <int COLS>
__device__ __forceinline__ int w_at(int k, int n) {
  return k * COLS + (COLS >= 64 ? (n ^ ((k & 1) << 5)) : n);
}

// T[lr][0 .. D) = (S x)[row0 + lr] or z's row, T[lr][D .. 2 D) = x's row; rows past n are zero.  G = min(64, D) lanes per
// row, NV = D / G consecutive columns per lane; at D = 32 the half-waves take one row each.
template <int D, int ROWS, int STRIDE>
__device__ __forceinline__ void fill_tile(float* __restrict__ T, const int64_t* __restrict__ rowptr,
                                          const int32_t* __restrict__ col, const float* __restrict__ val,
                                          const float* __restrict__ x, const float* __restrict__ z, int64_t row0, int64_t n) {
  constexpr int G = D >= 64 ? 64 : 32, NV = D / G, RPW = 64 / G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane % G, c0 = gl * NV;
  for (int lr = wave * RPW + lane / G; lr < ROWS; lr += 4 * RPW) {
    const int64_t r = row0 + lr;
    float zv[NV], xv[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) zv[j] = xv[j] = 0.f;
    if (r < n) {
#pragma unroll
      for (int j = 0; j < NV; ++j) xv[j] = x[r * D + c0 + j];
      if (z != nullptr) {
#pragma unroll
        for (int j = 0; j < NV; ++j) zv[j] = z[r * D + c0 + j];
      } else {
        int64_t e = rowptr[r];
        const int64_t e1 = rowptr[r + 1];
        for (; e + 8 <= e1; e += 8) {
          int32_t c[8];
          float v[8], g[8][NV];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            c[u] = col[e + u];
            v[u] = val != nullptr ? val[e + u] : 1.f;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < NV; ++j) g[u][j] = x[(int64_t)c[u] * D + c0 + j];
#pragma unroll
          for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < NV; ++j) zv[j] = fmaf(v[u], g[u][j], zv[j]);
        }
        for (; e < e1; ++e) {
          const int64_t c = col[e];
          const float v = val != nullptr ? val[e] : 1.f;
#pragma unroll
          for (int j = 0; j < NV; ++j) zv[j] = fmaf(v, x[c * D + c0 + j], zv[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      T[lr * STRIDE + c0 + j] = zv[j];
      T[lr * STRIDE + D + c0 + j] = xv[j];
    }
  }
}

template <int D, bool W_LDS>
__global__ __launch_bounds__(256) void diffuse_fwd_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const float* __restrict__ val, int64_t n, const float* __restrict__ x,
                                                          const float* __restrict__ z, const float* __restrict__ w,
                                                          float* __restrict__ h) {
  constexpr int ROWS = fwd_rows(D), K = 2 * D, STRIDE = K + 2, TN = D / 32, NT = (ROWS / 32) * TN, PER_WAVE = (NT + 3) / 4;
  __shared__ float T[ROWS * STRIDE];
  __shared__ float Wl[W_LDS ? K * D : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, hh = lane >> 5;
  if (W_LDS)
    for (int i = threadIdx.x; i < K * D; i += 256) Wl[w_at<D>(i / D, i % D)] = w[i];
  const int64_t ntiles = (n + ROWS - 1) / ROWS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * ROWS;
    fill_tile<D, ROWS, STRIDE>(T, rowptr, col, val, x, z, row0, n);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PER_WAVE; ++t) {
      const int ot = wave + 4 * t;
      if (ot < NT) {
        const int tm = ot / TN, tn = ot % TN;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* a_row = T + (32 * tm + c32) * STRIDE + hh;
#pragma unroll 8
        for (int k = 0; k < K; k += 2) {
          const float a = a_row[k];
          const float b = W_LDS ? Wl[w_at<D>(k + hh, 32 * tn + c32)] : w[(k + hh) * D + 32 * tn + c32];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = row0 + 32 * tm + (r & 3) + 8 * (r >> 2) + 4 * hh;     // C layout of the 32 x 32 accumulator
          const float v = acc[r];
          if (row < n) h[row * D + 32 * tn + c32] = v < 0.f ? 0.f : v;
        }
      }
    }
    __syncthreads();
  }
}

// wt [D, 2 D] = w^T: the backward's B operand of [p | q] = M W^T, coalesced
__global__ __launch_bounds__(256) void transpose_w_kernel(const float* __restrict__ w, int d, float* __restrict__ wt) {
  const int i = blockIdx.x * 256 + threadIdx.x;           // index into wt
  if (i < 2 * d * d) wt[i] = w[(i % (2 * d)) * d + i / (2 * d)];
}

template <int D, bool W_LDS>
__global__ __launch_bounds__(256) void diffuse_bwd_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const float* __restrict__ val, int64_t n, const float* __restrict__ x,
                                                          const float* __restrict__ z, const float* __restrict__ wt,
                                                          const float* __restrict__ h, const float* __restrict__ g,
                                                          float* __restrict__ p, float* __restrict__ q,
                                                          float* __restrict__ part) {
  constexpr int ROWS = BWD_ROWS, K = 2 * D, STRIDE = K + 2, MS = D + 2;
  constexpr int PQ_NT = K / 32, PQ_PER = (PQ_NT + 3) / 4;               // [p | q]: one row of 32 x 32 tiles
  constexpr int DW_TN = D / 32, DW_NT = (K / 32) * DW_TN, DW_PER = (DW_NT + 3) / 4;
  __shared__ float T[ROWS * STRIDE];
  __shared__ float M[ROWS * MS];
  __shared__ float Wl[W_LDS ? D * K : 1];                               // W^T [D][2 D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, hh = lane >> 5;
  if (W_LDS)
    for (int i = threadIdx.x; i < D * K; i += 256) Wl[w_at<K>(i / K, i % K)] = wt[i];
  f32x16 dw[DW_PER];
#pragma unroll
  for (int t = 0; t < DW_PER; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dw[t][r] = 0.f;
  const int64_t ntiles = (n + ROWS - 1) / ROWS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * ROWS;
    fill_tile<D, ROWS, STRIDE>(T, rowptr, col, val, x, z, row0, n);
    for (int i = threadIdx.x; i < ROWS * D; i += 256) {                 // M = g where h > 0
      const int lr = i / D, c = i % D;
      const int64_t r = row0 + lr;
      float m = 0.f;
      if (r < n) m = h[r * D + c] > 0.f ? g[r * D + c] : 0.f;
      M[lr * MS + c] = m;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PQ_PER; ++t) {
      const int tn = wave + 4 * t;
      if (tn < PQ_NT) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* a_row = M + c32 * MS + hh;
#pragma unroll 8
        for (int k = 0; k < D; k += 2) {
          const float a = a_row[k];
          const float b = W_LDS ? Wl[w_at<K>(k + hh, 32 * tn + c32)] : wt[(k + hh) * K + 32 * tn + c32];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        const int cc = 32 * tn + c32;                                   // column of [p | q]
        float* dst = cc < D ? p : q;
        const int dc = cc < D ? cc : cc - D;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          if (row < n) dst[row * D + dc] = acc[r];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < DW_PER; ++t) {
      const int ot = wave + 4 * t;
      if (ot < DW_NT) {
        const int tm = ot / DW_TN, tn = ot % DW_TN;
#pragma unroll 8
        for (int r = 0; r < ROWS; r += 2) {
          const float a = T[(r + hh) * STRIDE + 32 * tm + c32];
          const float b = M[(r + hh) * MS + 32 * tn + c32];
          dw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, dw[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  float* dst = part + (int64_t)blockIdx.x * (K * D);
#pragma unroll
  for (int t = 0; t < DW_PER; ++t) {
    const int ot = wave + 4 * t;
    if (ot < DW_NT) {
      const int tm = ot / DW_TN, tn = ot % DW_TN;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
        dst[(32 * tm + row) * D + 32 * tn + c32] = dw[t][r];
      }
    }
  }
}

// dw[k] = sum over the workgroups' partials in workgroup order, four lanes per output
__global__ __launch_bounds__(256) void diffuse_dw_reduce_kernel(const float* __restrict__ part, int nblocks, int elems,
                                                                float* __restrict__ out) {
  const int k = blockIdx.x * 64 + (threadIdx.x >> 2);
  const int qd = threadIdx.x & 3;
  const float s = gcr_fold_partials4(part, nblocks, elems, k, qd, k < elems);
  if (k < elems && qd == 0) out[k] = s;
}

int fwd_blocks(int64_t n, int d) { return (int)gcr_grid((n + fwd_rows(d) - 1) / fwd_rows(d), FWD_CAP); }
int bwd_blocks(int64_t n, int d) { return (int)gcr_grid((n + BWD_ROWS - 1) / BWD_ROWS, bwd_cap(d)); }

}  // namespace

extern "C" int32_t gcr_diffuse_supported(int32_t d) { return d == 32 || d == 64 || d == 128; }

extern "C" int64_t gcr_diffuse_workspace_bytes(int64_t n, int32_t d) {
  if (n <= 0 || !gcr_diffuse_supported(d)) return 0;
  return (int64_t)(1 + bwd_blocks(n, d)) * 2 * d * d * (int64_t)sizeof(float);      // W^T, then the partials of dw
}

extern "C" int32_t gcr_diffuse_fwd_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n, const float* x,
                                       const float* z, const float* w, int32_t d, float* h, void* stream) {
  GCR_CHECK_ARG(n >= 0 && gcr_diffuse_supported(d));
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(x != nullptr && w != nullptr && h != nullptr && h != x && aligned16(x, z, w, h));
  GCR_CHECK_ARG(z != nullptr || (rowptr != nullptr && col != nullptr));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)fwd_blocks(n, d));
  dispatch_value<32, 64, 128>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    hipLaunchKernelGGL((diffuse_fwd_kernel<D, (D <= 64)>), grid, dim3(256), 0, s, rowptr, col, val, n, x, z, w, h);
  });
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_diffuse_bwd_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n, const float* x,
                                       const float* z, const float* w, const float* h, const float* g, int32_t d, float* p,
                                       float* q, float* dw, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0 && gcr_diffuse_supported(d) && dw != nullptr && aligned16(dw));
  hipStream_t s = (hipStream_t)stream;
  const int elems = 2 * d * d;
  if (n == 0) return gcr_hip_status(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)elems, s));
  GCR_CHECK_ARG(x != nullptr && w != nullptr && h != nullptr && g != nullptr && p != nullptr && q != nullptr &&
                workspace != nullptr && aligned16(x, z, w, h, g, p, q, workspace));
  GCR_CHECK_ARG(z != nullptr || (rowptr != nullptr && col != nullptr));
  float* wt = reinterpret_cast<float*>(workspace);
  float* part = wt + elems;
  const int nb = bwd_blocks(n, d);
  hipLaunchKernelGGL(transpose_w_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, w, (int)d, wt);
  int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  dispatch_value<32, 64, 128>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    hipLaunchKernelGGL((diffuse_bwd_kernel<D, (D <= 64)>), dim3((unsigned)nb), dim3(256), 0, s, rowptr, col, val, n, x, z,
                       (const float*)wt, h, g, p, q, part);
  });
  st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  hipLaunchKernelGGL(diffuse_dw_reduce_kernel, dim3((unsigned)((elems + 63) / 64)), dim3(256), 0, s, (const float*)part, nb,
                     elems, dw);
  return GCR_LAUNCH_STATUS();
}
