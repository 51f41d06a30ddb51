// One GraphSAGE layer (torch_geometric's SAGEConv with mean aggregation, root weight and bias, as graphsage.py:21-30 uses
// it: conv, activation, F.dropout) as one kernel forward and one backward:
//     h = keep * keep_scale * act(z wl^T + x wr^T + bias),   z = mean_j x_j from the caller (the tuned SpMM)
// which composed in torch is two GEMMs, an add, a bias, an activation and a dropout over all n nodes, with z wl^T + ...,
// the activation's output and a mask kept for autograd.  gcr_diffuse.hip's layer with rectangular widths (DIN, DOUT
// independent), a bias and a selectable epilogue: a workgroup of four waves walks tiles of ROWS rows;
//   phase 1  copies the z and x rows into an LDS tile T [ROWS][2 DIN] (coalesced);
//   phase 2  the f32 MFMA (v_mfma_f32_32x32x2_f32, exact f32 products; operand layout as gcr_dense.hip's gram comment)
//            multiplies the tile by W = [wl^T; wr^T] [2 DIN, DOUT] (transposed once per call into the workspace, so that the
//            B operand's reads are coalesced) and the epilogue adds the bias, applies the activation and the keep bit and
//            writes h (and the pre-activation under gelu, whose derivative needs it).
// The backward rebuilds T from z and x, builds M [ROWS][DOUT] = g * keep * keep_scale * act'(pre) in a second tile (relu
// reads its mask from h > 0: a dropped element has h == 0 and gets no gradient either way) and gives
//   [p | q] = M [wl | wr]   (the host finishes dx = A^T p + q with the SpMM; skipped when nobody wants dx),
//   [dwl | dwr] += M^T T,   dbias += column sums of M
// with the 32 x 32 accumulators of [dwl | dwr] and dbias's sums held across the workgroup's tiles, written once per
// workgroup and folded in workgroup order by gcr_fold_partials4: no atomics, bitwise reproducible.
// LDS rows are padded by two words (gcr_diffuse.hip's bank rule).  W sits in LDS next to the tile when DIN * DOUT <= 4096
// (at most 32 KB: with the 33 KB tile two workgroups still share a CU's 160 KB) and is read through the caches otherwise
// ((64, 128) and (128, 64): 64 KB, (128, 128): 128 KB; four such workgroups share a CU).
#include "gcr_host.h"
#include "gcr_lanes.h"
#include "gcr_tile.h"   // f32x16

namespace {

// Workgroups of a launch, at most: four per CU.  A tile's phases (fill, product, epilogue) are serial inside a workgroup, so
// the CU overlaps them across workgroups: as many as LDS (33 - 70 KB each) and registers (2 - 4 waves per SIMD) admit are
// resident, the rest queue.  With 256 (one per CU, every latency exposed) the (64, 128) backward took 3.3 ms for 1.1M rows.
constexpr int FWD_CAP = 1024;
constexpr int BWD_CAP = 1024;     // also the number of partials of [dwl | dwr] and dbias (at most 129 KB each)
constexpr int BWD_ROWS = 32;
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2 };

__host__ __device__ constexpr int fwd_rows(int din) { return din <= 64 ? 64 : 32; }
__host__ __device__ constexpr bool w_in_lds(int din, int dout) { return din * dout <= 4096; }

// position of element [k][n] in the LDS copy of a [rows, COLS] matrix (gcr_diffuse.hip): from 64 columns on, rows of odd k
// swap their 32-column halves, so that the B operand's two half-waves (k, k + 1) read 64 distinct banks
template <int COLS>
__device__ __forceinline__ int w_at(int k, int n) {
  return k * COLS + (COLS >= 64 ? (n ^ ((k & 1) << 5)) : n);
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
// d/dv of gelu_erf: Phi(v) + v phi(v)
__device__ __forceinline__ float gelu_erf_grad(float v) {
  return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * __expf(-0.5f * v * v);
}

// bit (r, c) of the keep bitmap, bit index r * dout + c in int64
__device__ __forceinline__ bool kept(const uint32_t* __restrict__ keep, int64_t r, int dout, int c) {
  const int64_t at = r * dout + c;
  return (keep[at >> 5] >> (at & 31)) & 1u;
}

// T[lr][0 .. DIN) = z's row row0 + lr, T[lr][DIN .. 2 DIN) = x's row; rows past n are zero.  G = min(64, DIN) lanes per row,
// NV = DIN / G consecutive columns per lane; at DIN = 32 the half-waves take one row each.
template <int DIN, int ROWS, int STRIDE>
__device__ __forceinline__ void fill_tile(float* __restrict__ T, const float* __restrict__ x, const float* __restrict__ z,
                                          int64_t row0, int64_t n) {
  constexpr int G = DIN >= 64 ? 64 : 32, NV = DIN / G, RPW = 64 / G, IT = ROWS / (4 * RPW);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane % G, c0 = gl * NV, lr0 = wave * RPW + lane / G;
  // every load of the tile is issued before the first LDS store: a workgroup has one or two waves per SIMD, so the rows'
  // round trips must overlap each other (one row at a time, the tile's fill was a chain of IT memory latencies)
  float zv[IT][NV], xv[IT][NV];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int64_t r = row0 + lr0 + it * 4 * RPW;
#pragma unroll
    for (int j = 0; j < NV; ++j) zv[it][j] = xv[it][j] = 0.f;
    if (r < n) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        xv[it][j] = x[r * DIN + c0 + j];
        zv[it][j] = z[r * DIN + c0 + j];
      }
    }
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int lr = lr0 + it * 4 * RPW;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      T[lr * STRIDE + c0 + j] = zv[it][j];
      T[lr * STRIDE + DIN + c0 + j] = xv[it][j];
    }
  }
}

// wcat [2 din, dout] = [wl^T; wr^T]: the forward's B operand, coalesced
__global__ __launch_bounds__(256) void sage_wcat_kernel(const float* __restrict__ wl, const float* __restrict__ wr, int din,
                                                        int dout, float* __restrict__ wcat) {
  const int i = blockIdx.x * 256 + threadIdx.x;           // index into wcat
  if (i < 2 * din * dout) {
    const int k = i / dout, c = i % dout;
    wcat[i] = k < din ? wl[c * din + k] : wr[c * din + k - din];
  }
}

template <int DIN, int DOUT, bool W_LDS>
__global__ __launch_bounds__(256) void sage_fwd_kernel(int64_t n, const float* __restrict__ x, const float* __restrict__ z,
                                                       const float* __restrict__ wcat, const float* __restrict__ bias, int act,
                                                       const uint32_t* __restrict__ keep, float keep_scale,
                                                       float* __restrict__ h, float* __restrict__ pre) {
  constexpr int ROWS = fwd_rows(DIN), K = 2 * DIN, STRIDE = K + 2, TN = DOUT / 32, NT = (ROWS / 32) * TN, PER_WAVE = (NT + 3) / 4;
  __shared__ float T[ROWS * STRIDE];
  __shared__ float Wl[W_LDS ? K * DOUT : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, hh = lane >> 5;
  if (W_LDS)
    for (int i = threadIdx.x; i < K * DOUT; i += 256) Wl[w_at<DOUT>(i / DOUT, i % DOUT)] = wcat[i];
  const int64_t ntiles = (n + ROWS - 1) / ROWS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * ROWS;
    fill_tile<DIN, ROWS, STRIDE>(T, x, z, row0, n);
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
          const float b = W_LDS ? Wl[w_at<DOUT>(k + hh, 32 * tn + c32)] : wcat[(k + hh) * DOUT + 32 * tn + c32];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        const int cc = 32 * tn + c32;
        const float bv = bias != nullptr ? bias[cc] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = row0 + 32 * tm + (r & 3) + 8 * (r >> 2) + 4 * hh;     // C layout of the 32 x 32 accumulator
          if (row < n) {
            float v = acc[r] + bv;
            if (act == ACT_GELU) {
              pre[row * DOUT + cc] = v;
              v = gelu_erf(v);
            } else if (act == ACT_RELU) {
              v = v < 0.f ? 0.f : v;
            }
            const bool on = keep == nullptr || kept(keep, row, DOUT, cc);
            h[row * DOUT + cc] = on ? v * keep_scale : 0.f;
          }
        }
      }
    }
    __syncthreads();
  }
}

template <int DIN, int DOUT, bool W_LDS>
__global__ __launch_bounds__(256) void sage_bwd_kernel(int64_t n, const float* __restrict__ x, const float* __restrict__ z,
                                                       const float* __restrict__ wl, const float* __restrict__ wr,
                                                       const float* __restrict__ h, const float* __restrict__ pre,
                                                       const float* __restrict__ g, int act, const uint32_t* __restrict__ keep,
                                                       float keep_scale, float* __restrict__ p, float* __restrict__ q,
                                                       float* __restrict__ part) {
  constexpr int ROWS = BWD_ROWS, K = 2 * DIN, STRIDE = K + 2, MS = DOUT + 2;
  constexpr int PQ_NT = K / 32, PQ_PER = (PQ_NT + 3) / 4;               // [p | q]: one row of 32 x 32 tiles
  constexpr int DW_TN = K / 32, DW_NT = (DOUT / 32) * DW_TN, DW_PER = (DW_NT + 3) / 4;      // [dwl | dwr] [DOUT][2 DIN]
  constexpr int M_IT = ROWS * DOUT / 256, M_CHUNK = M_IT < 8 ? M_IT : 8;    // elements of M per thread, and per batch of loads
  __shared__ float T[ROWS * STRIDE];
  __shared__ float M[ROWS * MS];
  __shared__ float Wl[W_LDS ? DOUT * K : 1];                            // [wl | wr] [DOUT][2 DIN]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c32 = lane & 31, hh = lane >> 5;
  const bool want_pq = p != nullptr;
  if (W_LDS && want_pq)
    for (int i = threadIdx.x; i < DOUT * K; i += 256) {
      const int k = i / K, c = i % K;
      Wl[w_at<K>(k, c)] = c < DIN ? wl[k * DIN + c] : wr[k * DIN + c - DIN];
    }
  f32x16 dw[DW_PER];
#pragma unroll
  for (int t = 0; t < DW_PER; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dw[t][r] = 0.f;
  float db = 0.f;                                                       // dbias[threadIdx.x], threads below DOUT
  const int64_t ntiles = (n + ROWS - 1) / ROWS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * ROWS;
    fill_tile<DIN, ROWS, STRIDE>(T, x, z, row0, n);
    {                                                                   // M = g keep keep_scale act'(pre)
      // loads first, as in fill_tile.  aux is h (relu: the mask), pre (gelu) or g again (none: a second read of a line
      // already on its way, which keeps the loop free of branches); relu needs no keep bit (a dropped h is 0)
      const float* __restrict__ aux = act == ACT_RELU ? h : act == ACT_GELU ? pre : g;
      const bool bits = keep != nullptr && act != ACT_RELU;
#pragma unroll 1
      for (int it0 = 0; it0 < M_IT; it0 += M_CHUNK) {                   // eight loads of each kind in flight per lane
        float gv[M_CHUNK], av[M_CHUNK];
        uint32_t kw[M_CHUNK];
#pragma unroll
        for (int it = 0; it < M_CHUNK; ++it) {
          const int i = threadIdx.x + 256 * (it0 + it);
          const int64_t r = row0 + i / DOUT;
          gv[it] = av[it] = 0.f;
          kw[it] = ~0u;
          if (r < n) {
            const int64_t at = r * DOUT + i % DOUT;
            gv[it] = g[at];
            av[it] = aux[at];
            if (bits) kw[it] = keep[at >> 5] >> (at & 31);
          }
        }
#pragma unroll
        for (int it = 0; it < M_CHUNK; ++it) {
          const int i = threadIdx.x + 256 * (it0 + it);
          float m = gv[it] * keep_scale;                                // 0 in the rows past n
          if (act == ACT_RELU) m = av[it] > 0.f ? m : 0.f;
          else if (!(kw[it] & 1u)) m = 0.f;
          else if (act == ACT_GELU) m *= gelu_erf_grad(av[it]);
          M[(i / DOUT) * MS + i % DOUT] = m;
        }
      }
    }
    __syncthreads();
    if (want_pq) {
#pragma unroll
      for (int t = 0; t < PQ_PER; ++t) {
        const int tn = wave + 4 * t;
        if (tn < PQ_NT) {
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
          const float* a_row = M + c32 * MS + hh;
          const bool left = 32 * tn < DIN;                              // a 32-column tile lies in wl or in wr
          const float* wsrc = (left ? wl : wr) + (left ? 32 * tn : 32 * tn - DIN) + c32;
#pragma unroll 8
          for (int k = 0; k < DOUT; k += 2) {
            const float a = a_row[k];
            const float b = W_LDS ? Wl[w_at<K>(k + hh, 32 * tn + c32)] : wsrc[(k + hh) * DIN];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
          }
          float* dst = (left ? p : q) + (left ? 32 * tn : 32 * tn - DIN) + c32;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (row < n) dst[row * DIN] = acc[r];
          }
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
          const float a = M[(r + hh) * MS + 32 * tm + c32];
          const float b = T[(r + hh) * STRIDE + 32 * tn + c32];
          dw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, dw[t], 0, 0, 0);
        }
      }
    }
    if (threadIdx.x < DOUT) {
#pragma unroll 8
      for (int r = 0; r < ROWS; ++r) db += M[r * MS + threadIdx.x];
    }
    __syncthreads();
  }
  float* dst = part + (int64_t)blockIdx.x * (DOUT * K + DOUT);
#pragma unroll
  for (int t = 0; t < DW_PER; ++t) {
    const int ot = wave + 4 * t;
    if (ot < DW_NT) {
      const int tm = ot / DW_TN, tn = ot % DW_TN;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
        dst[(32 * tm + row) * K + 32 * tn + c32] = dw[t][r];
      }
    }
  }
  if (threadIdx.x < DOUT) dst[DOUT * K + threadIdx.x] = db;
}

// the workgroups' partials ([dout][2 din], then dbias [dout]) summed in workgroup order, four lanes per output
__global__ __launch_bounds__(256) void sage_dw_reduce_kernel(const float* __restrict__ part, int nblocks, int din, int dout,
                                                             float* __restrict__ dwl, float* __restrict__ dwr,
                                                             float* __restrict__ dbias) {
  const int elems = 2 * din * dout + dout;
  const int k = blockIdx.x * 64 + (threadIdx.x >> 2);
  const int qd = threadIdx.x & 3;
  const float s = gcr_fold_partials4(part, nblocks, elems, k, qd, k < elems);
  if (k < elems && qd == 0) {
    if (k < 2 * din * dout) {
      const int c = k / (2 * din), j = k % (2 * din);
      if (j < din) dwl[c * din + j] = s;
      else dwr[c * din + j - din] = s;
    } else if (dbias != nullptr) {
      dbias[k - 2 * din * dout] = s;
    }
  }
}

int fwd_blocks(int64_t n, int din) { return (int)gcr_grid((n + fwd_rows(din) - 1) / fwd_rows(din), FWD_CAP); }
int bwd_blocks(int64_t n) { return (int)gcr_grid((n + BWD_ROWS - 1) / BWD_ROWS, BWD_CAP); }
bool width_ok(int d) { return d == 32 || d == 64 || d == 128; }

// f(DIN, DOUT as integral constants) for a supported pair
template <class F>
void dispatch_pair(int din, int dout, F&& f) {
  dispatch_value<32, 64, 128>(din, [&](auto a) { dispatch_value<32, 64, 128>(dout, [&](auto b) { f(a, b); }); });
}

}  // namespace

extern "C" int32_t gcr_sage_supported(int32_t din, int32_t dout) { return width_ok(din) && width_ok(dout); }

extern "C" int64_t gcr_sage_workspace_bytes(int64_t n, int32_t din, int32_t dout) {
  if (n <= 0 || !gcr_sage_supported(din, dout)) return 0;
  const int64_t w = 2 * (int64_t)din * dout;                            // [wl^T; wr^T], then the partials of dwl, dwr, dbias
  return (w + (int64_t)bwd_blocks(n) * (w + dout)) * (int64_t)sizeof(float);
}

extern "C" int32_t gcr_sage_fwd_f32(int64_t n, const float* x, const float* z, const float* wl, const float* wr,
                                    const float* bias, int32_t din, int32_t dout, int32_t act, const uint32_t* keep_bits,
                                    float keep_scale, float* h, float* pre, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0 && gcr_sage_supported(din, dout) && act >= ACT_NONE && act <= ACT_GELU);
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(x != nullptr && z != nullptr && wl != nullptr && wr != nullptr && h != nullptr && workspace != nullptr &&
                h != x && h != z && aligned16(x, z, wl, wr, bias, h, pre, workspace) && aligned16(keep_bits));
  GCR_CHECK_ARG((pre != nullptr) == (act == ACT_GELU));
  hipStream_t s = (hipStream_t)stream;
  float* wcat = reinterpret_cast<float*>(workspace);
  const int elems = 2 * din * dout;
  hipLaunchKernelGGL(sage_wcat_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, wl, wr, (int)din, (int)dout, wcat);
  const int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  const dim3 grid((unsigned)fwd_blocks(n, din));
  dispatch_pair(din, dout, [&](auto a, auto b) {
    constexpr int DIN = decltype(a)::value, DOUT = decltype(b)::value;
    hipLaunchKernelGGL((sage_fwd_kernel<DIN, DOUT, w_in_lds(DIN, DOUT)>), grid, dim3(256), 0, s, n, x, z, (const float*)wcat,
                       bias, (int)act, keep_bits, keep_scale, h, pre);
  });
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_sage_bwd_f32(int64_t n, const float* x, const float* z, const float* wl, const float* wr, const float* h,
                                    const float* pre, const float* g, int32_t din, int32_t dout, int32_t act,
                                    const uint32_t* keep_bits, float keep_scale, float* p, float* q, float* dwl, float* dwr,
                                    float* dbias, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0 && gcr_sage_supported(din, dout) && act >= ACT_NONE && act <= ACT_GELU);
  GCR_CHECK_ARG(dwl != nullptr && dwr != nullptr && aligned16(dwl, dwr, dbias));
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    const size_t wbytes = sizeof(float) * (size_t)din * (size_t)dout;
    int32_t st = gcr_hip_status(hipMemsetAsync(dwl, 0, wbytes, s));
    if (st == GCR_OK) st = gcr_hip_status(hipMemsetAsync(dwr, 0, wbytes, s));
    if (st == GCR_OK && dbias != nullptr) st = gcr_hip_status(hipMemsetAsync(dbias, 0, sizeof(float) * (size_t)dout, s));
    return st;
  }
  GCR_CHECK_ARG(x != nullptr && z != nullptr && wl != nullptr && wr != nullptr && h != nullptr && g != nullptr &&
                workspace != nullptr && aligned16(x, z, wl, wr, h, pre, g, workspace) && aligned16(p, q) &&
                aligned16(keep_bits));
  GCR_CHECK_ARG((pre != nullptr) == (act == ACT_GELU) && (p != nullptr) == (q != nullptr));
  float* part = reinterpret_cast<float*>(workspace) + 2 * (int64_t)din * dout;
  const int nb = bwd_blocks(n);
  dispatch_pair(din, dout, [&](auto a, auto b) {
    constexpr int DIN = decltype(a)::value, DOUT = decltype(b)::value;
    hipLaunchKernelGGL((sage_bwd_kernel<DIN, DOUT, w_in_lds(DIN, DOUT)>), dim3((unsigned)nb), dim3(256), 0, s, n, x, z, wl, wr,
                       h, pre, g, (int)act, keep_bits, keep_scale, p, q, part);
  });
  const int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  const int elems = 2 * din * dout + dout;
  hipLaunchKernelGGL(sage_dw_reduce_kernel, dim3((unsigned)((elems + 63) / 64)), dim3(256), 0, s, (const float*)part, nb,
                     (int)din, (int)dout, dwl, dwr, dbias);
  return GCR_LAUNCH_STATUS();
}
