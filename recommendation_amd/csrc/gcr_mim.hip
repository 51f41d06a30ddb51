// MHCN's hierarchical mutual-information loss (univariate/mhcn.py:496-505) over em [n, d], edge = H em [n, d] and three
// row permutations p0, p1, p2 (gfx950).
//
//   pos = <em_r, edge_r>   neg1 = <em[p0 r], edge_r>   neg2 = <edge[p1 r], em_r>
//   g = mean_r edge_r      gpos = <edge_r, g>          gneg = <edge[p2 r], g>
//   L = sum_r sp(neg1 - pos) + sp(neg2 - neg1) + sp(gneg - gpos),   sp(x) = log(1 + e^x) = -log(sigmoid(-x))
//
// Replaces three gathered [n, d] copies, five row-dot reductions and three log-sigmoid chains per call, and in the
// backward the index_put_(accumulate=True) of every x[perm].
//
// Forward, two launches:
//   colsum   per-workgroup column sums of edge over a contiguous row range (double); the last workgroup to finish (an
//            integer ticket) adds the partials in workgroup order and writes g = sum / n.
//   rows     d / 4 lanes per row, one 16-byte load per lane and operand, sub-wave butterfly for the five dots; writes
//            a = -sigmoid(neg1 - pos), b = -sigmoid(neg2 - neg1), c = -sigmoid(gneg - gpos) as coef [3, n], and per-
//            workgroup partials (double) of L and of dg = sum_r c_r (edge_r - edge[p2 r]) — edge_r and edge[p2 r] are in
//            registers here, so the backward never reads them for dg; the last workgroup folds both, in workgroup order.
// Backward, two launches: q_k = p_k^-1 for all three k (a scatter with one writer per slot), then one pull per row
//   d_em_r   = a_r edge_r - b_r edge[p1 r] + (b - a)_{q0 r} edge_{q0 r}
//   d_edge_r = a_r em_r + (b_r - a_r) em[p0 r] - b_{q1 r} em_{q1 r} + (c_r - c_{q2 r}) g + dg / n
// scaled by the upstream scalar read from device memory.  Every output row has exactly one writer: no float atomics, and
// with the fixed-order partial sums the loss and both gradients are bitwise reproducible.
//
// Every indexed row is read only if 0 <= idx < n; an index outside (or a slot of q that no p_k fills, when p_k is not a
// permutation) contributes a zero row and a zero coefficient.
#include "gcr_host.h"
#include "gcr_lanes.h"

namespace {

constexpr int kMaxBlocks = 1024;

// row `idx` of x as this lane's float4, a zero row for an index outside [0, n)
template <int LPR>
__device__ __forceinline__ float4 row4(const float* __restrict__ x, int64_t idx, int64_t n, int gl) {
  if (idx < 0 || idx >= n) return make_float4(0.f, 0.f, 0.f, 0.f);
  return *reinterpret_cast<const float4*>(x + idx * (4 * LPR) + 4 * gl);
}

// sp(x) = log(1 + e^x) and sigmoid(x) without overflow at either end (not gcr_dense.hip's sigmoid_f32, 1 / (1 + e^-x): the two
// round differently)
__device__ __forceinline__ float softplus_f32(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float stable_sigmoid_f32(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

// true in exactly one workgroup of the launch: the last to arrive.  Its later reads see every other workgroup's
// partials (release fence before the ticket, acquire fence after).
__device__ __forceinline__ bool last_workgroup(unsigned* ticket, int* is_last) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) *is_last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
  __syncthreads();
  if (!*is_last) return false;
  __threadfence();
  return true;
}

__device__ __forceinline__ double load_part(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sum of part[first], part[first + stride], ... below `count`, added in that order; kFoldLoads loads are in flight at a time
// (the last workgroup's fold is a chain of dependent device-scope loads otherwise: 120 us for 977 partials)
constexpr int kFoldLoads = 16;
__device__ __forceinline__ double fold_strided(const double* part, int first, int stride, int count, int64_t pitch) {
  double s = 0.0;
  for (int b0 = first; b0 < count; b0 += stride * kFoldLoads) {
    double v[kFoldLoads];
#pragma unroll
    for (int k = 0; k < kFoldLoads; ++k) {
      const int b = b0 + k * stride;
      v[k] = b < count ? load_part(part + (int64_t)b * pitch) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kFoldLoads; ++k) s += v[k];
  }
  return s;
}

// out[c] = scale * sum_b part[b][c] for c < d (d <= 256), the workgroups' partials added in workgroup order: 256 / d
// interleaved chains per column, the chains then added in chain order.  All 256 threads call it; red: 256 doubles.
__device__ __forceinline__ void fold_columns(const double* part, int nb, int d, double scale, float* out, double* red) {
  const int chains = 256 / d;
  const int c = threadIdx.x % d, chain = threadIdx.x / d;
  const double s = chain < chains ? fold_strided(part + c, chain, chains, nb, d) : 0.0;
  __syncthreads();
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < d) {
    double t = red[threadIdx.x];
    for (int k = 1; k < chains; ++k) t += red[threadIdx.x + k * d];
    out[threadIdx.x] = (float)(t * scale);
  }
}

// the 256 threads' double4 (one per thread, groups of LPR lanes hold the same columns) summed over the groups in group
// order into part[0 .. 4 LPR)
template <int LPR>
__device__ __forceinline__ void fold_groups(const double (&v)[4], double* red, double* part) {
  constexpr int GROUPS = 256 / LPR;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k * 256 + threadIdx.x] = v[k];
  __syncthreads();
  if (threadIdx.x < LPR) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double t = red[k * 256 + threadIdx.x];
      for (int g = 1; g < GROUPS; ++g) t += red[k * 256 + threadIdx.x + g * LPR];
      part[4 * threadIdx.x + k] = t;
    }
  }
}

template <int LPR>
__global__ __launch_bounds__(256) void mim_colsum_kernel(const float* __restrict__ edge, int64_t n, int64_t rows_per_block,
                                                         double* __restrict__ cs_part, unsigned* __restrict__ ticket,
                                                         float* __restrict__ gvec) {
  constexpr int D = 4 * LPR, GROUPS = 256 / LPR;
  __shared__ double red[4 * 256];
  __shared__ int is_last;
  const int gl = threadIdx.x % LPR;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(n, r0 + rows_per_block);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = r0 + threadIdx.x / LPR; r < r1; r += GROUPS) {
    const float4 e = *reinterpret_cast<const float4*>(edge + r * D + 4 * gl);
    s[0] += (double)e.x; s[1] += (double)e.y; s[2] += (double)e.z; s[3] += (double)e.w;
  }
  fold_groups<LPR>(s, red, cs_part + (int64_t)blockIdx.x * D);
  if (!last_workgroup(ticket, &is_last)) return;
  fold_columns(cs_part, (int)gridDim.x, D, 1.0 / (double)n, gvec, red);
}

template <int LPR>
__global__ __launch_bounds__(256) void mim_rows_kernel(const float* __restrict__ em, const float* __restrict__ edge,
                                                       const int64_t* __restrict__ p0, const int64_t* __restrict__ p1,
                                                       const int64_t* __restrict__ p2, int64_t n, int64_t rows_per_block,
                                                       float* __restrict__ coef, double* __restrict__ loss_part,
                                                       double* __restrict__ dg_part, unsigned* __restrict__ ticket,
                                                       float* __restrict__ loss, float* __restrict__ gvec) {
  constexpr int D = 4 * LPR, GROUPS = 256 / LPR;
  __shared__ double red[4 * 256];
  __shared__ int is_last;
  const int gl = threadIdx.x % LPR, group = threadIdx.x / LPR;
  const float4 g4 = *reinterpret_cast<const float4*>(gvec + 4 * gl);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(n, r0 + rows_per_block);
  double dg[4] = {0.0, 0.0, 0.0, 0.0};
  double lsum = 0.0;
  for (int64_t r = r0 + group; r < r1; r += GROUPS) {
    const float4 u = *reinterpret_cast<const float4*>(em + r * D + 4 * gl);
    const float4 e = *reinterpret_cast<const float4*>(edge + r * D + 4 * gl);
    const float4 u0 = row4<LPR>(em, p0[r], n, gl);
    const float4 e1 = row4<LPR>(edge, p1[r], n, gl);
    const float4 e2 = row4<LPR>(edge, p2[r], n, gl);
    const float pos = gcr_group_sum<LPR>(gcr_dot4(u, e)), neg1 = gcr_group_sum<LPR>(gcr_dot4(u0, e));
    const float neg2 = gcr_group_sum<LPR>(gcr_dot4(e1, u));
    const float gpos = gcr_group_sum<LPR>(gcr_dot4(e, g4)), gneg = gcr_group_sum<LPR>(gcr_dot4(e2, g4));
    const float x1 = neg1 - pos, x2 = neg2 - neg1, x3 = gneg - gpos;
    const float c = -stable_sigmoid_f32(x3);
    if (gl == 0) {
      coef[r] = -stable_sigmoid_f32(x1);
      coef[n + r] = -stable_sigmoid_f32(x2);
      coef[2 * n + r] = c;
      lsum += (double)softplus_f32(x1) + (double)softplus_f32(x2) + (double)softplus_f32(x3);
    }
    dg[0] += (double)(c * (e.x - e2.x)); dg[1] += (double)(c * (e.y - e2.y));
    dg[2] += (double)(c * (e.z - e2.z)); dg[3] += (double)(c * (e.w - e2.w));
  }
  fold_groups<LPR>(dg, red, dg_part + (int64_t)blockIdx.x * D);
  __syncthreads();
  red[threadIdx.x] = lsum;                                   // non-zero in each group's first lane only
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < GROUPS; ++k) t += red[k * LPR];
    loss_part[blockIdx.x] = t;
  }
  if (!last_workgroup(ticket, &is_last)) return;
  const int nb = (int)gridDim.x;
  fold_columns(dg_part, nb, D, 1.0, gvec + D, red);
  if (threadIdx.x < GCR_WAVE) {
    const double t = gcr_wave_sum_f64(fold_strided(loss_part, (int)threadIdx.x, GCR_WAVE, nb, 1));
    if (threadIdx.x == 0) *loss = (float)t;
  }
}

// q[k][p_k[r]] = r for k < 3; q was filled with -1
__global__ __launch_bounds__(256) void mim_inverse_kernel(const int64_t* __restrict__ p0, const int64_t* __restrict__ p1,
                                                          const int64_t* __restrict__ p2, int64_t n, int64_t* __restrict__ q) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 3 * n; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i / n);
    const int64_t r = i - k * n;
    const int64_t p = (k == 0 ? p0 : k == 1 ? p1 : p2)[r];
    if (p >= 0 && p < n) q[k * n + p] = r;
  }
}

template <int LPR>
__global__ __launch_bounds__(256) void mim_bwd_kernel(const float* __restrict__ em, const float* __restrict__ edge,
                                                      const int64_t* __restrict__ p0, const int64_t* __restrict__ p1,
                                                      const int64_t* __restrict__ q, int64_t n, const float* __restrict__ coef,
                                                      const float* __restrict__ gvec, const float* __restrict__ g_out,
                                                      float* __restrict__ d_em, float* __restrict__ d_edge) {
  constexpr int D = 4 * LPR, GROUPS = 256 / LPR;
  const int gl = threadIdx.x % LPR;
  const float up = *g_out;
  const float inv_n = 1.0f / (float)n;
  const float4 g4 = *reinterpret_cast<const float4*>(gvec + 4 * gl);
  const float4 dg4 = *reinterpret_cast<const float4*>(gvec + D + 4 * gl);
  for (int64_t r = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LPR; r < n; r += (int64_t)gridDim.x * GROUPS) {
    const int64_t q0 = q[r], q1 = q[n + r], q2 = q[2 * n + r];
    const bool h0 = q0 >= 0 && q0 < n, h1 = q1 >= 0 && q1 < n, h2 = q2 >= 0 && q2 < n;
    const float a = coef[r], b = coef[n + r], c = coef[2 * n + r];
    const float ba_q0 = h0 ? coef[n + q0] - coef[q0] : 0.f;
    const float b_q1 = h1 ? coef[n + q1] : 0.f;
    const float c_q2 = h2 ? coef[2 * n + q2] : 0.f;
    const float4 u = *reinterpret_cast<const float4*>(em + r * D + 4 * gl);
    const float4 e = *reinterpret_cast<const float4*>(edge + r * D + 4 * gl);
    const float4 u0 = row4<LPR>(em, p0[r], n, gl);
    const float4 e1 = row4<LPR>(edge, p1[r], n, gl);
    const float4 eq0 = row4<LPR>(edge, q0, n, gl);
    const float4 uq1 = row4<LPR>(em, q1, n, gl);
    const float ba = b - a, cc = c - c_q2;
    float4 du, de;
    du.x = up * (a * e.x - b * e1.x + ba_q0 * eq0.x);
    du.y = up * (a * e.y - b * e1.y + ba_q0 * eq0.y);
    du.z = up * (a * e.z - b * e1.z + ba_q0 * eq0.z);
    du.w = up * (a * e.w - b * e1.w + ba_q0 * eq0.w);
    de.x = up * (a * u.x + ba * u0.x - b_q1 * uq1.x + cc * g4.x + dg4.x * inv_n);
    de.y = up * (a * u.y + ba * u0.y - b_q1 * uq1.y + cc * g4.y + dg4.y * inv_n);
    de.z = up * (a * u.z + ba * u0.z - b_q1 * uq1.z + cc * g4.z + dg4.z * inv_n);
    de.w = up * (a * u.w + ba * u0.w - b_q1 * uq1.w + cc * g4.w + dg4.w * inv_n);
    *reinterpret_cast<float4*>(d_em + r * D + 4 * gl) = du;
    *reinterpret_cast<float4*>(d_edge + r * D + 4 * gl) = de;
  }
}

int mim_blocks(int64_t n) {
  return (int)gcr_grid((n + 255) / 256, kMaxBlocks);         // >= 256 rows per workgroup
}

struct MimWorkspace {
  int64_t ticket, cs_part, dg_part, loss_part, q, total;     // byte offsets
};

MimWorkspace mim_layout(int64_t n, int d) {
  MimWorkspace w;
  WsCarve c;
  const int64_t nb = mim_blocks(n);
  w.ticket = c.take(64);                                     // two counters: colsum, rows
  w.cs_part = c.take(nb * d * (int64_t)sizeof(double));
  w.dg_part = c.take(nb * d * (int64_t)sizeof(double));
  w.loss_part = c.take(nb * (int64_t)sizeof(double));
  w.q = c.take(3 * n * (int64_t)sizeof(int64_t));
  w.total = c.at;
  return w;
}

}  // namespace

extern "C" int32_t gcr_mim_supported(int32_t d) { return d == 32 || d == 64 || d == 128 || d == 256; }

extern "C" int64_t gcr_mim_workspace_bytes(int64_t n, int32_t d) {
  if (n <= 0 || !gcr_mim_supported(d)) return 0;
  return mim_layout(n, d).total;
}

extern "C" int32_t gcr_mim_fwd_f32(const float* em, const float* edge, const int64_t* p0, const int64_t* p1, const int64_t* p2,
                                   int64_t n, int32_t d, float* loss, float* coef, float* gvec, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0);
  if (!gcr_mim_supported(d)) return GCR_EUNSUPPORTED;
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(em && edge && p0 && p1 && p2 && loss && coef && gvec && workspace);
  hipStream_t s = (hipStream_t)stream;
  const MimWorkspace w = mim_layout(n, d);
  char* ws = reinterpret_cast<char*>(workspace);
  unsigned* ticket = reinterpret_cast<unsigned*>(ws + w.ticket);
  double* cs_part = reinterpret_cast<double*>(ws + w.cs_part);
  double* dg_part = reinterpret_cast<double*>(ws + w.dg_part);
  double* loss_part = reinterpret_cast<double*>(ws + w.loss_part);
  const int nb = mim_blocks(n);
  const int64_t per = (n + nb - 1) / nb;
  hipError_t err = hipMemsetAsync(ticket, 0, 64, s);
  if (err != hipSuccess) return gcr_hip_status(err);
  dispatch_value<32, 64, 128, 256>(d, [&](auto dc) {
    constexpr int LPR = decltype(dc)::value / 4;
    hipLaunchKernelGGL((mim_colsum_kernel<LPR>), dim3((unsigned)nb), dim3(256), 0, s, edge, n, per, cs_part, ticket, gvec);
    hipLaunchKernelGGL((mim_rows_kernel<LPR>), dim3((unsigned)nb), dim3(256), 0, s, em, edge, p0, p1, p2, n, per, coef,
                       loss_part, dg_part, ticket + 1, loss, gvec);
  });
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_mim_bwd_f32(const float* em, const float* edge, const int64_t* p0, const int64_t* p1, const int64_t* p2,
                                   int64_t n, int32_t d, const float* coef, const float* gvec, const float* g_out, float* d_em,
                                   float* d_edge, void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0);
  if (!gcr_mim_supported(d)) return GCR_EUNSUPPORTED;
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(em && edge && p0 && p1 && p2 && coef && gvec && g_out && d_em && d_edge && workspace);
  hipStream_t s = (hipStream_t)stream;
  const MimWorkspace w = mim_layout(n, d);
  int64_t* q = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(workspace) + w.q);
  hipError_t err = hipMemsetAsync(q, 0xFF, sizeof(int64_t) * (size_t)(3 * n), s);       // -1: no row maps here
  if (err != hipSuccess) return gcr_hip_status(err);
  hipLaunchKernelGGL(mim_inverse_kernel, dim3((unsigned)gcr_grid((3 * n + 255) / 256, 16384)), dim3(256), 0, s, p0, p1, p2, n, q);
  int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  const int groups = 256 / (d / 4);
  const dim3 grid((unsigned)gcr_grid((n + groups * 2 - 1) / (groups * 2), 16384));
  dispatch_value<32, 64, 128, 256>(d, [&](auto dc) {
    hipLaunchKernelGGL((mim_bwd_kernel<decltype(dc)::value / 4>), grid, dim3(256), 0, s, em, edge, p0, p1, q, n, coef, gvec,
                       g_out, d_em, d_edge);
  });
  return GCR_LAUNCH_STATUS();
}
