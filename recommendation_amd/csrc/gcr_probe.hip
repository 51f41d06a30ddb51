// Memory-system probes for bench.py's roofline block ("confirm with a device-memcpy /
// STREAM probe on the box and report that too").  Three access shapes, all with 16 B per lane:
//   copy    dst[i] = src[i]                        1 read + 1 write per byte
//   read    sink += src[i]                         read only
//   gather  out[k] = sum of 64 table rows idx[64k..64k+63], 256-B rows, 16 loads in flight per
//           wave — the access shape of spmm_parts without its CSR streams
//   policy  the gather over a hot and a cold table at once, with a sequential stream read and row stores
//           beside it, each of the three optionally `nt`: does a cache-policy hint change what an L2 keeps?
// They are measurement aids, not part of the recommender path.
#include "gcr_common.h"

namespace {

// every block owns one contiguous slice; a thread keeps eight 16-B loads in flight, 4 KB apart
__global__ __launch_bounds__(256) void probe_copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                         int64_t n4) {
  const int64_t per = (n4 + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = min(n4, lo + per);
  int64_t i = lo + threadIdx.x;
  for (; i + 7 * 256 < hi; i += 8 * 256) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[i + 256 * u];
#pragma unroll
    for (int u = 0; u < 8; ++u) dst[i + 256 * u] = v[u];
  }
  for (; i < hi; i += 256) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void probe_read_kernel(const float4* __restrict__ src, int64_t n4,
                                                         float* __restrict__ sink) {
  const int64_t per = (n4 + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = min(n4, lo + per);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  int64_t i = lo + threadIdx.x;
  for (; i + 7 * 256 < hi; i += 8 * 256) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[i + 256 * u];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w;
    }
  }
  for (; i < hi; i += 256) {
    const float4 v = src[i];
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  const float s = gcr_wave_sum(a.x + a.y + a.z + a.w);
  // data-dependent store the compiler cannot drop; practically never taken on random data
  if (s == 1.2345678e33f && (threadIdx.x & 63) == 0) sink[0] = s;
}

__global__ __launch_bounds__(256) void probe_gather_kernel(const float* __restrict__ table,
                                                           const int32_t* __restrict__ idx, int64_t n_groups,
                                                           int n_rows, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_groups) return;
  const int my = min(max(idx[g * 64 + lane], 0), n_rows - 1);   // never dereference a bad id
  float acc = 0.f;
#pragma unroll
  for (int b = 0; b < 64; b += 16) {
    float r[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) r[u] = table[(int64_t)gcr_readlane_i(my, b + u) * 64 + lane];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc += r[u];
  }
  out[g * 64 + lane] = acc;
}

typedef float probe_f4 __attribute__((ext_vector_type(4)));

template <bool NT, class T>
__device__ __forceinline__ T probe_load(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

template <bool NT, class T>
__device__ __forceinline__ void probe_store(T* p, T v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// probe_gather_kernel's loop over two tables with the one-touch streams of a plain SpMM launch beside it: of every batch of
// 16 gathers the even ones read the hot table (always plain loads), the odd ones the cold table; every batch also reads
// 1 KiB of `stream` in order (64 B per gather, 16 B per lane) and stores its sum as one 256-B row of `out` (4 B per lane, as
// an SpMM row).  COLD_NT / STREAM_NT / STORE_NT put `nt` on the cold gathers, the stream loads and the row stores.
template <bool COLD_NT, bool STREAM_NT, bool STORE_NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void probe_policy_kernel(const float* __restrict__ hot, int n_hot,
                                                           const float* __restrict__ cold, int n_cold,
                                                           const int32_t* __restrict__ idx, int64_t n_groups,
                                                           const probe_f4* __restrict__ stream, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_groups) return;
  // even lanes name a hot row, odd lanes a cold one; never dereference a bad id
  const int my = min(max(idx[g * 64 + lane], 0), ((lane & 1) ? n_cold : n_hot) - 1);
#pragma unroll
  for (int b = 0; b < 64; b += 16) {
    const int64_t batch = g * 4 + b / 16;
    const probe_f4 s = probe_load<STREAM_NT>(stream + batch * 64 + lane);
    float r[16];
#pragma unroll
    for (int u = 0; u < 16; u += 2) {
      r[u] = hot[(int64_t)gcr_readlane_i(my, b + u) * 64 + lane];
      r[u + 1] = probe_load<COLD_NT>(cold + (int64_t)gcr_readlane_i(my, b + u + 1) * 64 + lane);
    }
    float acc = (s.x + s.y) + (s.z + s.w);
#pragma unroll
    for (int u = 0; u < 16; ++u) acc += r[u];
    probe_store<STORE_NT>(out + batch * 64 + lane, acc);
  }
}

}  // namespace

extern "C" int32_t gcr_probe_copy_f32(const float* src, float* dst, int64_t n_floats, void* stream) {
  GCR_CHECK_ARG(src != nullptr && dst != nullptr && n_floats >= 0 && (n_floats & 3) == 0);
  GCR_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst) & 15) == 0);
  if (n_floats == 0) return GCR_OK;
  hipLaunchKernelGGL(probe_copy_kernel, dim3(256 * 32), dim3(256), 0, (hipStream_t)stream, (const float4*)src,
                     (float4*)dst, n_floats / 4);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_probe_read_f32(const float* src, int64_t n_floats, float* sink, void* stream) {
  GCR_CHECK_ARG(src != nullptr && sink != nullptr && n_floats >= 0 && (n_floats & 3) == 0);
  GCR_CHECK_ARG(((uintptr_t)src & 15) == 0);
  if (n_floats == 0) return GCR_OK;
  hipLaunchKernelGGL(probe_read_kernel, dim3(256 * 32), dim3(256), 0, (hipStream_t)stream, (const float4*)src,
                     n_floats / 4, sink);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_probe_gather_rows_f32(const float* table, int64_t n_rows, const int32_t* idx, int64_t n_idx,
                                             float* out, void* stream) {
  GCR_CHECK_ARG(table != nullptr && idx != nullptr && out != nullptr);
  GCR_CHECK_ARG(n_rows > 0 && n_rows < (1ll << 31) && n_idx >= 0 && (n_idx & 63) == 0 && n_idx / 256 < (1ll << 31));
  if (n_idx == 0) return GCR_OK;
  const int64_t n_groups = n_idx / 64;
  hipLaunchKernelGGL(probe_gather_kernel, dim3((unsigned)((n_groups + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     table, idx, n_groups, (int)n_rows, out);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_probe_policy_rows_f32(const float* hot, int64_t n_hot, const float* cold, int64_t n_cold,
                                             const int32_t* idx, int64_t n_idx, const float* stream_in, float* out,
                                             uint32_t nt_flags, void* stream) {
  GCR_CHECK_ARG(hot != nullptr && cold != nullptr && idx != nullptr && stream_in != nullptr && out != nullptr);
  GCR_CHECK_ARG(n_hot > 0 && n_hot < (1ll << 31) && n_cold > 0 && n_cold < (1ll << 31) && nt_flags < 8u);
  GCR_CHECK_ARG(n_idx >= 0 && (n_idx & 63) == 0 && n_idx / 256 < (1ll << 31));
  GCR_CHECK_ARG(((uintptr_t)stream_in & 15) == 0);
  if (n_idx == 0) return GCR_OK;
  const int64_t n_groups = n_idx / 64;
  const dim3 grid((unsigned)((n_groups + 3) / 4)), block(256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, hot, (int)n_hot, cold, (int)n_cold, idx, n_groups,
                       (const probe_f4*)stream_in, out);
  };
  switch (nt_flags) {
    case 0: launch(probe_policy_kernel<false, false, false>); break;
    case 1: launch(probe_policy_kernel<true, false, false>); break;
    case 2: launch(probe_policy_kernel<false, true, false>); break;
    case 3: launch(probe_policy_kernel<true, true, false>); break;
    case 4: launch(probe_policy_kernel<false, false, true>); break;
    case 5: launch(probe_policy_kernel<true, false, true>); break;
    case 6: launch(probe_policy_kernel<false, true, true>); break;
    default: launch(probe_policy_kernel<true, true, true>); break;
  }
  return GCR_LAUNCH_STATUS();
}
