// BCE-with-logits over the all-pairs score matrix (lightgcn.py:109-113, loss_type == "bce"):
//   scores = user_vecs @ item_emb.T;  labels one-hot at pos_i;  F.binary_cross_entropy_with_logits(scores, labels)
//   = ( sum_ij softplus(s_ij) - sum_i s_{i, pos_i} ) / (M N).
// The M x N part is the row sum of softplus (forward) and (sigmoid(s)) weighted row / column sums of the operands
// (gradients) — the InfoNCE tile engine with another epilogue (gcr_pairs.h, gcr_pairs_loop.h); rows are NOT normalised here,
// so the launches run on three bf16 planes (d <= 64, the pipelined two-product loop, MODE 2 / 3), on two f16 planes with the
// rows scaled to unit norm inside (GCR_BCE_TWO_PLANES), or on the f32 MFMA (d = 128, 256, or forced).
// The positive-logit term is O(M d) and lives in the host-side op (functional.bce_softplus_rowsum's callers).
#include "gcr_pairs_loop.h"

namespace {

// rowsum[i] = ln2 * sum_s part[s][i].y ;  o[i, :] = sum_s opart[s][i, :]   (fixed order)
__global__ __launch_bounds__(256) void bce_merge_kernel(const float2* __restrict__ part, const float* __restrict__ opart,
                                                        int nsplit, int64_t m_rows, int d, float* __restrict__ rowsum,
                                                        float* __restrict__ o) {
  const int d4 = o != nullptr ? d / 4 : 1;
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m_rows * d4) return;
  const int64_t i = k / d4;
  const int c = (int)(k % d4);
  if (c == 0) {
    float l = 0.f;
    for (int s = 0; s < nsplit; ++s) l += part[(int64_t)s * m_rows + i].y;
    rowsum[i] = l * kLn2;
  }
  if (o != nullptr) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < nsplit; ++s) {
      const float4 v = reinterpret_cast<const float4*>(opart)[((int64_t)s * m_rows + i) * d4 + c];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    reinterpret_cast<float4*>(o)[i * d4 + c] = acc;
  }
}

// Pre-pass of the two-f16-plane BCE loops (EngH2, UNS): per row  inv = 1 / max(|x|, 1e-12)  (the operand scale that makes it a
// unit row),  nrm = max(|x|, 1e-12)  (what un-scales its scores) and  f = nrm * w  (the row's factor in the second product:
// sum_j sigmoid(s_ij) w_j y_j = sum_j (sigmoid(s_ij) nrm_j w_j) yhat_j).  D / 4 lanes per row, one float4 per lane.
template <int D>
__global__ __launch_bounds__(256) void bce_row_scales_kernel(const float* __restrict__ x, int64_t rows, const float* __restrict__ w,
                                                             float* __restrict__ inv, float* __restrict__ nrm, float* __restrict__ f) {
  constexpr int LPR = D / 4, GROUPS = 256 / LPR;
  const int gl = threadIdx.x % LPR;
  for (int64_t r = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LPR; r < rows; r += (int64_t)gridDim.x * GROUPS) {
    const float4 v = *reinterpret_cast<const float4*>(x + r * D + 4 * gl);
    float ss = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if (gl == 0) {
      const float n = fmaxf(sqrtf(ss), 1.0e-12f);
      inv[r] = 1.0f / n;
      nrm[r] = n;
      if (f != nullptr) f[r] = n * (w != nullptr ? w[r] : 1.0f);
    }
  }
}

template <int D>
void launch_bce_row_scales(const float* x, int64_t rows, const float* w, float* inv, float* nrm, float* f, hipStream_t s) {
  const int64_t want = (rows + 4 * (1024 / D) - 1) / (4 * (1024 / D));
  hipLaunchKernelGGL((bce_row_scales_kernel<D>), dim3((unsigned)gcr_grid(want, 8192)), dim3(256), 0, s, x,
                     rows, w, inv, nrm, f);
}

// the scratch of the two-plane path (plan_bce_fwd / plan_bce_bwd put it behind the partials)
struct BceScales { float *inv_x, *nrm_x, *inv_y, *nrm_y, *f_y, *hw; };
BceScales bce_scales_at(void* workspace, const PairsPath& q, int64_t mx, int64_t ny) {
  float* sc = ws_at<float>(workspace, q.scales);
  return {sc, sc + mx, sc + 2 * mx, sc + 2 * mx + ny, sc + 2 * mx + 2 * ny, ws_at<float>(workspace, q.hw)};
}

template <int D>
int32_t launch_bce_fwd(const float* a, int64_t m, const float* b, int64_t n, float* rowsum, float* o, void* workspace,
                       bool force_f32, bool two_planes, hipStream_t s) {
  const auto pl = plan_bce_fwd(m, n, D);
  const PairsPath& q = pl.path[bce_pipe(D, force_f32) ? kBceLoop : kBceF32];
  const FwdPlan& p = q.p;
  float2* part = ws_at<float2>(workspace, q.part);
  float* opart = ws_at<float>(workspace, q.opart);
  const dim3 grid((unsigned)(p.m_blocks * p.nsplit));
  const float* none = nullptr;
  bool with_o = false;
  if constexpr (D <= 64) {
    // MODE 2 of the loop; without o (SIDES 1) the same loop runs without its second product
    auto loop = [&](auto eng, const float* inv_a, const float* inv_b, const float* nrm_a, const float* nrm_b, const float* f_b,
                    const float* hw) {
      dispatch_bool(o != nullptr, [&](auto with) {
        hipLaunchKernelGGL((infonce_pipe_kernel<decltype(eng), D, 2, false, decltype(with)::value ? 0 : 1, 4>), grid, dim3(256), 0,
                           s, a, inv_a, m, b, inv_b, n, kLog2e, 1.0f, nrm_a, none, nrm_b, decltype(with)::value ? f_b : none,
                           p.nsplit, p.tiles_per_split, opart, part, decltype(with)::value ? hw : none);
      });
    };
    if (bce_pipe(D, force_f32) && two_planes) {
      // two f16 planes: both sides scaled to unit rows, scores un-scaled by the norms, o's streamed factor = the norm
      const BceScales c = bce_scales_at(workspace, q, m, n);
      launch_bce_row_scales<D>(a, m, nullptr, c.inv_x, c.nrm_x, nullptr, s);
      launch_bce_row_scales<D>(b, n, nullptr, c.inv_y, c.nrm_y, o != nullptr ? c.f_y : nullptr, s);
      if (o != nullptr) hipLaunchKernelGGL(h2_wscale_kernel, dim3(1), dim3(1024), 0, s, none, (int64_t)0, (const float*)c.f_y, n, c.hw);
      loop(EngH2{}, c.inv_x, c.inv_y, c.nrm_x, c.nrm_y, c.f_y, c.hw);
      with_o = true;
    } else if (bce_pipe(D, force_f32)) {
      loop(EngB3{}, none, none, none, none, none, none);
      with_o = true;
    }
  }
  if (!with_o) {
    if (o != nullptr) return GCR_EUNSUPPORTED;
    hipLaunchKernelGGL((infonce_fwd_kernel<D, false, false, true>), grid, dim3(256), 0, s, a, none, m, b, none, n, kLog2e,
                       p.nsplit, p.tiles_per_split, part, (float*)nullptr, 0.f);
  }
  int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  const int64_t threads = m * (o != nullptr ? D / 4 : 1);
  hipLaunchKernelGGL(bce_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, part, opart, p.nsplit, m, D,
                     rowsum, o);
  return GCR_LAUNCH_STATUS();
}

template <int D>
int32_t launch_bce_bwd(const float* x, int64_t mx, const float* y, int64_t ny, const float* w_x, const float* w_y, float* g,
                       void* workspace, bool force_f32, bool two_planes, hipStream_t s) {
  const float* none = nullptr;
  const auto pl = plan_bce_bwd(mx, ny, D);
  const PairsPath& q = pl.path[bce_pipe(D, force_f32) ? kBceLoop : kBceF32];
  const FwdPlan& p = q.p;
  float* gpart = p.nsplit == 1 ? g : ws_at<float>(workspace, q.part);
  const dim3 grid((unsigned)(p.m_blocks * p.nsplit));
  if constexpr (D <= 64) {
    if (bce_pipe(D, force_f32)) {
      if (two_planes && w_y != nullptr) {                  // (weights on the stationary rows stay on three planes)
        const BceScales c = bce_scales_at(workspace, q, mx, ny);
        launch_bce_row_scales<D>(x, mx, nullptr, c.inv_x, c.nrm_x, nullptr, s);
        launch_bce_row_scales<D>(y, ny, w_y, c.inv_y, c.nrm_y, c.f_y, s);
        hipLaunchKernelGGL(h2_wscale_kernel, dim3(1), dim3(1024), 0, s, none, (int64_t)0, (const float*)c.f_y, ny, c.hw);
        hipLaunchKernelGGL((infonce_pipe_kernel<EngH2, D, 3, false, 2, 4>), grid, dim3(256), 0, s, x, (const float*)c.inv_x, mx, y,
                           (const float*)c.inv_y, ny, kLog2e, 1.0f, (const float*)c.nrm_x, none, (const float*)c.nrm_y,
                           (const float*)c.f_y, p.nsplit, p.tiles_per_split, gpart, (float2*)nullptr, (const float*)c.hw);
      } else {                                             // SIDES 1 / 2: exactly one of w_x, w_y is there
        dispatch_bool(w_x != nullptr, [&](auto on_x) {
          hipLaunchKernelGGL((infonce_pipe_kernel<EngB3, D, 3, false, decltype(on_x)::value ? 1 : 2, 4>), grid, dim3(256), 0, s, x,
                             none, mx, y, none, ny, kLog2e, 1.0f, none, w_x, none, w_y, p.nsplit, p.tiles_per_split, gpart,
                             (float2*)nullptr, none);
        });
      }
      int32_t st = GCR_LAUNCH_STATUS();
      if (st != GCR_OK) return st;
      return reduce_splits(p, gpart, mx, D, g, s);
    }
  }
  for (int pass = 0; pass < BwdShape<D>::PASSES; ++pass) {
    hipLaunchKernelGGL((infonce_bwd_kernel<D, false, true>), grid, dim3(256), 0, s, x, none, mx, y, none, ny, kLog2e, 1.0f,
                       none, w_x, none, w_y, pass * BwdShape<D>::CT, p.nsplit, p.tiles_per_split, gpart);
    int32_t st = GCR_LAUNCH_STATUS();
    if (st != GCR_OK) return st;
  }
  return reduce_splits(p, gpart, mx, D, g, s);
}

}  // namespace

extern "C" int32_t gcr_bce_fwd_o_supported(int32_t d, uint32_t flags) {
  return (d == 32 || d == 64) && bce_pipe(d, (flags & GCR_INFONCE_ENGINE_F32) != 0) ? 1 : 0;
}

extern "C" int64_t gcr_bce_fwd_workspace_bytes(int64_t m, int64_t n, int32_t d) {
  if (m <= 0 || n <= 0 || !dim_supported(d)) return 0;
  return plan_bce_fwd(m, n, d).bytes();
}

extern "C" int32_t gcr_bce_fwd_f32(const float* a, int64_t m, const float* b, int64_t n, int32_t d, float* row_softplus,
                                   float* o, void* workspace, uint32_t flags, void* stream) {
  GCR_CHECK_ARG(m >= 0 && n >= 1);
  GCR_CHECK_ARG((flags & ~(uint32_t)(GCR_INFONCE_ENGINE_F32 | GCR_BCE_TWO_PLANES)) == 0);
  if (!dim_supported(d)) return GCR_EUNSUPPORTED;
  if (o != nullptr && !gcr_bce_fwd_o_supported(d, flags)) return GCR_EUNSUPPORTED;
  if (m == 0) return GCR_OK;
  GCR_CHECK_ARG(a != nullptr && b != nullptr && row_softplus != nullptr && workspace != nullptr);
  GCR_CHECK_ARG(m < (1ll << 40) && n < (1ll << 40));
  const bool f32 = (flags & GCR_INFONCE_ENGINE_F32) != 0, two = (flags & GCR_BCE_TWO_PLANES) != 0;
  return dispatch_dim(d, [&](auto dc) {
    return launch_bce_fwd<decltype(dc)::value>(a, m, b, n, row_softplus, o, workspace, f32, two, (hipStream_t)stream);
  });
}

extern "C" int64_t gcr_bce_bwd_workspace_bytes(int64_t mx, int64_t ny, int32_t d) {
  if (mx <= 0 || ny <= 0 || !dim_supported(d)) return 0;
  return plan_bce_bwd(mx, ny, d).bytes();
}

extern "C" int32_t gcr_bce_bwd_f32(const float* x, int64_t mx, const float* y, int64_t ny, int32_t d, const float* w_x,
                                   const float* w_y, float* g, void* workspace, uint32_t flags, void* stream) {
  GCR_CHECK_ARG(mx >= 0 && ny >= 1);
  GCR_CHECK_ARG((flags & ~(uint32_t)(GCR_INFONCE_ENGINE_F32 | GCR_BCE_TWO_PLANES)) == 0);
  if (!dim_supported(d)) return GCR_EUNSUPPORTED;
  if (mx == 0) return GCR_OK;
  GCR_CHECK_ARG(x != nullptr && y != nullptr && g != nullptr);
  GCR_CHECK_ARG((w_x != nullptr) != (w_y != nullptr));     // the weights sit on exactly one side
  GCR_CHECK_ARG(workspace != nullptr || plan_bce_bwd(mx, ny, d).bytes() == 0);
  const bool f32 = (flags & GCR_INFONCE_ENGINE_F32) != 0, two = (flags & GCR_BCE_TWO_PLANES) != 0;
  return dispatch_dim(d, [&](auto dc) {
    return launch_bce_bwd<decltype(dc)::value>(x, mx, y, ny, w_x, w_y, g, workspace, f32, two, (hipStream_t)stream);
  });
}
