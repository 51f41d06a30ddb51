// InfoNCE on the two-product kernels: the flash-style forward (lse and the softmax-weighted row sum o in one pass) and the
// backward.  The lse-only forward and the row ops are in gcr_infonce.hip, whose header comment describes the tile mapping;
// that unit also instantiates the f32-engine backward kernel, launched from here through gcr_infonce_bwd_f32_launch
// (gcr_pairs.h says why, and holds the launch plans).
#include "gcr_pairs_loop.h"

namespace {

template <int D>
int32_t launch_bwd(const float* x, const float* x_scale, int64_t mx, const float* y, const float* y_scale, int64_t ny,
                   float inv_tau, const float* lse_x, const float* w_x, const float* lse_y, const float* w_y, float* g,
                   void* workspace, bool exd, bool force_f32, bool unit_rows, hipStream_t s) {
  const auto pl = plan_infonce_bwd(mx, ny, D);
  const PairsPath& q = pl.path[use_b3(D, force_f32) ? kBwdSplit : kBwdF32];
  const FwdPlan& p = q.p;
  float* gpart = p.nsplit == 1 ? g : ws_at<float>(workspace, q.part);
  const dim3 grid((unsigned)(p.m_blocks * p.nsplit));
  const float scale2 = inv_tau * kLog2e;
  if constexpr (D <= 128) {
    if (use_b3(D, force_f32)) {
      // d <= 64: the cross-tile pipelined loop (infonce_pipe_kernel); d = 128: single-buffered (one tile with its
      // transposed copy is 54 KB of LDS)
      const bool h2 = use_h2_loop(D, inv_tau, unit_rows, force_f32);
      // (always the 256-thread form: the 512-thread form of the flash forward halves the STAGING work per MFMA, and the
      // backward stages from the pre-scaled image — two loads and two splits per lane.  At 100K x 100K the 512-thread
      // backward, 3-7 % ahead in round 2, is now behind: both sides 8.25 vs 7.44 ms, excluded diagonal 8.93 vs 8.45)
      const bool has_x = w_x != nullptr && lse_x != nullptr, has_y = w_y != nullptr && lse_y != nullptr;
      float* hw = ws_at<float>(workspace, q.hw);
      if (h2) {
        hipLaunchKernelGGL(h2_wscale_kernel, dim3(1), dim3(1024), 0, s, w_x, mx, w_y, ny, hw);
        int32_t st = GCR_LAUNCH_STATUS();
        if (st != GCR_OK) return st;
        // the loop's image of the streamed side (h2_prestage_kernel)
        float* img = ws_at<float>(workspace, q.image);
        const int64_t rows = fold_rows(ny);
        const dim3 pg((unsigned)((rows * (D / 4) + 255) / 256));
        const bool foldw = !exd && has_y && !has_x;      // SIDES = 2: weights into the exponent
        const bool stats = exd || has_y || !has_x;       // SIDES != 1: the loop reads the streamed rows' statistics
        if (foldw)
          hipLaunchKernelGGL((h2_prestage_kernel<D, true>), pg, dim3(256), 0, s, y, y_scale, w_y, lse_y, ny, (const float*)hw,
                             img, true);
        else
          hipLaunchKernelGGL((h2_prestage_kernel<D, false>), pg, dim3(256), 0, s, y, y_scale, has_y ? w_y : nullptr, lse_y, ny,
                             (const float*)hw, img, stats);
        st = GCR_LAUNCH_STATUS();
        if (st != GCR_OK) return st;
        if (stats) {
          lse_y = img;
          w_y = img + rows;
        }
        y = img + 2 * rows;
        y_scale = nullptr;
      }
      // EX: excluded diagonal; SIDES: which statistics are live (0 both, 1 the stationary rows', 2 the streamed rows')
      auto go = [&](auto ex, auto sides) {
        constexpr bool EX = decltype(ex)::value;
        constexpr int SIDES = decltype(sides)::value;
        auto pipe = [&](auto eng, const float* hwp) {
          using E = decltype(eng);
          hipLaunchKernelGGL((infonce_pipe_kernel<E, D, 0, EX, SIDES>), grid, dim3(256), 0, s, x, x_scale, mx, y, y_scale, ny,
                             scale2, inv_tau, lse_x, w_x, lse_y, w_y, p.nsplit, p.tiles_per_split, gpart, (float2*)nullptr, hwp);
        };
        if (h2) {
          pipe(EngH2{}, hw);
        } else if constexpr (D <= 64) {
          pipe(EngB3{}, nullptr);
        } else {
          hipLaunchKernelGGL((infonce_bwd_b3_kernel<D, EX, SIDES>), grid, dim3(256), 0, s, x, x_scale, mx, y, y_scale, ny,
                             scale2, inv_tau, lse_x, w_x, lse_y, w_y, p.nsplit, p.tiles_per_split, gpart);
        }
      };
      using std::integral_constant;
      if (exd) go(std::true_type{}, integral_constant<int, 0>{});
      else if (has_x && !has_y) go(std::false_type{}, integral_constant<int, 1>{});
      else if (has_y && !has_x) go(std::false_type{}, integral_constant<int, 2>{});
      else go(std::false_type{}, integral_constant<int, 0>{});
      int32_t st = GCR_LAUNCH_STATUS();
      if (st != GCR_OK) return st;
      return reduce_splits(p, gpart, mx, D, g, s);
    }
  }
  for (int pass = 0; pass < BwdShape<D>::PASSES; ++pass) {
    gcr_infonce_bwd_f32_launch(D, exd, grid, s, x, x_scale, mx, y, y_scale, ny, scale2, inv_tau, lse_x, w_x, lse_y, w_y,
                               pass * BwdShape<D>::CT, p.nsplit, p.tiles_per_split, gpart);
    int32_t st = GCR_LAUNCH_STATUS();
    if (st != GCR_OK) return st;
  }
  return reduce_splits(p, gpart, mx, D, g, s);
}

template <int D>
int32_t launch_fwd_o(const float* a, const float* a_scale, int64_t m, const float* b, const float* b_scale, int64_t n,
                     float inv_tau, float* lse, float* o, void* workspace, bool exd, bool unit_rows, hipStream_t s) {
  const bool h2o = use_h2_loop(D, inv_tau, unit_rows, false);
  const auto pl = plan_flash_fwd(m, n, D);
  const bool w8 = h2o && pl.path[kFlashRows8].open && h2_eight_waves(D, pl.path[kFlashRows8].p);
  const PairsPath& q = pl.path[w8 ? kFlashRows8 : kFlashRows4];
  const FwdPlan& p = q.p;
  float2* part = ws_at<float2>(workspace, q.part);
  float* opart = ws_at<float>(workspace, q.opart);
  const dim3 grid((unsigned)(p.m_blocks * p.nsplit));
  const float* none = nullptr;
  const float scale2 = inv_tau * kLog2e;
  const float h2_out = 1.0f / (EngH2::kSY * 16384.0f);               // streamed operand x kSY, P x 2^kPExp
  auto pipe = [&](auto eng, auto nw, float out_scale) {
    using E = decltype(eng);
    constexpr int NW = decltype(nw)::value;
    dispatch_bool(exd, [&](auto ex) {
      hipLaunchKernelGGL((infonce_pipe_kernel<E, D, 1, decltype(ex)::value, 0, NW>), grid, dim3(64 * NW), 0, s, a, a_scale, m,
                         b, b_scale, n, scale2, out_scale, none, none, none, none, p.nsplit, p.tiles_per_split, opart, part,
                         none);
    });
  };
  if (w8) {
    if constexpr (D == 64) pipe(EngH2{}, std::integral_constant<int, 8>{}, h2_out);
  } else if (h2o) {
    pipe(EngH2{}, std::integral_constant<int, 4>{}, h2_out);
  } else if constexpr (D <= 64) {
    pipe(EngB3{}, std::integral_constant<int, 4>{}, 1.0f);
  } else {
    dispatch_bool(exd, [&](auto ex) {
      hipLaunchKernelGGL((infonce_fwdo_b3_kernel<D, decltype(ex)::value>), grid, dim3(256), 0, s, a, a_scale, m, b, b_scale, n,
                         scale2, p.nsplit, p.tiles_per_split, part, opart);
    });
  }
  int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  const int64_t threads = m * (D / 4);
  hipLaunchKernelGGL(infonce_merge_o_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, part, opart,
                     p.nsplit, m, D, lse, o);
  return GCR_LAUNCH_STATUS();
}

}  // namespace

extern "C" int32_t gcr_infonce_fwd_o_supported(int32_t d, uint32_t flags) {
  return (d == 32 || d == 64 || d == 128) && use_b3(d, (flags & GCR_INFONCE_ENGINE_F32) != 0) ? 1 : 0;
}

extern "C" int64_t gcr_infonce_fwd_o_workspace_bytes(int64_t m, int64_t n, int32_t d) {
  if (m <= 0 || n <= 0 || !gcr_infonce_fwd_o_supported(d, 0)) return 0;
  return plan_flash_fwd(m, n, d).bytes();
}

extern "C" int32_t gcr_infonce_fwd_o_f32(const float* a, const float* a_scale, int64_t m, const float* b,
                                         const float* b_scale, int64_t n, int32_t d, float inv_tau, float* lse,
                                         float* o, void* workspace, uint32_t flags, void* stream) {
  GCR_CHECK_ARG(m >= 0 && n >= 1);
  GCR_CHECK_ARG((flags & ~(uint32_t)(GCR_INFONCE_EXCLUDE_DIAGONAL | GCR_INFONCE_ENGINE_F32 | GCR_INFONCE_UNIT_ROWS)) == 0);
  if (!gcr_infonce_fwd_o_supported(d, flags)) return GCR_EUNSUPPORTED;
  if (m == 0) return GCR_OK;
  GCR_CHECK_ARG(a != nullptr && b != nullptr && lse != nullptr && o != nullptr && workspace != nullptr);
  const bool exd = (flags & GCR_INFONCE_EXCLUDE_DIAGONAL) != 0;
  const bool unit = (flags & GCR_INFONCE_UNIT_ROWS) != 0;
  return dispatch_dim(d, [&](auto dc) -> int32_t {
    constexpr int D = decltype(dc)::value;
    if constexpr (D <= 128)                                 // (no flash forward at d = 256: refused above)
      return launch_fwd_o<D>(a, a_scale, m, b, b_scale, n, inv_tau, lse, o, workspace, exd, unit, (hipStream_t)stream);
    else
      return GCR_EUNSUPPORTED;
  });
}

extern "C" int64_t gcr_infonce_bwd_workspace_bytes(int64_t mx, int64_t ny, int32_t d) {
  if (mx <= 0 || ny <= 0 || !dim_supported(d)) return 0;
  return plan_infonce_bwd(mx, ny, d).bytes();
}

extern "C" int32_t gcr_infonce_bwd_ex_f32(const float* x, const float* x_scale, int64_t mx, const float* y,
                                          const float* y_scale, int64_t ny, int32_t d, float inv_tau,
                                          const float* lse_x, const float* w_x, const float* lse_y, const float* w_y,
                                          float* g, void* workspace, uint32_t flags, void* stream) {
  GCR_CHECK_ARG(mx >= 0 && ny >= 1);
  GCR_CHECK_ARG((flags & ~(uint32_t)(GCR_INFONCE_EXCLUDE_DIAGONAL | GCR_INFONCE_ENGINE_F32 | GCR_INFONCE_UNIT_ROWS)) == 0);
  const bool exd = (flags & GCR_INFONCE_EXCLUDE_DIAGONAL) != 0;
  const bool force_f32 = (flags & GCR_INFONCE_ENGINE_F32) != 0;
  const bool unit = (flags & GCR_INFONCE_UNIT_ROWS) != 0;
  if (!dim_supported(d)) return GCR_EUNSUPPORTED;
  if (mx == 0) return GCR_OK;
  GCR_CHECK_ARG(x != nullptr && y != nullptr && g != nullptr);
  GCR_CHECK_ARG((w_x == nullptr) == (lse_x == nullptr) && (w_y == nullptr) == (lse_y == nullptr));
  GCR_CHECK_ARG(workspace != nullptr || gcr_infonce_bwd_workspace_bytes(mx, ny, d) == 0);
  return dispatch_dim(d, [&](auto dc) {
    return launch_bwd<decltype(dc)::value>(x, x_scale, mx, y, y_scale, ny, inv_tau, lse_x, w_x, lse_y, w_y, g, workspace, exd,
                                           force_f32, unit, (hipStream_t)stream);
  });
}

extern "C" int32_t gcr_infonce_bwd_f32(const float* x, const float* x_scale, int64_t mx, const float* y,
                                       const float* y_scale, int64_t ny, int32_t d, float inv_tau, const float* lse_x,
                                       const float* w_x, const float* lse_y, const float* w_y, float* g,
                                       void* workspace, void* stream) {
  return gcr_infonce_bwd_ex_f32(x, x_scale, mx, y, y_scale, ny, d, inv_tau, lse_x, w_x, lse_y, w_y, g, workspace, 0u,
                                stream);
}
