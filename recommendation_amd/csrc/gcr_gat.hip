// GATConv's aggregation (gat.py:20-23, 34, 37 through torch_geometric's GATConv): the softmax over a target's in-edges and
// the weighted gather-sum, per head, forward and backward, with nothing of size E written.  PyG materialises alpha [E, H]
// and the messages [E, H, C], forward and again for autograd.  Here ONE walk serves the three passes:
//   FWD      row = target i:  out_i = sum_j alpha~_ij h_j + bias,   lse_i = max + log(sum)
//   BWD_ROW  row = target i:  D_i = sum_j alpha~_ij <g_i, h_j>,  da_dst_i = A_i - D_i B_i,  r_i = 1 / sum_j exp(e_ij - lse_i)
//   BWD_T    row = source j (CSR of the transpose):  dh_j = sum_i alpha~_ij g_i,  da_src_j = sum_i l' alpha_ij (q_ij - D_i)
// (alpha~ = alpha * keep * keep_scale, q_ij = keep * keep_scale * <g_i, h_j>, l' = leaky'(a_src[j] + a_dst[i]); gcr.h has
// the algebra).  A row's terms are its self loop (term 0, implicit: the CSR stores no diagonal) and its entries in stored
// order.  A wave takes 64 terms at a time:
//   sweep 1  one term per lane: the logits of the H heads from the [n, H] tables (4 H bytes per neighbour, cache
//            resident), the final weights of that term;
//   sweep 2  the 64 gathers of W = H C floats, eight in flight, column c0 .. c0 + NV of every row in one lane; node and
//            weight of term u come by readlane, so the addresses are scalar + lane offset.  Short batches are padded
//            with the row's own node at weight 0 (a cache hit), so every batch is eight loads deep.
// The forward runs a sweep 0 first (two-sweep softmax): per-lane online (max, sum) over the logits, merged over the wave.
// Scalar sums over a head's columns (A, D, da_src's dot part) are kept per lane and reduced ONCE per row, not per edge.
// A row of at most LONG_ROW entries is one wave's (four rows per workgroup); a longer one gets a whole workgroup
// (gat_long_kernel: its sixteen waves take the row's 64-term batches in turn and merge (max, sum), the accumulators and
// the scalar sums through LDS in wave order).  No atomics; every sum has a fixed order: bitwise reproducible.
// W = 32 (H = 1, C = 32): the upper half-wave repeats the lower one's columns and neither stores nor counts.
#include "gcr_host.h"
#include "gcr_lanes.h"

namespace {

constexpr int LONG_ROW = 512;       // entries of a row above which a whole workgroup walks it
constexpr int LONG_CAP = 1024;      // workgroups of the long-row launch, at most
constexpr int LONG_THREADS = 1024;  // of a long-row workgroup: sixteen waves on one row
enum { FWD = 0, BWD_ROW = 1, BWD_T = 2 };

struct GatArgs {
  const int64_t* rowptr;            // of the walked CSR (the transpose's in BWD_T)
  const int32_t* col;
  const int64_t* perm;              // BWD_T: entry e of the transpose is entry perm[e] of the forward CSR; NULL = identity
  const int64_t* rowptr_fwd;        // rowptr_fwd[n] = nnz: the self loop of node i is edge nnz + i of the bitmap
  int64_t n;
  const float* h;
  const float* a_src;
  const float* a_dst;
  const float* lse_in;
  const float* g;
  const float* dd_in;               // D [n, H] (BWD_T)
  const float* rinv_in;             // 1 / sum_j exp(e_ij - lse[i]) [n, H] (BWD_T)
  float slope;
  const uint32_t* keep;
  float keep_scale;
  const float* bias;
  float* out;                       // FWD: out;  BWD_T: dh
  float* lse;                       // FWD
  float* ds;                        // BWD_ROW: da_dst;  BWD_T: da_src
  float* dd_out;                    // BWD_ROW: D
  float* rinv_out;                  // BWD_ROW
};

template <int NV>
__device__ __forceinline__ void load_nv(const float* __restrict__ p, float (&v)[NV]) {
  if constexpr (NV == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (NV == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
    v[0] = *p;
  }
}

template <int NV>
__device__ __forceinline__ void store_nv(float* __restrict__ p, const float (&v)[NV]) {
  if constexpr (NV == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else if constexpr (NV == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  } else {
    *p = v[0];
  }
}

// butterfly sum of doubles over aligned groups of LPR lanes: every lane ends with its group's total
template <int LPR>
__device__ __forceinline__ double group_sum_f64(double v) {
#pragma unroll
  for (int off = LPR / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, GCR_WAVE);
  return v;
}

// w[head] of lane u, `head` this lane's own
template <int H>
__device__ __forceinline__ float pick_lane(const float (&w)[H], int u, int head) {
  float r = gcr_readlane_f(w[0], u);
#pragma unroll
  for (int k = 1; k < H; ++k) {
    const float t = gcr_readlane_f(w[k], u);
    r = head == k ? t : r;
  }
  return r;
}

// One row by WPR waves (1, or the 16 of a long-row workgroup; `wv` = this wave's number among them).  s_vec [WPR][W] and
// s_sc [WPR][4 H] are the merge buffers of WPR > 1.
// The backward's scalar sums (A, D, B and their like) are differences of sums several times their size: they are kept in
// float64 from the per-term product on (a float32 chain lost 1e-6 of the result at twenty terms), a few operations per
// gathered row.
template <int W, int H, int MODE, int WPR>
__device__ __forceinline__ void gat_row(const GatArgs& a, const int64_t row, const int wv, const int lane, float* s_vec,
                                        double* s_sc) {
  constexpr int NV = W >= 64 ? W / 64 : 1, C = W / H, G = W >= 64 ? 64 / H : 64;
  const int c0 = (lane * NV) % W;
  const int head = c0 / C;
  const bool owner = lane * NV < W;
  const int64_t e0 = a.rowptr[row];
  const int64_t nterm = a.rowptr[row + 1] - e0 + 1;
  const int64_t nnz = a.rowptr_fwd[a.n];
  // A node without in-edges: its softmax has one term, the self loop, whose logit gets no gradient (alpha = 1 whatever
  // the logit).  Computed, that zero is D_i's float32 rounding in da_src and the two float64 sums' in da_dst.
  const bool lone = MODE != FWD && a.rowptr_fwd[row + 1] == a.rowptr_fwd[row];
  const float* __restrict__ tab = MODE == BWD_T ? a.g : a.h;      // the gathered table

  float rs[H], rl[H];               // the row's own logit half, and its lse (BWD_ROW)
#pragma unroll
  for (int k = 0; k < H; ++k) {
    rs[k] = MODE == BWD_T ? a.a_src[row * H + k] : a.a_dst[row * H + k];
    rl[k] = MODE == BWD_ROW ? a.lse_in[row * H + k] : 0.f;
  }
  float loc[NV];                    // BWD_ROW: g_i;  BWD_T: h_j;  zero in the lanes that repeat columns
  if (MODE != FWD) {
    load_nv<NV>((MODE == BWD_ROW ? a.g : a.h) + row * W + c0, loc);
    if (!owner) {
#pragma unroll
      for (int j = 0; j < NV; ++j) loc[j] = 0.f;
    }
  }

  // sweep 0 (forward): max and sum of every head's logits over the row's terms
  float mx[H], inv[H];
  if (MODE == FWD) {
    float m[H], s[H];
#pragma unroll
    for (int k = 0; k < H; ++k) { m[k] = -INFINITY; s[k] = 0.f; }
    for (int64_t p = (int64_t)wv * 64 + lane; p < nterm; p += 64 * WPR) {
      const int64_t node = p == 0 ? row : (int64_t)a.col[e0 + p - 1];
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const float z = a.a_src[node * H + k] + rs[k];
        const float e = z > 0.f ? z : a.slope * z;
        const float mn = fmaxf(m[k], e);
        s[k] = s[k] * expf(m[k] - mn) + expf(e - mn);
        m[k] = mn;
      }
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const float M = gcr_wave_max(m[k]);
      s[k] = gcr_wave_sum(m[k] == -INFINITY ? 0.f : s[k] * expf(m[k] - M));
      m[k] = M;
    }
    if (WPR > 1) {
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < H; ++k) { s_sc[wv * 4 * H + 2 * k] = m[k]; s_sc[wv * 4 * H + 2 * k + 1] = s[k]; }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < H; ++k) {
        float M = -INFINITY, S = 0.f;
#pragma unroll 1
        for (int w = 0; w < WPR; ++w) M = fmaxf(M, (float)s_sc[w * 4 * H + 2 * k]);
#pragma unroll 1
        for (int w = 0; w < WPR; ++w) {
          const float mw = (float)s_sc[w * 4 * H + 2 * k];
          S += mw == -INFINITY ? 0.f : (float)s_sc[w * 4 * H + 2 * k + 1] * expf(mw - M);
        }
        m[k] = M; s[k] = S;
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {
      mx[k] = m[k];
      inv[k] = 1.f / (s[k] + 1e-16f);
      if (lane == 0 && wv == 0) a.lse[row * H + k] = m[k] + logf(s[k]);
    }
  }

  float acc[NV];                    // FWD: out_i;  BWD_T: dh_j
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.f;
  double dot_a = 0., dot_d = 0.;    // per-lane parts of A (BWD_ROW) or of da_src's dot part (BWD_T), and of D
  double sc[H], ss[H];              // BWD_ROW: B and the sum of the weights;  BWD_T: sum_i l' alpha_ij D_i
#pragma unroll
  for (int k = 0; k < H; ++k) sc[k] = ss[k] = 0.;

  for (int64_t base = (int64_t)wv * 64; base < nterm; base += 64 * WPR) {
    // sweep 1: this lane's term
    const int64_t p = base + lane;
    const bool live = p < nterm;
    int node = (int)row;
    int64_t eid = 0;
    if (live) {
      if (p == 0) {
        eid = nnz + row;
      } else {
        const int64_t e = e0 + p - 1;
        node = a.col[e];
        eid = a.perm != nullptr ? a.perm[e] : e;
      }
    }
    float wa[H], wb[H];             // the term's weight on the gathered row, and on its dot with `loc` (times l')
#pragma unroll
    for (int k = 0; k < H; ++k) {
      wa[k] = wb[k] = 0.f;
      if (live) {
        const int64_t nk = (int64_t)node * H + k;
        const float z = MODE == BWD_T ? rs[k] + a.a_dst[nk] : a.a_src[nk] + rs[k];
        const float e = z > 0.f ? z : a.slope * z;
        const float lp = z > 0.f ? 1.f : a.slope;
        float mk = 1.f;
        if (a.keep != nullptr) {
          const int64_t b = eid * H + k;
          mk = ((a.keep[b >> 5] >> (b & 31)) & 1u) ? a.keep_scale : 0.f;
        }
        if (MODE == FWD) {
          wa[k] = expf(e - mx[k]) * inv[k] * mk;
        } else if (MODE == BWD_ROW) {
          const float al = expf(e - rl[k]);     // times 1 / ss at the row's end: every sum is linear in it
          wa[k] = al * mk;
          wb[k] = lp * wa[k];
          sc[k] += (double)(lp * al);
          ss[k] += (double)al;
        } else {
          const float al = expf(e - a.lse_in[nk]) * a.rinv_in[nk];
          wa[k] = al * mk;
          if (!(lone && p == 0)) {              // the self loop of a lone node: no part in da_src
            wb[k] = lp * wa[k];
            sc[k] += (double)(lp * al) * (double)a.dd_in[nk];
          }
        }
      }
    }
    // sweep 2: the gathers
    const int cnt = (int)(nterm - base < 64 ? nterm - base : 64);
    for (int u = 0; u < cnt; u += 8) {
      float x[8][NV], fa[8], fb[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int nd = gcr_readlane_i(node, u + t);
        load_nv<NV>(tab + (int64_t)nd * W + c0, x[t]);
        fa[t] = pick_lane<H>(wa, u + t, head);
        if (MODE != FWD) fb[t] = pick_lane<H>(wb, u + t, head);
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        if (MODE == BWD_ROW) {
          float d = 0.f;
#pragma unroll
          for (int j = 0; j < NV; ++j) d = fmaf(loc[j], x[t][j], d);
          dot_d += (double)fa[t] * (double)d;
          dot_a += (double)fb[t] * (double)d;
        } else {
#pragma unroll
          for (int j = 0; j < NV; ++j) acc[j] = fmaf(fa[t], x[t][j], acc[j]);
          if (MODE == BWD_T) {
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) d = fmaf(loc[j], x[t][j], d);
            dot_a += (double)fb[t] * (double)d;
          }
        }
      }
    }
  }

  // the row's sums: over the waves (WPR > 1) in wave order, then over a head's lanes
  if (MODE != BWD_ROW) {
    if (WPR > 1) {
      if (owner) store_nv<NV>(s_vec + wv * W + c0, acc);
      __syncthreads();
      if (wv == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          float t = s_vec[c0 + j];
          for (int w = 1; w < WPR; ++w) t += s_vec[w * W + c0 + j];
          acc[j] = t;
        }
      }
    }
    if (wv == 0 && owner) {
      if (MODE == FWD && a.bias != nullptr) {
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] += a.bias[c0 + j];
      }
      store_nv<NV>(a.out + row * W + c0, acc);
    }
  }
  if (MODE != FWD) {
    double ta = group_sum_f64<G>(dot_a), td = group_sum_f64<G>(dot_d);
    double tsc = 0., tss = 0.;
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const double t = gcr_wave_sum_f64(sc[k]);
      tsc = head == k ? t : tsc;
      if (MODE == BWD_ROW) {
        const double u = gcr_wave_sum_f64(ss[k]);
        tss = head == k ? u : tss;
      }
    }
    if (WPR > 1) {
      __syncthreads();              // s_sc's readers of the last row are done (BWD rows have no sweep 0 barrier)
      if (lane % G == 0 && owner) {
        double* dst = s_sc + wv * 4 * H + 4 * head;
        dst[0] = ta; dst[1] = td; dst[2] = tsc; dst[3] = tss;
      }
      __syncthreads();
      ta = td = tsc = tss = 0.;
      for (int w = 0; w < WPR; ++w) {
        const double* src = s_sc + w * 4 * H + 4 * head;
        ta += src[0]; td += src[1]; tsc += src[2]; tss += src[3];
      }
    }
    if (wv == 0 && lane % G == 0 && owner) {
      if (MODE == BWD_ROW) {
        // lse is rounded to float32, which would scale the whole row's alpha by exp(rounding): renormalise by their sum
        const double rinv = 1. / tss;
        ta *= rinv; td *= rinv; tsc *= rinv;
        a.ds[row * H + head] = lone ? 0.f : (float)(ta - td * tsc);
        a.dd_out[row * H + head] = (float)td;
        a.rinv_out[row * H + head] = (float)rinv;
      } else {
        a.ds[row * H + head] = (float)(ta - tsc);
      }
    }
  }
  if (WPR > 1) __syncthreads();     // the merge buffers are free for the next row
}

template <int W, int H, int MODE>
__global__ __launch_bounds__(256) void gat_rows_kernel(const GatArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= a.n) return;
  if (a.rowptr[row + 1] - a.rowptr[row] > LONG_ROW) return;
  gat_row<W, H, MODE, 1>(a, row, 0, threadIdx.x & 63, nullptr, nullptr);
}

// Row r is looked at by workgroup r % gridDim.x (1024 of a workgroup's rows at a time, one per thread), so that long
// rows with neighbouring numbers (the most popular items of a catalogue sorted by popularity) go to different workgroups;
// a long row is walked by all sixteen waves.  Which workgroup walks a row changes no bit of its result.
template <int W, int H, int MODE>
__global__ __launch_bounds__(LONG_THREADS) void gat_long_kernel(const GatArgs a) {
  constexpr int WPR = LONG_THREADS / 64;
  __shared__ float s_vec[WPR * W];
  __shared__ double s_sc[WPR * 4 * H];
  __shared__ int s_long[LONG_THREADS];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t grid = gridDim.x;
  for (int64_t base = blockIdx.x; base < a.n; base += grid * LONG_THREADS) {
    const int64_t r = base + threadIdx.x * grid;
    const int is_long = r < a.n && a.rowptr[r + 1] - a.rowptr[r] > LONG_ROW;
    s_long[threadIdx.x] = is_long;
    if (__syncthreads_or(is_long)) {
      for (int t = 0; t < LONG_THREADS; ++t)
        if (s_long[t]) gat_row<W, H, MODE, WPR>(a, base + t * grid, wave, threadIdx.x & 63, s_vec, s_sc);
    }
    __syncthreads();
  }
}

bool gat_ok(int heads, int c) {
  return (c == 32 || c == 64 || c == 128) && (heads == 1 || heads == 2 || heads == 4) && heads * c <= 256;
}

// f(integral_constant<W>, integral_constant<H>) for the supported pair
template <class F>
void dispatch_gat(int heads, int c, F&& f) {
  const int w = heads * c;
  dispatch_value<1, 2, 4>(heads, [&](auto hc) {
    constexpr int H = decltype(hc)::value;
    dispatch_value<32, 64, 128, 256>(w, [&](auto wc) {
      constexpr int W = decltype(wc)::value;
      if constexpr (W / H >= 32 && W / H <= 128) f(wc, hc);
    });
  });
}

template <int MODE>
int32_t gat_launch(const GatArgs& a, int heads, int c, hipStream_t s) {
  const dim3 rows_grid((unsigned)((a.n + 3) / 4)), long_grid((unsigned)gcr_grid((a.n + LONG_THREADS - 1) / LONG_THREADS, LONG_CAP));
  int32_t st = GCR_OK;
  dispatch_gat(heads, c, [&](auto wc, auto hc) {
    constexpr int W = decltype(wc)::value, H = decltype(hc)::value;
    hipLaunchKernelGGL((gat_rows_kernel<W, H, MODE>), rows_grid, dim3(256), 0, s, a);
    st = GCR_LAUNCH_STATUS();
    if (st != GCR_OK) return;
    hipLaunchKernelGGL((gat_long_kernel<W, H, MODE>), long_grid, dim3(LONG_THREADS), 0, s, a);
    st = GCR_LAUNCH_STATUS();
  });
  return st;
}

}  // namespace

extern "C" int32_t gcr_gat_supported(int32_t heads, int32_t c) { return gat_ok(heads, c); }

extern "C" int64_t gcr_gat_workspace_bytes(int64_t n, int64_t nnz, int32_t heads, int32_t c) {
  if (n <= 0 || nnz < 0 || !gat_ok(heads, c)) return 0;
  return 2 * gcr_align(n * heads * (int64_t)sizeof(float), 64);    // D [n, H], 1 / (the row's sum of exp(e - lse)) [n, H]
}

extern "C" int32_t gcr_gat_fwd_f32(const int64_t* rowptr, const int32_t* col, int64_t n, const float* h, const float* a_src,
                                   const float* a_dst, int32_t heads, int32_t c, float negative_slope,
                                   const uint32_t* keep_bits, float keep_scale, const float* bias, float* out, float* lse,
                                   void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0);
  if (!gat_ok(heads, c)) return GCR_EUNSUPPORTED;
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(n < (int64_t(1) << 31));
  GCR_CHECK_ARG(rowptr != nullptr && col != nullptr && h != nullptr && a_src != nullptr && a_dst != nullptr &&
                out != nullptr && lse != nullptr && out != h);
  GCR_CHECK_ARG(aligned16(h, a_src, a_dst, bias, out, lse) && aligned16(rowptr, col, keep_bits));
  (void)workspace;
  GatArgs a{};
  a.rowptr = rowptr; a.col = col; a.rowptr_fwd = rowptr; a.n = n;
  a.h = h; a.a_src = a_src; a.a_dst = a_dst; a.slope = negative_slope;
  a.keep = keep_bits; a.keep_scale = keep_scale; a.bias = bias; a.out = out; a.lse = lse;
  return gat_launch<FWD>(a, heads, c, (hipStream_t)stream);
}

extern "C" int32_t gcr_gat_bwd_f32(const int64_t* rowptr, const int32_t* col, const int64_t* rowptr_t, const int32_t* col_t,
                                   const int64_t* perm_t, int64_t n, const float* h, const float* a_src, const float* a_dst,
                                   const float* lse, const float* g, int32_t heads, int32_t c, float negative_slope,
                                   const uint32_t* keep_bits, float keep_scale, float* dh, float* da_src, float* da_dst,
                                   void* workspace, void* stream) {
  GCR_CHECK_ARG(n >= 0);
  if (!gat_ok(heads, c)) return GCR_EUNSUPPORTED;
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(n < (int64_t(1) << 31));
  GCR_CHECK_ARG(rowptr != nullptr && col != nullptr && rowptr_t != nullptr && col_t != nullptr && h != nullptr &&
                a_src != nullptr && a_dst != nullptr && lse != nullptr && g != nullptr && dh != nullptr &&
                da_src != nullptr && da_dst != nullptr && workspace != nullptr && dh != h && dh != g);
  GCR_CHECK_ARG(keep_bits == nullptr || perm_t != nullptr);
  GCR_CHECK_ARG(aligned16(h, a_src, a_dst, lse, g, dh, da_src, da_dst) &&
                aligned16(rowptr, col, rowptr_t, col_t, perm_t, keep_bits) && aligned16(workspace));
  float* dd = reinterpret_cast<float*>(workspace);
  float* rinv = dd + gcr_align(n * heads * (int64_t)sizeof(float), 64) / (int64_t)sizeof(float);
  GatArgs a{};
  a.rowptr = rowptr; a.col = col; a.rowptr_fwd = rowptr; a.n = n;
  a.h = h; a.a_src = a_src; a.a_dst = a_dst; a.lse_in = lse; a.g = g; a.slope = negative_slope;
  a.keep = keep_bits; a.keep_scale = keep_scale; a.ds = da_dst; a.dd_out = dd; a.rinv_out = rinv;
  int32_t st = gat_launch<BWD_ROW>(a, heads, c, (hipStream_t)stream);
  if (st != GCR_OK) return st;
  a.rowptr = rowptr_t; a.col = col_t; a.perm = keep_bits != nullptr ? perm_t : nullptr;
  a.dd_in = dd; a.rinv_in = rinv; a.dd_out = nullptr; a.rinv_out = nullptr; a.out = dh; a.ds = da_src;
  return gat_launch<BWD_T>(a, heads, c, (hipStream_t)stream);
}
