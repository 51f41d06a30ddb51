// k-means E-step of NCL's prototype contrast (ncl.py:340-356): the nearest-centroid search, on the MFMA tile engines of
// gcr_tile.h / gcr_b3.h, then the centroid update and the re-seeding of empty clusters.  The reference delegates to
// faiss.Kmeans(d, k).train(x) — an un-vendored dependency, not installed: what is restated here is faiss' published
// Clustering::train loop (Clustering.cpp: compute_centroids + split_clusters), PARITY WITH FAISS UNPINNED (no fixture
// exists), checked against oracle_np.kmeans_lloyd.
//
// Nothing in here reads anything back to the host: an iteration is a fixed launch sequence (hipGraph-capturable), and the
// rare empty-cluster path runs inside a one-block kernel whose common case is one pass over the k counts.
#include <type_traits>

#include "gcr_b3.h"
#include "gcr_host.h"
#include "gcr_lanes.h"
#include "gcr_philox.h"

namespace {

// ------------------------------------------------------------------------------------------
// Nearest-centroid assignment for the NCL prototype step (ncl.py:340-356: faiss.Kmeans.train +
// index.search(x, 1)): argmin_k ||x_i - c_k||^2 = argmax_k (<x_i, c_k> - 0.5 ||c_k||^2).  Same MFMA
// tile engine as the InfoNCE forward (points stationary on the lanes, centroids streamed through
// LDS); the epilogue is an in-lane running arg-max instead of an exp2-sum.  Ties go to the
// smaller centroid id.
// ------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256, (D <= 64 ? 3 : 2)) void kmeans_assign_kernel(
    const float* __restrict__ x, int64_t n, const float* __restrict__ cent, const float* __restrict__ half_sq,
    int64_t k, int64_t* __restrict__ assign, float* __restrict__ best_out) {
  using S = Shape<D>;
  __shared__ __align__(16) float lds[2][kTileJ * S::STRIDE];
  __shared__ __align__(16) float st_bias[2][kTileJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * (32 * S::NT);
  float bfrag[S::NT][S::KH];
#pragma unroll
  for (int t = 0; t < S::NT; ++t) load_stationary<D>(x, nullptr, n, i0 + 32 * t + i32, h, 1.0f, bfrag[t]);
  float best[S::NT];
  int bidx[S::NT];
#pragma unroll
  for (int t = 0; t < S::NT; ++t) {
    best[t] = -INFINITY;
    bidx[t] = 0x7fffffff;
  }
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  float4 regs[S::NLD];
  float bias = 0.f;
  auto load_bias = [&](int64_t j0) {
    if (tid < kTileJ) bias = (j0 + tid < k) ? -half_sq[j0 + tid] : -INFINITY;  // rows past k never win
  };
  stage_load<D>(cent, nullptr, k, 0, tid, regs);
  load_bias(0);
  stage_store<D>(lds[0], tid, regs);
  if (tid < kTileJ) st_bias[0][tid] = bias;
  __syncthreads();
  for (int64_t tt = 0; tt < tiles; ++tt) {
    const int cur = (int)(tt & 1);
    const int64_t nxt = tt + 1 < tiles ? tt + 1 : tt;
    stage_load<D>(cent, nullptr, k, nxt * kTileJ, tid, regs);
    load_bias(nxt * kTileJ);
    f32x16 acc[S::NT];
    score_tile<D>(lds[cur], i32, h, bfrag, acc);
    const int j0 = (int)(tt * kTileJ);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bb = *reinterpret_cast<const float4*>(&st_bias[cur][8 * g + 4 * h]);
      const float be[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const int j = j0 + acc_row(r, h);
#pragma unroll
        for (int t = 0; t < S::NT; ++t) {
          const float v = acc[t][r] + be[e];
          const bool better = v > best[t] || (v == best[t] && j < bidx[t]);
          best[t] = better ? v : best[t];
          bidx[t] = better ? j : bidx[t];
        }
      }
    }
    stage_store<D>(lds[cur ^ 1], tid, regs);
    if (tid < kTileJ) st_bias[cur ^ 1][tid] = bias;
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < S::NT; ++t) {
    const float v_o = __shfl_xor(best[t], 32, 64);
    const int j_o = __shfl_xor(bidx[t], 32, 64);
    const bool other = v_o > best[t] || (v_o == best[t] && j_o < bidx[t]);
    const float v = other ? v_o : best[t];
    const int j = other ? j_o : bidx[t];
    const int64_t row = i0 + 32 * t + i32;
    if (h == 0 && row < n) {
      assign[row] = j;
      if (best_out != nullptr) best_out[row] = v;
    }
  }
}

// The same on the split-operand engine (d <= 128), software-pipelined by hand like the InfoNCE forward.
// -0.5 ||c||^2 rides in as the MFMA C operand of the tile's first product; the running arg-max costs
// three VALU instructions per score (compare, select the register number, max) plus one tile-number
// select per tile: a lane walks its rows in increasing centroid id, so a strict `>` keeps the smallest
// id among equal scores; the two lane halves are merged with an explicit id comparison at the end.
template <int D>
__global__ __launch_bounds__(256, 2) void kmeans_assign_b3_kernel(
    const float* __restrict__ x, int64_t n, const float* __restrict__ cent, const float* __restrict__ half_sq,
    int64_t k, int64_t* __restrict__ assign, float* __restrict__ best_out, float* __restrict__ acc_sums = nullptr,
    float* __restrict__ acc_counts = nullptr, int n_copies = 1) {
  using S = ShapeB3<D>;
  constexpr int NS = 6 * S::KC * S::NT, NU = 16 * S::NT + S::NLD;
  constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};
  __shared__ __align__(16) unsigned char lds[2][3 * S::PLANE];
  __shared__ __align__(16) float st_bias[2][kTileJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * (32 * S::NT);
  u32x4 bq[S::NT][3][S::KC];
#pragma unroll
  for (int t = 0; t < S::NT; ++t) load_stationary_e<EngB3, D>(x, nullptr, n, i0 + 32 * t + i32, h, 1.0f, bq[t]);
  float best[S::NT];
  int btile[S::NT], breg[S::NT];
#pragma unroll
  for (int t = 0; t < S::NT; ++t) {
    best[t] = -INFINITY;
    btile[t] = 0;
    breg[t] = 0;
  }
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  const int64_t last = tiles - 1;
  // One centroid tile's share of a lane between its global loads and its LDS stores.  The loads are LOADS ONLY — the rows
  // as they are (rows past k repeat the last centroid: their bias is -inf, they never win), ½|c|² as it is, from every
  // lane without a branch — and a tile is loaded a whole step before it is staged.  (The bias used to be negated and
  // selected on the spot inside `if (tid < 32)`, the rows multiplied by their 0/1 scale on the spot: every tile opened with
  // `global_load ...; s_waitcnt vmcnt(0)` in wave 0, a memory round trip that the other three waves sat out at the
  // barrier — half of the 1.9 us a tile took.)
  struct Staged {
    float4 v[S::NLD];
    float hb;
    bool live;
  };
  Staged ga, gb;
  auto load_tile = [&](int64_t t, Staged& g) {
    const int64_t j0 = min(t, last) * kTileJ;
#pragma unroll
    for (int u = 0; u < S::NLD; ++u) {
      const int idx = tid + 256 * u;
      const int row = idx / (D / 4), c4 = idx % (D / 4);
      const int64_t jj = min(j0 + row, k - 1);
      g.v[u] = *reinterpret_cast<const float4*>(cent + jj * D + 4 * c4);
    }
    const int64_t jb = j0 + (tid & (kTileJ - 1));
    g.hb = half_sq[min(jb, k - 1)];
    g.live = jb < k;
  };
  auto store_tile = [&](unsigned char* out, int sbuf, const Staged& g) {
#pragma unroll
    for (int u = 0; u < S::NLD; ++u) stage_store_e_one<EngB3, D>(out, tid, g.v[u], u);
    if (tid < kTileJ) st_bias[sbuf][tid] = g.live ? -g.hb : -INFINITY;          // rows past k never win
  };
  // one tile: scores of the tile in lds[buf] into `nxt` (C = bias), optionally interleaved with the
  // arg-max over `cur` (the previous tile, number tt) and the staging of the tile held in `st`
  auto tile = [&](auto with_cur, const f32x16 (&cur)[S::NT], f32x16 (&nxt)[S::NT], int64_t tt, int buf, const Staged& st) {
    constexpr bool CUR = decltype(with_cur)::value;
    const unsigned char* base = lds[buf] + i32 * S::ROWB + h * (S::KH * 2);
    unsigned char* out = lds[buf ^ 1];
    float binit[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bb = *reinterpret_cast<const float4*>(&st_bias[buf][8 * g + 4 * h]);
      binit[4 * g + 0] = bb.x; binit[4 * g + 1] = bb.y; binit[4 * g + 2] = bb.z; binit[4 * g + 3] = bb.w;
    }
    float bprev[S::NT];
#pragma unroll
    for (int t = 0; t < S::NT; ++t) bprev[t] = best[t];
    auto micro = [&](int m) {
      if (m < 16 * S::NT) {
        const int r = m / S::NT, t = m % S::NT;
        const float v = cur[t][r];
        breg[t] = v > best[t] ? r : breg[t];
        best[t] = fmaxf(best[t], v);
      } else {
        const int u = m - 16 * S::NT;
        stage_store_e_one<EngB3, D>(out, tid, st.v[u], u);
        if (u == 0 && tid < kTileJ) st_bias[buf ^ 1][tid] = st.live ? -st.hb : -INFINITY;
      }
    };
    u32x4 ap[2][3];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) ap[0][pl] = *reinterpret_cast<const u32x4*>(base + pl * S::PLANE);
#pragma unroll
    for (int c = 0; c < S::KC; ++c) {
      if (c + 1 < S::KC) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          ap[(c + 1) & 1][pl] = *reinterpret_cast<const u32x4*>(base + pl * S::PLANE + 16 * (c + 1));
      }
#pragma unroll
      for (int term = 0; term < 6; ++term) {
#pragma unroll
        for (int t = 0; t < S::NT; ++t) {
          const int slot = (c * 6 + term) * S::NT + t;
          f32x16 cin = nxt[t];
          if (c == 0 && term == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cin[r] = binit[r];
          }
          nxt[t] = mfma_bf16(ap[c & 1][TA[term]], bq[t][TB[term]][c], cin);
          if (CUR) {
#pragma unroll
            for (int u = slot * NU / NS; u < (slot + 1) * NU / NS; ++u) micro(u);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (CUR) {
#pragma unroll
      for (int t = 0; t < S::NT; ++t) {
        btile[t] = best[t] > bprev[t] ? (int)tt : btile[t];
        asm volatile("" : "+v"(best[t]), "+v"(breg[t]), "+v"(btile[t]));
      }
    }
  };
  auto argmax_only = [&](const f32x16 (&cur)[S::NT], int64_t tt) {
#pragma unroll
    for (int t = 0; t < S::NT; ++t) {
      const float bp = best[t];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        breg[t] = cur[t][r] > best[t] ? r : breg[t];
        best[t] = fmaxf(best[t], cur[t][r]);
      }
      btile[t] = best[t] > bp ? (int)tt : btile[t];
    }
  };
  f32x16 acc_a[S::NT], acc_b[S::NT];
  load_tile(0, ga);
  load_tile(1, gb);
  store_tile(lds[0], 0, ga);
  load_tile(2, ga);
  __syncthreads();
  tile(std::false_type{}, acc_b, acc_a, 0, 0, gb);      // scores of tile 0; nothing to reduce yet
  store_tile(lds[1], 1, gb);
  __syncthreads();
  int64_t tt = 0;
  for (; tt + 2 <= last; tt += 2) {                     // step tt stages tile tt + 2 (loaded a step ago), loads tile tt + 3
    load_tile(tt + 3, gb);
    tile(std::true_type{}, acc_a, acc_b, tt, 1, ga);
    __syncthreads();
    load_tile(tt + 4, ga);
    tile(std::true_type{}, acc_b, acc_a, tt + 1, 0, gb);
    __syncthreads();
  }
  if (tt < last) {
    tile(std::true_type{}, acc_a, acc_b, tt, 1, ga);
    __syncthreads();
    argmax_only(acc_b, last);
  } else {
    argmax_only(acc_a, last);
  }
#pragma unroll
  for (int t = 0; t < S::NT; ++t) {
    const int jl = best[t] > -INFINITY ? btile[t] * kTileJ + (breg[t] & 3) + 8 * (breg[t] >> 2) + 4 * h : 0x7fffffff;
    const float v_o = __shfl_xor(best[t], 32, 64);
    const int j_o = __shfl_xor(jl, 32, 64);
    const bool other = v_o > best[t] || (v_o == best[t] && j_o < jl);
    const float v = other ? v_o : best[t];
    const int j = other ? j_o : jl;
    const int64_t row = i0 + 32 * t + i32;
    if (h == 0 && row < n) {
      if (assign != nullptr) assign[row] = j;
      if (best_out != nullptr) best_out[row] = v;
    }
    btile[t] = j;                                         // kept for the fused centroid update below
  }
  // Lloyd update fused into the search (gcr_kmeans_assign_accumulate_f32): every point's row is added to its cluster's
  // sum straight away — 256-B float-atomic rows into private copy blockIdx % n_copies — instead of a second kernel that
  // re-reads the assignment.  The rows are re-read from L2 (the registers hold them as bf16 planes); 8 loads in flight.
  if (acc_sums != nullptr) {
    float* __restrict__ sb = acc_sums + (int64_t)(blockIdx.x % n_copies) * k * D;
    float* __restrict__ cb = acc_counts + (int64_t)(blockIdx.x % n_copies) * k;
    constexpr int NVX = (D + 63) / 64;
#pragma unroll
    for (int t = 0; t < S::NT; ++t) {
      // all rows of the tile in flight at once (d <= 64: 32 loads; a batch of 8 per round trip left the wave waiting on
      // eight dependent L2 round trips per tile: ~20 of the iteration's 53 us), then the row atomics
      constexpr int PB = NVX == 1 ? 32 : 8;
      for (int p0 = 0; p0 < 32; p0 += PB) {
        float xv[PB][NVX];
        int cj[PB];
#pragma unroll
        for (int q = 0; q < PB; ++q) {
          const int64_t row = i0 + 32 * t + p0 + q;
          cj[q] = __builtin_amdgcn_readlane(btile[t], p0 + q);
          if (row >= n || cj[q] < 0 || cj[q] >= k) cj[q] = -1;
          const float* xp = x + (row < n ? row : 0) * D;
#pragma unroll
          for (int c = 0; c < NVX; ++c) xv[q][c] = (lane + 64 * c < D) ? xp[lane + 64 * c] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) {
          if (cj[q] < 0) continue;                        // wave-uniform
#pragma unroll
          for (int c = 0; c < NVX; ++c)
            if (lane + 64 * c < D) atomicAdd(sb + (int64_t)cj[q] * D + lane + 64 * c, xv[q][c]);
          if (lane == 0) atomicAdd(cb + cj[q], 1.0f);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// The e_step's search at NCL's sizes (76.8 K sampled points x 300 centroids, 25 times per table and step) is a LATENCY
// problem: the launch above puts ~1 wave on every SIMD, and each of its ten centroid tiles costs a wave the tile's
// staging (split + LDS stores), a workgroup barrier and the first operand reads, none of it hidden — 19 us of search
// for 7 us of matrix work.  Here the centroids are split into their three bf16 planes ONCE per Lloyd iteration, by
// kmeans_image_kernel, into an image in MFMA-fragment order: for tile T, k-chunk c, plane p the 64 lanes' operand
// registers are 1 KB of consecutive memory — one coalesced global_load_dwordx4 per fragment, served by L2 (120 KB for
// k = 300).  A wave then needs no LDS, no barrier and no partner: 32 points stationary in registers (NT = 1: twice the
// waves of the tiled kernel, so that the 1024 SIMDs hold 2-3 each), the next tile's twelve fragments in flight while
// this tile's 24 MFMAs run, the running arg-max of the previous tile in their shadow.
// ------------------------------------------------------------------------------------------
// image[((T * KC + c) * 3 + p) * 64 + lane] = the 8 bf16 of plane p, features [h * KH + 8 c, + 8) of centroid 32 T + i32
// (lane = 32 h + i32); bias[32 T + r] = -0.5 |c|^2, -inf past k (such a row never wins).
template <int D>
__global__ __launch_bounds__(256) void kmeans_image_kernel(const float* __restrict__ cent, const float* __restrict__ half_sq,
                                                           int64_t k, u32x4* __restrict__ image, float* __restrict__ bias) {
  using S = ShapeB3<D>;
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one thread per (tile, chunk, lane)
  if (idx < tiles * kTileJ) bias[idx] = idx < k ? -half_sq[idx] : -INFINITY;
  if (idx >= tiles * S::KC * 64) return;
  const int lane = (int)(idx & 63);
  const int c = (int)((idx >> 6) % S::KC);
  const int64_t T = (idx >> 6) / S::KC;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t row = T * kTileJ + i32;
  float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
  if (row < k) {
    const float* p = cent + row * D + h * S::KH + 8 * c;
    v0 = *reinterpret_cast<const float4*>(p);
    v1 = *reinterpret_cast<const float4*>(p + 4);
  }
  unsigned q[3][4];
  split3(v0.x, v0.y, q[0][0], q[1][0], q[2][0]);
  split3(v0.z, v0.w, q[0][1], q[1][1], q[2][1]);
  split3(v1.x, v1.y, q[0][2], q[1][2], q[2][2]);
  split3(v1.z, v1.w, q[0][3], q[1][3], q[2][3]);
#pragma unroll
  for (int pl = 0; pl < 3; ++pl)
    image[((T * S::KC + c) * 3 + pl) * 64 + lane] = (u32x4){q[pl][0], q[pl][1], q[pl][2], q[pl][3]};
}

// One fragment of the same image (the layout of kmeans_image_kernel above), for the update kernels below that rewrite
// single centroids: the 8 features [8 * col8, + 8) of centroid `row`, three planes.
__device__ __forceinline__ void image_store_fragment(u32x4* __restrict__ image, int d, int64_t row, int col8, const float (&v)[8]) {
  const int kh = d / 2, kc = d / 16;
  const int feat = 8 * col8, h = feat / kh, c = (feat % kh) / 8;
  const int64_t T = row / kTileJ;
  const int lane = 32 * h + (int)(row % kTileJ);
  unsigned q[3][4];
  split3(v[0], v[1], q[0][0], q[1][0], q[2][0]);
  split3(v[2], v[3], q[0][1], q[1][1], q[2][1]);
  split3(v[4], v[5], q[0][2], q[1][2], q[2][2]);
  split3(v[6], v[7], q[0][3], q[1][3], q[2][3]);
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) image[((T * kc + c) * 3 + pl) * 64 + lane] = (u32x4){q[pl][0], q[pl][1], q[pl][2], q[pl][3]};
}

// LOWREG: the same search at <= 128 registers per lane (four waves per SIMD): fragments are fetched one k-chunk ahead
// (three 16-B loads in flight per lane instead of two tiles' worth), one accumulator, the arg-max right behind its tile —
// each wave now stalls on L2 latency, and the other three waves of the SIMD cover it.  What it buys is CO-RESIDENCE: a
// wave of this kernel fits into the registers the InfoNCE loops of the same training step leave free on a SIMD (2 x 176-192
// of 512), so the e_step's chain of small launches no longer waits for those grids to drain.
// INCR (gcr_kmeans_search_image_incr_f32): the cluster sums are kept in 64-bit FIXED POINT across the Lloyd iterations and
// only the points whose assignment CHANGED touch them — the row leaves its old cluster's sum and joins the new one's.
// Integer adds are exact and commute, so the incremental sums equal a fresh accumulation bit for bit, in any order: no
// drift over the 25 iterations, and the e_step becomes run-to-run reproducible (float row atomics are not).  After the first
// iterations a few per cent of the points move, and the accumulation — 15-19 of an iteration's ~46 us as float row atomics
// at the memory-side unit's rate — all but disappears (3-4 full passes' worth over 25 iterations instead of 25).
// q = round(x * qscale[0]), qscale[0] a power of two with |q| < 2^30 (set from max |x| by the caller).
template <int D, bool LOWREG = false, bool INCR = false>
__global__ __launch_bounds__(256, LOWREG ? 4 : 2) void kmeans_search_img_kernel(
    const float* __restrict__ x, int64_t n, const u32x4* __restrict__ image, const float* __restrict__ bias, int64_t k,
    int64_t* __restrict__ assign, float* __restrict__ acc_sums, float* __restrict__ acc_counts, int n_copies,
    int32_t* __restrict__ prev_assign = nullptr, const float* __restrict__ qscale = nullptr,
    long long* __restrict__ sums_q = nullptr, int32_t* __restrict__ counts_i = nullptr) {
  using S = ShapeB3<D>;
  constexpr int KC = S::KC, NF = 3 * KC;                   // fragments per centroid tile
  constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};     // (streamed plane, stationary plane), smallest terms first
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
  if (i0 >= n) return;                                      // (whole waves only: nothing below synchronises across waves)
  u32x4 bq[3][KC];
  load_stationary_e<EngB3, D>(x, nullptr, n, i0 + i32, h, 1.0f, bq);
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  float best = -INFINITY;
  int btile = 0, breg = 0;
  u32x4 fa[NF], fb[NF];
  float4 ba[4], bb[4];
  auto load_tile = [&](int64_t t, u32x4 (&f)[NF], float4 (&b4)[4]) {
    const int64_t tt = min(t, tiles - 1);
    const u32x4* base = image + tt * (NF * 64) + lane;
#pragma unroll
    for (int q = 0; q < NF; ++q) f[q] = base[q * 64];
#pragma unroll
    for (int g = 0; g < 4; ++g) b4[g] = *reinterpret_cast<const float4*>(bias + tt * kTileJ + 8 * g + 4 * h);
  };
  auto scores = [&](const u32x4 (&f)[NF], const float4 (&b4)[4], f32x16& acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      acc[4 * g + 0] = b4[g].x; acc[4 * g + 1] = b4[g].y; acc[4 * g + 2] = b4[g].z; acc[4 * g + 3] = b4[g].w;
    }
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
      for (int term = 0; term < 6; ++term) acc = mfma_bf16(f[c * 3 + TA[term]], bq[TB[term]][c], acc);
  };
  auto argmax = [&](const f32x16& acc, int64_t t) {
    const float bp = best;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      breg = acc[r] > best ? r : breg;
      best = fmaxf(best, acc[r]);
    }
    btile = best > bp ? (int)t : btile;                     // a lane walks its rows in increasing centroid id: strict > keeps the smallest
  };
  if constexpr (LOWREG) {
    const u32x4* fp = image + lane;
    u32x4 cur[3], nxt[3];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) cur[pl] = fp[pl * 64];
    for (int64_t t = 0; t < tiles; ++t) {
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 b4 = *reinterpret_cast<const float4*>(bias + t * kTileJ + 8 * g + 4 * h);
        acc[4 * g + 0] = b4.x; acc[4 * g + 1] = b4.y; acc[4 * g + 2] = b4.z; acc[4 * g + 3] = b4.w;
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        // the next chunk's three fragments (the next tile's first ones behind the last chunk; the image is read once past
        // its end by the last tile: clamped)
        const int64_t nq = min((t * KC + c + 1) * 3, (tiles * KC - 1) * 3);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) nxt[pl] = fp[(nq + pl) * 64];
#pragma unroll
        for (int term = 0; term < 6; ++term) acc = mfma_bf16(cur[TA[term]], bq[TB[term]][c], acc);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) cur[pl] = nxt[pl];
      }
      argmax(acc, t);
    }
  } else {
  f32x16 acc_a, acc_b;
  load_tile(0, fa, ba);
  load_tile(1, fb, bb);
  scores(fa, ba, acc_a);
  int64_t t = 0;
  for (; t + 2 < tiles; t += 2) {                           // tile t's scores are in acc_a, tile t + 1's fragments in fb
    load_tile(t + 2, fa, ba);
    scores(fb, bb, acc_b);
    argmax(acc_a, t);
    load_tile(t + 3, fb, bb);
    scores(fa, ba, acc_a);
    argmax(acc_b, t + 1);
  }
  argmax(acc_a, t);
  if (t + 1 < tiles) {
    scores(fb, bb, acc_b);
    argmax(acc_b, t + 1);
  }
  }
  const int jl = best > -INFINITY ? btile * kTileJ + (breg & 3) + 8 * (breg >> 2) + 4 * h : 0x7fffffff;
  const float v_o = __shfl_xor(best, 32, 64);
  const int j_o = __shfl_xor(jl, 32, 64);
  const bool other = v_o > best || (v_o == best && j_o < jl);
  const int j = other ? j_o : jl;
  const int64_t row = i0 + i32;
  if (h == 0 && row < n && assign != nullptr) assign[row] = j;
  if constexpr (INCR) {
    const float qs = qscale[0];
    // private copy = workgroup % n_copies (the first iterations move every point: 76.8 K 512-B rows onto a few hundred
    // rows of ONE copy serialise in the memory-side atomic unit: 144 us for the first launch); integer sums of the copies
    // add up exactly, whichever copy a row joined and whichever it leaves
    sums_q += (int64_t)(blockIdx.x % n_copies) * k * D;
    counts_i += (int64_t)(blockIdx.x % n_copies) * k;
    const int old_l = (h == 0 && row < n) ? prev_assign[row] : -1;
    const bool moved_l = h == 0 && row < n && old_l != j;
    if (moved_l) prev_assign[row] = j;
    unsigned long long moved = __ballot(moved_l);           // bit q: point q of the wave changed cluster
    while (moved != 0ull) {                                 // wave-uniform walk over the moved points only
      const int q = __builtin_ctzll(moved);
      moved &= moved - 1ull;
      const int cn = __builtin_amdgcn_readlane(j, q), co = __builtin_amdgcn_readlane(old_l, q);
      const float* xp = x + (i0 + q) * D;
#pragma unroll
      for (int c = 0; c < (D + 63) / 64; ++c) {
        if (lane + 64 * c < D) {
          const long long v = __float2ll_rn(xp[lane + 64 * c] * qs);
          if (cn >= 0 && cn < k) atomicAdd(reinterpret_cast<unsigned long long*>(sums_q + (int64_t)cn * D + lane + 64 * c), (unsigned long long)v);
          if (co >= 0 && co < k) atomicAdd(reinterpret_cast<unsigned long long*>(sums_q + (int64_t)co * D + lane + 64 * c), (unsigned long long)(-v));
        }
      }
      if (lane == 0) {
        if (cn >= 0 && cn < k) atomicAdd(counts_i + cn, 1);
        if (co >= 0 && co < k) atomicAdd(counts_i + co, -1);
      }
    }
    return;
  }
  if (acc_sums == nullptr) return;
  // Lloyd update fused in, as in kmeans_assign_b3_kernel: every point's row goes to its cluster's sum as one 256-B
  // float-atomic row (private copy = workgroup % n_copies), all 32 rows of the wave loaded before the first atomic
  float* __restrict__ sb = acc_sums + (int64_t)(blockIdx.x % n_copies) * k * D;
  float* __restrict__ cb = acc_counts + (int64_t)(blockIdx.x % n_copies) * k;
  constexpr int NVX = (D + 63) / 64;
  constexpr int PB = 32;                                    // rows in flight (the point planes are dead by now)
#pragma unroll
  for (int p0 = 0; p0 < 32; p0 += PB) {
    float xv[PB][NVX];
    int cj[PB];
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      const int64_t r = i0 + p0 + q;
      cj[q] = __builtin_amdgcn_readlane(j, p0 + q);
      if (r >= n || cj[q] < 0 || cj[q] >= k) cj[q] = -1;
      const float* xp = x + (r < n ? r : 0) * D;
#pragma unroll
      for (int c = 0; c < NVX; ++c) xv[q][c] = (lane + 64 * c < D) ? xp[lane + 64 * c] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      if (cj[q] < 0) continue;                              // wave-uniform
#pragma unroll
      for (int c = 0; c < NVX; ++c)
        if (lane + 64 * c < D) atomicAdd(sb + (int64_t)cj[q] * D + lane + 64 * c, xv[q][c]);
      if (lane == 0) atomicAdd(cb + cj[q], 1.0f);
    }
  }
}

// (Tried and removed in round 4: the image shared by a workgroup's four waves through a four-slot LDS ring filled by LDS-DMA
// three tiles ahead — global_load_lds issued from inline assembly so that hipcc does not drain it with vmcnt(0), counted
// vmcnt + one raw s_barrier per tile, 64 points per wave: an eighth of the L2 traffic, same assignments, 29.4 us against
// 27.4 us for the search alone and 8.74 against 8.42 ms for the NCL iteration.  The three designs — LDS staging with a
// barrier per tile 32 us, per-wave L2 streaming 27 us, LDS-DMA ring 29 us — all sit at ~2 us per centroid tile for 0.75 us
// of matrix work at 2.4 GHz: what they share is 2400 wave-tiles on 1024 SIMDs (2.3 per SIMD: a makespan of 3) and the
// clock the chip holds under 1024 SIMDs of back-to-back bf16 MFMAs, not their operand path.)

// ------------------------------------------------------------------------------------------
// The centroid update and the re-seeding of empty clusters.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kStreamSplit = 0x4B4D5350u;  // 'KMSP'

// sums[c] += x_i (256-B float-atomic rows), counts[c] += 1, one wave per point.  n_copies > 1: block b adds into private
// copy b % n_copies of (sums, counts) — with a few hundred clusters every point of a 77K-point training set would
// otherwise hit one of ~300 rows (the memory-side atomic unit serialises adds to one row); the finalize kernel sums the copies.
__global__ __launch_bounds__(256) void kmeans_accumulate_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                const int64_t* __restrict__ assign, int64_t k,
                                                                float* __restrict__ sums, float* __restrict__ counts,
                                                                int n_copies = 1) {
  const int lane = threadIdx.x & 63;
  sums += (int64_t)(blockIdx.x % n_copies) * k * d;
  counts += (int64_t)(blockIdx.x % n_copies) * k;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
    const int64_t c = assign[i];
    if (c < 0 || c >= k) continue;
    for (int col = lane; col < d; col += 64) atomicAdd(sums + c * d + col, x[i * d + col]);
    if (lane == 0) atomicAdd(counts + c, 1.0f);
  }
}

// The same sums from the points ORDERED by cluster (gcr_sort_index of `assign`): a wave walks 64 consecutive
// entries, adds every run of equal cluster ids in registers and issues one row atomic per run and chunk
// (1M x 64 points: 0.42 ms with one atomic row per point).
__global__ __launch_bounds__(256) void kmeans_accumulate_sorted_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                       const uint32_t* __restrict__ keys,
                                                                       const int32_t* __restrict__ perm, int64_t k,
                                                                       float* __restrict__ sums,
                                                                       float* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t n_chunks = (n + 63) / 64;
  for (int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); chunk < n_chunks; chunk += (int64_t)gridDim.x * 4) {
    const int64_t c0 = chunk * 64;
    const int cnt = (int)(n - c0 < 64 ? n - c0 : 64);
    uint32_t my_key = 0xFFFFFFFFu;
    int my_row = 0;
    if (lane < cnt) {
      my_key = keys[c0 + lane];
      my_row = perm[c0 + lane];
      if (my_key >= (uint32_t)k) my_key = 0xFFFFFFFFu;
    }
    uint32_t cur = 0xFFFFFFFFu;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float run = 0.f;
    auto flush = [&]() {
      if (cur != 0xFFFFFFFFu) {
        for (int v = 0; v < 4; ++v) {
          const int c = lane + 64 * v;
          if (c < d) atomicAdd(sums + (int64_t)cur * d + c, acc[v]);
        }
        if (lane == 0) atomicAdd(counts + cur, run);
      }
    };
    constexpr int kGather = 8;
    for (int e0 = 0; e0 < cnt; e0 += kGather) {
      uint32_t key[kGather];
      float row[kGather][4];
#pragma unroll
      for (int q = 0; q < kGather; ++q) {
        const int e = e0 + q < cnt ? e0 + q : cnt - 1;
        key[q] = e0 + q < cnt ? (uint32_t)__builtin_amdgcn_readlane((int)my_key, e) : 0xFFFFFFFFu;
        const int64_t r = key[q] != 0xFFFFFFFFu ? (int64_t)__builtin_amdgcn_readlane(my_row, e) : 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int c = lane + 64 * v;
          row[q][v] = c < d ? x[r * d + c] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < kGather; ++q) {
        if (key[q] == 0xFFFFFFFFu) continue;
        if (key[q] != cur) {
          flush();
          cur = key[q];
          run = 0.f;
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[v] = 0.f;
        }
        run += 1.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] += row[q][v];
      }
    }
    flush();
  }
}

// centroid = sum / count (empty clusters keep their previous centroid); half_sq = 0.5 ||c||^2
__global__ __launch_bounds__(256) void kmeans_finalize_kernel(const float* __restrict__ sums,
                                                              const float* __restrict__ counts, int64_t k, int d,
                                                              float* __restrict__ cent, float* __restrict__ half_sq) {
  const int l16 = threadIdx.x & 15;
  for (int64_t c = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); c < k; c += (int64_t)gridDim.x * 16) {
    const float cnt = counts != nullptr ? counts[c] : 0.f;
    float ss = 0.f;
    for (int col = l16; col < d; col += 16) {
      float v = cent[c * d + col];
      if (cnt > 0.f) {
        v = sums[c * d + col] / cnt;
        cent[c * d + col] = v;
      }
      ss += v * v;
    }
    ss = gcr_group16_sum(ss);
    if (l16 == 0) half_sq[c] = 0.5f * ss;
  }
}


// centroid = sum / count (empty clusters keep their previous centroid); half_sq = 0.5 ||c||^2; the sums are CLEARED on the
// way out (the next iteration's accumulate adds into zeros: no memset launches between iterations)
__global__ __launch_bounds__(256) void kmeans_finalize_clear_kernel(float* __restrict__ sums, float* __restrict__ counts,
                                                                    int64_t k, int d, float* __restrict__ cent,
                                                                    float* __restrict__ half_sq, int n_copies) {
  // one thread per centroid ELEMENT (a thread per row or a 16-lane group per row leaves a k = 300 update on 19
  // workgroups, each walking the copies serially: 18-22 us); d divides 256 (32 / 64 / 128 / 256), so a row never
  // straddles workgroups.  The copies are read with independent loads first and cleared afterwards.
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t idx = (int64_t)blockIdx.x * 256 + tid;
  const int64_t c = idx / d;
  const int col = (int)(idx % d);
  const bool valid = c < k;
  const int64_t kd = k * (int64_t)d;
  float cnt = 0.f, sum = 0.f, v = 0.f;
  if (valid) {
    for (int g = 0; g < n_copies; ++g) cnt += counts[(int64_t)g * k + c];      // copies in a fixed order
    const float* p = sums + c * d + col;
    int g = 0;
    for (; g + 4 <= n_copies; g += 4) {
      const float a0 = p[(int64_t)g * kd], a1 = p[(int64_t)(g + 1) * kd], a2 = p[(int64_t)(g + 2) * kd],
                  a3 = p[(int64_t)(g + 3) * kd];
      sum += a0;
      sum += a1;
      sum += a2;
      sum += a3;
    }
    for (; g < n_copies; ++g) sum += p[(int64_t)g * kd];
    v = cent[c * d + col];
    if (cnt > 0.f) {
      v = sum / cnt;
      cent[c * d + col] = v;
    }
    for (g = 0; g < n_copies; ++g) sums[(int64_t)g * kd + c * d + col] = 0.f;
  }
  float ss = v * v;
  if (d <= 64) {
    for (int off = d >> 1; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);     // butterfly inside the row's d lanes
  } else {
    ss = gcr_wave_sum(ss);
    if (lane == 0) red[tid >> 6] = ss;
    __syncthreads();
    const int w0 = (tid >> 6) / (d >> 6) * (d >> 6);                                 // first wave of this row
    ss = 0.f;
    for (int w = 0; w < (d >> 6); ++w) ss += red[w0 + w];
  }
  if (valid && col == 0) {
    half_sq[c] = 0.5f * ss;
    counts[c] = cnt;                                       // the total, for the split step (which clears it)
    for (int g = 1; g < n_copies; ++g) counts[(int64_t)g * k + c] = 0.f;
  }
}

// centroid = fixed-point sum / (scale * count) from the INCREMENTAL sums of gcr_kmeans_search_image_incr_f32 (nothing is
// cleared: the sums persist across the iterations); an empty cluster keeps its centroid; half_sq = 0.5 |c|^2; the float
// copy of the counts is what the split step reads (and clears).  One thread per centroid element, d divides 256.
__global__ __launch_bounds__(256) void kmeans_finalize_q_kernel(const long long* __restrict__ sums_q,
                                                                const int32_t* __restrict__ counts_i, const float* __restrict__ qscale,
                                                                int64_t k, int d, float* __restrict__ cent, float* __restrict__ half_sq,
                                                                float* __restrict__ counts_f, u32x4* __restrict__ image,
                                                                float* __restrict__ bias, int n_copies) {
  __shared__ float red[4];
  __shared__ float rowbuf[256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t idx = (int64_t)blockIdx.x * 256 + tid;
  const int64_t c = idx / d;
  const int col = (int)(idx % d);
  const bool valid = c < k;
  float v = 0.f;
  int cnt = 0;
  if (valid) {
    long long sum = 0;
    for (int g = 0; g < n_copies; ++g) {                     // integer sums: exact in any order
      cnt += counts_i[(int64_t)g * k + c];
      sum += sums_q[((int64_t)g * k + c) * d + col];
    }
    v = cent[c * d + col];
    if (cnt > 0) {
      v = (float)((double)sum * (double)qscale[1] / (double)cnt);
      cent[c * d + col] = v;
    }
  }
  float ss = v * v;
  if (d <= 64) {
    for (int off = d >> 1; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
  } else {
    ss = gcr_wave_sum(ss);
    if (lane == 0) red[tid >> 6] = ss;
    __syncthreads();
    const int w0 = (tid >> 6) / (d >> 6) * (d >> 6);
    ss = 0.f;
    for (int w = 0; w < (d >> 6); ++w) ss += red[w0 + w];
  }
  if (valid && col == 0) {
    half_sq[c] = 0.5f * ss;
    counts_f[c] = (float)cnt;
    if (bias != nullptr) bias[c] = -0.5f * ss;
  }
  if (image != nullptr) {                                  // this row's fragments of the search kernel's operand image
    rowbuf[tid] = v;
    __syncthreads();
    if (valid && (col & 7) == 0) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = rowbuf[tid + e];
      image_store_fragment(image, d, c, col >> 3, f);
    }
  }
}

constexpr int kSplitThreads = 256;    // (1024 at first: beside the backward of the NCL step a sixteen-wave workgroup waited up to 0.6 ms for a CU)

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* sh, Op op) {
  // 1024 threads = 16 waves: wave butterfly, then wave 0 folds the 16 wave results; every thread gets the result
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  __syncthreads();                                   // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = sh[0];
#pragma unroll
  for (int w = 1; w < kSplitThreads / 64; ++w) r = op(r, sh[w]);
  return r;
}

// faiss Clustering.cpp `split_clusters`: every empty cluster ci (ascending) takes over a copy of the centroid of a cluster
// cj found by walking cj = 0, 1, ..., k-1, 0, ... and accepting cj with probability (size_cj - 1) / (n - k) (so never an
// empty or one-point cluster); the two copies are pushed apart by the symmetric perturbation (1 +- 1/1024) alternating
// over the dimensions; the sizes are split in half.  faiss draws from a generator seeded 1234 inside the call; here trial
// q of the e-th empty cluster of iteration `iter` is the Philox word x of counter (q, e, iter, 'KMSP') under key `seed`
// (oracle_np.kmeans_split_clusters restates it).  A walk of 64 k trials without a hit (probability < e^-60 unless nearly
// every cluster has <= 1 point) falls back to the largest cluster (smallest id among ties) when it has >= 2 points, and
// leaves the centroid alone otherwise.  One block; the common case (no empty cluster) is one pass over the counts.
// The counts are CLEARED on the way out.
__global__ __launch_bounds__(kSplitThreads) void kmeans_split_kernel(float* __restrict__ counts, int64_t k, int d,
                                                                     float* __restrict__ cent, float* __restrict__ half_sq,
                                                                     int64_t n_points, uint64_t seed, uint32_t iter,
                                                                     int32_t* __restrict__ n_split_out,
                                                                     u32x4* __restrict__ image = nullptr,
                                                                     float* __restrict__ bias = nullptr) {
  __shared__ long long sh_ll[kSplitThreads / 64];
  __shared__ float sh_f[kSplitThreads / 64];
  const int tid = threadIdx.x;
  auto min_ll = [](long long a, long long b) { return a < b ? a : b; };
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const double denom = (double)(n_points - k);
  long long last = -1;
  int n_split = 0;
  for (uint32_t e = 0;; ++e) {
    // next empty cluster after `last` (the set of empty clusters is fixed: a split gives ci >= 1 point and leaves cj >= 1)
    long long ci = k;
    for (long long c = last + 1 + tid; c < k; c += kSplitThreads)
      if (counts[c] == 0.f) { ci = c; break; }
    ci = block_reduce<long long>(ci, sh_ll, min_ll);
    if (ci >= k) break;
    last = ci;
    long long hit = -1;
    if (denom > 0.0) {
      const long long max_trials = 64 * (long long)k;
      for (long long q0 = 0; q0 < max_trials && hit < 0; q0 += kSplitThreads) {
        const long long q = q0 + tid;
        long long mine = max_trials;
        if (q < max_trials) {
          const long long cj = q % k;
          const float p = (float)(((double)counts[cj] - 1.0) / denom);
          const U4 r = philox4x32_10(U4{(uint32_t)q, e, iter, kStreamSplit}, k0 + (uint32_t)((uint64_t)q >> 32), k1);
          const float u = (float)(r.x >> 8) * (1.0f / 16777216.0f);
          if (u < p) mine = q;
        }
        const long long first = block_reduce<long long>(mine, sh_ll, min_ll);
        if (first < max_trials) hit = first % k;
      }
    }
    if (hit < 0) {                      // fallback: the largest cluster, if it can be split at all
      float best = -1.f;
      long long arg = k;
      for (long long c = tid; c < k; c += kSplitThreads)
        if (counts[c] > best) { best = counts[c]; arg = c; }
      const float bmax = block_reduce<float>(best, sh_f, [](float a, float b) { return a > b ? a : b; });
      const long long barg = block_reduce<long long>(best == bmax ? arg : (long long)k, sh_ll, min_ll);
      if (bmax >= 2.f) hit = barg;
    }
    if (hit >= 0) {
      const long long cj = hit;
      float ss_i = 0.f, ss_j = 0.f;
      for (int col = tid; col < d; col += kSplitThreads) {
        const float c0 = cent[cj * d + col];
        const float up = c0 * (1.0f + 1.0f / 1024.0f), dn = c0 * (1.0f - 1.0f / 1024.0f);
        const float vi = (col & 1) == 0 ? up : dn, vj = (col & 1) == 0 ? dn : up;
        cent[ci * d + col] = vi;
        cent[cj * d + col] = vj;
        ss_i += vi * vi;
        ss_j += vj * vj;
      }
      auto add_f = [](float a, float b) { return a + b; };
      ss_i = block_reduce<float>(ss_i, sh_f, add_f);
      ss_j = block_reduce<float>(ss_j, sh_f, add_f);
      if (image != nullptr) {                                // the two rewritten rows in the search kernel's operand image
        __syncthreads();                                     // (this block's own stores to cent above)
        if (tid < 2 * (d / 8)) {
          const long long row = tid < d / 8 ? ci : cj;
          const int col8 = tid % (d / 8);
          float f[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = cent[row * d + 8 * col8 + e];
          image_store_fragment(image, d, row, col8, f);
        }
        if (tid == 0) {
          bias[ci] = -0.5f * ss_i;
          bias[cj] = -0.5f * ss_j;
        }
      }
      if (tid == 0) {
        half_sq[ci] = 0.5f * ss_i;
        half_sq[cj] = 0.5f * ss_j;
        const float ni = floorf(counts[cj] * 0.5f);       // hassign[ci] = hassign[cj] / 2 on integral floats
        counts[ci] = ni;
        counts[cj] -= ni;
      }
      ++n_split;
    }
    __syncthreads();                    // counts / centroids of this split visible to the next walk
  }
  __syncthreads();
  for (long long c = tid; c < k; c += kSplitThreads) counts[c] = 0.f;
  if (tid == 0 && n_split_out != nullptr && n_split > 0) atomicAdd(n_split_out, n_split);
}

}  // namespace

extern "C" int64_t gcr_kmeans_image_bytes(int64_t k, int32_t d) {
  if (k < 1 || !(d == 32 || d == 64 || d == 128)) return 0;
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  return tiles * (3 * (d / 16) * 64 * 16 + kTileJ * (int64_t)sizeof(float));      // fragments, then the bias rows
}

extern "C" int32_t gcr_kmeans_centroid_image_f32(const float* centroids, const float* half_sqnorm, int64_t k, int32_t d,
                                                 void* image, void* stream) {
  GCR_CHECK_ARG(k >= 1 && k < (1ll << 31));
  if (!(d == 32 || d == 64 || d == 128)) return GCR_EUNSUPPORTED;
  GCR_CHECK_ARG(centroids && half_sqnorm && image);
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  u32x4* img = reinterpret_cast<u32x4*>(image);
  float* bias = reinterpret_cast<float*>(img + tiles * 3 * (d / 16) * 64);
  const int64_t threads = tiles * (d / 16) * 64;           // >= tiles * 32: covers the bias rows too
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((threads + 255) / 256));
  switch (d) {
    case 32: hipLaunchKernelGGL((kmeans_image_kernel<32>), grid, dim3(256), 0, s, centroids, half_sqnorm, k, img, bias); break;
    case 64: hipLaunchKernelGGL((kmeans_image_kernel<64>), grid, dim3(256), 0, s, centroids, half_sqnorm, k, img, bias); break;
    default: hipLaunchKernelGGL((kmeans_image_kernel<128>), grid, dim3(256), 0, s, centroids, half_sqnorm, k, img, bias); break;
  }
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_kmeans_search_image_f32(const float* x, int64_t n, const void* image, int64_t k, int32_t d,
                                               int64_t* assign, float* sums, float* counts, int32_t n_copies, uint32_t flags,
                                               void* stream) {
  GCR_CHECK_ARG(n >= 0 && k >= 1 && k < (1ll << 31) && (flags & ~(uint32_t)GCR_KMEANS_SEARCH_LOW_REGISTERS) == 0);
  if (!(d == 32 || d == 64)) return GCR_EUNSUPPORTED;      // (d = 128: the point planes + two tiles of fragments exceed 256 registers)
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(x && image && (assign || sums));
  GCR_CHECK_ARG((sums == nullptr) == (counts == nullptr) && (sums == nullptr || (n_copies >= 1 && n_copies <= 64)));
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  const u32x4* img = reinterpret_cast<const u32x4*>(image);
  const float* bias = reinterpret_cast<const float*>(img + tiles * 3 * (d / 16) * 64);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + 127) / 128));
  const bool low = (flags & GCR_KMEANS_SEARCH_LOW_REGISTERS) != 0;
  dispatch_value<32, 64>(d, [&](auto dc) {
    dispatch_bool(low, [&](auto lo) {
      hipLaunchKernelGGL((kmeans_search_img_kernel<decltype(dc)::value, decltype(lo)::value>), grid, dim3(256), 0, s, x, n, img,
                         bias, k, assign, sums, counts, (int)n_copies);
    });
  });
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_kmeans_search_image_incr_f32(const float* x, int64_t n, const void* image, int64_t k, int32_t d,
                                                    int32_t* prev_assign, const float* qscale, int64_t* sums_q,
                                                    int32_t* counts, int32_t n_copies, uint32_t flags, void* stream) {
  GCR_CHECK_ARG(n >= 0 && k >= 1 && k < (1ll << 31) && (flags & ~(uint32_t)GCR_KMEANS_SEARCH_LOW_REGISTERS) == 0);
  GCR_CHECK_ARG(n_copies >= 1 && n_copies <= 64);
  if (!(d == 32 || d == 64)) return GCR_EUNSUPPORTED;
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(x && image && prev_assign && qscale && sums_q && counts);
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  const u32x4* img = reinterpret_cast<const u32x4*>(image);
  const float* bias = reinterpret_cast<const float*>(img + tiles * 3 * (d / 16) * 64);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + 127) / 128));
  const bool low = (flags & GCR_KMEANS_SEARCH_LOW_REGISTERS) != 0;
  long long* sq = reinterpret_cast<long long*>(sums_q);
  dispatch_value<32, 64>(d, [&](auto dc) {
    dispatch_bool(low, [&](auto lo) {
      hipLaunchKernelGGL((kmeans_search_img_kernel<decltype(dc)::value, decltype(lo)::value, true>), grid, dim3(256), 0, s, x, n,
                         img, bias, k, (int64_t*)nullptr, (float*)nullptr, (float*)nullptr, (int)n_copies, prev_assign, qscale,
                         sq, counts);
    });
  });
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_kmeans_assign_f32(const float* x, int64_t n, const float* centroids, const float* half_sqnorm,
                                         int64_t k, int32_t d, int64_t* assign, float* best_score, void* stream) {
  GCR_CHECK_ARG(n >= 0 && k >= 1 && k < (1ll << 31));
  if (!dim_supported(d)) return GCR_EUNSUPPORTED;
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(x && centroids && half_sqnorm && assign);
  hipStream_t s = (hipStream_t)stream;
  const bool b3 = use_b3(d);
  dispatch_value<32, 64, 128, 256>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    if constexpr (D <= 128) {                                  // the split-operand engine has no d = 256 form
      if (b3) {
        constexpr int ROWS = ShapeB3<D>::ANCHORS_PER_BLOCK;
        hipLaunchKernelGGL((kmeans_assign_b3_kernel<D>), dim3((unsigned)((n + ROWS - 1) / ROWS)), dim3(256), 0, s, x, n,
                           centroids, half_sqnorm, k, assign, best_score);
        return;
      }
    }
    constexpr int ROWS = Shape<D>::ANCHORS_PER_BLOCK;
    hipLaunchKernelGGL((kmeans_assign_kernel<D>), dim3((unsigned)((n + ROWS - 1) / ROWS)), dim3(256), 0, s, x, n, centroids,
                       half_sqnorm, k, assign, best_score);
  });
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_kmeans_assign_accumulate_f32(const float* x, int64_t n, const float* centroids,
                                                    const float* half_sqnorm, int64_t k, int32_t d, int64_t* assign,
                                                    float* sums, float* counts, int32_t n_copies, void* stream) {
  GCR_CHECK_ARG(n >= 0 && k >= 1 && k < (1ll << 31) && n_copies >= 1 && n_copies <= 64);
  if (!dim_supported(d) || !use_b3(d)) return GCR_EUNSUPPORTED;      // split-operand engine only (d <= 128)
  if (n == 0) return GCR_OK;
  GCR_CHECK_ARG(x && centroids && half_sqnorm && sums && counts);
  hipStream_t s = (hipStream_t)stream;
  dispatch_value<32, 64, 128>(d, [&](auto dc) {
    constexpr int D = decltype(dc)::value, ROWS = ShapeB3<D>::ANCHORS_PER_BLOCK;
    hipLaunchKernelGGL((kmeans_assign_b3_kernel<D>), dim3((unsigned)((n + ROWS - 1) / ROWS)), dim3(256), 0, s, x, n, centroids,
                       half_sqnorm, k, assign, (float*)nullptr, sums, counts, (int)n_copies);
  });
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_kmeans_update_f32(const float* x, int64_t n, int32_t d, const int64_t* assign, int64_t k,
                                         float* centroids, float* half_sqnorm, float* sums, float* counts,
                                         void* stream) {
  GCR_CHECK_ARG(n >= 0 && k >= 1 && d >= 1);
  GCR_CHECK_ARG(centroids && half_sqnorm);
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    GCR_CHECK_ARG(x && assign && sums && counts);
    hipError_t err = hipMemsetAsync(sums, 0, sizeof(float) * (size_t)(k * d), s);
    if (err == hipSuccess) err = hipMemsetAsync(counts, 0, sizeof(float) * (size_t)k, s);
    if (err != hipSuccess) return gcr_hip_status(err);
    hipLaunchKernelGGL(kmeans_accumulate_kernel, dim3((unsigned)gcr_grid((n + 3) / 4, 16384)), dim3(256), 0, s, x, n, d,
                       assign, k, sums, counts, 1);
  }
  hipLaunchKernelGGL(kmeans_finalize_kernel, dim3((unsigned)gcr_grid((k + 15) / 16, 4096)), dim3(256), 0, s, sums,
                     n > 0 ? counts : nullptr, k, d, centroids, half_sqnorm);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_kmeans_update_sorted_f32(const float* x, int64_t n, int32_t d, const uint32_t* keys_sorted,
                                                const int32_t* perm, int64_t k, float* centroids, float* half_sqnorm,
                                                float* sums, float* counts, void* stream) {
  GCR_CHECK_ARG(n >= 1 && n < (1ll << 31) && k >= 1 && d >= 1 && d <= 256);
  GCR_CHECK_ARG(x && keys_sorted && perm && centroids && half_sqnorm && sums && counts);
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipMemsetAsync(sums, 0, sizeof(float) * (size_t)(k * d), s);
  if (err == hipSuccess) err = hipMemsetAsync(counts, 0, sizeof(float) * (size_t)k, s);
  if (err != hipSuccess) return gcr_hip_status(err);
  hipLaunchKernelGGL(kmeans_accumulate_sorted_kernel, dim3((unsigned)gcr_grid(((n + 63) / 64 + 3) / 4, 65536)), dim3(256), 0,
                     s, x, n, d, keys_sorted, perm, k, sums, counts);
  hipLaunchKernelGGL(kmeans_finalize_kernel, dim3((unsigned)gcr_grid((k + 15) / 16, 4096)), dim3(256), 0, s, sums, counts, k,
                     d, centroids, half_sqnorm);
  return GCR_LAUNCH_STATUS();
}


extern "C" int32_t gcr_kmeans_lloyd_update_f32(const float* x, int64_t n, int32_t d, const int64_t* assign,
                                               const uint32_t* keys_sorted, const int32_t* perm, int64_t k,
                                               float* centroids, float* half_sqnorm, float* sums, float* counts,
                                               int32_t n_copies, uint64_t seed, int32_t iter, int32_t* n_split,
                                               void* stream) {
  GCR_CHECK_ARG(n >= 1 && n < (1ll << 31) && k >= 1 && k < (1ll << 31) && d >= 1 && d <= 256 && iter >= 0);
  GCR_CHECK_ARG(n_copies >= 1 && n_copies <= 64);
  GCR_CHECK_ARG(x && centroids && half_sqnorm && sums && counts);
  GCR_CHECK_ARG((keys_sorted != nullptr) == (perm != nullptr));
  hipStream_t s = (hipStream_t)stream;
  if (keys_sorted == nullptr && assign == nullptr) {
    // sums / counts already hold this iteration's accumulation (gcr_kmeans_assign_accumulate_f32)
  } else if (keys_sorted != nullptr) {
    hipLaunchKernelGGL(kmeans_accumulate_sorted_kernel, dim3((unsigned)gcr_grid(((n + 63) / 64 + 3) / 4, 65536)), dim3(256), 0,
                       s, x, n, d, keys_sorted, perm, k, sums, counts);
  } else {
    hipLaunchKernelGGL(kmeans_accumulate_kernel, dim3((unsigned)gcr_grid((n + 3) / 4, 16384)), dim3(256), 0, s, x, n, d,
                       assign, k, sums, counts, (int)n_copies);
  }
  GCR_CHECK_ARG(256 % d == 0 && k * (int64_t)d < (1ll << 39));       // rows must not straddle workgroups (d in 32..256)
  hipLaunchKernelGGL(kmeans_finalize_clear_kernel, dim3((unsigned)((k * (int64_t)d + 255) / 256)), dim3(256), 0, s, sums,
                     counts, k, d, centroids, half_sqnorm, keys_sorted != nullptr ? 1 : (int)n_copies);
  hipLaunchKernelGGL(kmeans_split_kernel, dim3(1), dim3(kSplitThreads), 0, s, counts, k, d, centroids, half_sqnorm, n, seed,
                     (uint32_t)iter, n_split);
  return GCR_LAUNCH_STATUS();
}

extern "C" int32_t gcr_kmeans_lloyd_update_q_f32(const int64_t* sums_q, const int32_t* counts, const float* qscale, int64_t k,
                                                 int32_t d, float* centroids, float* half_sqnorm, float* counts_scratch,
                                                 int64_t n_points, uint64_t seed, int32_t iter, int32_t* n_split, void* image,
                                                 int32_t n_copies, void* stream) {
  GCR_CHECK_ARG(k >= 1 && k < (1ll << 31) && d >= 1 && d <= 256 && 256 % d == 0 && iter >= 0 && n_points >= 1);
  GCR_CHECK_ARG(n_copies >= 1 && n_copies <= 64);
  GCR_CHECK_ARG(sums_q && counts && qscale && centroids && half_sqnorm && counts_scratch);
  GCR_CHECK_ARG(image == nullptr || d == 32 || d == 64 || d == 128);
  hipStream_t s = (hipStream_t)stream;
  u32x4* img = reinterpret_cast<u32x4*>(image);
  const int64_t tiles = (k + kTileJ - 1) / kTileJ;
  float* bias = image != nullptr ? reinterpret_cast<float*>(img + tiles * 3 * (d / 16) * 64) : nullptr;
  hipLaunchKernelGGL(kmeans_finalize_q_kernel, dim3((unsigned)((k * (int64_t)d + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const long long*>(sums_q), counts, qscale, k, d, centroids, half_sqnorm, counts_scratch, img,
                     bias, (int)n_copies);
  hipLaunchKernelGGL(kmeans_split_kernel, dim3(1), dim3(kSplitThreads), 0, s, counts_scratch, k, d, centroids, half_sqnorm,
                     n_points, seed, (uint32_t)iter, n_split, img, bias);
  return GCR_LAUNCH_STATUS();
}
