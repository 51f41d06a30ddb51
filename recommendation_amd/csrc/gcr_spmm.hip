// CSR x dense SpMM for the LightGCN message pass on gfx950 (MI355X).
//
// Replaces torch.sparse.mm(A, emb) (ncl.py:419, directau.py:290, selfcf.py:479, sept.py:223,
// buir.py:317, mhcn.py:440-456) and LGConv (lightgcn.py:25), with the layer combine of
// lightgcn.py:26 / ncl.py:421 and the row normalise of sept.py:224 fused into the epilogue.
//
// Mapping (HBM-bound gather; no MFMA on purpose):
//   * one 64-lane wavefront per *partition* of <= L consecutive non-zeros (host plan, see
//     gcr_spmm_plan_*): a partition is either up to 64 whole rows or one chunk of a long row, so
//     every wave moves the same number of bytes whatever the degree skew;
//   * lane l owns feature columns l, l+64, ...: with d = 64 one neighbour row is exactly one
//     coalesced 256-B wave load.  Its base is wave-uniform, but what is compiled is a 64-bit VGPR address per gather in
//     flight: v_readlane of the column, s_mul_hi / s_mul by d, v_lshl_add_u64 onto x + lane*4, global_load_dword
//     v, v[a:a+1], off.  The SGPR-base form (a 32-bit offset per gather) was built and measured: 0.3-0.8 % of a cfg2
//     layer, below the bar, so it is not here (EXPERIMENTS.md "SpMM: the walk's scalar work");
//   * column ids / values of 64 non-zeros are fetched with one coalesced vector load each and
//     handed out with v_readlane (scalar), so all control flow (row boundaries, edge mask,
//     tails) is scalar and divergence-free;
//   * UNR (16 at d <= 64) gathers are issued back to back before the first FMA to keep >= 4 KiB per
//     wave in flight; at 8 waves/SIMD that is >= 128 KiB per CU;
//   * a row end does not drain that pipeline: acc_in of the next rows of a whole-row partition is loaded BEFORE a batch's
//     gathers are issued and held in a short register queue, so the combine at the flush waits with a counted vmcnt on a
//     load that is older than every gather still in flight (it used to load at the flush and wait vmcnt(0): all remaining
//     gathers, all earlier stores and one fresh HBM round trip per row, 1.1 M times per cfg2 layer);
//   * long rows: chunk partial sums go to a workspace and are added in chunk order by
//     spmm_long_rows (deterministic; no float atomics).
//
// Kernels: `spmm_parts` is the generic walk (every width, mask and epilogue) and the reference the bit-for-bit tests compare
// the others against.  The other six are shells around two shared pieces:
//   * `walk_partition`, one wave's walk over a partition at d <= 64 on a tighter schedule, with a row sink for what happens
//     at a row end: `spmm_hub_parts` stores the sum (the windowed companion), `spmm_rows` combines it with acc_in through
//     a two-entry queue (the plain launch), `spmm_layer` is both in one grid, a range of blocks each (the windowed launch);
//   * `sum_partials`, the fixed-order 4-wave sum of partial rows: `spmm_long_rows` over the chunks of a split row,
//     `spmm_long_rows_pair` over those of the companion and of the main plan in one grid, `spmm_hub_rows` over the windows
//     of a hub row, each followed by store_row or a plain store.
// A windowed launch at d <= 64 (gcr_spmm_windowed_f32) is `spmm_layer`, `spmm_long_rows_pair`, `spmm_hub_rows`: three
// launches; gcr_spmm_hub_parts_f32 + gcr_spmm_hub_reduce_f32 + gcr_spmm_rows_f32 are the same words in five.
#include "gcr_common.h"

#include <type_traits>

namespace {

// gathers in flight per wave before the first FMA: interleaved A/B on MI355X (scripts/perf_spmm_ab.py, round 1)
// 4 -> 0.647 ms, 8 -> 0.612 ms, 16 -> 0.598 ms per cfg2 layer (cfg4: 7.52 / 7.06 / 6.91 ms)
template <int NV>
constexpr int unroll_for() { return NV == 1 ? 16 : 8; }

// rows of acc_in a whole-row partition holds in registers ahead of their flush (one VGPR each at d <= 64; a batch of 16
// gathers ends 1.6 rows on average at the mean degree 10 of the user rows).  Interleaved A/B, ms per cfg2 / cfg4 layer:
// 2 rows 0.6534 / 7.136 against the parent's 0.6655 / 7.457.  With the next block's col / val loaded early as well (a
// variant that did not stay) 4 rows were slower than 2, 0.658 / 7.14 against 0.645 / 7.00: the refill is scalar work in
// front of every batch.  None for d > 64 (NV registers per row) and none for the ACC2 form (two addends per row; that
// instantiation has no registers to spare at 8 waves per SIMD).
template <int NV, bool ACC2>
constexpr int acc_queue_for() { return (NV == 1 && !ACC2) ? 2 : 0; }

// One-touch traffic of the kernels below the generic one: the CSR words, acc_in, the output rows and the partial rows are
// each touched once per launch, and every line of them an L2 allocates pushes out a gathered row that would have been hit
// again.  `nt` on such a load or store lowers what its line displaces (measured with gcr_probe_policy_rows_f32:
// EXPERIMENTS.md "SpMM: cache-policy hints, the gate"); the gathers themselves stay plain.  Same words, same order.
template <bool NT = true, class T>
__device__ __forceinline__ T stream_load(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT = true, class T>
__device__ __forceinline__ void stream_store(T* p, T v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

struct Epilogue {
  float val_scale;
  float* y;
  const float* acc_in;
  float* acc_out;
  float acc_scale;
  uint32_t flags;
  float* inv_norm_out;
  float* y_raw;          // second output under ROW_L2NORM: the product before the row normalise (mhcn.py:440-442)
  const float* acc_in2;  // second addend of the combine, with its own scale (the per-layer gradient of the Horner backward)
  float acc_in2_scale;
  const uint32_t* col_bits;   // host-side dispatch only (COLMASK instantiation): never read through the struct on the device
};

// ACC2: the second-addend form is its own instantiation — read unconditionally, its pointer and scale cost the hot
// instantiation 9 SGPRs (96 -> 105), which is one wave per SIMD of occupancy and 4 % of the cfg2 layer time
// have_pre: `pre` already holds acc_in[row] (loaded a gather batch ago by the caller's queue), so the combine below issues
// no load and waits for none.  The two arms are kept apart on purpose: a load in one arm of a diamond makes the wait at
// the join a vmcnt(0) for both.
// STREAM: the reducers' form, acc_in and the output rows as one-touch traffic (stream_load / stream_store); the generic
// kernel keeps plain accesses.
template <int NV, bool D64, bool ACC2, bool STREAM = false>
__device__ __forceinline__ void store_row(const Epilogue& ep, int64_t row, int d, int lane, float (&acc)[NV],
                                          bool have_pre, const float (&pre)[NV]) {
  // No contraction anywhere in the epilogue: `acc * val_scale` and the add of acc_in stay two roundings in both arms.  The
  // parent build never contracted here (its ISA has v_mul, v_add, v_mul; the replay test reproduced it bit for bit), so
  // this pins what it did, the row normalise below included (its fmaf is explicit and stays one).
#pragma clang fp contract(off)
  float yv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) yv[v] = acc[v] * ep.val_scale;
  if (ep.flags & GCR_SPMM_ROW_L2NORM) {
    if (ep.y_raw != nullptr) {
      const int64_t rb = row * (int64_t)d;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = lane + 64 * v;
        if (D64 || c < d) stream_store<STREAM>(ep.y_raw + rb + c, yv[v]);
      }
    }
    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) ss = fmaf(yv[v], yv[v], ss);
    ss = gcr_wave_sum(ss);
    const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int v = 0; v < NV; ++v) yv[v] *= inv;
    if (ep.inv_norm_out != nullptr && lane == 0) ep.inv_norm_out[row] = inv;
  }
  const int64_t base = row * (int64_t)d;
  if (ep.y != nullptr) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = lane + 64 * v;
      if (D64 || c < d) stream_store<STREAM>(ep.y + base + c, yv[v]);
    }
  }
  if (ep.acc_out == nullptr) return;
  if (have_pre) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = lane + 64 * v;
      if (D64 || c < d) stream_store<STREAM>(ep.acc_out + base + c, (pre[v] + yv[v]) * ep.acc_scale);
    }
  } else {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = lane + 64 * v;
      if (D64 || c < d) {
        float prev = ep.acc_in != nullptr ? stream_load<STREAM>(ep.acc_in + base + c) : 0.f;
        if (ACC2) prev = fmaf(stream_load<STREAM>(ep.acc_in2 + base + c), ep.acc_in2_scale, prev);
        stream_store<STREAM>(ep.acc_out + base + c, (prev + yv[v]) * ep.acc_scale);
      }
    }
  }
}

// COLMASK: `keep_bits` is a bitmap over the COLUMNS (bit c set = row c of x may be non-zero) instead of over the stored
// non-zeros: non-zeros whose column is clear are skipped before their 256-B gather — the first launch of a backward pass
// whose incoming gradient has a few thousand non-zero rows of a million (the NCL step: DESIGN 4.5) reads the CSR and
// writes its output, but gathers almost nothing.
template <int NV, bool D64, bool HAS_VAL, bool MASKED, int UNR, bool ACC2, bool COLMASK = false>
// amdgpu_num_sgpr(96): the queued forms' extra scalar state pushes the allocator past the 102 SGPRs that 8 waves per
// SIMD allow (it takes all 106 when nothing stops it: 7 waves, DESIGN 4.1 puts that at 4 %); capped, the few coldest
// scalars live in VGPR lanes instead (v_writelane / v_readlane outside the gather batches) and every d <= 128
// instantiation keeps 8 waves.  The attribute takes a literal only, so it also covers the ACC2 forms, which keep the
// parent's schedule: they move 2-19 cold scalars to VGPR lanes at unchanged occupancy (not timed separately).
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96))) void spmm_parts(const int64_t* __restrict__ desc,
                                                  int64_t n_parts,
                                                  const int64_t* __restrict__ rowptr,
                                                  const int32_t* __restrict__ col,
                                                  const float* __restrict__ val,
                                                  const uint32_t* __restrict__ keep_bits,
                                                  const float* __restrict__ x, int d, Epilogue ep,
                                                  float* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  // workgroups go round-robin over the 8 XCDs, so neighbouring partitions (cheap user rows, expensive item
  // rows) are mixed on every XCD; giving each XCD one contiguous eighth was measured slower
  const int64_t part = (int64_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (part >= n_parts) return;
  const int64_t nnz0 = desc[4 * part + 0];
  const int64_t nnz1 = desc[4 * part + 1];
  const int64_t rowinfo = desc[4 * part + 2];
  const int64_t slot = desc[4 * part + 3];
  const int row0 = (int)(rowinfo & 0xffffffffll);
  const int nrows = (int)(rowinfo >> 32);
  const int n = (int)(nnz1 - nnz0);
  const bool whole_rows = slot < 0;

  float acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.f;

  // local end offsets of the (<= 64) rows of a whole-row partition, one per lane
  int ends_v = 0x7fffffff;
  int cur = 0, cur_end = 0x7fffffff;
  if (whole_rows) {
    if (lane < nrows) ends_v = (int)(rowptr[row0 + lane + 1] - nnz0);
    cur_end = gcr_readlane_i(ends_v, 0);
  }

  // acc_in of rows cur .. cur + nq - 1, loaded ahead of their flush: the rows of a whole-row partition are consecutive,
  // so their addresses are known from the start.  refill() runs at a fixed point, BEFORE a batch of gathers is issued:
  // by the time the first of those gathers has been consumed every queue entry has landed (loads return in order), so
  // neither the combine at a row end nor the shift of the queue waits for anything a gather was not already waited for.
  // In place (acc_in == acc_out) stays correct: a row is read before this wave, its only writer, stores it.
  constexpr int PQ = acc_queue_for<NV, ACC2>();
  float q[PQ > 0 ? PQ : 1][NV];
  int nq = 0;
  // rows this partition may prefetch: none for chunks, y-only launches and acc_in == NULL (no new loads there)
  const int qrows = (PQ > 0 && whole_rows && ep.acc_in != nullptr && ep.acc_out != nullptr) ? nrows : 0;
  auto refill = [&]() {
    if (PQ == 0) return;
#pragma unroll
    for (int k = 0; k < PQ; ++k) {
      if (k >= nq && cur + k < qrows) {
        const float* ap = ep.acc_in + ((int64_t)row0 + cur + k) * d;
#pragma unroll
        for (int v = 0; v < NV; ++v) q[k][v] = (D64 || lane + 64 * v < d) ? ap[lane + 64 * v] : 0.f;
      }
    }
    nq = max(nq, min(PQ, qrows - cur));
  };

  auto flush = [&]() {
    // fewer queued rows than row ends in one batch (degree-1 runs), or nothing to prefetch: store_row loads at the flush
    const bool pre = PQ > 0 && nq > 0;
    store_row<NV, D64, ACC2>(ep, (int64_t)row0 + cur, d, lane, acc, pre, q[0]);
    if (pre) {
#pragma unroll
      for (int k = 0; k + 1 < PQ; ++k)
#pragma unroll
        for (int v = 0; v < NV; ++v) q[k][v] = q[k + 1][v];
      --nq;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.f;
    ++cur;
    cur_end = cur < nrows ? gcr_readlane_i(ends_v, cur) : 0x7fffffff;
  };

  // column id, value and edge-mask word of the 64 non-zeros of block b, one per lane
  auto load_block = [&](int b, int& cv_o, float& vv_o, uint32_t& kw_o) {
    cv_o = 0;
    vv_o = 0.f;
    kw_o = 0u;
    if (lane < n - b) {
      const int64_t e = nnz0 + b + lane;
      cv_o = col[e];
      vv_o = HAS_VAL ? val[e] : 1.0f;
      if (MASKED && !COLMASK) kw_o = keep_bits[e >> 5];
    }
  };

  // the next block's words are loaded after this block's last FMA.  Loading them before this block's gathers was measured:
  // +1.2 % on cfg4 on top of the queue, but inside the noise margin on cfg2, so it did not stay (EXPERIMENTS.md)
  int cv_n;
  float vv_n;
  uint32_t kw_n;
  load_block(0, cv_n, vv_n, kw_n);
  for (int b = 0; b < n; b += 64) {
    const int m = min(64, n - b);
    const int cv = cv_n;
    const float vv = vv_n;
    const uint32_t kw = kw_n;
    bool keep = lane < m;
    if (MASKED && !COLMASK) keep = keep && ((kw >> ((nnz0 + b + lane) & 31)) & 1u);
    if (COLMASK) {
      if (keep) keep = (keep_bits[cv >> 5] >> (cv & 31)) & 1u;
    }
    unsigned long long todo = (MASKED || COLMASK) ? __ballot(keep) : (m == 64 ? ~0ull : ((1ull << m) - 1ull));
    int cnt = __builtin_popcountll(todo);

    // one batch: UNR gathers issued back to back, then consumed in order with the row ends between them
    auto batch = [&]() {
      refill();
      int js[UNR];
      float xr[UNR][NV];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        js[u] = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const float* xp = x + (int64_t)gcr_readlane_i(cv, js[u]) * d;
#pragma unroll
        for (int v = 0; v < NV; ++v) xr[u][v] = (D64 || lane + 64 * v < d) ? xp[lane + 64 * v] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (whole_rows) {
          while (b + js[u] >= cur_end) flush();
        }
        const float w = gcr_readlane_f(vv, js[u]);
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = fmaf(w, xr[u][v], acc[v]);
      }
    };
    while (cnt >= UNR) {
      batch();
      cnt -= UNR;
    }
    if (cnt > 0) refill();
    while (cnt > 0) {
      const int j = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const float* xp = x + (int64_t)gcr_readlane_i(cv, j) * d;
      float xr[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) xr[v] = (D64 || lane + 64 * v < d) ? xp[lane + 64 * v] : 0.f;
      if (whole_rows) {
        while (b + j >= cur_end) flush();
      }
      const float w = gcr_readlane_f(vv, j);
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] = fmaf(w, xr[v], acc[v]);
      --cnt;
    }
    if (b + 64 < n) load_block(b + 64, cv_n, vv_n, kw_n);
  }

  if (whole_rows) {
    while (cur < nrows) {
      if (nq == 0) refill();
      flush();
    }
  } else {
    const int64_t base = slot * (int64_t)d;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (D64 || lane + 64 * v < d) partials[base + lane + 64 * v] = acc[v];
  }
}

// The sum of `count` partial rows p0, p0 + stride, ... (stride in floats) by one 4-wave block: wave w adds partials w,
// w+4, ... (4 loads in flight), the four wave sums are combined through LDS in wave order.  Returns whether this wave
// holds the sum in `acc`.  The order of additions is fixed by the plan — per wave in steps of 16 with the four loads of a
// step added in order, the remainder in steps of 4, then ((w0 + w1) + w2) + w3 — so the result stays bitwise
// reproducible: no float atomics.  (One wave per row took 24 us per cfg2 layer — hub rows have ~100 chunks — i.e. 3 % of
// the layer.)
template <int NV, bool D64>
__device__ __forceinline__ bool sum_partials(const float* __restrict__ p0, int64_t stride, int count, int d,
                                             float (&acc)[NV]) {
  __shared__ float red[3][NV * 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.f;
  int k = wave;
  for (; k + 12 < count; k += 16) {
    float t[4][NV];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < NV; ++v)
        t[u][v] = (D64 || lane + 64 * v < d) ? stream_load(p0 + (int64_t)(k + 4 * u) * stride + lane + 64 * v) : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] += t[u][v];
  }
  for (; k < count; k += 4)
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (D64 || lane + 64 * v < d) acc[v] += stream_load(p0 + (int64_t)k * stride + lane + 64 * v);
  if (wave > 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) red[wave - 1][v * 64 + lane] = acc[v];
  }
  __syncthreads();
  if (wave > 0) return false;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] += red[w][v * 64 + lane];
  return true;
}

// one block per long row: its chunk partials, slots s0 .. s1 - 1 of the workspace, in chunk order, then the common epilogue
template <int NV, bool D64, bool ACC2>
__global__ __launch_bounds__(256) void spmm_long_rows(const int32_t* __restrict__ long_row,
                                                      const int32_t* __restrict__ long_slot0, int64_t n_long,
                                                      const float* __restrict__ partials, int d, Epilogue ep) {
  const int64_t i = blockIdx.x;
  const int s0 = long_slot0[i], s1 = long_slot0[i + 1];
  float acc[NV];
  if (sum_partials<NV, D64>(partials + (int64_t)s0 * d, d, s1 - s0, d, acc))
    store_row<NV, D64, ACC2, true>(ep, (int64_t)long_row[i], d, threadIdx.x & 63, acc, false, acc);
}

// The windowed companion's reduction (graph.py HubPlan), one block per hub row: hub row h was multiplied window by window
// into partials[w * n_hub + h]; they are added in window order, then the common epilogue with the launch's real scales.
template <int NV, bool D64>
__global__ __launch_bounds__(256) void spmm_hub_rows(const int32_t* __restrict__ hub_row, int64_t n_hub, int n_win,
                                                     const float* __restrict__ partials, int d, Epilogue ep) {
  const int64_t h = blockIdx.x;
  float acc[NV];
  if (sum_partials<NV, D64>(partials + h * d, n_hub * d, n_win, d, acc))
    store_row<NV, D64, false, true>(ep, (int64_t)hub_row[h], d, threadIdx.x & 63, acc, false, acc);
}

// The partition of this wave in a range of blocks that starts at block `block0`: four waves per block, one partition each.
__device__ __forceinline__ int64_t wave_partition(unsigned block0) {
  return (int64_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x - block0) * 4u + (threadIdx.x >> 6)));
}

// One wave's walk over partition `part` at d <= 64 (one accumulator register per lane), shared by the kernels below.  One
// wave per partition in the hardware's dispatch order and one fmaf per non-zero from 0 in stored order, as `spmm_parts`; a
// whole-row partition hands every row's sum to its row sink (empty rows zeros), a chunk partition stores its slot.  What
// differs from `spmm_parts` is the schedule:
//   * the successor's col / val are loaded BEFORE a block's gathers and are back with the first of them, so the copy at the
//     block's end waits for nothing the last batch's last FMA has not waited for (the generic kernel loads them after that
//     FMA: one exposed round trip per block);
//   * what a block holds below a full batch of 16 goes out in batches of 8, 4, 2 and 1 instead of one gather, one wait at a
//     time: the companion's partitions average 96 non-zeros, so 7-8 of a partition's gathers were such single round trips
//     beside the six batches that carried the rest, and that is where its waves waited (EXPERIMENTS.md "SpMM:
//     spmm_hub_parts, the companion's own kernel").
// What happens at a row end is the sink's: sink.begin(row0) names the partition's first row, once; sink.refill(n) runs in
// front of every batch of gathers (n rows of the partition have not ended yet; n = 0 in a chunk), sink.flush(acc) at every
// row end, in row order.  The rows of a partition are consecutive, so a sink steps its row addresses from one flush to the
// next and multiplies a row by d once per partition, in begin().
// A mapped sink (Sink::mapped, the row-ordered plan of graph.py RowOrder): the partition's rows are rows of a row-permuted
// copy P of the CSR, and row_id[P row] names the row of the caller's arrays each of them stands for.  The ids of the
// partition's (<= 64) rows are loaded one per lane beside ends_v and handed to the sink once (begin_mapped); refill and flush
// get the local index of the row that ends next, and the sink reads that row's id, and the next one's, by v_readlane.
template <bool D64, bool HAS_VAL, class Sink>
__device__ __forceinline__ void walk_partition(const int64_t part, const int64_t* __restrict__ desc, int64_t n_parts,
                                               const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                               const float* __restrict__ val, const float* __restrict__ x, int d,
                                               float* __restrict__ partials, Sink& sink,
                                               const int32_t* __restrict__ row_id = nullptr) {
  constexpr int UNR = 16;
  const int lane = threadIdx.x & 63;
  if (part >= n_parts) return;
  const int64_t nnz0 = desc[4 * part + 0];
  const int n = (int)(desc[4 * part + 1] - nnz0);
  const int64_t rowinfo = desc[4 * part + 2];
  const int64_t slot = desc[4 * part + 3];
  const int row0 = (int)(rowinfo & 0xffffffffll);
  const int nrows = (int)(rowinfo >> 32);
  const bool whole_rows = slot < 0;
  const bool on = D64 || lane < d;

  // local end offsets of the (<= 64) rows of a whole-row partition, one per lane
  int ends_v = 0x7fffffff;
  if (whole_rows && lane < nrows) ends_v = (int)(stream_load(rowptr + row0 + lane + 1) - nnz0);
  int cur = 0;
  int cur_end = whole_rows ? gcr_readlane_i(ends_v, 0) : 0x7fffffff;

  float acc = 0.f;
  if constexpr (Sink::mapped) {
    int rid_v = 0;
    if (whole_rows && lane < nrows) rid_v = stream_load(row_id + row0 + lane);
    sink.begin_mapped(rid_v);
  } else {
    sink.begin((int64_t)row0);
  }
  auto refill = [&]() {
    if constexpr (Sink::mapped) sink.refill(whole_rows ? nrows - cur : 0, cur);
    else sink.refill(whole_rows ? nrows - cur : 0);
  };
  auto flush = [&]() {
    if constexpr (Sink::mapped) sink.flush(acc, cur);
    else sink.flush(acc);
    acc = 0.f;
    ++cur;
    cur_end = cur < nrows ? gcr_readlane_i(ends_v, cur) : 0x7fffffff;
  };
  // column id and value of the 64 non-zeros of block b, one per lane
  auto load_block = [&](int b, int& cv_o, float& vv_o) {
    cv_o = 0;
    vv_o = 0.f;
    if (lane < n - b) {
      const int64_t e = nnz0 + b + lane;
      cv_o = stream_load(col + e);
      vv_o = HAS_VAL ? stream_load(val + e) : 1.0f;
    }
  };

  int cv, cv_n = 0;
  float vv, vv_n = 0.f;
  load_block(0, cv, vv);
  if (Sink::queued) {
    // The first block's words are waited for here, once, and not at the first v_readlane of the batch loop: that wait would
    // sit behind refill() in the loop body and hold every batch of the block until the acc_in it has just asked for is back.
    asm volatile("" ::"v"(cv), "v"(vv));
  }
  for (int b = 0; b < n; b += 64) {
    const bool more = b + 64 < n;
    if (more) load_block(b + 64, cv_n, vv_n);
    const int m = more ? 64 : n - b;
    // B gathers from non-zero jb of the block on, issued back to back, then consumed in stored order with the row ends
    // between them; returns B
    auto batch = [&](auto bc, const int jb) {
      constexpr int B = decltype(bc)::value;
      refill();
      float xr[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const float* xp = x + (int64_t)gcr_readlane_i(cv, jb + u) * d;
        xr[u] = on ? xp[lane] : 0.f;
      }
      // The row end relative to this batch, so that position u compares a constant with one scalar; a chunk needs no test
      // of its own, its cur_end is the sentinel 0x7fffffff and stays above every position.
      int end = cur_end - (b + jb);
#pragma unroll
      for (int u = 0; u < B; ++u) {
        while (u >= end) {
          flush();
          end = cur_end - (b + jb);
        }
        const float w = HAS_VAL ? gcr_readlane_f(vv, jb + u) : 1.0f;
        acc = fmaf(w, xr[u], acc);
      }
      return B;
    };
    // One loop for every block.  `spmm_rows` used to have a second path for blocks with a successor (always 64 non-zeros,
    // four full batches); this loop measured level with it on cfg2 and cfg4, so that path is gone (EXPERIMENTS.md "SpMM: one
    // partition walk, one partial reducer").
    int j = 0;
    while (m - j >= UNR) j += batch(std::integral_constant<int, UNR>{}, j);
    if (m - j >= 8) j += batch(std::integral_constant<int, 8>{}, j);
    if (m - j >= 4) j += batch(std::integral_constant<int, 4>{}, j);
    if (m - j >= 2) j += batch(std::integral_constant<int, 2>{}, j);
    if (m - j >= 1) j += batch(std::integral_constant<int, 1>{}, j);
    if (more) {
      cv = cv_n;
      vv = vv_n;
    }
  }

  if (whole_rows) {
    while (cur < nrows) {
      refill();
      flush();
    }
  } else {
    if (on) stream_store(partials + slot * (int64_t)d + lane, acc);
  }
}

// Row sink of the windowed companion: no epilogue and no acc_in, a row's sum is stored as it stands (`spmm_parts` multiplied
// it by a val_scale of 1.0).  `y` is the row of the next flush: a wave-uniform pointer, so a store is that SGPR pair plus the
// lane's byte offset, and a row end moves it on by d floats with one 64-bit scalar add (the output may exceed 4 GiB).
template <bool D64>
struct StoreSink {
  static constexpr bool queued = false;
  static constexpr bool mapped = false;
  float* __restrict__ y;
  int d, lane;
  __device__ __forceinline__ void begin(int64_t row0) { y += row0 * d; }
  __device__ __forceinline__ void refill(int) {}
  __device__ __forceinline__ void flush(float acc) {
    if (D64 || lane < d) stream_store(y + lane, acc);
    y += d;
  }
};

// Row sink of the plain launch: y = acc * val_scale and / or acc_out = (acc_in + y) * acc_scale with store_row's two
// roundings, and the two-entry acc_in queue of `spmm_parts`: acc_in of the next two rows to end is loaded in front of a
// batch's gathers, so the combine at a row end waits for nothing younger than a gather it has already waited for.  Nothing
// is queued for chunks (n = 0), y-only launches and acc_in == NULL.  In place (acc_in == acc_out) stays correct: a row is
// read before this wave, its only writer, stores it.
// HORNER: acc_in and acc_out are given (they may be the same array) and y is not, known at compile time.  It is what a
// LightGCN layer launches forward and backward; none of the tests of launch-uniform pointers below is left in that
// instantiation, refill and flush branch on the queue's fill and nothing else.  The other forms read the pointers at run time.
// `y`, `acc_in` and `acc_out` are wave-uniform row pointers once begin() has run: y and acc_out the row of the next flush,
// acc_in the row of the next load, which is the row of the next flush + nq whichever arm loads it (acc_in is read only
// when rows are queued).  Each moves on by d floats with one 64-bit scalar add; a NULL pointer is never moved.
// MAPPED: the rows of a partition are not consecutive in y / acc_in / acc_out (walk_partition's row map).  The pointers
// stay at the arrays' bases; `rid_v` holds the ids of the partition's rows, one per lane, and a row's offset is its id by
// v_readlane times d: the row of the next flush is local row `cur`, the queue's q0 is row cur and q1 row cur + 1, which is
// what the stepped pointer visits (the row of the next load is cur + nq).  Same loads, same stores, same roundings.
template <bool D64, bool HORNER, bool MAPPED = false>
struct CombineSink {
  static constexpr bool queued = true;
  static constexpr bool mapped = MAPPED;
  float val_scale, acc_scale;
  float* y;
  const float* acc_in;
  float* acc_out;
  int d, lane;
  float q0 = 0.f, q1 = 0.f;
  int nq = 0;
  int rid_v = 0;
  const bool has_y = !HORNER && y != nullptr;
  const bool has_out = HORNER || acc_out != nullptr;
  const bool queues = HORNER || (acc_in != nullptr && acc_out != nullptr);
  __device__ __forceinline__ void begin(int64_t row0) {
    if (has_y) y += row0 * d;
    if (has_out) acc_out += row0 * d;
    if (queues) acc_in += row0 * d;
  }
  __device__ __forceinline__ float load_next() {
    const float v = (D64 || lane < d) ? stream_load(acc_in + lane) : 0.f;
    acc_in += d;
    return v;
  }
  __device__ __forceinline__ void refill(int n) {
    if (!queues) n = 0;
    if (nq < 1 && 0 < n) q0 = load_next();
    if (nq < 2 && 1 < n) q1 = load_next();
    nq = max(nq, min(2, n));
  }
  __device__ __forceinline__ void flush(float acc) {
    // two roundings, as store_row: `acc * val_scale`, then the add of acc_in, never contracted
#pragma clang fp contract(off)
    const bool on = D64 || lane < d;
    const float yv = acc * val_scale;
    if (has_y) {
      if (on) stream_store(y + lane, yv);
      y += d;
    }
    if (has_out) {
      if (nq > 0) {
        if (on) stream_store(acc_out + lane, (q0 + yv) * acc_scale);
        q0 = q1;
        --nq;
      } else {
        // fewer queued rows than row ends in one batch (degree-1 runs), or nothing to prefetch: load at the flush
        const float prev = queues ? load_next() : 0.f;
        if (on) stream_store(acc_out + lane, (prev + yv) * acc_scale);
      }
      acc_out += d;
    }
  }
  // the mapped forms: `cur` is the local index of the row that ends next
  __device__ __forceinline__ void begin_mapped(int ids) { rid_v = ids; }
  __device__ __forceinline__ int64_t row_offset(int k) const { return (int64_t)gcr_readlane_i(rid_v, k) * d; }
  __device__ __forceinline__ float load_row(int k) const {
    return (D64 || lane < d) ? stream_load(acc_in + row_offset(k) + lane) : 0.f;
  }
  __device__ __forceinline__ void refill(int n, int cur) {
    if (!queues) n = 0;
    if (nq < 1 && 0 < n) q0 = load_row(cur);
    if (nq < 2 && 1 < n) q1 = load_row(cur + 1);
    nq = max(nq, min(2, n));
  }
  __device__ __forceinline__ void flush(float acc, int cur) {
#pragma clang fp contract(off)
    const bool on = D64 || lane < d;
    const float yv = acc * val_scale;
    const int64_t ro = row_offset(cur);
    if (has_y) {
      if (on) stream_store(y + ro + lane, yv);
    }
    if (has_out) {
      if (nq > 0) {
        if (on) stream_store(acc_out + ro + lane, (q0 + yv) * acc_scale);
        q0 = q1;
        --nq;
      } else {
        const float prev = queues ? load_row(cur) : 0.f;
        if (on) stream_store(acc_out + ro + lane, (prev + yv) * acc_scale);
      }
    }
  }
};

// What one arm of `spmm_layer` walks: a plan's descriptors, the CSR they partition and the split rows' workspace.
struct WalkSet {
  const int64_t* desc;
  int64_t n_parts;
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  float* partials;
};

// The plain launch's walk of partition `part`, for `spmm_rows` and the main arm of `spmm_layer`.
template <bool D64, bool HAS_VAL, bool HORNER, bool MAPPED>
__device__ __forceinline__ void walk_combine(int64_t part, const WalkSet& w, const float* __restrict__ x, int d,
                                             float val_scale, float* y, const float* acc_in, float* acc_out,
                                             float acc_scale, const int32_t* __restrict__ row_id) {
  CombineSink<D64, HORNER, MAPPED> sink{val_scale, acc_scale, y, acc_in, acc_out, d, (int)(threadIdx.x & 63)};
  walk_partition<D64, HAS_VAL>(part, w.desc, w.n_parts, w.rowptr, w.col, w.val, x, d, w.partials, sink, row_id);
}

// The windowed companion's own kernel (graph.py HubPlan, step 1 of a windowed launch: partials = H x, nothing else), d <= 64:
// the words it writes are those of `spmm_parts` on H with y only.  No mask, no epilogue, no acc_in queue.
template <bool D64, bool HAS_VAL>
__global__ __launch_bounds__(256) void spmm_hub_parts(const int64_t* __restrict__ desc, int64_t n_parts,
                                                      const int64_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const float* __restrict__ val,
                                                      const float* __restrict__ x, int d, float* __restrict__ y,
                                                      float* __restrict__ partials) {
  StoreSink<D64> sink{y, d, (int)(threadIdx.x & 63)};
  walk_partition<D64, HAS_VAL>(wave_partition(0u), desc, n_parts, rowptr, col, val, x, d, partials, sink);
}

// The plain launch's own kernel (gcr_spmm_rows_f32), d <= 64: what `spmm_parts<1, D64, HAS_VAL, false, 16, false>` is used
// for and nothing else.  No edge or column mask, no second addend, no row normalise, no second output; every word written
// equals `spmm_parts`'s.  50 VGPRs / 62 SGPRs at d = 64 with values in the Horner form, 46 / 81 in the others, 8 waves per
// SIMD without an SGPR cap and without lane spills (`spmm_parts`: 63 / 94 capped, 18 scalars in VGPR lanes).
// Measurements: EXPERIMENTS.md "SpMM: spmm_rows" and "SpMM: the walk's scalar work".
// HORNER: the host entry saw acc_in and acc_out and no y (is_horner), the compile-time form of CombineSink.
// MAPPED (gcr_spmm_rows_mapped_f32): the CSR is a row-permuted copy and row_id names each of its rows in y / acc_in / acc_out;
// the last argument, unused and not loaded otherwise, so the unmapped instantiations keep their code.
template <bool D64, bool HAS_VAL, bool HORNER, bool MAPPED = false>
__global__ __launch_bounds__(256) void spmm_rows(const int64_t* __restrict__ desc, int64_t n_parts,
                                                 const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const float* __restrict__ val, const float* __restrict__ x, int d,
                                                 float val_scale, float* y, const float* acc_in, float* acc_out,
                                                 float acc_scale, float* __restrict__ partials,
                                                 const int32_t* __restrict__ row_id) {
  walk_combine<D64, HAS_VAL, HORNER, MAPPED>(wave_partition(0u), WalkSet{desc, n_parts, rowptr, col, val, partials}, x, d,
                                             val_scale, y, acc_in, acc_out, acc_scale, row_id);
}

// The windowed launch's two walks in one grid (gcr_spmm_windowed_f32), d <= 64: blocks [hub_block0, hub_block0 +
// hub_blocks) are `spmm_hub_parts` on the companion (row sums into hub_y), every other block is `spmm_rows` on the main plan
// counted from main_block0.  Nothing either walk reads is written by the other, so the chip never drains between them.  The
// choice is wave-uniform and made once; each arm is its own call of walk_partition, so each keeps the schedule and the
// registers of the kernel it replaces, and a partition's words do not depend on where in the grid it runs.  hub_block0 is a
// multiple of 8: the companion's descriptors are laid out per XCD (reorder.xcd_grouped_order) and blocks go round-robin
// over the 8 XCDs.  Blocks past a range's partitions (the padding in front of a hub range that comes second) return at once.
// amdgpu_num_sgpr(96): uncapped, the allocator takes 97 SGPRs at d = 64 with values (the larger arm, `spmm_rows`, takes 81
// alone; the rest are kernel arguments of both arms loaded in front of the branch).  The hardware allocates in steps of 16,
// so 97 is 112 and 7 waves per SIMD, although the compiler's report says 8: each arm launched alone through this kernel
// was slower than its own kernel, the companion's 127.5 against 112.5 us and the main plan's 420.0 against 409.8 per cfg2
// layer, which ate the whole gain of the one grid.  Capped it was 94 (96 allocated, 8 waves) with two scalars written to
// VGPR lanes once in the prologue.  With the stepped row addresses the Horner form takes 79 SGPRs and 46 VGPRs and the
// other forms 94 and 46, neither with a scalar in a VGPR lane; the cap stays for the other forms.
// MAPPED (gcr_spmm_windowed_mapped_f32): the main arm walks a row-ordered copy with its row map, as `spmm_rows`.
template <bool D64, bool HAS_VAL, bool HORNER, bool MAPPED = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96))) void spmm_layer(WalkSet hub, WalkSet rest, unsigned hub_block0, unsigned hub_blocks,
                                                  unsigned main_block0, const float* __restrict__ x, int d,
                                                  float* __restrict__ hub_y, float val_scale, float* y,
                                                  const float* acc_in, float* acc_out, float acc_scale,
                                                  const int32_t* __restrict__ row_id) {
  if (blockIdx.x - hub_block0 < hub_blocks) {
    StoreSink<D64> sink{hub_y, d, (int)(threadIdx.x & 63)};
    walk_partition<D64, HAS_VAL>(wave_partition(hub_block0), hub.desc, hub.n_parts, hub.rowptr, hub.col, hub.val, x, d,
                                 hub.partials, sink);
  } else {
    walk_combine<D64, HAS_VAL, HORNER, MAPPED>(wave_partition(main_block0), rest, x, d, val_scale, y, acc_in, acc_out,
                                               acc_scale, row_id);
  }
}

// The split rows of both plans of a windowed launch in one grid, d <= 64: blocks [0, n_long_hub) sum the companion's split
// segments into hub_y as they stand (`spmm_long_rows` with a val_scale of 1.0 and y only), the others the main plan's
// split rows with the launch's epilogue.  One call of sum_partials, so one LDS buffer; its order is `spmm_long_rows`'s.
template <bool D64>
__global__ __launch_bounds__(256) void spmm_long_rows_pair(const int32_t* __restrict__ hub_long_row,
                                                           const int32_t* __restrict__ hub_slot0, unsigned n_long_hub,
                                                           const float* __restrict__ hub_partials,
                                                           float* __restrict__ hub_y,
                                                           const int32_t* __restrict__ main_long_row,
                                                           const int32_t* __restrict__ main_slot0,
                                                           const float* __restrict__ main_partials, int d, Epilogue ep) {
  const bool is_hub = blockIdx.x < n_long_hub;
  const unsigned i = is_hub ? blockIdx.x : blockIdx.x - n_long_hub;
  const int32_t* slot0 = is_hub ? hub_slot0 : main_slot0;
  const float* partials = is_hub ? hub_partials : main_partials;
  const int s0 = slot0[i], s1 = slot0[i + 1];
  const int lane = threadIdx.x & 63;
  float acc[1];
  if (!sum_partials<1, D64>(partials + (int64_t)s0 * d, d, s1 - s0, d, acc)) return;
  if (is_hub) {
    if (D64 || lane < d) stream_store(hub_y + (int64_t)hub_long_row[i] * d + lane, acc[0]);
  } else {
    store_row<1, D64, false, true>(ep, (int64_t)main_long_row[i], d, lane, acc, false, acc);
  }
}

__global__ void csr_validate_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                    int64_t n_rows, int64_t n_cols, int64_t nnz,
                                    unsigned long long* __restrict__ n_errors) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += stride)
    bad += rowptr[i + 1] < rowptr[i];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride)
    bad += (col[e] < 0) | ((int64_t)col[e] >= n_cols);
  if (blockIdx.x == 0 && threadIdx.x == 0) bad += (rowptr[0] != 0) + (rowptr[n_rows] != nnz);
  if (bad) atomicAdd(n_errors, bad);
}

// the plan head every SpMM entry point takes (gcr_spmm_plan_*), the CSR it was made for and the split rows' workspace
struct Plan {
  const int64_t* desc;
  int64_t n_parts;
  const int32_t* long_row;
  const int32_t* long_slot0;
  int64_t n_long;
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  float* partials;
};

// What every plan-taking entry point checks first.  GCR_LAUNCH: go on to the entry's own conditions and launch; anything
// else is the entry's answer — a width above max_d (the entry's own kernel) is GCR_EUNSUPPORTED and an empty plan GCR_OK,
// both before any pointer is looked at.
constexpr int32_t GCR_LAUNCH = 1;
int32_t check_plan(const Plan& p, int64_t n_rows, int64_t n_cols, int d, int max_d) {
  GCR_CHECK_ARG(p.n_parts >= 0 && p.n_long >= 0 && n_rows >= 0 && n_cols >= 0);
  GCR_CHECK_ARG(p.n_parts < (1ll << 31) - 4 && n_rows < (1ll << 31) && n_cols < (1ll << 31));
  GCR_CHECK_ARG(d >= 1 && d <= 256);
  if (d > max_d) return GCR_EUNSUPPORTED;
  if (n_rows == 0 || p.n_parts == 0) return GCR_OK;
  GCR_CHECK_ARG(p.desc != nullptr && p.rowptr != nullptr);
  GCR_CHECK_ARG(p.n_long == 0 || (p.long_row != nullptr && p.long_slot0 != nullptr && p.partials != nullptr));
  return GCR_LAUNCH;
}

// the epilogue of a plain launch; the normalising and second-addend entries set their own fields on top
Epilogue make_epilogue(float val_scale, float* y, const float* acc_in, float* acc_out, float acc_scale) {
  return Epilogue{val_scale, y, acc_in, acc_out, acc_scale};   // every later field zero / NULL
}

// the one place a width picks its registers per lane: f(integral_constant<int, NV>, bool_constant<D64>)
template <class F>
int32_t dispatch_d(int d, F f) {
  if (d == 64) return f(std::integral_constant<int, 1>{}, std::true_type{});
  if (d <= 64) return f(std::integral_constant<int, 1>{}, std::false_type{});
  if (d <= 128) return f(std::integral_constant<int, 2>{}, std::false_type{});
  if (d <= 192) return f(std::integral_constant<int, 3>{}, std::false_type{});
  return f(std::integral_constant<int, 4>{}, std::false_type{});
}

// the split rows of a plan, after the launch that wrote their chunk partials
template <int NV, bool D64, bool ACC2>
int32_t launch_long_rows(const Plan& p, int d, const Epilogue& ep, hipStream_t stream) {
  if (p.n_long == 0) return GCR_OK;
  hipLaunchKernelGGL((spmm_long_rows<NV, D64, ACC2>), dim3((unsigned)p.n_long), dim3(256), 0, stream, p.long_row,
                     p.long_slot0, p.n_long, p.partials, d, ep);
  return GCR_LAUNCH_STATUS();
}

template <int NV, bool D64, bool ACC2>
int32_t launch_spmm(const Plan& p, const uint32_t* keep_bits, const float* x, int d, const Epilogue& ep,
                    hipStream_t stream) {
  const unsigned blocks = (unsigned)((p.n_parts + 3) / 4);
#define GCR_SPMM_LAUNCH(HV, MK, CM, BITS)                                                                          \
  hipLaunchKernelGGL((spmm_parts<NV, D64, HV, MK, unroll_for<NV>(), ACC2, CM>), dim3(blocks), dim3(256), 0, stream, \
                     p.desc, p.n_parts, p.rowptr, p.col, p.val, BITS, x, d, ep, p.partials)
  if (ep.col_bits != nullptr) {
    if (p.val != nullptr) GCR_SPMM_LAUNCH(true, false, true, ep.col_bits);
    else GCR_SPMM_LAUNCH(false, false, true, ep.col_bits);
  } else if (p.val != nullptr) {
    if (keep_bits != nullptr) GCR_SPMM_LAUNCH(true, true, false, keep_bits);
    else GCR_SPMM_LAUNCH(true, false, false, keep_bits);
  } else {
    if (keep_bits != nullptr) GCR_SPMM_LAUNCH(false, true, false, keep_bits);
    else GCR_SPMM_LAUNCH(false, false, false, keep_bits);
  }
#undef GCR_SPMM_LAUNCH
  const int32_t st = GCR_LAUNCH_STATUS();
  if (st != GCR_OK) return st;
  return launch_long_rows<NV, D64, ACC2>(p, d, ep, stream);
}

// every entry point that runs `spmm_parts`: the instantiation by width and by whether the combine has a second addend
int32_t launch_spmm_d(const Plan& p, const uint32_t* keep_bits, const float* x, int d, const Epilogue& ep, void* stream) {
  return dispatch_d(d, [&](auto nv, auto d64) {
    constexpr int NV = decltype(nv)::value;
    constexpr bool D64 = decltype(d64)::value;
    if (ep.acc_in2 != nullptr) return launch_spmm<NV, D64, true>(p, keep_bits, x, d, ep, (hipStream_t)stream);
    return launch_spmm<NV, D64, false>(p, keep_bits, x, d, ep, (hipStream_t)stream);
  });
}

// The two entry points with a kernel of their own at d <= 64: `launch` starts its <D64, HAS_VAL> instantiation on the
// partitions, then the split rows go through `spmm_long_rows` with epilogue `ep`, exactly as gcr_spmm_csr_f32 runs them.
template <class Launch>
int32_t launch_walk(const Plan& p, int d, const Epilogue& ep, hipStream_t stream, Launch launch) {
  const dim3 blocks((unsigned)((p.n_parts + 3) / 4));
  auto go = [&](auto d64) {
    constexpr bool D64 = decltype(d64)::value;
    if (p.val != nullptr) launch(d64, std::true_type{}, blocks);
    else launch(d64, std::false_type{}, blocks);
    const int32_t st = GCR_LAUNCH_STATUS();
    if (st != GCR_OK) return st;
    return launch_long_rows<1, D64, false>(p, d, ep, stream);
  };
  return d == 64 ? go(std::true_type{}) : go(std::false_type{});
}

// The form CombineSink's HORNER instantiation is for: acc_in and acc_out given (in place included), no y.
bool is_horner(const float* y, const float* acc_in, const float* acc_out) {
  return y == nullptr && acc_in != nullptr && acc_out != nullptr;
}

// f(bool_constant<b>): a launch-time fact becomes a template argument
template <class F>
void dispatch_bool(bool b, F f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace

extern "C" int32_t gcr_spmm_csr_acc2_f32(const int64_t* desc, int64_t n_parts, const int32_t* long_row,
                                         const int32_t* long_slot0, int64_t n_long_rows, const int64_t* rowptr,
                                         const int32_t* col, const float* val, const uint32_t* keep_bits,
                                         float val_scale, const float* x, int32_t d, float* y, const float* acc_in,
                                         const float* acc_in2, float acc_in2_scale, float* acc_out, float acc_scale,
                                         uint32_t flags, float* inv_norm_out, float* partials, int64_t n_rows,
                                         int64_t n_cols, const uint32_t* col_active_bits, void* stream) {
  const Plan p{desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, partials};
  const int32_t st = check_plan(p, n_rows, n_cols, d, 256);
  if (st != GCR_LAUNCH) return st;
  GCR_CHECK_ARG(x != nullptr && (y != nullptr || acc_out != nullptr));
  GCR_CHECK_ARG(acc_in2 == nullptr || acc_out != nullptr);
  GCR_CHECK_ARG(col_active_bits == nullptr || keep_bits == nullptr);       // one predicate per launch
  GCR_CHECK_ARG((flags & ~GCR_SPMM_ROW_L2NORM) == 0);
  Epilogue ep = make_epilogue(val_scale, y, acc_in, acc_out, acc_scale);
  ep.flags = flags;
  ep.inv_norm_out = inv_norm_out;
  ep.acc_in2 = acc_in2;
  ep.acc_in2_scale = acc_in2_scale;
  ep.col_bits = col_active_bits;
  return launch_spmm_d(p, keep_bits, x, d, ep, stream);
}

extern "C" int32_t gcr_spmm_csr_f32(const int64_t* desc, int64_t n_parts, const int32_t* long_row,
                                    const int32_t* long_slot0, int64_t n_long_rows, const int64_t* rowptr,
                                    const int32_t* col, const float* val, const uint32_t* keep_bits,
                                    float val_scale, const float* x, int32_t d, float* y, const float* acc_in,
                                    float* acc_out, float acc_scale, uint32_t flags, float* inv_norm_out,
                                    float* partials, int64_t n_rows, int64_t n_cols, void* stream) {
  return gcr_spmm_csr_acc2_f32(desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, keep_bits, val_scale,
                               x, d, y, acc_in, nullptr, 0.f, acc_out, acc_scale, flags, inv_norm_out, partials, n_rows,
                               n_cols, nullptr, stream);
}

extern "C" int32_t gcr_spmm_csr_dual_f32(const int64_t* desc, int64_t n_parts, const int32_t* long_row,
                                         const int32_t* long_slot0, int64_t n_long_rows, const int64_t* rowptr,
                                         const int32_t* col, const float* val, const uint32_t* keep_bits,
                                         float val_scale, const float* x, int32_t d, float* y_raw, float* y_norm,
                                         float* inv_norm_out, float* partials, int64_t n_rows, int64_t n_cols,
                                         void* stream) {
  const Plan p{desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, partials};
  const int32_t st = check_plan(p, n_rows, n_cols, d, 256);
  if (st != GCR_LAUNCH) return st;
  GCR_CHECK_ARG(x != nullptr && y_raw != nullptr && y_norm != nullptr);
  GCR_CHECK_ARG(y_raw != y_norm);
  Epilogue ep = make_epilogue(val_scale, y_norm, nullptr, nullptr, 1.0f);
  ep.flags = GCR_SPMM_ROW_L2NORM;
  ep.inv_norm_out = inv_norm_out;
  ep.y_raw = y_raw;
  return launch_spmm_d(p, keep_bits, x, d, ep, stream);
}

// The dual launch with the layer-list accumulation folded in (mhcn.py:440-457 appends the normalised product of every layer
// to a list that is summed afterwards): acc_out = acc_in + normalize(A x) from the same pass; y_norm may be NULL — the backward
// rebuilds the normalised rows from y_raw and inv_norm_out (gcr_normalize_bwd_raw_f32).
extern "C" int32_t gcr_spmm_csr_dual_acc_f32(const int64_t* desc, int64_t n_parts, const int32_t* long_row,
                                             const int32_t* long_slot0, int64_t n_long_rows, const int64_t* rowptr,
                                             const int32_t* col, const float* val, const uint32_t* keep_bits,
                                             float val_scale, const float* x, int32_t d, float* y_raw, float* y_norm,
                                             const float* acc_in, float* acc_out, float* inv_norm_out, float* partials,
                                             int64_t n_rows, int64_t n_cols, void* stream) {
  const Plan p{desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, partials};
  const int32_t st = check_plan(p, n_rows, n_cols, d, 256);
  if (st != GCR_LAUNCH) return st;
  GCR_CHECK_ARG(x != nullptr && y_raw != nullptr && acc_out != nullptr);
  GCR_CHECK_ARG(y_raw != y_norm && y_raw != acc_out && (y_norm != nullptr || inv_norm_out != nullptr));
  Epilogue ep = make_epilogue(val_scale, y_norm, acc_in, acc_out, 1.0f);
  ep.flags = GCR_SPMM_ROW_L2NORM;
  ep.inv_norm_out = inv_norm_out;
  ep.y_raw = y_raw;
  return launch_spmm_d(p, keep_bits, x, d, ep, stream);
}

// out[hub_row[h]] = epilogue(sum over the n_windows window partials of hub row h): see spmm_hub_rows.
extern "C" int32_t gcr_spmm_hub_reduce_f32(const int32_t* hub_row, int64_t n_hub, int32_t n_windows, const float* partials,
                                           int32_t d, float val_scale, float* y, const float* acc_in, float* acc_out,
                                           float acc_scale, int64_t n_rows, void* stream) {
  GCR_CHECK_ARG(n_hub >= 0 && n_windows >= 1 && n_rows >= 0 && n_rows < (1ll << 31));
  GCR_CHECK_ARG(n_hub <= n_rows && n_hub * (int64_t)n_windows < (1ll << 31));
  GCR_CHECK_ARG(d >= 1 && d <= 256);
  if (n_hub == 0) return GCR_OK;
  GCR_CHECK_ARG(hub_row != nullptr && partials != nullptr);
  GCR_CHECK_ARG(y != nullptr || acc_out != nullptr);
  const Epilogue ep = make_epilogue(val_scale, y, acc_in, acc_out, acc_scale);
  return dispatch_d(d, [&](auto nv, auto d64) {
    hipLaunchKernelGGL((spmm_hub_rows<decltype(nv)::value, decltype(d64)::value>), dim3((unsigned)n_hub), dim3(256), 0,
                       (hipStream_t)stream, hub_row, n_hub, n_windows, partials, d, ep);
    return GCR_LAUNCH_STATUS();
  });
}

// Step 1 of a windowed launch (graph.py HubPlan) for d <= 64: y[H rows] = H x by `spmm_hub_parts`, then the companion's own
// split segments through `spmm_long_rows`, exactly as gcr_spmm_csr_f32 on H with y only would have run them.
extern "C" int32_t gcr_spmm_hub_parts_f32(const int64_t* desc, int64_t n_parts, const int32_t* long_row,
                                          const int32_t* long_slot0, int64_t n_long_rows, const int64_t* rowptr,
                                          const int32_t* col, const float* val, const float* x, int32_t d, float* y,
                                          float* partials, int64_t n_rows, int64_t n_cols, void* stream) {
  const Plan p{desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, partials};
  const int32_t st = check_plan(p, n_rows, n_cols, d, 64);
  if (st != GCR_LAUNCH) return st;
  GCR_CHECK_ARG(col != nullptr && x != nullptr && y != nullptr);
  hipStream_t s = (hipStream_t)stream;
  return launch_walk(p, d, make_epilogue(1.0f, y, nullptr, nullptr, 1.0f), s, [&](auto d64, auto hv, dim3 blocks) {
    hipLaunchKernelGGL((spmm_hub_parts<decltype(d64)::value, decltype(hv)::value>), blocks, dim3(256), 0, s, desc, n_parts,
                       rowptr, col, val, x, d, y, partials);
  });
}

// The plain launch at d <= 64 (no mask, no second addend, no row normalise): `spmm_rows` on the partitions, then the split
// rows through `spmm_long_rows` with the same epilogue, exactly as gcr_spmm_csr_f32 runs them.  Every word written equals
// that launch's.  d > 64: GCR_EUNSUPPORTED (the caller keeps gcr_spmm_csr_f32).
// row_id: NULL, or the row map of a row-ordered plan (gcr_spmm_rows_mapped_f32), the MAPPED instantiations.
namespace {
int32_t spmm_rows_entry(const Plan& p, const int32_t* row_id, float val_scale, const float* x, int32_t d, float* y,
                        const float* acc_in, float* acc_out, float acc_scale, int64_t n_rows, int64_t n_cols, void* stream) {
  const int32_t st = check_plan(p, n_rows, n_cols, d, 64);
  if (st != GCR_LAUNCH) return st;
  GCR_CHECK_ARG(x != nullptr && (y != nullptr || acc_out != nullptr));
  hipStream_t s = (hipStream_t)stream;
  return launch_walk(p, d, make_epilogue(val_scale, y, acc_in, acc_out, acc_scale), s,
                     [&](auto d64, auto hv, dim3 blocks) {
                       dispatch_bool(is_horner(y, acc_in, acc_out), [&](auto horner) {
                         dispatch_bool(row_id != nullptr, [&](auto mapped) {
                           hipLaunchKernelGGL((spmm_rows<decltype(d64)::value, decltype(hv)::value, decltype(horner)::value,
                                                         decltype(mapped)::value>),
                                              blocks, dim3(256), 0, s, p.desc, p.n_parts, p.rowptr, p.col, p.val, x, d,
                                              val_scale, y, acc_in, acc_out, acc_scale, p.partials, row_id);
                         });
                       });
                     });
}
}  // namespace

extern "C" int32_t gcr_spmm_rows_f32(const int64_t* desc, int64_t n_parts, const int32_t* long_row,
                                     const int32_t* long_slot0, int64_t n_long_rows, const int64_t* rowptr,
                                     const int32_t* col, const float* val, float val_scale, const float* x, int32_t d,
                                     float* y, const float* acc_in, float* acc_out, float acc_scale, float* partials,
                                     int64_t n_rows, int64_t n_cols, void* stream) {
  const Plan p{desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, partials};
  return spmm_rows_entry(p, nullptr, val_scale, x, d, y, acc_in, acc_out, acc_scale, n_rows, n_cols, stream);
}

// gcr_spmm_rows_f32 on a row-ordered plan (graph.py RowOrder): rowptr / col / val are the row-permuted copy P the plan
// partitions, row_id[P row] is the row of y / acc_in / acc_out that P row stands for, long_row holds such rows already.
// n_rows: of y / acc_in / acc_out.  Every row keeps its non-zeros in stored order, so every word written equals the
// unmapped launch's on the caller's own CSR.
extern "C" int32_t gcr_spmm_rows_mapped_f32(const int64_t* desc, int64_t n_parts, const int32_t* long_row,
                                            const int32_t* long_slot0, int64_t n_long_rows, const int64_t* rowptr,
                                            const int32_t* col, const float* val, const int32_t* row_id, float val_scale,
                                            const float* x, int32_t d, float* y, const float* acc_in, float* acc_out,
                                            float acc_scale, float* partials, int64_t n_rows, int64_t n_cols,
                                            void* stream) {
  GCR_CHECK_ARG(row_id != nullptr || n_parts == 0);
  const Plan p{desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, partials};
  return spmm_rows_entry(p, row_id, val_scale, x, d, y, acc_in, acc_out, acc_scale, n_rows, n_cols, stream);
}

// A whole windowed launch at d <= 64 (graph.py HubPlan) in three launches instead of five: `spmm_layer` walks the companion
// and the main plan in one grid, `spmm_long_rows_pair` sums the split rows of both, `spmm_hub_rows` reduces the window
// partials.  Every word written -- outputs, hub partials, both split-row workspaces -- equals what gcr_spmm_hub_parts_f32,
// gcr_spmm_hub_reduce_f32 and gcr_spmm_rows_f32 write when called in that order.  main_first: the main plan's blocks come
// first in the grid and the companion's start at the next multiple of 8 blocks; otherwise the companion's come first.
// row_id: NULL, or the row map of a row-ordered main plan (gcr_spmm_windowed_mapped_f32), the MAPPED instantiations.
namespace {
int32_t spmm_windowed_entry(
    const int64_t* hub_desc, int64_t hub_n_parts, const int32_t* hub_long_row, const int32_t* hub_long_slot0,
    int64_t hub_n_long_rows, const int64_t* hub_rowptr, const int32_t* hub_col, const float* hub_val, float* hub_split,
    const int64_t* desc, int64_t n_parts, const int32_t* long_row, const int32_t* long_slot0, int64_t n_long_rows,
    const int64_t* rowptr, const int32_t* col, const float* val, const int32_t* row_id, float* partials,
    const int32_t* hub_row, int64_t n_hub, int32_t n_windows, float* hub_partials, const float* x, int32_t d,
    float val_scale, float* y, const float* acc_in, float* acc_out, float acc_scale, int32_t main_first, int64_t n_rows,
    int64_t n_cols, void* stream) {
  GCR_CHECK_ARG(n_hub >= 0 && n_windows >= 1 && n_rows >= 0 && n_rows < (1ll << 31));
  GCR_CHECK_ARG(n_hub <= n_rows && n_hub * (int64_t)n_windows < (1ll << 31));
  GCR_CHECK_ARG(main_first >= 0 && main_first <= 2);
  Plan ph{hub_desc, hub_n_parts, hub_long_row, hub_long_slot0, hub_n_long_rows, hub_rowptr, hub_col, hub_val, hub_split};
  Plan pm{desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, partials};
  const int32_t sh = check_plan(ph, n_hub * (int64_t)n_windows, n_cols, d, 64);
  if (sh != GCR_LAUNCH && sh != GCR_OK) return sh;
  const int32_t sm = check_plan(pm, n_rows, n_cols, d, 64);
  if (sm != GCR_LAUNCH && sm != GCR_OK) return sm;
  if (sh == GCR_OK) ph.n_parts = ph.n_long = 0;          // an empty plan: its range of the grid is empty
  if (sm == GCR_OK) pm.n_parts = pm.n_long = 0;
  if (n_hub == 0 && pm.n_parts == 0) return GCR_OK;
  GCR_CHECK_ARG(x != nullptr && (y != nullptr || acc_out != nullptr));
  GCR_CHECK_ARG(n_hub == 0 || (hub_row != nullptr && hub_partials != nullptr));
  GCR_CHECK_ARG(ph.n_parts == 0 || (hub_col != nullptr && hub_partials != nullptr));
  GCR_CHECK_ARG(ph.n_parts == 0 || pm.n_parts == 0 || (hub_val == nullptr) == (val == nullptr));
  GCR_CHECK_ARG(ph.n_parts + pm.n_parts < (1ll << 31) - 64 && ph.n_long + pm.n_long < (1ll << 31));
  hipStream_t s = (hipStream_t)stream;
  const Epilogue ep = make_epilogue(val_scale, y, acc_in, acc_out, acc_scale);
  const unsigned hub_blocks = (unsigned)((ph.n_parts + 3) / 4), main_blocks = (unsigned)((pm.n_parts + 3) / 4);
  const unsigned hub_block0 = main_first ? (main_blocks + 7u) / 8u * 8u : 0u;
  const unsigned main_block0 = main_first ? 0u : hub_blocks;
  const unsigned blocks = main_first ? hub_block0 + hub_blocks : hub_blocks + main_blocks;
  const WalkSet wh{ph.desc, ph.n_parts, ph.rowptr, ph.col, ph.val, ph.partials};
  const WalkSet wm{pm.desc, pm.n_parts, pm.rowptr, pm.col, pm.val, pm.partials};
  const bool has_val = ph.n_parts > 0 ? hub_val != nullptr : val != nullptr;
  auto go = [&](auto d64) {
    constexpr bool D64 = decltype(d64)::value;
    // one grid, or (main_first == 2, the A/B script's cell for the merged split-row launch alone) one per range
    auto walk = [&](unsigned n_blocks, unsigned hb0, unsigned hb, unsigned mb0) {
      if (n_blocks == 0) return (int32_t)GCR_OK;
      dispatch_bool(is_horner(y, acc_in, acc_out), [&](auto horner) {
        constexpr bool HORNER = decltype(horner)::value;
        dispatch_bool(row_id != nullptr, [&](auto mapped) {
          constexpr bool MAPPED = decltype(mapped)::value;
          if (has_val)
            hipLaunchKernelGGL((spmm_layer<D64, true, HORNER, MAPPED>), dim3(n_blocks), dim3(256), 0, s, wh, wm, hb0, hb, mb0,
                               x, d, hub_partials, val_scale, y, acc_in, acc_out, acc_scale, row_id);
          else
            hipLaunchKernelGGL((spmm_layer<D64, false, HORNER, MAPPED>), dim3(n_blocks), dim3(256), 0, s, wh, wm, hb0, hb, mb0,
                               x, d, hub_partials, val_scale, y, acc_in, acc_out, acc_scale, row_id);
        });
      });
      return (int32_t)GCR_LAUNCH_STATUS();
    };
    int32_t st = main_first == 2 ? walk(hub_blocks, 0u, hub_blocks, 0u) : walk(blocks, hub_block0, hub_blocks, main_block0);
    if (st == GCR_OK && main_first == 2) st = walk(main_blocks, 0u, 0u, 0u);
    if (st != GCR_OK) return st;
    if (ph.n_long + pm.n_long > 0) {
      hipLaunchKernelGGL((spmm_long_rows_pair<D64>), dim3((unsigned)(ph.n_long + pm.n_long)), dim3(256), 0, s, ph.long_row,
                         ph.long_slot0, (unsigned)ph.n_long, ph.partials, hub_partials, pm.long_row, pm.long_slot0,
                         pm.partials, d, ep);
      const int32_t st = GCR_LAUNCH_STATUS();
      if (st != GCR_OK) return st;
    }
    if (n_hub == 0) return (int32_t)GCR_OK;
    hipLaunchKernelGGL((spmm_hub_rows<1, D64>), dim3((unsigned)n_hub), dim3(256), 0, s, hub_row, n_hub, n_windows,
                       hub_partials, d, ep);
    return (int32_t)GCR_LAUNCH_STATUS();
  };
  return d == 64 ? go(std::true_type{}) : go(std::false_type{});
}
}  // namespace

extern "C" int32_t gcr_spmm_windowed_f32(
    const int64_t* hub_desc, int64_t hub_n_parts, const int32_t* hub_long_row, const int32_t* hub_long_slot0,
    int64_t hub_n_long_rows, const int64_t* hub_rowptr, const int32_t* hub_col, const float* hub_val, float* hub_split,
    const int64_t* desc, int64_t n_parts, const int32_t* long_row, const int32_t* long_slot0, int64_t n_long_rows,
    const int64_t* rowptr, const int32_t* col, const float* val, float* partials, const int32_t* hub_row, int64_t n_hub,
    int32_t n_windows, float* hub_partials, const float* x, int32_t d, float val_scale, float* y, const float* acc_in,
    float* acc_out, float acc_scale, int32_t main_first, int64_t n_rows, int64_t n_cols, void* stream) {
  return spmm_windowed_entry(hub_desc, hub_n_parts, hub_long_row, hub_long_slot0, hub_n_long_rows, hub_rowptr, hub_col,
                             hub_val, hub_split, desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val,
                             nullptr, partials, hub_row, n_hub, n_windows, hub_partials, x, d, val_scale, y, acc_in,
                             acc_out, acc_scale, main_first, n_rows, n_cols, stream);
}

// gcr_spmm_windowed_f32 with a row-ordered main plan (graph.py RowOrder): rowptr / col / val are the row-permuted copy of
// the non-hub rows the main plan partitions, row_id its row map, long_row rows of the caller's arrays, as for
// gcr_spmm_rows_mapped_f32; the companion and the hub reduction are untouched.  Every word written equals the unmapped
// launch's.
extern "C" int32_t gcr_spmm_windowed_mapped_f32(
    const int64_t* hub_desc, int64_t hub_n_parts, const int32_t* hub_long_row, const int32_t* hub_long_slot0,
    int64_t hub_n_long_rows, const int64_t* hub_rowptr, const int32_t* hub_col, const float* hub_val, float* hub_split,
    const int64_t* desc, int64_t n_parts, const int32_t* long_row, const int32_t* long_slot0, int64_t n_long_rows,
    const int64_t* rowptr, const int32_t* col, const float* val, const int32_t* row_id, float* partials,
    const int32_t* hub_row, int64_t n_hub, int32_t n_windows, float* hub_partials, const float* x, int32_t d,
    float val_scale, float* y, const float* acc_in, float* acc_out, float acc_scale, int32_t main_first, int64_t n_rows,
    int64_t n_cols, void* stream) {
  GCR_CHECK_ARG(row_id != nullptr || n_parts == 0);
  return spmm_windowed_entry(hub_desc, hub_n_parts, hub_long_row, hub_long_slot0, hub_n_long_rows, hub_rowptr, hub_col,
                             hub_val, hub_split, desc, n_parts, long_row, long_slot0, n_long_rows, rowptr, col, val, row_id,
                             partials, hub_row, n_hub, n_windows, hub_partials, x, d, val_scale, y, acc_in, acc_out,
                             acc_scale, main_first, n_rows, n_cols, stream);
}

extern "C" int32_t gcr_csr_validate(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_cols,
                                    int64_t nnz, int64_t* n_errors_dev, void* stream) {
  GCR_CHECK_ARG(rowptr != nullptr && n_errors_dev != nullptr && n_rows >= 0 && nnz >= 0 && n_cols >= 0);
  GCR_CHECK_ARG(nnz == 0 || col != nullptr);
  hipLaunchKernelGGL(csr_validate_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, rowptr, col, n_rows,
                     n_cols, nnz, (unsigned long long*)n_errors_dev);
  return GCR_LAUNCH_STATUS();
}
