// kernels_regex.hip — regular-expression search (tfidf_regex_terms*,
// tfidf_search_regex*): the vocabulary terms that belong to each pattern's
// language, found by streaming passes over the snapshot's device dictionary.
// The host compiles every pattern to a minimal DFA table (regex_plan.h); the
// match is a table walk, one LDS class read and one LDS transition read per
// code point.  Everything after the match (the (pattern, df) sort, the
// selection, the posting union) is the wildcard route's, as it is.
//
//   k_rx_scan      a chunk of tables (staged in LDS, kRxStageWords words at
//                  most) against every occupied slot with df >= 1: a lane takes
//                  a slot, decodes its exact key in registers and walks each
//                  table whose length bounds admit the term.  <false> counts
//                  the matches per pattern (LDS counters, flushed once per
//                  workgroup) and compacts the hashed slots it passes; <true>
//                  appends (sort key, slot) at positions taken from one
//                  wave-aggregated atomic per wave and pattern, never past the
//                  capacity the counts gave
//   k_rx_hashed    the same test for the compacted hashed slots (long terms),
//                  read from their reference occurrence in the corpus
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "regex_plan.h"
#include "tfidf_internal.h"
#include "wave_ops.h"

namespace tfidf {

constexpr uint32_t kRxThreads = 256;

// 33 796 bytes: 4 workgroups (16 waves) stay resident in the 160 KiB of a CU
struct RxLds {
  uint32_t off[kWcChunkPatterns + 1];
  uint32_t cnt[kWcChunkPatterns];
  uint32_t tab[kRxStageWords];
};

__device__ __forceinline__ void rx_stage(const FzScan &a, RxLds &L) {
  for (uint32_t i = threadIdx.x; i <= a.n_terms; i += kRxThreads) L.off[i] = min(a.t_off[i] - a.t_off[0], kRxStageWords);
  for (uint32_t i = threadIdx.x; i < a.n_terms; i += kRxThreads) L.cnt[i] = 0;
  const uint32_t w0 = a.t_off[0], nw = min(a.t_off[a.n_terms] - w0, kRxStageWords);
  for (uint32_t i = threadIdx.x; i < nw; i += kRxThreads) L.tab[i] = a.t_cps[w0 + i];
  __syncthreads();
}

__device__ __forceinline__ void rx_flush(const FzScan &a, RxLds &L) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < a.n_terms; i += kRxThreads)
    if (L.cnt[i]) atomicAdd(a.counts + i, L.cnt[i]);
}

// the chunk's tables against this lane's candidate (have: the lane holds one);
// every lane of the wave runs the loop, so the ballots are wave-uniform
template <bool FILL, class Cursor>
__device__ __forceinline__ void rx_test_patterns(const FzScan &a, RxLds &L, bool have, const Cursor &c, uint32_t n_cand,
                                                 uint32_t df, uint32_t slot, uint32_t lane) {
  for (uint32_t t = 0; t < a.n_terms; t++) {
    const uint32_t o = L.off[t];
    const uint32_t nw = L.off[t + 1] - o;
    if (nw < kRxHeaderWords + 32 || L.tab[o] != nw) continue;        // no table (a pattern that matches nothing), or not a whole one
    const bool hit = have && rx_match(L.tab + o, c, n_cand);
    if (FILL) {
      const uint32_t pos = wc_wave_pos(a.cursor, hit, lane);
      if (hit && pos < a.cap) {
        a.keys[pos] = wc_sort_key(t, df);
        a.slots[pos] = slot;
      }
    } else if (hit) {
      atomicAdd(&L.cnt[t], 1u);
    }
  }
}

template <bool FILL>
__global__ void __launch_bounds__(kRxThreads) k_rx_scan(const FzScan a) {
  __shared__ RxLds L;
  rx_stage(a, L);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *dlo = a.dict, *dhi = a.dict + a.C;
  for (uint64_t s0 = (uint64_t)blockIdx.x * kRxThreads; s0 < a.C; s0 += (uint64_t)gridDim.x * kRxThreads) {
    const uint64_t s = s0 + threadIdx.x;
    const bool in = s < a.C;
    const uint64_t lo = in ? dlo[s] : 0;
    const uint32_t df = lo ? a.df[s] : 0;
    const bool occ = lo != 0 && df >= 1;
    const bool hashed = occ && key_is_hashed(lo);
    if (!FILL && a.hs_list) {                                        // the hashed slots: k_rx_hashed's work list
      const uint32_t pos = wc_wave_pos(a.hs_count, hashed, lane);
      if (hashed && pos < a.hs_cap) a.hs_list[pos] = (uint32_t)s;
    }
    const bool exact = occ && !hashed;
    if (!__any(exact)) continue;
    FzWordCursor c{0, 0, 0};
    uint32_t n_cand = 0;
    if (exact) fz_key_words(lo, dhi[s], &c, &n_cand);
    rx_test_patterns<FILL>(a, L, exact, c, n_cand, df, (uint32_t)s, lane);
  }
  if (!FILL) rx_flush(a, L);
}

template <bool FILL>
__global__ void __launch_bounds__(kRxThreads) k_rx_hashed(const FzScan a, const uint8_t *__restrict__ text,
                                                          uint64_t text_bytes) {
  __shared__ RxLds L;
  rx_stage(a, L);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *dref = a.dict + 2 * (uint64_t)a.C;
  for (uint32_t i0 = blockIdx.x * kRxThreads; i0 < a.hs_n; i0 += gridDim.x * kRxThreads) {
    const uint32_t i = i0 + threadIdx.x;
    bool have = i < a.hs_n;
    uint32_t slot = 0, df = 0, n_cand = 0;
    FzTextCursor c{text, 0, 0};
    if (have) {
      slot = a.hs_list[i];
      have = slot < a.C;
    }
    if (have) {
      df = a.df[slot];
      const uint64_t r = dref[slot];
      const uint64_t off = dict_ref_off(r);
      const uint32_t len = dict_ref_len(r);
      have = r != 0 && off + len <= text_bytes;                      // a reference always lies inside the corpus
      if (have) {
        c.s = text + off;
        c.n = len;
        n_cand = fz_text_cps(c.s, len);
        have = n_cand != 0;
      }
    }
    if (!__any(have)) continue;
    rx_test_patterns<FILL>(a, L, have, c, n_cand, df, slot, lane);
  }
  if (!FILL) rx_flush(a, L);
}

// --- launch wrappers (tfidf_capi.hip) ---
static unsigned rx_grid(uint64_t n, int max_grid) {
  const uint64_t g = (n + kRxThreads - 1) / kRxThreads;
  return (unsigned)(g < 1 ? 1 : (g > (uint64_t)max_grid ? (uint64_t)max_grid : g));
}

hipError_t launch_rx_scan(bool fill, const FzScan &a, int max_grid, hipStream_t s) {
  const dim3 grid(rx_grid(a.C, max_grid)), block(kRxThreads);
  if (fill)
    hipLaunchKernelGGL(k_rx_scan<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(k_rx_scan<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rx_hashed(bool fill, const FzScan &a, const uint8_t *text, uint64_t text_bytes, int max_grid,
                            hipStream_t s) {
  if (a.hs_n == 0) return hipSuccess;
  const dim3 grid(rx_grid(a.hs_n, max_grid)), block(kRxThreads);
  if (fill)
    hipLaunchKernelGGL(k_rx_hashed<true>, grid, block, 0, s, a, text, text_bytes);
  else
    hipLaunchKernelGGL(k_rx_hashed<false>, grid, block, 0, s, a, text, text_bytes);
  return hipGetLastError();
}

}  // namespace tfidf
