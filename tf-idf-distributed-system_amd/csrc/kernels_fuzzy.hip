// kernels_fuzzy.hip — fuzzy term lookup (tfidf_fuzzy_terms*): the vocabulary
// terms within max_edits <= 2 edits of each input term, found by streaming
// passes over the snapshot's device dictionary.  The filter, the banded OSA
// distance and the sort key are the shared functions of fuzzy_plan.h.
//
//   k_fz_scan      a chunk of input terms (code points, staged in LDS) against
//                  every occupied slot with df >= 1: a lane takes a slot,
//                  decodes its exact key in registers and tests the chunk's
//                  terms (character-set signature, length, prefix, then the
//                  DP).  <false> counts the survivors per term (LDS counters,
//                  flushed once per workgroup) and compacts the numbers of the
//                  hashed slots it passes; <true> appends (sort key, slot) at
//                  positions taken from one wave-aggregated atomic per wave and
//                  term, never past the capacity the counts gave.  For the
//                  fuzzy search (FzScan::search) a candidate also needs
//                  fzs_keep and the key is fzs_sort_key (fuzzy_search_plan.h)
//   k_fz_hashed    the same test for the compacted hashed slots (long terms):
//                  a lane reads its slot's reference occurrence from the corpus
//                  and lower-cases it on the way
//   fz_sort        (term, dist, df descending) order of a candidate chunk
//                  (hipCUB radix sort of the packed keys, slots as values)
//   k_fz_select    per term: how many of its sorted candidates the host needs:
//                  the first max_out and every later one that ties with the
//                  max_out-th on (dist, df)
//   k_fz_gather    those candidates of every term, packed
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "fuzzy_plan.h"
#include "fuzzy_search_plan.h"
#include "tfidf_internal.h"

namespace tfidf {

constexpr uint32_t kFzThreads = 256;

struct FzLds {
  uint32_t off[kFzChunkTerms + 1];
  uint32_t cnt[kFzChunkTerms];
  uint32_t cps[kFzChunkCps];
  uint64_t sig[kFzChunkTerms];     // fz_sig_term per staged term
};

__device__ __forceinline__ void fz_stage(const FzScan &a, FzLds &L) {
  for (uint32_t i = threadIdx.x; i <= a.n_terms; i += kFzThreads) L.off[i] = a.t_off[i];
  for (uint32_t i = threadIdx.x; i < a.n_terms; i += kFzThreads) L.cnt[i] = 0;
  const uint32_t nc = a.t_off[a.n_terms];
  for (uint32_t i = threadIdx.x; i < nc; i += kFzThreads) L.cps[i] = a.t_cps[i];
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < a.n_terms; i += kFzThreads)
    L.sig[i] = fz_sig_term(L.cps + L.off[i], L.off[i + 1] - L.off[i]);
  __syncthreads();
}

__device__ __forceinline__ void fz_flush(const FzScan &a, FzLds &L) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < a.n_terms; i += kFzThreads)
    if (L.cnt[i]) atomicAdd(a.counts + i, L.cnt[i]);
}

// wave-aggregated append: the lanes with `take` get consecutive positions from one atomicAdd
__device__ __forceinline__ uint32_t fz_wave_pos(uint32_t *cursor, bool take, uint32_t lane) {
  const uint64_t m = __ballot(take);
  if (m == 0) return 0;
  const uint32_t leader = (uint32_t)__builtin_ctzll(m);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(cursor, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, (int)leader, 64);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
}

// the chunk's terms against this lane's candidate (have: the lane holds one);
// every lane of the wave runs the loop, so the ballots are wave-uniform
template <bool FILL, class Cursor>
__device__ __forceinline__ void fz_test_terms(const FzScan &a, FzLds &L, bool have, const Cursor &c, uint32_t n_cand,
                                              uint32_t df, uint32_t slot, uint32_t lane) {
  const uint64_t sig = have ? fz_sig(c, n_cand) : 0;
  for (uint32_t t = 0; t < a.n_terms; t++) {
    const uint32_t o = L.off[t], n = L.off[t + 1] - o;
    if (n == 0) continue;                                            // a term without candidates
    uint32_t d = kFzFar;
    if (have && fz_sig_ok(L.sig[t], sig, a.max_edits))
      d = fz_match(L.cps + o, n, c, n_cand, a.max_edits, a.prefix_len);
    const uint32_t m = fzs_min_len(n, n_cand);
    if (a.search && d != kFzFar && !fzs_keep(d, m)) d = kFzFar;     // fuzzy search: a boost of 0 or less is no candidate
    const bool hit = d != kFzFar;
    if (FILL) {
      const uint32_t pos = fz_wave_pos(a.cursor, hit, lane);
      if (hit && pos < a.cap) {
        a.keys[pos] = a.search ? fzs_sort_key(t, d, m) : fz_sort_key(t, d, df);
        a.slots[pos] = slot;
      }
    } else if (hit) {
      atomicAdd(&L.cnt[t], 1u);
    }
  }
}

template <bool FILL>
__global__ void __launch_bounds__(kFzThreads) k_fz_scan(const FzScan a) {
  __shared__ FzLds L;
  fz_stage(a, L);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *dlo = a.dict, *dhi = a.dict + a.C;
  for (uint64_t s0 = (uint64_t)blockIdx.x * kFzThreads; s0 < a.C; s0 += (uint64_t)gridDim.x * kFzThreads) {
    const uint64_t s = s0 + threadIdx.x;
    const bool in = s < a.C;
    const uint64_t lo = in ? dlo[s] : 0;
    const uint32_t df = lo ? a.df[s] : 0;
    const bool occ = lo != 0 && df >= 1;
    const bool hashed = occ && key_is_hashed(lo);
    if (!FILL && a.hs_list) {                                        // the hashed slots: k_fz_hashed's work list
      const uint32_t pos = fz_wave_pos(a.hs_count, hashed, lane);
      if (hashed && pos < a.hs_cap) a.hs_list[pos] = (uint32_t)s;
    }
    const bool exact = occ && !hashed;
    if (!__any(exact)) continue;
    FzWordCursor c{0, 0, 0};
    uint32_t n_cand = 0;
    if (exact) fz_key_words(lo, dhi[s], &c, &n_cand);
    fz_test_terms<FILL>(a, L, exact, c, n_cand, df, (uint32_t)s, lane);
  }
  if (!FILL) fz_flush(a, L);
}

template <bool FILL>
__global__ void __launch_bounds__(kFzThreads) k_fz_hashed(const FzScan a, const uint8_t *__restrict__ text,
                                                          uint64_t text_bytes) {
  __shared__ FzLds L;
  fz_stage(a, L);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *dref = a.dict + 2 * (uint64_t)a.C;
  for (uint32_t i0 = blockIdx.x * kFzThreads; i0 < a.hs_n; i0 += gridDim.x * kFzThreads) {
    const uint32_t i = i0 + threadIdx.x;
    bool have = i < a.hs_n;
    uint32_t slot = 0, df = 0, n_cand = 0;
    FzTextCursor c{text, 0, 0};
    if (have) {
      slot = a.hs_list[i];
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
    fz_test_terms<FILL>(a, L, have, c, n_cand, df, slot, lane);
  }
  if (!FILL) fz_flush(a, L);
}

// sorted keys of term t: [seg[t], seg[t + 1]); take[t] = the candidates the
// host orders: all when there are at most max_out, else the first max_out and
// the rest of the (dist, df) tie group the max_out-th belongs to
__global__ void __launch_bounds__(256) k_fz_select(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg,
                                                   uint32_t n_terms, uint32_t max_out, uint32_t *__restrict__ take) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_terms) return;
  const uint32_t o = seg[t], c = seg[t + 1] - o;
  if (c <= max_out) { take[t] = c; return; }
  const uint64_t k = keys[o + max_out - 1];
  uint32_t lo = o + max_out, hi = o + c;                             // first key > k
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] <= k) lo = mid + 1; else hi = mid;
  }
  take[t] = lo - o;
}

__global__ void __launch_bounds__(256) k_fz_gather(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ slots,
                                                   const uint32_t *__restrict__ seg, const uint32_t *__restrict__ out_off,
                                                   uint64_t *__restrict__ o_keys, uint32_t *__restrict__ o_slots) {
  const uint32_t t = blockIdx.x;
  const uint32_t src = seg[t], dst = out_off[t], n = out_off[t + 1] - dst;
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    o_keys[dst + i] = keys[src + i];
    o_slots[dst + i] = slots[src + i];
  }
}

// --- launch wrappers (tfidf_capi.hip) ---
static unsigned fz_grid(uint64_t n, int max_grid) {
  const uint64_t g = (n + kFzThreads - 1) / kFzThreads;
  return (unsigned)(g < 1 ? 1 : (g > (uint64_t)max_grid ? (uint64_t)max_grid : g));
}

hipError_t launch_fz_scan(bool fill, const FzScan &a, int max_grid, hipStream_t s) {
  const dim3 grid(fz_grid(a.C, max_grid)), block(kFzThreads);
  if (fill)
    hipLaunchKernelGGL(k_fz_scan<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(k_fz_scan<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_fz_hashed(bool fill, const FzScan &a, const uint8_t *text, uint64_t text_bytes, int max_grid,
                            hipStream_t s) {
  if (a.hs_n == 0) return hipSuccess;
  const dim3 grid(fz_grid(a.hs_n, max_grid)), block(kFzThreads);
  if (fill)
    hipLaunchKernelGGL(k_fz_hashed<true>, grid, block, 0, s, a, text, text_bytes);
  else
    hipLaunchKernelGGL(k_fz_hashed<false>, grid, block, 0, s, a, text, text_bytes);
  return hipGetLastError();
}

// tmp == nullptr: *tmp_bytes = the scratch the sort of n pairs needs
hipError_t fz_sort(void *tmp, size_t *tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *slots_in,
                   uint32_t *slots_out, uint32_t n, hipStream_t s) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, keys_in, keys_out, slots_in, slots_out, (int)n, 0, 48, s);
}

hipError_t launch_fz_select(const uint64_t *keys, const uint32_t *seg, uint32_t n_terms, uint32_t max_out,
                            uint32_t *take, hipStream_t s) {
  if (n_terms == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fz_select, dim3((n_terms + 255) / 256), dim3(256), 0, s, keys, seg, n_terms, max_out, take);
  return hipGetLastError();
}

hipError_t launch_fz_gather(const uint64_t *keys, const uint32_t *slots, const uint32_t *seg, const uint32_t *out_off,
                            uint32_t n_terms, uint64_t *o_keys, uint32_t *o_slots, hipStream_t s) {
  if (n_terms == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fz_gather, dim3(n_terms), dim3(256), 0, s, keys, slots, seg, out_off, o_keys, o_slots);
  return hipGetLastError();
}

}  // namespace tfidf
