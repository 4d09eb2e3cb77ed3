// kernels_wildcard.hip — wildcard and prefix search (tfidf_wildcard_terms*,
// tfidf_search_wildcard*): the vocabulary terms that match each pattern, found
// by streaming passes over the snapshot's device dictionary, and the union of
// their posting rows as one ascending document list per pattern.  The parse,
// the cheap tests and the matcher are the shared functions of wildcard_plan.h.
//
//   k_wc_scan      a chunk of patterns (elements, staged in LDS with their
//                  prefix length and minimum count) against every occupied
//                  slot with df >= 1: a lane takes a slot, decodes its exact
//                  key in registers and tests the chunk's patterns.  <false>
//                  counts the matches per pattern (LDS counters, flushed once
//                  per workgroup) and compacts the hashed slots it passes;
//                  <true> appends (sort key, slot) at positions taken from one
//                  wave-aggregated atomic per wave and pattern, never past the
//                  capacity the counts gave
//   k_wc_hashed    the same test for the compacted hashed slots (long terms),
//                  read from their reference occurrence in the corpus
//   (the terms route then orders and selects with fz_sort / k_fz_select /
//   k_fz_gather as they are; the sort also groups the slots by pattern)
//   k_wc_union_block   block-major: one workgroup per (pattern, 8 192-document
//                  block) with the block's bitmap in LDS (1 KiB).  A lane takes
//                  a matched column (slot -> column through crank) and reads
//                  its segment bounds in the block; most are empty.  Short
//                  segments are ORed in by their lane, long ones by the wave
//   k_wc_rows / k_wc_union_term   term-major: the matched rows' lengths (then
//                  scanned), and their flattened (term, posting) pairs, one
//                  per lane, ORed into the patterns' global bitmaps
//   k_wc_count     bits per (pattern, block) (then scanned into offsets)
//   k_wc_expand    the set bits of a (pattern, block) as ascending doc ids
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfidf_internal.h"
#include "wave_ops.h"
#include "wildcard_plan.h"

namespace tfidf {

constexpr uint32_t kWcThreads = 256;
constexpr uint32_t kWcBlockWords = kBlockDocs / 32;     // bitmap words of a document block
static_assert(kWcBlockWords == kWcThreads, "one bitmap word per thread");
constexpr uint32_t kWcSerial = 4;                       // postings of a segment its own lane ORs in

struct WcLds {
  uint32_t off[kWcChunkPatterns + 1];
  uint32_t cnt[kWcChunkPatterns];
  WcMeta meta[kWcChunkPatterns];
  uint32_t el[kWcChunkElems];
};

__device__ __forceinline__ void wc_stage(const FzScan &a, WcLds &L) {
  for (uint32_t i = threadIdx.x; i <= a.n_terms; i += kWcThreads) L.off[i] = a.t_off[i] - a.t_off[0];
  for (uint32_t i = threadIdx.x; i < a.n_terms; i += kWcThreads) L.cnt[i] = 0;
  const uint32_t e0 = a.t_off[0], ne = min(a.t_off[a.n_terms] - e0, kWcChunkElems);
  for (uint32_t i = threadIdx.x; i < ne; i += kWcThreads) L.el[i] = a.t_cps[e0 + i];
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < a.n_terms; i += kWcThreads)
    L.meta[i] = wc_meta(L.el + L.off[i], L.off[i + 1] - L.off[i]);
  __syncthreads();
}

__device__ __forceinline__ void wc_flush(const FzScan &a, WcLds &L) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < a.n_terms; i += kWcThreads)
    if (L.cnt[i]) atomicAdd(a.counts + i, L.cnt[i]);
}

// the chunk's patterns against this lane's candidate (have: the lane holds
// one); every lane of the wave runs the loop, so the ballots are wave-uniform
template <bool FILL, class Cursor>
__device__ __forceinline__ void wc_test_patterns(const FzScan &a, WcLds &L, bool have, const Cursor &c, uint32_t n_cand,
                                                 uint32_t df, uint32_t slot, uint32_t lane) {
  for (uint32_t t = 0; t < a.n_terms; t++) {
    const uint32_t o = L.off[t], n = L.off[t + 1] - o;
    if (n == 0) continue;                                            // a pattern that matches nothing
    const bool hit = have && wc_match(L.el + o, n, L.meta[t], c, n_cand);
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
__global__ void __launch_bounds__(kWcThreads) k_wc_scan(const FzScan a) {
  __shared__ WcLds L;
  wc_stage(a, L);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *dlo = a.dict, *dhi = a.dict + a.C;
  for (uint64_t s0 = (uint64_t)blockIdx.x * kWcThreads; s0 < a.C; s0 += (uint64_t)gridDim.x * kWcThreads) {
    const uint64_t s = s0 + threadIdx.x;
    const bool in = s < a.C;
    const uint64_t lo = in ? dlo[s] : 0;
    const uint32_t df = lo ? a.df[s] : 0;
    const bool occ = lo != 0 && df >= 1;
    const bool hashed = occ && key_is_hashed(lo);
    if (!FILL && a.hs_list) {                                        // the hashed slots: k_wc_hashed's work list
      const uint32_t pos = wc_wave_pos(a.hs_count, hashed, lane);
      if (hashed && pos < a.hs_cap) a.hs_list[pos] = (uint32_t)s;
    }
    const bool exact = occ && !hashed;
    if (!__any(exact)) continue;
    FzWordCursor c{0, 0, 0};
    uint32_t n_cand = 0;
    if (exact) fz_key_words(lo, dhi[s], &c, &n_cand);
    wc_test_patterns<FILL>(a, L, exact, c, n_cand, df, (uint32_t)s, lane);
  }
  if (!FILL) wc_flush(a, L);
}

template <bool FILL>
__global__ void __launch_bounds__(kWcThreads) k_wc_hashed(const FzScan a, const uint8_t *__restrict__ text,
                                                          uint64_t text_bytes) {
  __shared__ WcLds L;
  wc_stage(a, L);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *dref = a.dict + 2 * (uint64_t)a.C;
  for (uint32_t i0 = blockIdx.x * kWcThreads; i0 < a.hs_n; i0 += gridDim.x * kWcThreads) {
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
    wc_test_patterns<FILL>(a, L, have, c, n_cand, df, slot, lane);
  }
  if (!FILL) wc_flush(a, L);
}

// --- the union ---

__global__ void __launch_bounds__(kWcThreads) k_wc_union_block(const WcUnion a) {
  __shared__ uint32_t bits[kWcBlockWords];
  const uint32_t b = blockIdx.x, p = blockIdx.y, lane = threadIdx.x & 63u;
  bits[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t m0 = a.seg[p], m1 = a.seg[p + 1];
  const uint32_t *row = a.blk + (size_t)b * a.NC;
  const uint64_t bb = a.bbase[b], be = a.bbase[b + 1];
  const uint32_t blen = be >= bb && be <= a.post_words ? (uint32_t)min(be - bb, (uint64_t)0xFFFFFFFFu) : 0u;
  const uint32_t *post = a.post32 + bb;
  // every lane of a wave runs the same trips (the ballot below needs them all)
  for (uint32_t base = m0 + (threadIdx.x & ~63u); base < m1; base += kWcThreads) {
    const uint32_t m = base + lane;
    uint32_t s0 = 0, len = 0;
    if (m < m1) {
      const uint32_t slot = a.slots[m];
      if (slot < a.C) {
        const uint2 e = a.crank[slot >> 5];
        const uint32_t col = e.y + (uint32_t)__popc(e.x & ((1u << (slot & 31u)) - 1u));
        if (col < a.NC) {
          s0 = row[col];
          const uint32_t s1 = col + 1 < a.NC ? row[col + 1] : blen;
          len = s1 > s0 && s1 <= blen ? s1 - s0 : 0u;                // a segment always lies inside its block
        }
      }
    }
    const uint32_t ser = len < kWcSerial ? len : kWcSerial;
    for (uint32_t i = 0; i < ser; i++) {
      const uint32_t d = post[s0 + i] & (kBlockDocs - 1);
      atomicOr(&bits[d >> 5], 1u << (d & 31u));
    }
    uint64_t big = __ballot(len > kWcSerial);
    while (big) {
      const int l = __builtin_ctzll(big);
      big &= big - 1;
      const uint32_t w0 = (uint32_t)__shfl((int)s0, l, 64), wl = (uint32_t)__shfl((int)len, l, 64);
      for (uint32_t i = kWcSerial + lane; i < wl; i += 64) {
        const uint32_t d = post[w0 + i] & (kBlockDocs - 1);
        atomicOr(&bits[d >> 5], 1u << (d & 31u));
      }
    }
  }
  __syncthreads();
  a.bits[((uint64_t)p * a.n_blocks + b) * kWcBlockWords + threadIdx.x] = bits[threadIdx.x];
}

__global__ void __launch_bounds__(256) k_wc_rows(const WcUnion a, uint32_t M) {
  const uint32_t m = a.seg[0] + blockIdx.x * 256 + threadIdx.x;
  if (m >= a.seg[0] + M) return;
  const uint32_t slot = a.slots[m];
  uint64_t n = 0;
  if (slot < a.C) {
    const uint64_t t0 = a.toff[slot], t1 = a.toff[slot + 1];
    if (t1 >= t0 && t1 <= a.post_words) n = t1 - t0;                 // a row always lies inside the postings
  }
  a.row_off[m - a.seg[0]] = n;
}

// last i in [0, n) with off[i] <= e
template <class T>
__device__ __forceinline__ uint32_t wc_last_le(const T *off, uint32_t n, uint64_t e) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kWcThreads) k_wc_union_term(const WcUnion a, uint32_t M) {
  const uint64_t total = a.row_off[M];
  const uint32_t m_first = a.seg[0];
  const uint64_t words = (uint64_t)a.n_blocks * kWcBlockWords;
  for (uint64_t e = (uint64_t)blockIdx.x * kWcThreads + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kWcThreads) {
    const uint32_t mi = wc_last_le(a.row_off, M, e);
    const uint32_t slot = a.slots[m_first + mi];
    if (slot >= a.C) continue;
    const uint64_t i = a.toff[slot] + (e - a.row_off[mi]);
    if (i >= a.post_words) continue;
    const uint32_t doc = (uint32_t)a.post[i];
    if (doc >= a.n_docs) continue;
    const uint32_t p = wc_last_le(a.seg, a.n_pat, (uint64_t)(m_first + mi));   // patterns without matches share a start: the last one holds mi
    atomicOr(a.bits + (uint64_t)p * words + (doc >> 5), 1u << (doc & 31u));
  }
}

__global__ void __launch_bounds__(kWcThreads) k_wc_count(const WcUnion a) {
  __shared__ uint32_t tot;
  if (threadIdx.x == 0) tot = 0;
  __syncthreads();
  const uint64_t idx = (uint64_t)blockIdx.y * a.n_blocks + blockIdx.x;
  const uint32_t c = (uint32_t)__popc(a.bits[idx * kWcBlockWords + threadIdx.x]);
  if (c) atomicAdd(&tot, c);
  __syncthreads();
  if (threadIdx.x == 0) a.cnt[idx] = tot;
}

__global__ void __launch_bounds__(kWcThreads) k_wc_expand(const WcUnion a) {
  __shared__ uint32_t sum[kWcThreads];
  const uint64_t idx = (uint64_t)blockIdx.y * a.n_blocks + blockIdx.x;
  uint32_t w = a.bits[idx * kWcBlockWords + threadIdx.x];
  const uint32_t c = (uint32_t)__popc(w);
  sum[threadIdx.x] = c;
  __syncthreads();
  for (uint32_t d = 1; d < kWcThreads; d <<= 1) {                    // inclusive scan of the words' counts
    const uint32_t v = threadIdx.x >= d ? sum[threadIdx.x - d] : 0u;
    __syncthreads();
    sum[threadIdx.x] += v;
    __syncthreads();
  }
  uint64_t at = a.cnt[idx] + (sum[threadIdx.x] - c);                 // cnt: scanned, so the (pattern, block)'s first hit
  const uint32_t d0 = blockIdx.x * kBlockDocs + threadIdx.x * 32u;
  while (w) {
    const uint32_t bit = (uint32_t)__builtin_ctz(w);
    w &= w - 1;
    if (at < a.out_cap) a.out[at] = d0 + bit;
    at++;
  }
}

// --- launch wrappers (tfidf_capi.hip) ---
static unsigned wc_grid(uint64_t n, int max_grid) {
  const uint64_t g = (n + kWcThreads - 1) / kWcThreads;
  return (unsigned)(g < 1 ? 1 : (g > (uint64_t)max_grid ? (uint64_t)max_grid : g));
}

hipError_t launch_wc_scan(bool fill, const FzScan &a, int max_grid, hipStream_t s) {
  const dim3 grid(wc_grid(a.C, max_grid)), block(kWcThreads);
  if (fill)
    hipLaunchKernelGGL(k_wc_scan<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(k_wc_scan<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wc_hashed(bool fill, const FzScan &a, const uint8_t *text, uint64_t text_bytes, int max_grid,
                            hipStream_t s) {
  if (a.hs_n == 0) return hipSuccess;
  const dim3 grid(wc_grid(a.hs_n, max_grid)), block(kWcThreads);
  if (fill)
    hipLaunchKernelGGL(k_wc_hashed<true>, grid, block, 0, s, a, text, text_bytes);
  else
    hipLaunchKernelGGL(k_wc_hashed<false>, grid, block, 0, s, a, text, text_bytes);
  return hipGetLastError();
}

hipError_t launch_wc_union_block(const WcUnion &a, hipStream_t s) {
  if (a.n_pat == 0 || a.n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wc_union_block, dim3(a.n_blocks, a.n_pat), dim3(kWcThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wc_rows(const WcUnion &a, uint32_t M, hipStream_t s) {
  if (M == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wc_rows, dim3((M + 255) / 256), dim3(256), 0, s, a, M);
  return hipGetLastError();
}

hipError_t launch_wc_union_term(const WcUnion &a, uint32_t M, uint64_t n_post_bound, int max_grid, hipStream_t s) {
  if (M == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wc_union_term, dim3(wc_grid(n_post_bound, max_grid)), dim3(kWcThreads), 0, s, a, M);
  return hipGetLastError();
}

hipError_t launch_wc_count(const WcUnion &a, hipStream_t s) {
  if (a.n_pat == 0 || a.n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wc_count, dim3(a.n_blocks, a.n_pat), dim3(kWcThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wc_expand(const WcUnion &a, hipStream_t s) {
  if (a.n_pat == 0 || a.n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wc_expand, dim3(a.n_blocks, a.n_pat), dim3(kWcThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace tfidf
