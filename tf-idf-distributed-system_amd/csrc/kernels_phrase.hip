// kernels_phrase.hip — exact phrase search on the device corpus
// (tfidf_search_phrase*): re-scan only the candidate documents (the conjunction
// of the phrase's terms), count the phrase's occurrences and score them.  The
// scan, the frequency rule, the score and the ordering key are the shared
// functions of phrase_plan.h; the work split is snippet_plan.h's.
//
//   k_ph_scan      one wave per (row, chunk) item, one lane per slice, against
//                  the key segment of the row's phrase: <false> counts each
//                  slice's tokens and its listed tokens, <true> writes (token
//                  position in the document, ordinal) per listed token at the
//                  slice's scanned offset; the fill never writes more than
//                  the counting pass reported for its slice
//   k_ph_freq      one wave per row: the lanes take the row's listed tokens as
//                  starts (ph_match_at), a wave reduction gives freq
//   k_ph_sloppy_freq  (tfidf_search_phrase_slop*) one wave per row, freq as a
//                  float: k_ph_freq's count for a row at slop 0 or of one term,
//                  else the SloppyPhraseMatcher walk, one lane per cursor
//   k_ph_score     row -> score, sort key, hit flag (freq >= 1); k_ph_score_f
//                  for the float frequency
//   k_ph_compact   the hits' keys and row indices, packed by the scanned flags
//   k_ph_phrase_of sorted hit -> its phrase, the key of the second (stable) pass
//   k_ph_emit      sorted hit -> (doc, score, freq)
// The two stable radix passes (score/doc, then phrase) order the hits of a row
// chunk by (phrase, score descending, doc ascending).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "phrase_plan.h"
#include "tfidf_internal.h"

namespace tfidf {

constexpr uint32_t kPhScanWaves = 4;   // waves (items) per k_ph_scan workgroup
constexpr uint32_t kPhFreqWaves = 4;   // waves (rows) per k_ph_freq workgroup

// items [i0, i0 + ni) of an item chunk; all / listed: per slice counts (count
// pass) or their exclusive scans (fill), indexed by item * kHlLanes + lane over
// the whole item chunk; first[row] = the row's first item; m_base = the first
// listed token the arrays hold
template <bool FILL>
__global__ void __launch_bounds__(64 * kPhScanWaves) k_ph_scan(
    const uint8_t *__restrict__ text, const uint64_t *__restrict__ ext, const HlItem *__restrict__ items, uint32_t i0,
    uint32_t ni, const HlKey *__restrict__ keys, const uint32_t *__restrict__ key_off,
    const uint32_t *__restrict__ row_q, uint64_t seed, const uint64_t *__restrict__ first, uint64_t *__restrict__ all,
    uint64_t *__restrict__ listed, uint64_t m_base, uint32_t *__restrict__ o_pos, uint32_t *__restrict__ o_ord) {
  const uint32_t rel = blockIdx.x * kPhScanWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (rel >= ni) return;
  const uint32_t item = i0 + rel;
  const HlItem it = items[item];
  const HlKey *seg;
  uint32_t n_keys;
  hl_segment(keys, key_off, row_q[it.row], &seg, &n_keys);
  const uint64_t d0 = ext[2 * (uint64_t)it.row], L = ext[2 * (uint64_t)it.row + 1] - d0;
  const uint8_t *doc = text + d0;
  uint64_t cs, ce, pos, stop;
  hl_chunk(doc, L, it.chunk, &cs, &ce);
  hl_slice(doc, cs, ce, lane, &pos, &stop);
  const uint64_t at = (uint64_t)item * kHlLanes + lane;
  uint32_t n_all = 0;
  if (FILL) {
    const uint64_t c0 = listed[at], cn = listed[at + 1] - c0;
    if (cn == 0) return;                           // nothing listed in this slice
    const uint64_t base = c0 - m_base;
    const uint64_t tok0 = all[at] - all[first[it.row] * kHlLanes];
    ph_scan_slice(doc, L, pos, stop, seg, n_keys, seed, &n_all, [&](uint32_t i, uint32_t k, uint32_t o) {
      if (i < cn) {
        o_pos[base + i] = (uint32_t)(tok0 + k);
        o_ord[base + i] = o;
      }
    });
  } else {
    listed[at] = ph_scan_slice(doc, L, pos, stop, seg, n_keys, seed, &n_all, [](uint32_t, uint32_t, uint32_t) {});
    all[at] = n_all;
  }
}

// rows [0, n): row_off[r] - m_base = the row's first listed token in pos / ord
__global__ void __launch_bounds__(64 * kPhFreqWaves) k_ph_freq(
    const uint64_t *__restrict__ row_off, uint64_t m_base, const uint32_t *__restrict__ pos,
    const uint32_t *__restrict__ ord, const uint32_t *__restrict__ row_q, const uint32_t *__restrict__ seq,
    const uint32_t *__restrict__ seq_off, uint64_t n, uint32_t *__restrict__ freq) {
  const uint64_t row = (uint64_t)blockIdx.x * kPhFreqWaves + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (row >= n) return;
  const uint64_t m0 = row_off[row] - m_base, cnt = row_off[row + 1] - row_off[row];
  const uint32_t q = row_q[row];
  const uint32_t *sq = seq + seq_off[q];
  const uint32_t m = seq_off[q + 1] - seq_off[q];
  uint32_t mine = 0;
  for (uint64_t i = lane; i < cnt; i += 64) mine += ph_match_at(pos + m0, ord + m0, cnt, i, sq, m) ? 1u : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d, 64);
  if (lane == 0) freq[row] = mine;
}

// --- sloppy phrases: the float frequency of SloppyPhraseMatcher (phrase_plan.h) ---

__device__ __forceinline__ uint64_t ph_uniform(uint64_t v) {   // a value every lane holds, as a scalar
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v),
                 hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ uint64_t ph_wave_min(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    v = o < v ? o : v;
  }
  return ph_uniform(v);
}

// the first of a row's n list entries at or after from whose ordinal is j, n
// when there is none: 64 entries per ballot (from, j wave-uniform)
__device__ __forceinline__ uint64_t ph_wave_next(const uint32_t *__restrict__ ord, uint64_t n, uint32_t j,
                                                 uint64_t from, uint32_t lane) {
  for (; from < n; from += 64) {
    const uint64_t i = from + lane;
    const uint64_t b = __ballot(i < n && ord[i] == j);
    if (b) return from + (uint64_t)(__ffsll((long long)b) - 1);
  }
  return n;
}

// rows [0, n) as k_ph_freq takes them, freq as a float.  A row whose phrase has
// slop 0 or one term counts ph_match_at starts (the exact rule).  Any other row
// (2 <= m <= 64 distinct terms, checked on the host) walks ph_sloppy_freq's
// steps with lane j holding cursor j: the queue is the lanes' keys, pop-min and
// top are wave minima with the popped lane masked out, end / next / matchLength
// / freq are wave-uniform, and a cursor advances by a ballot over the 64 list
// entries after it.
__global__ void __launch_bounds__(64 * kPhFreqWaves) k_ph_sloppy_freq(
    const uint64_t *__restrict__ row_off, uint64_t m_base, const uint32_t *__restrict__ pos,
    const uint32_t *__restrict__ ord, const uint32_t *__restrict__ row_q, const uint32_t *__restrict__ seq,
    const uint32_t *__restrict__ seq_off, const uint32_t *__restrict__ slop, uint64_t n, float *__restrict__ freq) {
  const uint64_t row = (uint64_t)blockIdx.x * kPhFreqWaves + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (row >= n) return;
  const uint64_t m0 = row_off[row] - m_base, cnt = row_off[row + 1] - row_off[row];
  const uint32_t q = row_q[row];
  const uint32_t m = seq_off[q + 1] - seq_off[q];
  const uint32_t *rp = pos + m0, *ro = ord + m0;
  if (slop[q] == 0 || m < 2) {
    const uint32_t *sq = seq + seq_off[q];
    uint32_t mine = 0;
    for (uint64_t i = lane; i < cnt; i += 64) mine += ph_match_at(rp, ro, cnt, i, sq, m) ? 1u : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d, 64);
    if (lane == 0) freq[row] = (float)mine;
    return;
  }
  if (m > kPhMaxSloppyTerms) {                       // never launched: the host refuses the phrase
    if (lane == 0) freq[row] = 0.0f;
    return;
  }
  const int64_t max_len = ph_slop(slop[q]);
  const bool live = lane < m;
  uint64_t at = cnt;
  for (uint32_t j = 0; j < m; j++) {
    const uint64_t f = ph_wave_next(ro, cnt, j, 0, lane);
    if (lane == j) at = f;
  }
  if (__ballot(live && at == cnt)) {                 // a term without a listed token: no match
    if (lane == 0) freq[row] = 0.0f;
    return;
  }
  uint64_t key = live ? ph_cursor_key((int64_t)rp[at] - lane, lane) : ~0ull;
  int64_t end = ph_key_position(~ph_wave_min(live ? ~key : ~0ull));   // the greatest live key holds the greatest position
  uint64_t top = ph_wave_min(key);
  uint32_t pp = (uint32_t)(top & 0xFFu);
  int64_t next = ph_key_position(ph_wave_min(lane == pp ? ~0ull : key));
  int64_t match_length = end - ph_key_position(top);
  float f = 0.0f;
  for (;;) {
    const uint64_t cur = ph_uniform((uint64_t)__shfl((unsigned long long)at, (int)pp, 64));
    const uint64_t nx = ph_wave_next(ro, cnt, pp, cur + 1, lane);
    if (nx == cnt) break;
    const int64_t p = (int64_t)rp[nx] - pp;
    if (lane == pp) {
      at = nx;
      key = ph_cursor_key(p, pp);
    }
    if (p > end) end = p;
    if (p > next) {
      if (match_length <= max_len) f = ph_sloppy_add(f, match_length);
      top = ph_wave_min(key);
      pp = (uint32_t)(top & 0xFFu);
      next = ph_key_position(ph_wave_min(lane == pp ? ~0ull : key));
      match_length = end - ph_key_position(top);
    } else {
      const int64_t l = end - p;
      if (l < match_length) match_length = l;
    }
  }
  if (match_length <= max_len) f = ph_sloppy_add(f, match_length);
  if (lane == 0) freq[row] = f;
}

// k_ph_score for a float frequency.  The frequency is never negative, so a row
// is a hit when its 32-bit word is not 0: k_ph_compact and k_ph_emit carry
// that word as they carry a count.
__global__ void __launch_bounds__(256) k_ph_score_f(const float *__restrict__ freq, const uint32_t *__restrict__ docs,
                                                    const uint32_t *__restrict__ row_q, const float *__restrict__ w,
                                                    const float *__restrict__ cache, const uint8_t *__restrict__ norm,
                                                    uint64_t n, uint64_t *__restrict__ key,
                                                    uint64_t *__restrict__ flag) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float f = freq[r];
  const uint32_t d = docs[r];
  const float sc = f > 0.0f ? ph_score_f(w[row_q[r]], f, cache[norm[d]]) : 0.0f;
  key[r] = ph_sort_key(__float_as_uint(sc), d);
  flag[r] = f > 0.0f ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_ph_score(const uint32_t *__restrict__ freq, const uint32_t *__restrict__ docs,
                                                  const uint32_t *__restrict__ row_q, const float *__restrict__ w,
                                                  const float *__restrict__ cache, const uint8_t *__restrict__ norm,
                                                  uint64_t n, uint64_t *__restrict__ key, uint64_t *__restrict__ flag) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const uint32_t f = freq[r], d = docs[r];
  const float sc = f ? ph_score(w[row_q[r]], f, cache[norm[d]]) : 0.0f;
  key[r] = ph_sort_key(__float_as_uint(sc), d);
  flag[r] = f ? 1u : 0u;
}

// at: the exclusive scan of the flags (n + 1 entries)
__global__ void __launch_bounds__(256) k_ph_compact(const uint64_t *__restrict__ key, const uint32_t *__restrict__ freq,
                                                    const uint64_t *__restrict__ at, uint64_t n,
                                                    uint64_t *__restrict__ o_key, uint32_t *__restrict__ o_row) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n || !freq[r]) return;
  o_key[at[r]] = key[r];
  o_row[at[r]] = (uint32_t)r;
}

__global__ void __launch_bounds__(256) k_ph_phrase_of(const uint32_t *__restrict__ rows,
                                                      const uint32_t *__restrict__ row_q, uint32_t q0, uint64_t n,
                                                      uint32_t *__restrict__ o_q) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) o_q[i] = row_q[rows[i]] - q0;
}

__global__ void __launch_bounds__(256) k_ph_emit(const uint32_t *__restrict__ rows, const uint64_t *__restrict__ key,
                                                 const uint32_t *__restrict__ freq, uint64_t n,
                                                 uint32_t *__restrict__ o_doc, float *__restrict__ o_score,
                                                 uint32_t *__restrict__ o_freq) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = rows[i];
  const uint64_t k = key[r];
  o_doc[i] = ph_key_doc(k);
  o_score[i] = __uint_as_float(ph_key_score_bits(k));
  o_freq[i] = freq[r];
}

// --- launch wrappers (tfidf_capi.hip) ---
static unsigned ph_grid(uint64_t n, uint32_t per) { return (unsigned)((n + per - 1) / per); }

hipError_t launch_ph_scan(bool fill, const uint8_t *text, const uint64_t *ext, const HlItem *items, uint32_t i0,
                          uint32_t ni, const HlKey *keys, const uint32_t *key_off, const uint32_t *row_q,
                          uint64_t seed, const uint64_t *first, uint64_t *all, uint64_t *listed, uint64_t m_base,
                          uint32_t *o_pos, uint32_t *o_ord, hipStream_t s) {
  if (ni == 0) return hipSuccess;
  const dim3 grid(ph_grid(ni, kPhScanWaves)), block(64 * kPhScanWaves);
  if (fill)
    hipLaunchKernelGGL(k_ph_scan<true>, grid, block, 0, s, text, ext, items, i0, ni, keys, key_off, row_q, seed, first,
                       all, listed, m_base, o_pos, o_ord);
  else
    hipLaunchKernelGGL(k_ph_scan<false>, grid, block, 0, s, text, ext, items, i0, ni, keys, key_off, row_q, seed,
                       first, all, listed, m_base, o_pos, o_ord);
  return hipGetLastError();
}

hipError_t launch_ph_freq(const uint64_t *row_off, uint64_t m_base, const uint32_t *pos, const uint32_t *ord,
                          const uint32_t *row_q, const uint32_t *seq, const uint32_t *seq_off, uint64_t n,
                          uint32_t *freq, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ph_freq, dim3(ph_grid(n, kPhFreqWaves)), dim3(64 * kPhFreqWaves), 0, s, row_off, m_base, pos,
                     ord, row_q, seq, seq_off, n, freq);
  return hipGetLastError();
}

hipError_t launch_ph_sloppy_freq(const uint64_t *row_off, uint64_t m_base, const uint32_t *pos, const uint32_t *ord,
                                 const uint32_t *row_q, const uint32_t *seq, const uint32_t *seq_off,
                                 const uint32_t *slop, uint64_t n, float *freq, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ph_sloppy_freq, dim3(ph_grid(n, kPhFreqWaves)), dim3(64 * kPhFreqWaves), 0, s, row_off, m_base,
                     pos, ord, row_q, seq, seq_off, slop, n, freq);
  return hipGetLastError();
}

hipError_t launch_ph_score_f(const float *freq, const uint32_t *docs, const uint32_t *row_q, const float *w,
                             const float *cache, const uint8_t *norm, uint64_t n, uint64_t *key, uint64_t *flag,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ph_score_f, dim3(ph_grid(n, 256)), dim3(256), 0, s, freq, docs, row_q, w, cache, norm, n, key,
                     flag);
  return hipGetLastError();
}

hipError_t launch_ph_score(const uint32_t *freq, const uint32_t *docs, const uint32_t *row_q, const float *w,
                           const float *cache, const uint8_t *norm, uint64_t n, uint64_t *key, uint64_t *flag,
                           hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ph_score, dim3(ph_grid(n, 256)), dim3(256), 0, s, freq, docs, row_q, w, cache, norm, n, key,
                     flag);
  return hipGetLastError();
}

hipError_t launch_ph_compact(const uint64_t *key, const uint32_t *freq, const uint64_t *at, uint64_t n,
                             uint64_t *o_key, uint32_t *o_row, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ph_compact, dim3(ph_grid(n, 256)), dim3(256), 0, s, key, freq, at, n, o_key, o_row);
  return hipGetLastError();
}

// tmp == nullptr: *tmp_bytes = the scratch either pass over n hits needs
hipError_t ph_sort_bytes(size_t *tmp_bytes, uint32_t n) {
  size_t a = 0, b = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, 64,
                                                    (hipStream_t) nullptr);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                         (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, 32,
                                         (hipStream_t) nullptr);
  *tmp_bytes = a > b ? a : b;
  return e;
}

// The n hits (key_in, row_in) of phrases [q0, q0 + n_q) ordered by (phrase, key):
// a stable pass over the 64-bit key, then (n_q > 1) a stable pass over the
// phrase.  The ordered rows end in row_a (n_q == 1) or row_in (n_q > 1):
// returned in *rows_out.  key_a, row_a, q_a, q_b: n entries each.
hipError_t ph_sort(void *tmp, size_t tmp_bytes, const uint64_t *key_in, uint64_t *key_a, uint32_t *row_in,
                   uint32_t *row_a, uint32_t *q_a, uint32_t *q_b, const uint32_t *row_q, uint32_t q0, uint32_t n_q,
                   uint32_t n, const uint32_t **rows_out, hipStream_t s) {
  *rows_out = row_a;
  if (n == 0) return hipSuccess;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, key_in, key_a, (const uint32_t *)row_in, row_a,
                                                    (int)n, 0, 64, s);
  if (e != hipSuccess || n_q <= 1) return e;
  hipLaunchKernelGGL(k_ph_phrase_of, dim3(ph_grid(n, 256)), dim3(256), 0, s, row_a, row_q, q0, (uint64_t)n, q_a);
  int bits = 1;
  while (bits < 32 && (1u << bits) < n_q) bits++;
  e = hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const uint32_t *)q_a, q_b, (const uint32_t *)row_a, row_in,
                                         (int)n, 0, bits, s);
  *rows_out = row_in;
  return e;
}

hipError_t launch_ph_emit(const uint32_t *rows, const uint64_t *key, const uint32_t *freq, uint64_t n, uint32_t *o_doc,
                          float *o_score, uint32_t *o_freq, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ph_emit, dim3(ph_grid(n, 256)), dim3(256), 0, s, rows, key, freq, n, o_doc, o_score, o_freq);
  return hipGetLastError();
}

}  // namespace tfidf
