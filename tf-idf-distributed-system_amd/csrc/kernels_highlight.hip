// kernels_highlight.hip — hit highlighting on the device corpus
// (tfidf_matches, tfidf_snippets): re-scan only the requested documents and
// return match offsets and one short passage per document.  The scan, the
// work split and the passage rule are the shared functions of snippet_plan.h.
//
//   k_hl_extents   row -> corpus byte range of its document (one gather)
//   k_hl_scan      one wave per (row, chunk) item of the host's plan, one lane
//                  per slice, against the key segment of the row's query:
//                  <false> counts each slice's matches, <true> writes them at
//                  the slice's offset (counts scanned between the two passes),
//                  so the matches of a row are contiguous and ascending by
//                  start and the fill never exceeds the total the counting
//                  pass reported; the match arrays start at a row chunk's
//                  first match.  A single-query call is a batch of one query.
//   k_hl_row_offsets   row -> its first match (the scanned counts at its first
//                  item), relative to a row chunk's first match
//   k_hl_rank      one wave per row: every lane ranks the candidate windows it
//                  owns, the wave's best gives the byte range [a, b); then the
//                  run of matches inside [a, b)
//   k_hl_gather    one workgroup per row: the snippet bytes, packed
//   k_hl_emit      one workgroup per row: the in-snippet matches, packed,
//                  starts relative to a
// Every offset is 64-bit (a shard's text exceeds 4 GiB).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snippet_plan.h"
#include "tfidf_internal.h"

namespace tfidf {

constexpr uint32_t kHlScanWaves = 4;   // waves (items) per k_hl_scan workgroup

__global__ void __launch_bounds__(256) k_hl_extents(const uint64_t *__restrict__ offsets,
                                                    const uint32_t *__restrict__ staged, uint64_t n,
                                                    uint64_t *__restrict__ ext) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t st = staged[i];
  ext[2 * i] = offsets[st];
  ext[2 * i + 1] = offsets[st + 1];
}

// one wave's item: slice `lane` of chunk it.chunk of row it.row against the
// sorted keys[0, n_keys); the fill writes match i of the slice at
// counts[at] - m_base + i (m_base: the first match of the rows in the match arrays)
template <bool FILL>
__device__ __forceinline__ void hl_scan_item(const uint8_t *__restrict__ text, const uint64_t *__restrict__ ext,
                                             const HlItem it, uint32_t item, uint32_t lane,
                                             const HlKey *__restrict__ keys, uint32_t n_keys, uint64_t seed,
                                             uint64_t *__restrict__ counts, uint64_t m_base,
                                             uint64_t *__restrict__ starts, uint32_t *__restrict__ lens,
                                             uint32_t *__restrict__ ords) {
  const uint64_t d0 = ext[2 * (uint64_t)it.row], L = ext[2 * (uint64_t)it.row + 1] - d0;
  const uint8_t *doc = text + d0;
  uint64_t cs, ce, pos, stop;
  hl_chunk(doc, L, it.chunk, &cs, &ce);
  hl_slice(doc, cs, ce, lane, &pos, &stop);
  const uint64_t at = (uint64_t)item * kHlLanes + lane;
  if (FILL) {
    const uint64_t c0 = counts[at];
    if (counts[at + 1] == c0) return;            // nothing counted in this slice
    const uint64_t base = c0 - m_base;
    hl_scan_slice(doc, L, pos, stop, keys, n_keys, seed, [&](uint32_t i, uint64_t s, uint32_t len, uint32_t o) {
      starts[base + i] = s;
      lens[base + i] = len;
      ords[base + i] = o;
    });
  } else {
    counts[at] = hl_scan_slice(doc, L, pos, stop, keys, n_keys, seed, [](uint32_t, uint64_t, uint32_t, uint32_t) {});
  }
}

// The keys are the segment of the row's query (hl_segment; wave-uniform, so the
// two loads are scalar), and the match arrays hold only the rows from the one
// whose first match is m_base on.
template <bool FILL>
__global__ void __launch_bounds__(64 * kHlScanWaves) k_hl_scan(
    const uint8_t *__restrict__ text, const uint64_t *__restrict__ ext, const HlItem *__restrict__ items,
    uint32_t n_items, const HlKey *__restrict__ keys, const uint32_t *__restrict__ key_off,
    const uint32_t *__restrict__ row_q, uint64_t seed, uint64_t *__restrict__ counts, uint64_t m_base,
    uint64_t *__restrict__ starts, uint32_t *__restrict__ lens, uint32_t *__restrict__ ords) {
  const uint32_t item = blockIdx.x * kHlScanWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (item >= n_items) return;
  const HlItem it = items[item];
  const HlKey *seg;
  uint32_t n_keys;
  hl_segment(keys, key_off, row_q[it.row], &seg, &n_keys);
  hl_scan_item<FILL>(text, ext, it, item, lane, seg, n_keys, seed, counts, m_base, starts, lens, ords);
}

// offsets relative to the first match the arrays hold (base; 0 for the rows of a whole item chunk)
__global__ void __launch_bounds__(256) k_hl_row_offsets(const uint64_t *__restrict__ scanned,
                                                        const uint64_t *__restrict__ first, uint64_t n,
                                                        uint64_t base, uint64_t *__restrict__ row_off) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i <= n) row_off[i] = scanned[first[i] * kHlLanes] - base;
}

__global__ void __launch_bounds__(64) k_hl_rank(const uint8_t *__restrict__ text, const uint64_t *__restrict__ ext,
                                                const uint64_t *__restrict__ row_off,
                                                const uint64_t *__restrict__ starts,
                                                const uint32_t *__restrict__ lens, const uint32_t *__restrict__ ords,
                                                uint32_t W, uint64_t *__restrict__ sn_a, uint64_t *__restrict__ sn_len,
                                                uint64_t *__restrict__ in_first, uint64_t *__restrict__ in_cnt) {
  __shared__ HlCand cand[64];
  __shared__ uint64_t rng[2];
  __shared__ unsigned long long sh_first;
  __shared__ uint32_t sh_cnt;
  const uint64_t row = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const uint64_t d0 = ext[2 * row], L = ext[2 * row + 1] - d0;
  const uint64_t m0 = row_off[row], n = row_off[row + 1] - m0;
  const uint64_t *st = starts + m0;
  const uint32_t *ln = lens + m0, *od = ords + m0;
  HlCand best{0, 0, 0, 0, 0, 0};
  for (uint64_t i = lane; i < n; i += 64) {
    const HlCand c = hl_window(st, ln, od, n, i, W);
    if (hl_better(c, best)) best = c;
  }
  cand[lane] = best;
  if (lane == 0) { sh_first = ~0ull; sh_cnt = 0; }
  __syncthreads();
  if (lane == 0) {
    for (uint32_t l = 1; l < 64; l++)
      if (hl_better(cand[l], best)) best = cand[l];
    uint64_t a, b;
    hl_range(text + d0, L, W, best, &a, &b);
    rng[0] = a;
    rng[1] = b;
    sn_a[row] = a;
    sn_len[row] = b - a;
  }
  __syncthreads();
  // the matches wholly inside [a, b): one run, the matches being sorted and disjoint
  const uint64_t a = rng[0], b = rng[1];
  uint32_t mine = 0;
  uint64_t mfirst = ~0ull;
  for (uint64_t i = lane; i < n; i += 64)
    if (st[i] >= a && st[i] + ln[i] <= b) {
      if (!mine) mfirst = i;
      mine++;
    }
  if (mine) {
    atomicAdd(&sh_cnt, mine);
    atomicMin(&sh_first, (unsigned long long)mfirst);
  }
  __syncthreads();
  if (lane == 0) {
    in_cnt[row] = sh_cnt;
    in_first[row] = sh_cnt ? m0 + sh_first : m0;
  }
}

__global__ void __launch_bounds__(256) k_hl_gather(const uint8_t *__restrict__ text, const uint64_t *__restrict__ ext,
                                                   const uint64_t *__restrict__ sn_a,
                                                   const uint64_t *__restrict__ text_off, uint8_t *__restrict__ out) {
  const uint64_t row = blockIdx.x;
  const uint8_t *src = text + ext[2 * row] + sn_a[row];
  const uint64_t o = text_off[row], len = text_off[row + 1] - o;
  for (uint64_t i = threadIdx.x; i < len; i += 256) out[o + i] = src[i];
}

__global__ void __launch_bounds__(256) k_hl_emit(const uint64_t *__restrict__ starts, const uint32_t *__restrict__ lens,
                                                 const uint32_t *__restrict__ ords, const uint64_t *__restrict__ sn_a,
                                                 const uint64_t *__restrict__ in_first,
                                                 const uint64_t *__restrict__ m_off, uint64_t *__restrict__ o_starts,
                                                 uint32_t *__restrict__ o_lens, uint32_t *__restrict__ o_ords) {
  const uint64_t row = blockIdx.x;
  const uint64_t src = in_first[row], dst = m_off[row], n = m_off[row + 1] - dst, a = sn_a[row];
  for (uint64_t i = threadIdx.x; i < n; i += 256) {
    o_starts[dst + i] = starts[src + i] - a;
    o_lens[dst + i] = lens[src + i];
    o_ords[dst + i] = ords[src + i];
  }
}

// --- launch wrappers (tfidf_capi.hip) ---
static unsigned hl_grid(uint64_t n, uint32_t per) { return (unsigned)((n + per - 1) / per); }

hipError_t launch_hl_extents(const uint64_t *offsets, const uint32_t *staged, uint64_t n, uint64_t *ext,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_hl_extents, dim3(hl_grid(n, 256)), dim3(256), 0, s, offsets, staged, n, ext);
  return hipGetLastError();
}

// fill == false: counts[item * kHlLanes + lane] = matches of the slice;
// fill == true: counts holds their exclusive scan (n_items * kHlLanes + 1 entries).
// items [0, n_items) of a row chunk (rows relative to ext / row_q), m_base the
// first match the arrays hold
hipError_t launch_hl_scan(bool fill, const uint8_t *text, const uint64_t *ext, const HlItem *items, uint32_t n_items,
                          const HlKey *keys, const uint32_t *key_off, const uint32_t *row_q, uint64_t seed,
                          uint64_t *counts, uint64_t m_base, uint64_t *starts, uint32_t *lens, uint32_t *ords,
                          hipStream_t s) {
  if (n_items == 0) return hipSuccess;
  const dim3 grid(hl_grid(n_items, kHlScanWaves)), block(64 * kHlScanWaves);
  if (fill)
    hipLaunchKernelGGL(k_hl_scan<true>, grid, block, 0, s, text, ext, items, n_items, keys, key_off, row_q, seed,
                       counts, m_base, starts, lens, ords);
  else
    hipLaunchKernelGGL(k_hl_scan<false>, grid, block, 0, s, text, ext, items, n_items, keys, key_off, row_q,
                       seed, counts, m_base, starts, lens, ords);
  return hipGetLastError();
}

hipError_t launch_hl_row_offsets(const uint64_t *scanned, const uint64_t *first, uint64_t n, uint64_t base,
                                 uint64_t *row_off, hipStream_t s) {
  hipLaunchKernelGGL(k_hl_row_offsets, dim3(hl_grid(n + 1, 256)), dim3(256), 0, s, scanned, first, n, base, row_off);
  return hipGetLastError();
}

hipError_t launch_hl_rank(const uint8_t *text, const uint64_t *ext, const uint64_t *row_off, const uint64_t *starts,
                          const uint32_t *lens, const uint32_t *ords, uint32_t W, uint64_t n, uint64_t *sn_a,
                          uint64_t *sn_len, uint64_t *in_first, uint64_t *in_cnt, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_hl_rank, dim3((unsigned)n), dim3(64), 0, s, text, ext, row_off, starts, lens, ords, W, sn_a,
                     sn_len, in_first, in_cnt);
  return hipGetLastError();
}

hipError_t launch_hl_pack(const uint8_t *text, const uint64_t *ext, const uint64_t *sn_a, const uint64_t *text_off,
                          uint8_t *out, const uint64_t *starts, const uint32_t *lens, const uint32_t *ords,
                          const uint64_t *in_first, const uint64_t *m_off, uint64_t *o_starts, uint32_t *o_lens,
                          uint32_t *o_ords, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_hl_gather, dim3((unsigned)n), dim3(256), 0, s, text, ext, sn_a, text_off, out);
  hipLaunchKernelGGL(k_hl_emit, dim3((unsigned)n), dim3(256), 0, s, starts, lens, ords, sn_a, in_first, m_off,
                     o_starts, o_lens, o_ords);
  return hipGetLastError();
}

}  // namespace tfidf
