// kernels_mlt.hip — more-like-this (tfidf_mlt_terms*, tfidf_more_like_this*):
// the interesting terms of many seed documents, read from the seeds' own
// forward rows of the snapshot (padded CSR, rsplit, tf escapes) and the per-slot
// df.  The filter, the score and the sort key are the shared functions of
// mlt_plan.h; the idf of a df is read from the host-built table, so the device
// evaluates no log and the scores are the host rule's bit for bit.
//
//   k_mlt_extents  per seed: first CSR entry of its row and the row's length
//                  (the lengths are then scanned: exclusive_scan_u64)
//   k_mlt_scan     the flattened entries of a range of seeds, one per lane: the
//                  lane finds its seed by binary search in the scanned offsets
//                  (a 100 000-term row and a 40-term row balance alike),
//                  decodes slot and tf and applies the filters.  <false> counts
//                  the survivors per seed (one atomic per wave when the wave
//                  sits inside one row); <true> appends (key, value) at
//                  positions taken from one wave-aggregated atomic, never past
//                  the capacity the counts gave
//   mlt_sort       (seed, score descending) order of a candidate chunk (hipCUB
//                  radix sort of the packed keys, slot | tf as values)
//   k_mlt_select   per seed: how many of its sorted candidates the host needs:
//                  the first max_terms and every later one that ties with the
//                  max_terms-th on the score
//   k_mlt_gather   those candidates of every seed, packed
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "mlt_plan.h"
#include "tfidf_internal.h"

namespace tfidf {

constexpr uint32_t kMltThreads = 256;

__global__ void __launch_bounds__(256) k_mlt_extents(const uint64_t *__restrict__ offsets,
                                                     const uint32_t *__restrict__ doc_nuniq,
                                                     const uint32_t *__restrict__ seed_doc,
                                                     const uint32_t *__restrict__ seed_staged, uint32_t n,
                                                     uint64_t *__restrict__ row_base, uint64_t *__restrict__ row_len) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  row_base[i] = csr_row_base(offsets, seed_staged[i]);
  row_len[i] = doc_nuniq[seed_doc[i]];
}

template <bool FILL>
__global__ void __launch_bounds__(kMltThreads) k_mlt_scan(const MltScan a) {
  const uint64_t e0 = a.row_off[a.s0], e1 = a.row_off[a.s1];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rs = a.range_shift, esc = csr_esc_value(rs);
  const MltRules rules{a.min_tf, a.min_df, a.max_df, 0};
  // every lane of a wave runs the same trips (the ballots below need them all)
  for (uint64_t b = e0 + (uint64_t)blockIdx.x * kMltThreads; b < e1; b += (uint64_t)gridDim.x * kMltThreads) {
    const uint64_t e = b + threadIdx.x;
    bool keep = false;
    uint32_t seed = 0, slot = 0, tf = 0;
    float score = 0.0f;
    if (e < e1) {
      seed = a.s0 + mlt_seed_of(a.row_off + a.s0, a.s1 - a.s0, e);
      const uint32_t i = (uint32_t)(e - a.row_off[seed]);
      const uint64_t idx = a.row_base[seed] + i;
      if (idx < a.csr_words) {                                        // a row always lies inside the buffer
        const uint32_t w = a.csr[idx];
        const uint32_t r = a.R > 1 ? mlt_range_of(a.rsplit + (uint64_t)a.seed_doc[seed] * a.R, a.R, i) : 0u;
        slot = (r << rs) | csr_local(w, rs);
        tf = csr_tf_field(w, rs);
        if (tf == esc) tf = csr_esc_tf(a.csr_esc, a.n_esc, idx);
        if (slot < a.C) {
          const uint32_t df = a.df[slot];
          keep = mlt_keep(rules, tf, df);
          if (FILL && keep) score = mlt_score(tf, a.idf[df < a.n_docs ? df : a.n_docs]);
        }
      }
    }
    const unsigned long long m = __ballot(keep);
    if (m == 0) continue;
    const int leader = __ffsll((long long)m) - 1;
    const uint32_t n_keep = (uint32_t)__popcll(m);
    if (!FILL) {
      const uint32_t s_first = __shfl(seed, leader);
      if (__all(!keep || seed == s_first)) {
        if ((int)lane == leader) atomicAdd(a.counts + s_first, n_keep);
      } else if (keep) {
        atomicAdd(a.counts + seed, 1u);
      }
    } else {
      uint32_t base = 0;
      if ((int)lane == leader) base = atomicAdd(a.cursor, n_keep);
      base = __shfl(base, leader);
      if (keep) {
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (at < a.cap) {
          a.keys[at] = mlt_key(seed - a.s0, score);
          a.vals[at] = mlt_val(slot, tf);
        }
      }
    }
  }
}

// sorted keys of seed t: [seg[t], seg[t + 1])
__global__ void __launch_bounds__(256) k_mlt_select(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg,
                                                    uint32_t n_seeds, uint32_t max_terms, uint32_t *__restrict__ take) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_seeds) return;
  take[t] = mlt_select(keys + seg[t], seg[t + 1] - seg[t], max_terms);
}

__global__ void __launch_bounds__(256) k_mlt_gather(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ vals,
                                                    const uint32_t *__restrict__ seg, const uint32_t *__restrict__ out_off,
                                                    uint64_t *__restrict__ o_keys, uint64_t *__restrict__ o_vals) {
  const uint32_t t = blockIdx.x;
  const uint32_t src = seg[t], dst = out_off[t], n = out_off[t + 1] - dst;
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    o_keys[dst + i] = keys[src + i];
    o_vals[dst + i] = vals[src + i];
  }
}

// --- launch wrappers (tfidf_capi.hip) ---
hipError_t launch_mlt_extents(const uint64_t *offsets, const uint32_t *doc_nuniq, const uint32_t *seed_doc,
                              const uint32_t *seed_staged, uint32_t n, uint64_t *row_base, uint64_t *row_len,
                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mlt_extents, dim3((n + 255) / 256), dim3(256), 0, s, offsets, doc_nuniq, seed_doc, seed_staged, n,
                     row_base, row_len);
  return hipGetLastError();
}

// n_entries: the flattened entries of seeds [s0, s1) when the host knows them, else an upper bound (grid size only)
hipError_t launch_mlt_scan(bool fill, const MltScan &a, uint64_t n_entries, int max_grid, hipStream_t s) {
  const uint64_t g = (n_entries + kMltThreads - 1) / kMltThreads;
  const dim3 grid((unsigned)(g < 1 ? 1 : (g > (uint64_t)max_grid ? (uint64_t)max_grid : g))), block(kMltThreads);
  if (fill)
    hipLaunchKernelGGL(k_mlt_scan<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(k_mlt_scan<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

// tmp == nullptr: *tmp_bytes = the scratch the sort of n pairs needs
hipError_t mlt_sort(void *tmp, size_t *tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint64_t *vals_in,
                    uint64_t *vals_out, uint32_t n, int end_bit, hipStream_t s) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, end_bit, s);
}

hipError_t launch_mlt_select(const uint64_t *keys, const uint32_t *seg, uint32_t n_seeds, uint32_t max_terms,
                             uint32_t *take, hipStream_t s) {
  if (n_seeds == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mlt_select, dim3((n_seeds + 255) / 256), dim3(256), 0, s, keys, seg, n_seeds, max_terms, take);
  return hipGetLastError();
}

hipError_t launch_mlt_gather(const uint64_t *keys, const uint64_t *vals, const uint32_t *seg, const uint32_t *out_off,
                             uint32_t n_seeds, uint64_t *o_keys, uint64_t *o_vals, hipStream_t s) {
  if (n_seeds == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mlt_gather, dim3(n_seeds), dim3(256), 0, s, keys, vals, seg, out_off, o_keys, o_vals);
  return hipGetLastError();
}

}  // namespace tfidf
