// kernels_fuzzy_search.hip — fuzzy search (tfidf_fuzzy_expand*,
// tfidf_search_fuzzy*): the selection of each input term's expansion from its
// candidates, sorted by (term, boost descending) (k_fz_scan / k_fz_hashed with
// FzScan::search, fz_sort).  The rules are those of fuzzy_search_plan.h.
//
//   k_fzs_select   one wave per input term.  The candidates ahead of the boost
//                  group that straddles position E are taken as they stand
//                  (fzs_straddle).  Of the straddling group the wave keeps the r
//                  smallest by bytes, one per lane in ascending order: it
//                  streams the group 64 candidates at a time, each lane tests
//                  its candidate against the worst entry kept, and the
//                  survivors are inserted one by one (a ballot of "kept entry
//                  is smaller" gives the position, the lanes behind it shift up
//                  by one).  Once the list holds small entries almost nothing
//                  passes the test, so a group of tens of thousands costs about
//                  one comparison per lane and 64 candidates.  At the end the E
//                  or fewer entries, one per lane, are ranked by (boost, bytes):
//                  entries of different boost by their keys alone.  A term with
//                  E or fewer candidates, or a group that ends at E, streams
//                  nothing.  A lane reads a candidate's dictionary entry once
//                  (FzsPacked: an exact key's two words in registers, a hashed
//                  key's reference occurrence as offset and length); entries
//                  travel between lanes by shuffles, so the serial insertions
//                  and ranking rounds load nothing for exact keys, and hashed
//                  keys are read from the corpus, lower-cased on the way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dict_device.h"
#include "fuzzy_search_plan.h"
#include "tfidf_internal.h"

namespace tfidf {

constexpr uint32_t kFzsWaves = 4;            // waves (input terms) per workgroup
constexpr uint32_t kFzsText = 1u << 31;      // FzsPacked::n: a hashed key, a = offset in the corpus, b = byte length
static_assert(kFzsMaxExpansions == 64, "one expansion entry per lane of a wave64");

// a candidate in registers: an exact key's bytes (a, b) or a hashed key's reference occurrence, and its code points
struct FzsPacked {
  uint64_t a, b;
  uint32_t n;
};

// the candidate in dictionary slot `slot`; no code points where the slot cannot be read
__device__ __forceinline__ FzsPacked fzs_pack(const FzsSelect &q, uint32_t slot) {
  FzsPacked p{0, 0, 0};
  if (slot >= q.C) return p;
  const uint64_t lo = q.dict[slot];
  if (lo == 0) return p;
  FzWordCursor w{0, 0, 0};
  if (fz_key_words(lo, q.dict[(uint64_t)q.C + slot], &w, &p.n)) {
    p.a = w.w0;
    p.b = w.w1;
    return p;
  }
  const uint64_t r = q.dict[2 * (uint64_t)q.C + slot];
  const uint64_t off = dict_ref_off(r);
  const uint32_t len = dict_ref_len(r);
  if (r == 0 || off + len > q.text_bytes) return p;                  // a reference always lies inside the corpus
  p.a = off;
  p.b = len;
  p.n = fz_text_cps(q.text + off, len) | kFzsText;
  return p;
}

__device__ __forceinline__ FzsCand fzs_unpack(const FzsSelect &q, const FzsPacked &p) {
  if (p.n & kFzsText)
    return FzsCand{FzWordCursor{0, 0, 0}, FzTextCursor{q.text + p.a, (uint32_t)p.b, 0}, p.n & ~kFzsText, true};
  return fzs_cand_words(FzWordCursor{p.a, p.b, 0}, p.n);
}

__device__ __forceinline__ int fzs_cmp(const FzsSelect &q, const FzsPacked &x, const FzsPacked &y) {
  return fzs_compare(fzs_unpack(q, x), fzs_unpack(q, y));
}

__device__ __forceinline__ uint64_t fzs_shfl64(uint64_t v, uint32_t src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t fzs_shfl_up64(uint64_t v) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1, 64);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1, 64);
  return ((uint64_t)hi << 32) | lo;
}
// lane src's candidate in every lane / the previous lane's candidate
__device__ __forceinline__ FzsPacked fzs_bcast(const FzsPacked &p, uint32_t src) {
  return FzsPacked{fzs_shfl64(p.a, src), fzs_shfl64(p.b, src), (uint32_t)__shfl((int)p.n, (int)src, 64)};
}
__device__ __forceinline__ FzsPacked fzs_prev(const FzsPacked &p) {
  return FzsPacked{fzs_shfl_up64(p.a), fzs_shfl_up64(p.b), (uint32_t)__shfl_up((int)p.n, 1, 64)};
}

__global__ void __launch_bounds__(kFzsWaves * 64) k_fzs_select(const FzsSelect a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t = blockIdx.x * kFzsWaves + (threadIdx.x >> 6);
  if (t >= a.n_terms) return;                                        // the whole wave
  const uint32_t o = a.seg[t], c = a.seg[t + 1] - o, E = a.E;
  const uint64_t *keys = a.keys + o;
  const uint32_t *slots = a.slots + o;
  const uint32_t n = c < E ? c : E;
  uint32_t g0, g1, r;
  fzs_straddle(keys, c, E, &g0, &g1, &r);                            // the same in every lane

  // the lanes' entries: [0, g0) as they stand
  uint64_t my_key = 0;
  uint32_t my_slot = 0xFFFFFFFFu;
  FzsPacked my{0, 0, 0};
  if (lane < g0 && lane < n) {
    my_key = keys[lane];
    my_slot = slots[lane];
    my = fzs_pack(a, my_slot);
  }

  if (r) {
    // lanes [0, cnt) keep the cnt <= r smallest of the group so far, ascending: slot, distance and the candidate
    uint32_t ks = 0xFFFFFFFFu, kd = 0, cnt = 0;
    FzsPacked kp{0, 0, 0};
    for (uint32_t base = g0; base < g1; base += 64) {
      const uint32_t i = base + lane;
      const bool have = i < g1;
      const uint32_t cs = have ? slots[i] : 0xFFFFFFFFu;
      const uint32_t cd = have ? fzs_key_dist(keys[i]) : 0;
      const FzsPacked cp = fzs_pack(a, cs);                          // 64 dictionary entries at once
      bool surv = have;
      if (cnt == r) {                                                // a full list: only what beats its worst entry
        const FzsPacked worst = fzs_bcast(kp, r - 1);
        if (have) surv = fzs_cmp(a, cp, worst) < 0;
      }
      uint64_t m = __ballot(surv);
      while (m) {
        const uint32_t src = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const uint32_t ns = (uint32_t)__shfl((int)cs, (int)src, 64);
        const uint32_t nd = (uint32_t)__shfl((int)cd, (int)src, 64);
        const FzsPacked np = fzs_bcast(cp, src);
        bool less = false;
        if (lane < cnt) less = fzs_cmp(a, kp, np) < 0;
        const uint32_t pos = (uint32_t)__popcll(__ballot(less));     // the kept entries ascend: the smaller ones are a prefix
        const uint32_t us = (uint32_t)__shfl_up((int)ks, 1, 64), ud = (uint32_t)__shfl_up((int)kd, 1, 64);
        const FzsPacked up = fzs_prev(kp);
        if (pos >= r) continue;                                      // an earlier survivor of this round displaced it
        if (lane > pos) {
          ks = us;
          kd = ud;
          kp = up;
        } else if (lane == pos) {
          ks = ns;
          kd = nd;
          kp = np;
        }
        if (cnt < r) cnt++;
      }
    }
    // the kept entries follow the g0 taken ones (the group holds more than r, so cnt == r)
    const uint32_t from = lane >= g0 ? lane - g0 : 0;
    const uint32_t s2 = (uint32_t)__shfl((int)ks, (int)from, 64), d2 = (uint32_t)__shfl((int)kd, (int)from, 64);
    const FzsPacked p2 = fzs_bcast(kp, from);
    if (lane >= g0 && lane < g0 + cnt && lane < n) {
      my_slot = s2;
      my_key = (fzs_key_group(keys[E - 1]) << 8) | (uint64_t)d2;
      my = p2;
    }
  }

  // selection order: rank of each entry among the n by (boost group, bytes)
  const bool mine = lane < n;
  uint32_t rank = 0;
  for (uint32_t j = 0; j < n; j++) {
    const uint64_t gj = fzs_key_group(fzs_shfl64(my_key, j)), gm = fzs_key_group(my_key);
    const FzsPacked pj = fzs_bcast(my, j);
    if (!mine || j == lane) continue;
    bool before = gj < gm;
    if (gj == gm) {
      const int cmp = fzs_cmp(a, pj, my);
      before = cmp < 0 || (cmp == 0 && j < lane);                    // distinct slots never compare equal
    }
    rank += before ? 1u : 0u;
  }
  if (mine) {                                                        // rank < n <= kFzsMaxExpansions
    a.out_keys[(uint64_t)t * kFzsMaxExpansions + rank] = my_key;
    a.out_slots[(uint64_t)t * kFzsMaxExpansions + rank] = my_slot;
  }
  if (lane == 0) a.out_n[t] = n;
}

hipError_t launch_fzs_select(const FzsSelect &a, hipStream_t s) {
  if (a.n_terms == 0) return hipSuccess;
  if (a.E < 1 || a.E > kFzsMaxExpansions) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fzs_select, dim3((a.n_terms + kFzsWaves - 1) / kFzsWaves), dim3(kFzsWaves * 64), 0, s, a);
  return hipGetLastError();
}

}  // namespace tfidf
