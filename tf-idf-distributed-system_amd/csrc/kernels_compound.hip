// kernels_compound.hip — compound queries (tfidf_search_compound*): the Boolean
// combination of many queries' clause rows on the device.  The match rule, the
// score and the merge key are the shared functions of compound_plan.h.
//
// A chunk's clause rows arrive flattened, clause after clause, as (doc, score
// bits) entries in whatever order their routes gave them.
//
//   k_cq_bin<false>  counts the entries per (clause, 8192-document block) bin:
//                    one lane per entry, the lane finds its clause by binary
//                    search in the row offsets
//   (exclusive_scan_u64 turns the counts into bin starts)
//   k_cq_bin<true>   scatters every entry into its bin; the bin's start is the
//                    cursor (one atomic per entry), so after the pass it is the
//                    bin's end and the bin before it ends where this one starts.
//                    The order inside a bin is free
//   k_cq_combine     one workgroup per (query, block).  A pair none of whose
//                    clauses has an entry in the block, or one of whose MUST /
//                    FILTER clauses has none, leaves an empty run.  Otherwise
//                    the block is taken as four tiles of 2048 documents, one
//                    after the other: per tile the state of every document
//                    (MUST + FILTER presence count, veto and SHOULD bits, the
//                    two double sums: 18 bytes, 36 KiB) lives in LDS, and the
//                    query's clauses update it in clause order with a barrier
//                    between clauses.  A document occurs once in a row, so an
//                    entry owns its slot: no atomics, and the sums run in clause
//                    order by construction.  The survivors of a tile are
//                    appended to the pair's run as merge keys; after the last
//                    tile the run (at most 8192 keys, 64 KiB: the same LDS) is
//                    sorted descending and written back.
//
//   k_cqn_combine    the nested calls' combine (tfidf_search_nested*): the same
//                    pairs, bins and runs, a stack of per-document group states
//                    in place of the one state; described at the kernel
//
// The runs have the layout k_score_blocks leaves for k = 0 (run q * R2 + b,
// kBlockDocs keys apart, hits_n per run), so launch_hits_order_batch orders each
// query's runs.  Every index read from an entry is checked before use: the doc
// against n_docs where the entry is binned, the tile slot against the tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compound_plan.h"
#include "compound_tree_plan.h"
#include "tfidf_internal.h"

namespace tfidf {

static_assert(kCqBlockDocs == kBlockDocs, "a bin is a doc block of the scorer");

constexpr uint32_t kCqBinThreads = 256;
constexpr uint32_t kCqThreads = 512;                          // k_cq_combine
constexpr uint32_t kCqPerThread = kCqTileDocs / kCqThreads;   // documents a thread evaluates per tile
static_assert(kCqTileDocs % kCqThreads == 0, "whole documents per thread");
constexpr uint32_t kCqLdsBytes = kCqBlockDocs * 8;            // the sort's keys; the tile state (36 KiB) aliases them
static_assert(kCqTileDocs * 18 <= kCqLdsBytes, "the tile state fits the sort buffer");

template <bool FILL>
__global__ void __launch_bounds__(kCqBinThreads) k_cq_bin(const CqPass p) {
  const uint64_t stride = (uint64_t)gridDim.x * kCqBinThreads;
  const uint64_t n_bins = (uint64_t)p.n_c * p.n_blocks;
  for (uint64_t e = (uint64_t)blockIdx.x * kCqBinThreads + threadIdx.x; e < p.n_e; e += stride) {
    const uint2 ent = p.rows[e];
    if (ent.x >= p.n_docs) continue;                          // no such document: the entry is dropped in both passes
    const uint32_t c = cq_clause_of(p.c_off, p.n_c, e);
    const uint64_t bin = cq_bin(c, ent.x, p.n_blocks);
    if (bin >= n_bins) continue;
    if (!FILL) {
      atomicAdd(reinterpret_cast<unsigned long long *>(p.bin_cnt + bin), 1ull);
    } else {
      const uint64_t at = atomicAdd(reinterpret_cast<unsigned long long *>(p.bin_off + bin), 1ull);
      if (at < p.n_e) p.binned[at] = ent;
    }
  }
}

__device__ __forceinline__ uint32_t cq_block_excl_scan(uint32_t v, uint32_t *sh, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = kCqThreads >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  __syncthreads();                                            // the last scan's reads of sh are done
  if (lane == 63) sh[wid] = x;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (uint32_t w = 0; w < nw; w++) {
    const uint32_t s = sh[w];
    if (w < wid) base += s;
    tot += s;
  }
  *total = tot;
  return base + x - v;
}

// a run's nhit <= kBlockDocs keys, sorted descending in LDS (bitonic, as k_score_blocks sorts a block's hits)
__device__ __forceinline__ void cq_sort_run(uint64_t *keys, uint64_t *out, uint32_t nhit) {
  const uint32_t tid = threadIdx.x;
  if (nhit <= 1) return;
  uint32_t P = 2;
  while (P < nhit) P <<= 1;
  for (uint32_t i = tid; i < P; i += kCqThreads) keys[i] = i < nhit ? out[i] : 0ull;
  __syncthreads();
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = tid; i < P / 2; i += kCqThreads) {
        const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const uint64_t a = keys[lo], c = keys[hi];
        if ((lo & size) == 0 ? a < c : a > c) { keys[lo] = c; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < nhit; i += kCqThreads) out[i] = keys[i];
}

__global__ void __launch_bounds__(kCqThreads) k_cq_combine(const CqPass p) {
  extern __shared__ __align__(16) uint8_t cq_lds[];
  __shared__ uint32_t sh_scan[kCqThreads / 64];
  __shared__ uint64_t sh_lo[kCqMaxClausesPerQuery], sh_hi[kCqMaxClausesPerQuery];
  __shared__ uint32_t sh_occ[kCqMaxClausesPerQuery];
  __shared__ uint32_t sh_any, sh_req_empty;
  double *must = reinterpret_cast<double *>(cq_lds);
  double *shd = must + kCqTileDocs;
  uint8_t *req = reinterpret_cast<uint8_t *>(shd + kCqTileDocs);
  uint8_t *flags = req + kCqTileDocs;
  uint64_t *keys = reinterpret_cast<uint64_t *>(cq_lds);

  const uint32_t tid = threadIdx.x, q = blockIdx.x / p.n_blocks, b = blockIdx.x - q * p.n_blocks;
  const uint32_t run = q * p.R2 + b;
  const uint32_t c0 = p.q_coff[q];
  uint32_t nc = p.q_coff[q + 1] - c0;
  if (nc > kCqMaxClausesPerQuery) nc = kCqMaxClausesPerQuery;  // validated by the host; the LDS tables hold no more
  if (tid == 0) { sh_any = 0; sh_req_empty = 0; }
  __syncthreads();
  const uint64_t n_bins = (uint64_t)p.n_c * p.n_blocks;
  if (tid < nc) {
    const uint64_t bin = cq_bin(c0 + tid, b * kCqBlockDocs, p.n_blocks);
    uint64_t lo = 0, hi = 0;
    if (bin < n_bins) {
      lo = bin ? p.bin_off[bin - 1] : 0ull;                   // after the scatter bin_off[i] is bin i's end
      hi = p.bin_off[bin];
      if (hi > p.n_e) hi = p.n_e;
      if (lo > hi) lo = hi;
    }
    const uint32_t occ = p.c_occur[c0 + tid];
    sh_lo[tid] = lo;
    sh_hi[tid] = hi;
    sh_occ[tid] = occ;
    if (hi > lo) atomicOr(&sh_any, 1u);
    else if (occ == TFIDF_OCCUR_MUST || occ == TFIDF_OCCUR_FILTER) atomicOr(&sh_req_empty, 1u);
  }
  __syncthreads();
  if (!sh_any || sh_req_empty) {
    if (tid == 0) p.hits_n[run] = 0;
    return;
  }
  CqNeeds needs{0, 0};
  for (uint32_t c = 0; c < nc; c++) cq_needs_add(&needs, sh_occ[c]);

  uint64_t *out = p.hits + (size_t)run * kBlockDocs;
  uint32_t nhit = 0;
  for (uint32_t t = 0; t < kCqBlockDocs / kCqTileDocs; t++) {
    const uint32_t d0 = b * kCqBlockDocs + t * kCqTileDocs;
    if (d0 >= p.n_docs) break;
    for (uint32_t i = tid; i < kCqTileDocs; i += kCqThreads) {
      must[i] = 0.0;
      shd[i] = 0.0;
      req[i] = 0;
      flags[i] = 0;
    }
    __syncthreads();
    for (uint32_t c = 0; c < nc; c++) {
      const uint32_t occ = sh_occ[c];
      const uint64_t hi = sh_hi[c];
      for (uint64_t i = sh_lo[c] + tid; i < hi; i += kCqThreads) {
        const uint2 ent = p.binned[i];
        const uint32_t ld = ent.x - d0;                        // unsigned: a document before the tile wraps past it
        if (ld < kCqTileDocs) cq_apply(occ, __uint_as_float(ent.y), &req[ld], &flags[ld], &must[ld], &shd[ld]);
      }
      __syncthreads();                                         // clause order: the next clause sees this one's sums
    }
    uint64_t kv[kCqPerThread];
    uint32_t n = 0;
#pragma unroll
    for (uint32_t i = 0; i < kCqPerThread; i++) {
      const uint32_t ld = tid * kCqPerThread + i;
      const uint32_t doc = d0 + ld;
      if (doc < p.n_docs && cq_match(needs, req[ld], flags[ld]))
        kv[n++] = cq_hit_key(cq_score(needs, flags[ld], must[ld], shd[ld]), doc);
    }
    uint32_t tot;
    uint32_t at = nhit + cq_block_excl_scan(n, sh_scan, &tot);
    for (uint32_t i = 0; i < n; i++)
      if (at < kBlockDocs) out[at++] = kv[i];
    nhit += tot;
    __syncthreads();                                           // the state is read; the next tile clears it
  }
  if (nhit > kBlockDocs) nhit = kBlockDocs;
  cq_sort_run(keys, out, nhit);
  if (tid == 0) p.hits_n[run] = nhit;
}

// Nested queries: the chunk's "clauses" are the nodes of its queries' trees, a
// group's row empty.  One workgroup per (query, block), as k_cq_combine; per tile
// a stack of per-document group states, one level per open group, and the
// query's nodes walked in pre-order (cqn_next) with a barrier after every step:
// opening a group clears its level, a leaf applies its bin's entries to its
// parent's level, closing a group evaluates its level (cqn_match, cq_score) and
// applies the result to the level below as one child, closing the root packs the
// survivors.  An entry owns its document's slot, and a lane that closes a group
// owns that document's slot on both levels: no atomics, sums in child order.
// The tile follows the chunk's deepest query (cqn_tile_docs), so the levels take
// the 38 912 bytes of the flat pass's single level and alias the sort's 64 KiB.
constexpr uint32_t kCqnMaxPerThread = 2048 / kCqThreads;      // documents a thread closes per tile, at the largest tile
static_assert(kCqnMinTileDocs % kCqThreads == 0, "whole documents per thread at every tile size");
static_assert(kCqnMaxDepth * kCqnMinTileDocs * kCqnStateBytes <= kCqLdsBytes, "the levels fit the sort buffer");

__global__ void __launch_bounds__(kCqThreads) k_cqn_combine(const CqPass p) {
  extern __shared__ __align__(16) uint8_t cq_lds[];
  __shared__ uint32_t sh_scan[kCqThreads / 64];
  __shared__ uint64_t sh_lo[kCqnMaxNodes], sh_hi[kCqnMaxNodes];
  __shared__ CqnNode sh_nd[kCqnMaxNodes];
  __shared__ CqNeeds sh_needs[kCqnMaxNodes];
  __shared__ uint8_t sh_live[kCqnMaxNodes], sh_bad[kCqnMaxNodes], sh_can[kCqnMaxNodes];
  __shared__ uint32_t sh_go;
  uint32_t levels = p.levels;                                  // chosen by the host; the LDS holds no more
  if (levels < 1) levels = 1;
  if (levels > kCqnMaxDepth) levels = kCqnMaxDepth;
  const uint32_t tile = cqn_tile_docs(levels), per = tile / kCqThreads;
  double *must = reinterpret_cast<double *>(cq_lds);           // [levels][tile] each
  double *shd = must + levels * tile;
  uint8_t *req = reinterpret_cast<uint8_t *>(shd + levels * tile);
  uint8_t *nsh = req + levels * tile;
  uint8_t *flags = nsh + levels * tile;
  uint64_t *keys = reinterpret_cast<uint64_t *>(cq_lds);

  const uint32_t tid = threadIdx.x, q = blockIdx.x / p.n_blocks, b = blockIdx.x - q * p.n_blocks;
  const uint32_t run = q * p.R2 + b;
  const uint32_t c0 = p.q_coff[q];
  uint32_t nc = p.q_coff[q + 1] - c0;
  if (nc > kCqnMaxNodes) nc = kCqnMaxNodes;                    // validated by the host; the LDS tables hold no more
  const uint64_t n_bins = (uint64_t)p.n_c * p.n_blocks;
  if (tid < nc) {
    const uint64_t bin = cq_bin(c0 + tid, b * kCqBlockDocs, p.n_blocks);
    uint64_t lo = 0, hi = 0;
    if (bin < n_bins) {
      lo = bin ? p.bin_off[bin - 1] : 0ull;                   // after the scatter bin_off[i] is bin i's end
      hi = p.bin_off[bin];
      if (hi > p.n_e) hi = p.n_e;
      if (lo > hi) lo = hi;
    }
    const uint32_t occ = p.c_occur[c0 + tid];
    sh_lo[tid] = lo;
    sh_hi[tid] = hi;
    sh_nd[tid] = CqnNode{p.c_parent[c0 + tid], p.c_msm[c0 + tid], (uint8_t)(occ & 0xFF), (uint8_t)(occ >> 8 & 1)};
    sh_live[tid] = hi > lo;
  }
  __syncthreads();
  if (tid == 0) {
    cqn_count_children(sh_nd, nc, sh_needs);
    sh_go = cqn_feasible(sh_nd, sh_needs, nc, sh_live, sh_bad, sh_can);
  }
  __syncthreads();
  if (!sh_go) {                                                // the root can match nothing in this block
    if (tid == 0) p.hits_n[run] = 0;
    return;
  }

  uint64_t *out = p.hits + (size_t)run * kBlockDocs;
  uint32_t nhit = 0;
  for (uint32_t t = 0; t < kCqBlockDocs / tile; t++) {
    const uint32_t d0 = b * kCqBlockDocs + t * tile;
    if (d0 >= p.n_docs) break;
    uint64_t kv[kCqnMaxPerThread];
    uint32_t n = 0;
    CqnWalk w;
    for (;;) {
      uint32_t node = 0, level = 0;
      const int ev = cqn_next(&w, sh_nd, nc, &node, &level);
      if (ev == kCqnEnd || level >= levels || node >= nc) break;   // the same on every lane: the tables are shared
      const uint32_t base = level * tile;
      if (ev == kCqnOpen) {
        for (uint32_t i = tid; i < tile; i += kCqThreads) {
          must[base + i] = 0.0;
          shd[base + i] = 0.0;
          req[base + i] = 0;
          nsh[base + i] = 0;
          flags[base + i] = 0;
        }
      } else if (ev == kCqnLeaf) {
        const uint32_t occ = sh_nd[node].occur;
        const uint64_t hi = sh_hi[node];
        for (uint64_t i = sh_lo[node] + tid; i < hi; i += kCqThreads) {
          const uint2 ent = p.binned[i];
          const uint32_t ld = ent.x - d0;                      // unsigned: a document before the tile wraps past it
          if (ld < tile)
            cqn_apply(occ, __uint_as_float(ent.y), &req[base + ld], &nsh[base + ld], &flags[base + ld],
                      &must[base + ld], &shd[base + ld]);
        }
      } else {
        const CqNeeds needs = sh_needs[node];
        const uint32_t msm = sh_nd[node].min_should, occ = sh_nd[node].occur;
#pragma unroll
        for (uint32_t i = 0; i < kCqnMaxPerThread; i++) {
          if (i >= per) break;
          const uint32_t ld = i * kCqThreads + tid, at = base + ld;
          if (!cqn_match(needs, msm, req[at], nsh[at], flags[at])) continue;
          const float score = cq_score(needs, flags[at], must[at], shd[at]);
          if (level == 0) {
            if (d0 + ld < p.n_docs && n < kCqnMaxPerThread) kv[n++] = cq_hit_key(score, d0 + ld);
          } else {
            const uint32_t up = base - tile + ld;              // this document's slot one level down the stack
            cqn_apply(occ, score, &req[up], &nsh[up], &flags[up], &must[up], &shd[up]);
          }
        }
      }
      __syncthreads();                                         // node order: the next step sees this one's state
    }
    uint32_t tot;
    uint32_t at = nhit + cq_block_excl_scan(n, sh_scan, &tot);
    for (uint32_t i = 0; i < n; i++)
      if (at < kBlockDocs) out[at++] = kv[i];
    nhit += tot;
    __syncthreads();
  }
  if (nhit > kBlockDocs) nhit = kBlockDocs;
  cq_sort_run(keys, out, nhit);
  if (tid == 0) p.hits_n[run] = nhit;
}

hipError_t launch_compound_pass(const CqPass &p, int grid, hipStream_t s) {
  const uint64_t n_bins = (uint64_t)p.n_c * p.n_blocks;
  hipError_t e = hipMemsetAsync(p.hits_n, 0, (size_t)p.n_q * p.R2 * 4, s);
  if (e != hipSuccess) return e;
  if (p.n_e == 0 || n_bins == 0) return hipSuccess;           // every run is empty
  e = hipMemsetAsync(p.bin_cnt, 0, (n_bins + 1) * 8, s);
  if (e != hipSuccess) return e;
  const uint64_t want = (p.n_e + kCqBinThreads - 1) / kCqBinThreads;
  const int g = (int)(want < (uint64_t)grid ? want : (uint64_t)grid);
  hipLaunchKernelGGL(k_cq_bin<false>, dim3(g), dim3(kCqBinThreads), 0, s, p);
  e = exclusive_scan_u64(p.bin_cnt, p.bin_off, n_bins, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cq_bin<true>, dim3(g), dim3(kCqBinThreads), 0, s, p);
  static std::atomic<uint64_t> big{0}, big_tree{0};
  if (p.c_parent) {
    allow_dyn_lds((const void *)k_cqn_combine, (int)kCqLdsBytes, big_tree);
    hipLaunchKernelGGL(k_cqn_combine, dim3(p.n_blocks * p.n_q), dim3(kCqThreads), kCqLdsBytes, s, p);
  } else {
    allow_dyn_lds((const void *)k_cq_combine, (int)kCqLdsBytes, big);
    hipLaunchKernelGGL(k_cq_combine, dim3(p.n_blocks * p.n_q), dim3(kCqThreads), kCqLdsBytes, s, p);
  }
  return hipGetLastError();
}

}  // namespace tfidf
