// wave_ops.h — wave-level helpers shared by the index and query kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfidf {

// Lanes of the wave holding the same BITS-bit key (active lanes only): one
// ballot per key bit.  Used to turn same-address LDS atomics (hot terms hit
// one cursor from most lanes of a wave) into one atomic per distinct key.
template <int BITS>
__device__ __forceinline__ uint64_t peer_mask(uint32_t key) {
  uint64_t peers = __ballot(1);
#pragma unroll
  for (int b = 0; b < BITS; b++) {
    const uint64_t m = __ballot((key >> b) & 1u);
    peers &= ((key >> b) & 1u) ? m : ~m;
  }
  return peers;
}

// Wave-aggregated cursor bump: returns the old cursor value + this lane's rank
// among its peers (same result as one atomicAdd(cur + key, 1) per lane).
template <int BITS>
__device__ __forceinline__ uint32_t cursor_bump(uint32_t *cur, uint32_t key, uint32_t lane) {
  const uint64_t peers = peer_mask<BITS>(key);
  const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
  const uint32_t leader = (uint32_t)__builtin_ctzll(peers);
  uint32_t base = 0;
  if (rank == 0) base = atomicAdd(cur + key, (uint32_t)__popcll(peers));
  base = (uint32_t)__shfl((int)base, (int)leader, 64);
  return base + rank;
}

// cursor_bump for lanes with `in` only (the others touch no cursor and get 0):
// for cursors in global memory, where an idle lane's bump of a spare cursor
// would be one more device-wide atomic on a word every workgroup shares.
template <int BITS>
__device__ __forceinline__ uint32_t cursor_bump_if(uint32_t *cur, uint32_t key, bool in, uint32_t lane) {
  const uint64_t peers = peer_mask<BITS>(key) & __ballot(in);
  const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
  const uint32_t leader = in ? (uint32_t)__builtin_ctzll(peers) : lane;
  uint32_t base = 0;
  if (in && rank == 0) base = atomicAdd(cur + key, (uint32_t)__popcll(peers));
  base = (uint32_t)__shfl((int)base, (int)leader, 64);
  return in ? base + rank : 0u;
}

// Wave-aggregated append (the wildcard and regex scans): the lanes with `take` get consecutive positions from one atomicAdd
__device__ __forceinline__ uint32_t wc_wave_pos(uint32_t *cursor, bool take, uint32_t lane) {
  const uint64_t m = __ballot(take);
  if (m == 0) return 0;
  const uint32_t leader = (uint32_t)__builtin_ctzll(m);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(cursor, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, (int)leader, 64);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
}

}  // namespace tfidf
