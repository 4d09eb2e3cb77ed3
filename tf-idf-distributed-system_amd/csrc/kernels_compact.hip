// kernels_compact.hip — tfidf_compact's copy: a segmented gather of the live
// runs of the staged corpus into a new, dense corpus buffer.
//
// The runs (compact_plan.h) tile the destination exactly, ascending in dst.
// One workgroup copies one fixed tile of the destination; a lane owns 16-byte
// destination chunks (16-byte aligned) and writes each with one 16-byte store.
// A chunk inside one run reads its 16 source bytes as two aligned 16-byte
// loads and a byte shift (src - dst is arbitrary); a chunk that crosses a run
// boundary, or the last partial one, is gathered piece by piece (one piece per
// run it touches, each read the same way and masked to its bytes) and padded
// with zeros past the end of the live text.  A byte-by-byte gather there (up
// to 16 dependent one-byte loads in one lane while its wave waits) was the
// kernel's bound at runs of a few kilobytes.  Every offset is 64-bit: a
// shard's text exceeds 4 GiB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compact_plan.h"
#include "tfidf_internal.h"

namespace tfidf {

constexpr uint32_t kCompactThreads = 256;

struct alignas(16) Chunk16 {
  uint64_t lo, hi;
};

// Bytes [s, s + n) of the corpus (1 <= n <= 16) in the low n bytes of the
// result (the rest is unspecified), by aligned 16-byte loads: the second one
// only when the bytes reach into it, so nothing is read beyond the aligned
// block of byte s + n - 1, i.e. less than 16 bytes past s + n.
__device__ __forceinline__ Chunk16 load_bytes(const uint8_t *src, uint64_t s, uint32_t n) {
  const uint32_t a = (uint32_t)s & 15u;
  const Chunk16 *p = reinterpret_cast<const Chunk16 *>(src + (s - a));
  const Chunk16 x = p[0];
  if (a == 0) return x;
  const Chunk16 y = p[a + n > 16u ? 1 : 0];
  uint64_t q0 = x.lo, q1 = x.hi, q2 = y.lo, q3 = y.hi;
  if (a >= 8) { q0 = q1; q1 = q2; q2 = q3; }
  const uint32_t sh = (a & 7u) * 8u;
  Chunk16 out;
  if (sh) {
    out.lo = (q0 >> sh) | (q1 << (64u - sh));
    out.hi = (q1 >> sh) | (q2 << (64u - sh));
  } else {
    out.lo = q0;
    out.hi = q1;
  }
  return out;
}

// the low n bytes of w (1 <= n <= 16), moved up by k bytes (k + n <= 16), zero elsewhere
__device__ __forceinline__ Chunk16 place_bytes(Chunk16 w, uint32_t n, uint32_t k) {
  if (n < 8) { w.lo &= (1ull << (8u * n)) - 1; w.hi = 0; }
  else if (n < 16) w.hi &= (1ull << (8u * (n - 8u))) - 1;
  if (k >= 8) { w.hi = w.lo << (8u * (k - 8u)); w.lo = 0; }
  else if (k) { w.hi = (w.hi << (8u * k)) | (w.lo >> (64u - 8u * k)); w.lo <<= 8u * k; }
  return w;
}

// the last run with dst <= pos, among runs [a, z) (runs[a].dst <= pos)
__device__ __forceinline__ uint64_t run_of(const CompactRun *runs, uint64_t a, uint64_t z, uint64_t pos) {
  while (z - a > 1) {
    const uint64_t m = a + (z - a) / 2;
    if (runs[m].dst <= pos) a = m; else z = m;
  }
  return a;
}

__global__ __launch_bounds__(kCompactThreads) void k_compact_text(const uint8_t *__restrict__ src,
                                                                  uint8_t *__restrict__ dst,
                                                                  const CompactRun *__restrict__ runs, uint64_t n_runs,
                                                                  uint64_t total, uint32_t tile_log2) {
  const uint64_t t0 = (uint64_t)blockIdx.x << tile_log2;
  const uint64_t t1 = min(t0 + (1ull << tile_log2), total);
  // the tile's runs: [r0, r1]
  const uint64_t r0 = run_of(runs, 0, n_runs, t0);
  const uint64_t r1 = run_of(runs, r0, n_runs, t1 - 1);
  for (uint64_t d = t0 + (uint64_t)threadIdx.x * 16; d < t1; d += (uint64_t)kCompactThreads * 16) {
    uint64_t r = run_of(runs, r0, r1 + 1, d);
    CompactRun run = runs[r];
    Chunk16 out;
    if (d + 16 <= run.dst + run.len) {
      // fast path: [s, s + 16) lies in the run; the aligned loads reach less
      // than 16 bytes past the run's end
      out = load_bytes(src, run.src + (d - run.dst), 16);
    } else {
      // slow path: a run boundary or the end of the text inside the chunk;
      // one piece per run, the last run ends at `total`
      out.lo = out.hi = 0;
      const uint64_t end = min(d + 16, total);
      for (uint64_t pos = d; pos < end;) {
        while (pos >= run.dst + run.len) run = runs[++r];   // runs tile [0, total): r + 1 < n_runs here
        const uint32_t n = (uint32_t)(min(end, run.dst + run.len) - pos);
        const Chunk16 w = place_bytes(load_bytes(src, run.src + (pos - run.dst), n), n, (uint32_t)(pos - d));
        out.lo |= w.lo;
        out.hi |= w.hi;
        pos += n;
      }
    }
    *reinterpret_cast<Chunk16 *>(dst + d) = out;
  }
}

uint32_t compact_tile_log2() {
  uint32_t lg = 14;                                        // 16 KiB
  if (const char *e = knob("TFIDF_COMPACT_TILE_LOG2")) {   // tests: tile edges anywhere
    const int v = atoi(e);
    if (v >= 10 && v <= 16) lg = (uint32_t)v;
  }
  return lg;
}

// dst[0 .. round_up(total, 16)) is written; src and dst are 16-byte aligned
// buffers, dst with room for the last chunk.
hipError_t launch_compact_text(const uint8_t *src, uint8_t *dst, const CompactRun *runs, uint64_t n_runs,
                               uint64_t total, hipStream_t s) {
  if (total == 0 || n_runs == 0) return hipSuccess;
  const uint32_t lg = compact_tile_log2();
  const uint64_t tiles = (total + (1ull << lg) - 1) >> lg;
  if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_compact_text, dim3((unsigned)tiles), dim3(kCompactThreads), 0, s, src, dst, runs, n_runs, total,
                     lg);
  return hipGetLastError();
}

}  // namespace tfidf
