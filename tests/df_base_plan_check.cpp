// The kept df base of an incremental commit (csrc/commit_plan.h df_base_plan,
// remap_base_value, df_slots_kept) against a naive recomputation, over random
// commit histories of one index with its two snapshots.  A history grows the
// shard by 0, 1, a few hundred, exactly up to a block edge and by several
// blocks; its documents bring new dictionary slots that sort between the old
// ones (so kept rows and the base are remapped); commits fail, are forced full
// (TFIDF_FULL_COMMIT's plan.full, TFIDF_FULL_INVERSION), run under
// TFIDF_DF_FROM_ROWS, and the corpus is cut short now and then.  Each commit
// runs the formula k_df_sum runs, with the plan's numbers, on a model of the
// snapshot: an untrusted base holds garbage and must not be read; a failed
// commit leaves garbage and inv_docs = 0.  After every commit df must equal
// the sum over all blocks and the base the sum over the full blocks.
// Stand-alone; built with -fsanitize=address,undefined by test_df_base_plan_cpu.py.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "commit_plan.h"

using namespace tfidf;

static int checks = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    checks++;                                                       \
    if (!(c)) {                                                     \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);           \
      return 1;                                                     \
    }                                                               \
  } while (0)

constexpr uint32_t kSlots = 64, kWords = kSlots / 32;
constexpr uint32_t kGarbage = 0xDEADBEEFu;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

struct Crank {                       // {occupancy bits, occupied slots before} per 32 slots, as col_rank leaves it
  uint32_t bits[kWords] = {}, base[kWords] = {};
  uint32_t NC = 0;
};

// The corpus: document d holds two slots out of a set that widens with d, in
// an order that puts the later slots between the earlier ones.
struct Corpus {
  uint32_t perm[kSlots];
  uint64_t N = 0;
  std::vector<std::vector<uint32_t>> cnt;    // [block][slot]: documents of the block that hold the slot
  void slots_of(uint64_t d, uint32_t *a, uint32_t *b) const {
    const uint64_t h = (d + 1) * 0xD6E8FEB86659FD93ull;
    const uint32_t width = (uint32_t)std::min<uint64_t>(kSlots, 2 + d / 2500);
    *a = perm[(h >> 20) % width];
    *b = perm[(h >> 40) % width];
  }
  void set_docs(uint64_t n) {
    N = n;
    const size_t blocks = (size_t)((n + kPlanBlockDocs - 1) / kPlanBlockDocs);
    cnt.assign(blocks, std::vector<uint32_t>(kSlots, 0));
    for (uint64_t d = 0; d < n; d++) {
      uint32_t a, b;
      slots_of(d, &a, &b);
      cnt[d / kPlanBlockDocs][a]++;
      if (b != a) cnt[d / kPlanBlockDocs][b]++;
    }
  }
  Crank crank() const {
    Crank c;
    for (const auto &row : cnt)
      for (uint32_t s = 0; s < kSlots; s++)
        if (row[s]) c.bits[s >> 5] |= 1u << (s & 31);
    for (uint32_t w = 0; w < kWords; w++) {
      c.base[w] = c.NC;
      c.NC += (uint32_t)__builtin_popcount(c.bits[w]);
    }
    return c;
  }
};

struct Snap {
  uint64_t inv_docs = 0;
  Crank crank_inv;
  std::vector<uint32_t> df_base;     // [NC_inv], count form
};

// one commit of `c` into `S`; *df_out: df per column
static int commit(const Corpus &c, Snap &S, bool full, const char *inv_knob, const char *rows_knob, bool fails) {
  const Crank now = c.crank();
  const uint64_t N = c.N;
  const uint32_t n_blocks = (uint32_t)c.cnt.size();
  const uint64_t kept_inv = S.inv_docs;
  S.inv_docs = 0;                                                    // covers nothing until the build has succeeded
  const InversionPlan inv = inversion_plan(full, false, kept_inv, N, now.NC, S.crank_inv.NC, inv_knob);
  const DfBasePlan p = df_base_plan(inv, false, N, rows_knob);
  // the plan's own numbers
  CHECK(p.trusted == (inv.first_block > 0));
  CHECK(p.base_before == inv.first_block && p.fold_first == inv.first_block);
  CHECK(p.base_after == N / kPlanBlockDocs);
  CHECK(p.fold_end >= p.fold_first && p.fold_end <= n_blocks && p.fold_end == std::max(p.base_after, p.fold_first));
  CHECK(p.remap == inv.remap);
  CHECK(!p.from_rows || p.trusted);
  if (p.trusted) {
    CHECK(!full && kept_inv != 0 && kept_inv <= N);
    CHECK(p.base_before == kept_inv / kPlanBlockDocs);               // what the last good commit left the base at
    CHECK(p.base_before <= p.base_after);
  }
  // the base in this commit's columns
  std::vector<uint32_t> base(now.NC, kGarbage);
  if (p.trusted && p.remap) {
    CHECK(S.df_base.size() == S.crank_inv.NC);
    for (uint32_t w = 0; w < kWords; w++) {
      uint32_t bits = now.bits[w], col = now.base[w];
      CHECK((S.crank_inv.bits[w] & ~now.bits[w]) == 0);              // the dictionary only gains slots
      while (bits) {
        const uint32_t bit = (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1;
        const bool old = (S.crank_inv.bits[w] >> bit) & 1u;
        if (old) CHECK(remap_old_col(S.crank_inv.bits[w], S.crank_inv.base[w], bit) < S.df_base.size());
        base[col] = remap_base_value(S.df_base.data(), S.crank_inv.bits[w], S.crank_inv.base[w], bit);
        if (!old) CHECK(base[col] == 0);                             // a new column: no posting in a kept block
        col++;
      }
    }
  } else if (p.trusted) {
    CHECK(S.df_base.size() == now.NC && now.NC == S.crank_inv.NC);
    base = S.df_base;
  }
  // k_df_sum, per column
  std::vector<uint32_t> df(now.NC), next_base(now.NC);
  for (uint32_t w = 0; w < kWords; w++) {
    uint32_t bits = now.bits[w], col = now.base[w];
    while (bits) {
      const uint32_t s = 32 * w + (uint32_t)__builtin_ctz(bits);
      bits &= bits - 1;
      const uint32_t b0 = p.trusted ? base[col] : 0u;
      uint32_t run = b0, fold = b0;
      if (p.from_rows) {                                             // the kept rows themselves
        run = 0;
        for (uint32_t b = 0; b < inv.first_block; b++) run += c.cnt[b][s];
        CHECK(run == b0);                                            // ... say what the base says
      }
      for (uint32_t b = inv.first_block; b < n_blocks; b++) {
        run += c.cnt[b][s];
        if (b < p.fold_end) fold += c.cnt[b][s];
      }
      uint32_t want_df = 0, want_base = 0;
      for (uint32_t b = 0; b < n_blocks; b++) {
        want_df += c.cnt[b][s];
        if ((uint64_t)(b + 1) * kPlanBlockDocs <= N) want_base += c.cnt[b][s];
      }
      CHECK(run == want_df);
      CHECK(fold == want_base);
      df[col] = run;
      // the kernel stores the base only when it is rebuilt or a row joins it
      next_base[col] = (!inv.first_block || p.fold_end > inv.first_block) ? fold : base[col];
      CHECK(next_base[col] == want_base);
      col++;
    }
  }
  if (fails) {                                                       // the base may be half written: garbage, never trusted
    S.df_base.assign(now.NC, kGarbage);
    S.crank_inv = now;
    return 0;
  }
  S.df_base = next_base;
  S.crank_inv = now;
  S.inv_docs = N;
  return 0;
}

static int history(uint32_t seed) {
  rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)seed * 0xBF58476D1CE4E5B9ull);
  rnd();
  Corpus c;
  for (uint32_t i = 0; i < kSlots; i++) c.perm[i] = i;
  for (uint32_t i = kSlots - 1; i > 0; i--) std::swap(c.perm[i], c.perm[rnd() % (i + 1)]);
  Snap snaps[2];
  uint32_t target = 0;
  uint64_t N = 1 + rnd() % 20000;
  c.set_docs(N);
  for (int step = 0; step < 40; step++) {
    switch (rnd() % 8) {
      case 0: case 1: break;                                                    // nothing added
      case 2: N += 1; break;
      case 3: N += 100 + rnd() % 400; break;
      case 4: N = (N / kPlanBlockDocs + 1) * kPlanBlockDocs; break;             // exactly up to the next block edge
      case 5: N += kPlanBlockDocs * (1 + rnd() % 3) + rnd() % 700; break;       // across several edges
      case 6: N += rnd() % 3 ? 0 : kPlanBlockDocs; break;                       // a whole block from an edge, or nothing
      default: if (rnd() % 4 == 0) N = 1 + N / 2; else N += 200; break;         // (a cut corpus: inv_docs > N)
    }
    N = std::min<uint64_t>(N, 26 * kPlanBlockDocs);
    const bool cut = N < c.N;
    if (N != c.N) c.set_docs(N);
    const bool full = cut || rnd() % 9 == 0;                                    // a cut is an epoch change; else the knob, dead documents, a retry
    const char *inv_knob = rnd() % 9 == 0 ? "1" : rnd() % 7 == 0 ? "0" : nullptr;
    const char *rows_knob = rnd() % 4 == 0 ? "1" : rnd() % 9 == 0 ? "0" : nullptr;
    const bool fails = rnd() % 7 == 0;
    for (int twice = 0; twice < 1 + (int)(rnd() % 2); twice++) {                // often both snapshots
      if (commit(c, snaps[target], full && twice == 0, inv_knob, rows_knob, fails && twice == 0)) {
        printf("  at seed %u step %d N %llu target %u\n", seed, step, (unsigned long long)N, target);
        return 1;
      }
      target ^= 1u;                                                             // the published one stays; the spare is next
    }
  }
  return 0;
}

int main() {
  // the states the GPU test builds: 16 500 (+200, +0), a tail filled to 3 x 8192 (+0, +1), 16 500 -> 25 200
  {
    InversionPlan inv = inversion_plan(false, false, 16500, 16700, 400, 400, nullptr);
    DfBasePlan p = df_base_plan(inv, false, 16700, nullptr);
    CHECK(p.trusted && p.base_before == 2 && p.base_after == 2 && p.fold_first == 2 && p.fold_end == 2 && !p.remap);
    inv = inversion_plan(false, false, 16700, 24576, 400, 400, nullptr);
    p = df_base_plan(inv, false, 24576, nullptr);
    CHECK(p.trusted && p.base_before == 2 && p.base_after == 3 && p.fold_end == 3);
    inv = inversion_plan(false, false, 24576, 24576, 400, 400, nullptr);      // no row inverted: df is the base alone
    p = df_base_plan(inv, false, 24576, nullptr);
    CHECK(p.trusted && inv.first_block == 3 && p.base_before == 3 && p.base_after == 3 && p.fold_end == 3);
    inv = inversion_plan(false, false, 16500, 25200, 400, 390, nullptr);      // two rows fold, the new tail does not; remapped
    p = df_base_plan(inv, false, 25200, "1");
    CHECK(p.trusted && p.base_before == 2 && p.base_after == 3 && p.fold_end == 3 && p.remap && p.from_rows);
    inv = inversion_plan(false, false, 8191, 8192, 400, 400, nullptr);        // nothing kept yet: the base starts here
    p = df_base_plan(inv, false, 8192, "1");
    CHECK(!p.trusted && p.base_before == 0 && p.base_after == 1 && p.fold_end == 1 && !p.from_rows);
    inv = inversion_plan(false, false, 30000, 30000, 400, 400, "1");          // TFIDF_FULL_INVERSION
    p = df_base_plan(inv, false, 30000, nullptr);
    CHECK(!p.trusted && p.fold_first == 0 && p.fold_end == 3 && p.base_after == 3);
    inv = inversion_plan(false, false, 0, 30000, 400, 400, nullptr);          // a failed build before
    CHECK(!df_base_plan(inv, false, 30000, nullptr).trusted);
    inv = inversion_plan(true, false, 30000, 30000, 400, 400, nullptr);       // plan.full
    CHECK(!df_base_plan(inv, false, 30000, nullptr).trusted);
    p = df_base_plan(InversionPlan{}, true, 30000, "1");                      // term-major: no base
    CHECK(!p.trusted && !p.from_rows && p.fold_end == 0 && p.base_after == 0);
  }
  // per-slot df stands only when nothing it is made from changed
  {
    MirrorPlan none = mirror_plan(false, false, 1000, true, 1024, 400, 400, 0, kDfDeltaCap, nullptr);
    CHECK(none.delta && none.df == kMirrorNone && none.dict == kMirrorNone);
    CHECK(df_slots_kept(none, 1000, 1000, false, 400, 400, nullptr));
    CHECK(df_slots_kept(none, 1000, 1000, false, 400, 400, "0"));
    CHECK(!df_slots_kept(none, 1000, 1000, false, 400, 400, "1"));            // the A/B switch
    CHECK(!df_slots_kept(none, 999, 1000, false, 400, 400, nullptr));         // documents the last build did not cover
    CHECK(!df_slots_kept(none, 0, 0, false, 400, 400, nullptr));
    CHECK(!df_slots_kept(none, 1000, 1000, true, 400, 400, nullptr));
    CHECK(!df_slots_kept(none, 1000, 1000, false, 401, 400, nullptr));
    CHECK(!df_slots_kept(mirror_plan(false, false, 1000, true, 1024, 400, 400, 5, kDfDeltaCap, nullptr), 1000, 1000, false,
                         400, 400, nullptr));                                 // postings were tokenized
    CHECK(!df_slots_kept(mirror_plan(false, false, 1000, false, 1024, 400, 400, 0, kDfDeltaCap, nullptr), 1000, 1000, false,
                         400, 400, nullptr));                                 // the mirrors were not valid
    CHECK(!df_slots_kept(mirror_plan(true, false, 1000, true, 1024, 400, 400, 0, kDfDeltaCap, nullptr), 1000, 1000, false,
                         400, 400, nullptr));                                 // a full build
    CHECK(!df_slots_kept(mirror_plan(false, false, 1000, true, 1024, 400, 400, 0, kDfDeltaCap, "1"), 1000, 1000, false, 400,
                         400, nullptr));                                      // TFIDF_FULL_MIRROR
  }
  for (uint32_t seed = 1; seed <= 120; seed++)
    if (history(seed)) return 1;
  printf("ok %d checks\n", checks);
  return 0;
}
