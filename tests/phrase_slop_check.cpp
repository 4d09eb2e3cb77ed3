// phrase_slop_check.cpp — stand-alone run of the sloppy phrase rule of
// csrc/phrase_plan.h on the host (built with -fsanitize=address,undefined and
// run as a child process by test_phrase_slop_cpu.py).
//
//   phrase_slop_check CASES
// runs ph_has_repeat, ph_sloppy_freq, the ph_match_at count and ph_score_f over
// rows of listed tokens.  Input, little endian:
//   u32 n_cases, then per case: u32 m, m x u32 ordinal (seq), u32 slop,
//       f32 weight, f32 cache[norm], u32 n, n x u32 position, n x u32 ordinal
// Output per case: "case <i> <repeat> <sloppy freq bits> <exact count> <score
// bits>" where the sloppy frequency is 0 for a phrase the rule does not take
// (a repeat, m < 2, m > 64) and the score is ph_score_f over the frequency the
// search would use (the count at slop 0 or m = 1, else the sloppy frequency);
// then "ok <n_cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "phrase_plan.h"

using namespace tfidf;

static long long g_case = -1;
#define CHECK(c)                                                                         \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      fprintf(stderr, "%s:%d: %s failed (case %lld)\n", __FILE__, __LINE__, #c, g_case); \
      exit(1);                                                                           \
    }                                                                                    \
  } while (0)

static FILE *g_f;
static void rd(void *p, size_t n) { CHECK(n == 0 || fread(p, 1, n, g_f) == n); }
template <class T> static T get() {
  T v;
  rd(&v, sizeof(T));
  return v;
}
static uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: phrase_slop_check CASES\n"); return 2; }
  g_f = fopen(argv[1], "rb");
  if (!g_f) { perror(argv[1]); return 2; }
  const uint32_t n_cases = get<uint32_t>();
  for (uint32_t c = 0; c < n_cases; c++) {
    g_case = c;
    const uint32_t m = get<uint32_t>();
    CHECK(m >= 1 && m <= kPhMaxTerms);
    // exact-size heap blocks (a read past an array is an ASan error)
    uint32_t *seq = (uint32_t *)malloc(m * 4);
    rd(seq, m * 4);
    const uint32_t slop = get<uint32_t>();
    const float w = get<float>(), cn = get<float>();
    const uint32_t n = get<uint32_t>();
    uint32_t *pos = (uint32_t *)malloc(n ? n * 4 : 1), *ord = (uint32_t *)malloc(n ? n * 4 : 1);
    rd(pos, (size_t)n * 4);
    rd(ord, (size_t)n * 4);
    for (uint32_t i = 1; i < n; i++) CHECK(pos[i] > pos[i - 1]);
    const bool repeat = ph_has_repeat(seq, m);
    uint32_t count = 0;
    for (uint32_t i = 0; i < n; i++) count += ph_match_at(pos, ord, n, i, seq, m) ? 1u : 0u;
    const bool walk = !repeat && m >= 2 && m <= kPhMaxSloppyTerms;
    const float sloppy = walk ? ph_sloppy_freq(pos, ord, n, m, slop) : 0.0f;
    const float freq = slop == 0 || m < 2 ? (float)count : sloppy;
    const float sc = freq > 0.0f ? ph_score_f(w, freq, cn) : 0.0f;
    if (slop == 0 || m < 2) CHECK(bits_of(ph_score(w, count, cn)) == bits_of(ph_score_f(w, (float)count, cn)));
    printf("case %u %d %u %u %u\n", c, repeat ? 1 : 0, bits_of(sloppy), count, bits_of(sc));
    free(seq);
    free(pos);
    free(ord);
  }
  printf("ok %u\n", n_cases);
  fclose(g_f);
  return 0;
}
