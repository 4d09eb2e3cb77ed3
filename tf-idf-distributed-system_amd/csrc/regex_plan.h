// regex_plan.h — regular-expression search (tfidf_regex_terms*,
// tfidf_search_regex*): the rules shared by the device scan of the dictionary
// (kernels_regex.hip), the host around it (tfidf_capi.hip) and a stand-alone
// host checker (tests/regex_check.cpp).
//
// A pattern is a byte string, decoded as strict UTF-8 into code points.  It is
// NOT lower-cased (Lucene's RegexpQuery does not lower-case either, and the
// wildcard calls do, on purpose): the vocabulary is lower-case, so `Foo.*`
// matches nothing.  A vocabulary term matches when the whole term belongs to
// the pattern's language, over code points.  The grammar restates Lucene 9.8
// RegExp ("Regular-expression search"):
//
//   union   := inter ('|' inter)*
//   inter   := concat ('&' concat)*
//   concat  := repeat+                       (stops at ')', '|', '&', end)
//   repeat  := compl ('?' | '*' | '+' | '{n}' | '{n,}' | '{n,m}')*
//   compl   := '~' compl | class
//   class   := '[' '^'? item+ ']' | simple
//   item    := charexp ('-' charexp)?
//   simple  := '.' | '#' | '@' | '"' (not '"')* '"' | '(' ')' | '(' union ')'
//            | '\d' '\D' '\s' '\S' '\w' '\W' | charexp
//   charexp := '\' any code point | any code point that is not reserved
//
// Reserved outside a class: | & ? * + { } [ ] ( ) . # @ " ~ \ <.  `<` (named
// automata, numeric intervals) answers kRxUnsupported.  A pattern that is not
// strict UTF-8 compiles to no table and matches nothing; the empty pattern is
// the empty-string language, which holds no term.
//
// The host compiles a pattern to a Thompson NFA over the base classes (the
// partition of [0, 0x10FFFF] by the pattern's range ends), determinises it,
// minimises the DFA (Hopcroft), merges classes with equal columns and numbers the states
// canonically: state 0 is the dead state (always present), the live states are
// 1, 2, ... in breadth-first order from the start state, by class order.  Two
// patterns of one language serialise to the same words.  Complement and
// intersection determinise their operands first.  Every step counts into one
// effort budget, so a pattern fails fast (kRxUnsupported, Lucene's
// TooComplexToDeterminizeException) instead of allocating without bound.
//
// The serialised table (uint32_t words):
//   [0] words of the whole table   [1] states | classes << 16   [2] non-ASCII intervals
//   [3] start state (0: the empty language)   [4] min code points   [5] max (kRxNoMax: none)
//   ASCII class map: 128 bytes; interval starts: u32 each, ascending from 128;
//   interval classes: u8 each, padded to a word; transitions: u16
//   [state][class], padded to a word; accept bits: one word per 32 states.
// The matcher is a table walk: one class lookup (the map for ASCII, a binary
// search of the interval starts otherwise) and one transition read per code
// point, leaving on the dead state.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "fuzzy_plan.h"
#include "wildcard_plan.h"

namespace tfidf {

// --- limits ---
// LDS staging of one scan: at most kWcChunkPatterns tables of at most
// kRxStageWords words together.  32 KiB of tables + 1 KiB of offsets and
// counters per workgroup keeps 4 workgroups of 256 lanes resident in the 160
// KiB of a CU.
constexpr uint32_t kRxStageWords = 8192;
constexpr uint32_t kRxStageBytes = kRxStageWords * 4;
// the per-pattern limit: a table of at most this many bytes.  257 states (256
// live + dead) x 32 classes x 2 bytes = 16 448 bytes + 700 bytes of maps fit.
constexpr uint32_t kRxMaxTableBytes = kRxStageBytes;
constexpr uint32_t kRxMaxClasses = 255;            // a class is a byte
constexpr uint32_t kRxMaxNfaStates = 8192;         // of one NFA (repeat expansion included)
constexpr uint32_t kRxMaxWorkStates = 4096;        // subset / product states before minimisation
constexpr uint32_t kRxMaxBaseClasses = 1024;       // intervals the pattern's range ends cut
constexpr uint32_t kRxMaxDepth = 200;              // nesting of '(' and '~', and the height of the syntax tree (a
                                                   // repeat operator, a complement, an operator with operands: one
                                                   // level each), which bounds every recursion of the compiler
constexpr uint64_t kRxMaxEffort = 1ull << 25;      // elementary steps of one compilation
constexpr uint32_t kRxMaxRepeat = 1u << 20;        // a larger {n} is clamped (and then over the NFA limit)
constexpr uint32_t kRxNoMax = 0xFFFFFFFFu;
constexpr uint32_t kRxMaxCp = 0x10FFFFu;
constexpr uint32_t kRxHeaderWords = 6;

enum : int { kRxOk = 0, kRxSyntax = 1, kRxUnsupported = 2 };

// --- the table walk (host and device) ---

struct RxView {
  const uint8_t *ascii, *iv_class;
  const uint32_t *iv_start, *accept;
  const uint16_t *trans;
  uint32_t n_states, n_classes, n_iv, start, min_cps, max_cps;
};

TFIDF_HD RxView rx_view(const uint32_t *t) {
  RxView v;
  v.n_states = t[1] & 0xFFFFu;
  v.n_classes = t[1] >> 16;
  v.n_iv = t[2];
  v.start = t[3];
  v.min_cps = t[4];
  v.max_cps = t[5];
  const uint32_t *p = t + kRxHeaderWords;
  v.ascii = reinterpret_cast<const uint8_t *>(p);
  p += 32;
  v.iv_start = p;
  p += v.n_iv;
  v.iv_class = reinterpret_cast<const uint8_t *>(p);
  p += (v.n_iv + 3) >> 2;
  v.trans = reinterpret_cast<const uint16_t *>(p);
  p += (v.n_states * v.n_classes + 1) >> 1;
  v.accept = p;
  return v;
}

TFIDF_HD uint32_t rx_class(const RxView &v, uint32_t cp) {
  if (cp < 128u) return v.ascii[cp];
  uint32_t lo = 0, hi = v.n_iv;                    // last interval with start <= cp (iv_start[0] = 128)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v.iv_start[mid] <= cp) lo = mid; else hi = mid;
  }
  return v.iv_class[lo];
}

TFIDF_HD uint32_t rx_step(const RxView &v, uint32_t state, uint32_t cp) {
  return v.trans[state * v.n_classes + rx_class(v, cp)];
}

TFIDF_HD bool rx_accepts(const RxView &v, uint32_t state) { return (v.accept[state >> 5] >> (state & 31u)) & 1u; }

// Does the candidate (n_cand code points behind the cursor, taken by value) belong to the table's language?
template <class Cursor>
TFIDF_HD bool rx_match(const uint32_t *table, Cursor c, uint32_t n_cand) {
  const RxView v = rx_view(table);
  if (n_cand < v.min_cps || n_cand > v.max_cps) return false;
  uint32_t s = v.start;
  for (uint32_t i = 0; i < n_cand && s != 0; i++) s = rx_step(v, s, c.next());
  return s != 0 && rx_accepts(v, s);
}

// --- the host plan ---
// Scan chunks: consecutive patterns whose tables (n_bytes[i]; 0 = a pattern
// that matches nothing, staged nowhere but still a member of its chunk) stay
// within `budget` bytes together, at most kWcChunkPatterns of them; one
// pattern always forms a chunk.  Appends the cut points 0, ..., n.
inline void rx_plan_scan_chunks(const uint32_t *n_bytes, uint64_t n, uint64_t budget, std::vector<uint64_t> *cuts) {
  if (budget > kRxStageBytes) budget = kRxStageBytes;
  fz_plan_scan_chunks(n_bytes, n, kWcChunkPatterns, (uint32_t)budget, cuts);
}

// --- the compiler (host only) ---

struct RxRange {
  uint32_t lo, hi;
};

struct RxNode {
  enum Kind : uint8_t { NONE, EPS, ANYSTR, SET, UNION, INTER, CONCAT, REPEAT, COMPL } kind;
  std::vector<RxRange> set;       // SET: sorted, disjoint
  std::vector<uint32_t> kids;     // UNION / INTER / CONCAT: all; REPEAT / COMPL: one
  uint32_t rmin = 0, rmax = 0;    // REPEAT (rmax kRxNoMax: unbounded)
  int dfa = -1;                   // COMPL / INTER: the cached automaton
  uint32_t height = 1;            // of the syntax tree below and with this node
};

// a complete DFA over base classes; state 0 is the start
struct RxDfa {
  uint32_t nb = 0;
  std::vector<uint32_t> t;        // [state][class]
  std::vector<uint8_t> acc;
  uint32_t n() const { return (uint32_t)acc.size(); }
};

struct RxNfaState {
  std::vector<uint32_t> eps;
  std::vector<uint32_t> tr;       // triples: first class, last class, target
};

struct RxCompiler {
  std::vector<uint32_t> cps;      // the pattern's code points and their byte offsets (+ the end)
  std::vector<uint64_t> at;
  size_t p = 0;
  int status = kRxOk;
  uint64_t err_at = 0;
  uint64_t effort = 0;
  uint32_t depth = 0;
  std::vector<RxNode> nodes;
  std::vector<uint32_t> cuts;     // base class i = [cuts[i], cuts[i + 1])
  std::vector<RxDfa> dfas;

  bool ok() const { return status == kRxOk; }
  bool fail(int st) {
    if (status == kRxOk) {
      status = st;
      err_at = at[p < at.size() ? p : at.size() - 1];
    }
    return false;
  }
  bool spend(uint64_t n) {
    effort += n;
    return effort <= kRxMaxEffort ? true : fail(kRxUnsupported);
  }
  bool more() const { return p < cps.size(); }
  bool peek(uint32_t c) const { return p < cps.size() && cps[p] == c; }
  bool take(uint32_t c) {
    if (!peek(c)) return false;
    p++;
    return true;
  }
  uint32_t add(RxNode::Kind k) {
    nodes.push_back(RxNode{});
    nodes.back().kind = k;
    return (uint32_t)nodes.size() - 1;
  }
  // an inner node over its operands; -1 (kRxUnsupported) where the tree grows past kRxMaxDepth
  int add_over(RxNode::Kind k, const std::vector<uint32_t> &kids) {
    uint32_t h = 0;
    for (uint32_t c : kids) h = std::max(h, nodes[c].height);
    if (h + 1 > kRxMaxDepth) { fail(kRxUnsupported); return -1; }
    const uint32_t u = add(k);
    nodes[u].kids = kids;
    nodes[u].height = h + 1;
    return (int)u;
  }
  uint32_t add_set(std::vector<RxRange> r) {
    std::sort(r.begin(), r.end(), [](const RxRange &a, const RxRange &b) { return a.lo < b.lo; });
    std::vector<RxRange> m;
    for (const RxRange &x : r) {
      if (!m.empty() && x.lo <= m.back().hi + 1 && m.back().hi != kRxMaxCp) m.back().hi = std::max(m.back().hi, x.hi);
      else if (!m.empty() && m.back().hi == kRxMaxCp) continue;
      else m.push_back(x);
    }
    const uint32_t n = add(RxNode::SET);
    nodes[n].set = m;
    return n;
  }
  static std::vector<RxRange> negate(std::vector<RxRange> r) {
    std::sort(r.begin(), r.end(), [](const RxRange &a, const RxRange &b) { return a.lo < b.lo; });
    std::vector<RxRange> out;
    uint64_t next = 0;
    for (const RxRange &x : r) {
      if (x.lo > next) out.push_back(RxRange{(uint32_t)next, x.lo - 1});
      next = std::max<uint64_t>(next, (uint64_t)x.hi + 1);
    }
    if (next <= kRxMaxCp) out.push_back(RxRange{(uint32_t)next, kRxMaxCp});
    return out;
  }

  // ---- the parser (recursive descent; the first error met, left to right, is the answer) ----
  static bool reserved(uint32_t c) {
    switch (c) {
      case '|': case '&': case '?': case '*': case '+': case '{': case '}': case '[': case ']': case '(': case ')':
      case '.': case '#': case '@': case '"': case '~': case '\\': case '<':
        return true;
    }
    return false;
  }
  int parse_union() {
    int n = parse_inter();
    if (n < 0) return n;
    std::vector<uint32_t> kids{(uint32_t)n};
    while (take('|')) {
      n = parse_inter();
      if (n < 0) return n;
      kids.push_back((uint32_t)n);
    }
    if (kids.size() == 1) return (int)kids[0];
    return add_over(RxNode::UNION, kids);
  }
  int parse_inter() {
    int n = parse_concat();
    if (n < 0) return n;
    std::vector<uint32_t> kids{(uint32_t)n};
    while (take('&')) {
      n = parse_concat();
      if (n < 0) return n;
      kids.push_back((uint32_t)n);
    }
    if (kids.size() == 1) return (int)kids[0];
    return add_over(RxNode::INTER, kids);
  }
  int parse_concat() {
    std::vector<uint32_t> kids;
    do {
      const int n = parse_repeat();                 // at ')', '|', '&' or the end first: an empty alternative
      if (n < 0) return n;
      kids.push_back((uint32_t)n);
    } while (more() && !peek(')') && !peek('|') && !peek('&'));
    if (kids.size() == 1) return (int)kids[0];
    return add_over(RxNode::CONCAT, kids);
  }
  bool parse_int(uint32_t *v) {
    if (!more() || cps[p] < '0' || cps[p] > '9') return fail(kRxSyntax);
    uint64_t x = 0;
    while (more() && cps[p] >= '0' && cps[p] <= '9') {
      x = std::min<uint64_t>(x * 10 + (cps[p] - '0'), kRxMaxRepeat);
      p++;
    }
    *v = (uint32_t)x;
    return true;
  }
  int parse_repeat() {
    int n = parse_compl();
    if (n < 0) return n;
    for (;;) {
      uint32_t lo, hi;
      if (take('?')) { lo = 0; hi = 1; }
      else if (take('*')) { lo = 0; hi = kRxNoMax; }
      else if (take('+')) { lo = 1; hi = kRxNoMax; }
      else if (take('{')) {
        if (!parse_int(&lo)) return -1;
        hi = lo;
        if (take(',')) {
          hi = kRxNoMax;
          if (more() && cps[p] >= '0' && cps[p] <= '9' && !parse_int(&hi)) return -1;
        }
        if (!take('}')) { fail(kRxSyntax); return -1; }
      } else {
        break;
      }
      if (hi < lo) {
        n = (int)add(RxNode::NONE);                 // {n,m} with m < n: the empty language
      } else {
        n = add_over(RxNode::REPEAT, {(uint32_t)n});
        if (n < 0) return n;
        nodes[n].rmin = lo;
        nodes[n].rmax = hi;
      }
    }
    return n;
  }
  int parse_compl() {
    if (take('~')) {
      if (++depth > kRxMaxDepth) { fail(kRxUnsupported); return -1; }
      const int n = parse_compl();
      depth--;
      if (n < 0) return n;
      return add_over(RxNode::COMPL, {(uint32_t)n});
    }
    return parse_class();
  }
  bool parse_charexp(uint32_t *c, bool in_class) {
    if (!more()) return fail(kRxSyntax);
    if (cps[p] == '\\') {
      p++;
      if (!more()) return fail(kRxSyntax);          // a dangling backslash
      *c = cps[p++];
      return true;
    }
    if (!in_class && reserved(cps[p])) return fail(cps[p] == '<' ? kRxUnsupported : kRxSyntax);
    *c = cps[p++];
    return true;
  }
  int parse_class() {
    if (!take('[')) return parse_simple();
    const bool neg = take('^');
    std::vector<RxRange> r;
    do {                                            // the first item always, then until ']'
      uint32_t lo, hi;
      if (!parse_charexp(&lo, true)) return -1;
      hi = lo;
      if (take('-')) {
        if (!parse_charexp(&hi, true)) return -1;
        if (hi < lo) { fail(kRxSyntax); return -1; }
      }
      r.push_back(RxRange{lo, hi});
      if (!spend(1)) return -1;
    } while (more() && !peek(']'));
    if (!take(']')) { fail(kRxSyntax); return -1; }
    return (int)add_set(neg ? negate(r) : r);
  }
  int parse_simple() {
    if (!more()) { fail(kRxSyntax); return -1; }
    if (take('.')) return (int)add_set({RxRange{0, kRxMaxCp}});
    if (take('#')) return (int)add(RxNode::NONE);
    if (take('@')) return (int)add(RxNode::ANYSTR);
    if (take('"')) {
      std::vector<uint32_t> kids;
      while (more() && !peek('"')) kids.push_back(add_set({RxRange{cps[p], cps[p]}})), p++;
      if (!take('"')) { fail(kRxSyntax); return -1; }
      if (kids.empty()) return (int)add(RxNode::EPS);
      if (kids.size() == 1) return (int)kids[0];
      return add_over(RxNode::CONCAT, kids);
    }
    if (take('(')) {
      if (take(')')) return (int)add(RxNode::EPS);
      if (++depth > kRxMaxDepth) { fail(kRxUnsupported); return -1; }
      const int n = parse_union();
      depth--;
      if (n < 0) return n;
      if (!take(')')) { fail(kRxSyntax); return -1; }
      return n;
    }
    if (peek('\\') && p + 1 < cps.size()) {
      const std::vector<RxRange> d{{'0', '9'}}, s{{'\t', '\n'}, {'\r', '\r'}, {' ', ' '}},
          w{{'0', '9'}, {'A', 'Z'}, {'_', '_'}, {'a', 'z'}};
      const std::vector<RxRange> *cl = nullptr;
      bool neg = false;
      switch (cps[p + 1]) {
        case 'd': cl = &d; break;
        case 'D': cl = &d; neg = true; break;
        case 's': cl = &s; break;
        case 'S': cl = &s; neg = true; break;
        case 'w': cl = &w; break;
        case 'W': cl = &w; neg = true; break;
      }
      if (cl) {
        p += 2;
        return (int)add_set(neg ? negate(*cl) : *cl);
      }
    }
    uint32_t c;
    if (!parse_charexp(&c, false)) return -1;
    return (int)add_set({RxRange{c, c}});
  }

  // ---- automata ----
  uint32_t class_of(uint32_t cp) const {            // base class holding cp
    return (uint32_t)(std::upper_bound(cuts.begin(), cuts.end(), cp) - cuts.begin()) - 1;
  }
  uint32_t nb() const { return (uint32_t)cuts.size() - 1; }

  struct Frag {
    uint32_t s, e;
  };
  typedef std::vector<RxNfaState> Nfa;
  bool new_state(Nfa &N, uint32_t *id) {
    if (N.size() >= kRxMaxNfaStates) return fail(kRxUnsupported);
    if (!spend(1)) return false;
    N.emplace_back();
    *id = (uint32_t)N.size() - 1;
    return true;
  }
  // every fragment adds at least one state, so the NFA limit also bounds the work of repeat expansion;
  // the recursion (build, and dfa_of -> build under a complement or an intersection) goes one
  // syntax node down per call, so the tree's height (<= kRxMaxDepth) bounds its depth
  bool build(uint32_t ni, Nfa &N, Frag *f) {
    if (!new_state(N, &f->s) || !new_state(N, &f->e)) return false;
    const RxNode::Kind kind = nodes[ni].kind;
    switch (kind) {
      case RxNode::NONE:
        return true;
      case RxNode::EPS:
        N[f->s].eps.push_back(f->e);
        return true;
      case RxNode::ANYSTR:
        N[f->s].eps.push_back(f->e);
        N[f->e].tr.insert(N[f->e].tr.end(), {0u, nb() - 1, f->e});
        return true;
      case RxNode::SET:
        for (size_t i = 0; i < nodes[ni].set.size(); i++) {
          const RxRange r = nodes[ni].set[i];
          N[f->s].tr.insert(N[f->s].tr.end(), {class_of(r.lo), class_of(r.hi), f->e});
        }
        return true;
      case RxNode::UNION:
        for (size_t i = 0; i < nodes[ni].kids.size(); i++) {
          Frag k;
          if (!build(nodes[ni].kids[i], N, &k)) return false;
          N[f->s].eps.push_back(k.s);
          N[k.e].eps.push_back(f->e);
        }
        return true;
      case RxNode::CONCAT: {
        uint32_t last = f->s;
        for (size_t i = 0; i < nodes[ni].kids.size(); i++) {
          Frag k;
          if (!build(nodes[ni].kids[i], N, &k)) return false;
          N[last].eps.push_back(k.s);
          last = k.e;
        }
        N[last].eps.push_back(f->e);
        return true;
      }
      case RxNode::REPEAT: {
        const uint32_t kid = nodes[ni].kids[0], lo = nodes[ni].rmin, hi = nodes[ni].rmax;
        uint32_t last = f->s;
        Frag k{0, 0};
        for (uint32_t i = 0; i < lo; i++) {
          if (!build(kid, N, &k)) return false;
          N[last].eps.push_back(k.s);
          last = k.e;
        }
        if (hi == kRxNoMax) {
          if (lo == 0) {                            // kid*
            if (!build(kid, N, &k)) return false;
            N[last].eps.push_back(k.s);
            N[k.s].eps.push_back(k.e);
            last = k.e;
          }
          N[k.e].eps.push_back(k.s);                // the last copy again, any number of times
        } else {
          for (uint32_t i = lo; i < hi; i++) {      // optional copies: each may leave for the end
            if (!build(kid, N, &k)) return false;
            N[last].eps.push_back(k.s);
            N[last].eps.push_back(f->e);
            last = k.e;
          }
        }
        N[last].eps.push_back(f->e);
        return true;
      }
      case RxNode::INTER:
      case RxNode::COMPL: {
        if (nodes[ni].dfa < 0) {
          RxDfa d;
          if (!dfa_of(nodes[ni].kids[0], &d)) return false;
          if (kind == RxNode::COMPL) {
            for (uint8_t &a : d.acc) a = !a;
          } else {
            for (size_t i = 1; i < nodes[ni].kids.size(); i++) {
              RxDfa o, prod;
              if (!dfa_of(nodes[ni].kids[i], &o) || !product(d, o, &prod)) return false;
              d.t.swap(prod.t);
              d.acc.swap(prod.acc);
            }
          }
          dfas.push_back(d);
          nodes[ni].dfa = (int)dfas.size() - 1;
        }
        return embed(dfas[nodes[ni].dfa], N, *f);
      }
    }
    return fail(kRxUnsupported);
  }
  // a DFA as a fragment: its states, runs of classes with one target as transitions
  bool embed(const RxDfa &d, Nfa &N, Frag f) {
    const uint32_t base = (uint32_t)N.size();
    for (uint32_t s = 0; s < d.n(); s++) {
      uint32_t id;
      if (!new_state(N, &id)) return false;
    }
    N[f.s].eps.push_back(base);
    for (uint32_t s = 0; s < d.n(); s++) {
      if (!spend(d.nb)) return false;
      for (uint32_t c = 0; c < d.nb;) {
        uint32_t c1 = c;
        const uint32_t t = d.t[(size_t)s * d.nb + c];
        while (c1 + 1 < d.nb && d.t[(size_t)s * d.nb + c1 + 1] == t) c1++;
        N[base + s].tr.insert(N[base + s].tr.end(), {c, c1, base + t});
        c = c1 + 1;
      }
      if (d.acc[s]) N[base + s].eps.push_back(f.e);
    }
    return true;
  }
  bool dfa_of(uint32_t ni, RxDfa *d) {
    Nfa N;
    Frag f;
    return build(ni, N, &f) && determinise(N, f, d);
  }
  // subset construction over the base classes
  bool determinise(const Nfa &N, Frag f, RxDfa *d) {
    const uint32_t B = nb();
    d->nb = B;
    d->t.clear();
    d->acc.clear();
    std::vector<uint32_t> mark(N.size(), 0), stack;
    uint32_t stamp = 0;
    auto closure = [&](std::vector<uint32_t> &set) -> bool {   // in place; sorted on return
      stamp++;
      stack.clear();
      for (uint32_t s : set) {
        if (mark[s] != stamp) {
          mark[s] = stamp;
          stack.push_back(s);
        }
      }
      set.clear();
      while (!stack.empty()) {
        const uint32_t s = stack.back();
        stack.pop_back();
        set.push_back(s);
        if (!spend(1 + N[s].eps.size())) return false;
        for (uint32_t e : N[s].eps)
          if (mark[e] != stamp) {
            mark[e] = stamp;
            stack.push_back(e);
          }
      }
      std::sort(set.begin(), set.end());
      return true;
    };
    std::map<std::vector<uint32_t>, uint32_t> ids;
    std::vector<std::vector<uint32_t>> sets;
    std::vector<uint32_t> first{f.s};
    if (!closure(first)) return false;
    ids[first] = 0;
    sets.push_back(first);
    std::vector<std::vector<uint32_t>> tgt(B);
    for (uint32_t q = 0; q < sets.size(); q++) {
      d->acc.push_back(std::binary_search(sets[q].begin(), sets[q].end(), f.e));
      d->t.resize((size_t)(q + 1) * B);
      for (uint32_t c = 0; c < B; c++) tgt[c].clear();
      if (!spend(B)) return false;
      for (uint32_t s : sets[q])
        for (size_t i = 0; i < N[s].tr.size(); i += 3) {
          if (!spend(N[s].tr[i + 1] - N[s].tr[i] + 1)) return false;
          for (uint32_t c = N[s].tr[i]; c <= N[s].tr[i + 1]; c++) tgt[c].push_back(N[s].tr[i + 2]);
        }
      for (uint32_t c = 0; c < B; c++) {
        if (!spend(1 + tgt[c].size())) return false;
        if (c && tgt[c] == tgt[c - 1]) {            // the same moves as the class before (common: '.')
          d->t[(size_t)q * B + c] = d->t[(size_t)q * B + c - 1];
          continue;
        }
        std::vector<uint32_t> set = tgt[c];
        if (!closure(set)) return false;
        auto it = ids.find(set);
        if (it == ids.end()) {
          if (sets.size() >= kRxMaxWorkStates) return fail(kRxUnsupported);
          it = ids.emplace(set, (uint32_t)sets.size()).first;
          sets.push_back(set);
        }
        d->t[(size_t)q * B + c] = it->second;
      }
    }
    return true;
  }
  // the reachable pairs of two complete DFAs, accepting where both do
  bool product(const RxDfa &a, const RxDfa &b, RxDfa *d) {
    const uint32_t B = a.nb;
    d->nb = B;
    d->t.clear();
    d->acc.clear();
    std::map<uint64_t, uint32_t> ids;
    std::vector<uint64_t> pairs{0};
    ids[0] = 0;
    for (uint32_t q = 0; q < pairs.size(); q++) {
      const uint32_t x = (uint32_t)(pairs[q] >> 32), y = (uint32_t)pairs[q];
      d->acc.push_back(a.acc[x] && b.acc[y]);
      d->t.resize((size_t)(q + 1) * B);
      if (!spend(4 * (uint64_t)B)) return false;
      for (uint32_t c = 0; c < B; c++) {
        const uint64_t k = ((uint64_t)a.t[(size_t)x * B + c] << 32) | b.t[(size_t)y * B + c];
        auto it = ids.find(k);
        if (it == ids.end()) {
          if (pairs.size() >= kRxMaxWorkStates) return fail(kRxUnsupported);
          it = ids.emplace(k, (uint32_t)pairs.size()).first;
          pairs.push_back(k);
        }
        d->t[(size_t)q * B + c] = it->second;
      }
    }
    return true;
  }

  // classes with equal columns become one (numbered by their first member): map[c] -> merged class
  bool merge_classes(const RxDfa &d, std::vector<uint32_t> *map, RxDfa *out) {
    const uint32_t n = d.n(), B = d.nb;
    if (!spend((uint64_t)n * B)) return false;
    std::map<std::vector<uint32_t>, uint32_t> seen;
    std::vector<uint32_t> col(n), keep;
    map->assign(B, 0);
    for (uint32_t c = 0; c < B; c++) {
      for (uint32_t s = 0; s < n; s++) col[s] = d.t[(size_t)s * B + c];
      auto it = seen.find(col);
      if (it == seen.end()) {
        it = seen.emplace(col, (uint32_t)keep.size()).first;
        keep.push_back(c);
      }
      (*map)[c] = it->second;
    }
    out->nb = (uint32_t)keep.size();
    out->acc = d.acc;
    out->t.resize((size_t)n * keep.size());
    for (uint32_t s = 0; s < n; s++)
      for (size_t k = 0; k < keep.size(); k++) out->t[s * keep.size() + k] = d.t[(size_t)s * B + keep[k]];
    return true;
  }
  // Hopcroft's partition refinement: a block that was split off (or the smaller half) becomes a
  // splitter; the predecessors of a splitter under one class are marked at the front of their
  // blocks and the marked part, where it is not the whole block, becomes a block of its own.
  // A long chain (`a{2000}`) costs a step per state, not a round per state.
  bool minimise(const RxDfa &d, std::vector<uint32_t> *block, uint32_t *n_blocks) {
    const uint32_t n = d.n(), B = d.nb;
    if (!spend(2 * (uint64_t)n * B)) return false;
    // predecessors: inv[inv_off[c * n + t] ..] = the states s with t[s][c] == t
    std::vector<uint32_t> inv_off((size_t)n * B + 1, 0), inv((size_t)n * B);
    for (uint32_t s = 0; s < n; s++)
      for (uint32_t c = 0; c < B; c++) inv_off[(size_t)c * n + d.t[(size_t)s * B + c] + 1]++;
    for (size_t i = 0; i < (size_t)n * B; i++) inv_off[i + 1] += inv_off[i];
    {
      std::vector<uint32_t> at(inv_off.begin(), inv_off.end() - 1);
      for (uint32_t s = 0; s < n; s++)
        for (uint32_t c = 0; c < B; c++) inv[at[(size_t)c * n + d.t[(size_t)s * B + c]]++] = s;
    }
    // the partition: elems holds the states block by block; a block is elems[first .. first + size)
    std::vector<uint32_t> elems(n), loc(n), blk(n), first, size, marked, work, touched, members;
    std::vector<uint8_t> in_work;
    uint32_t n_acc = 0;
    for (uint32_t s = 0; s < n; s++) n_acc += d.acc[s];
    uint32_t at_acc = 0, at_rej = n_acc;
    for (uint32_t s = 0; s < n; s++) {
      const uint32_t i = d.acc[s] ? at_acc++ : at_rej++;
      elems[i] = s;
      loc[s] = i;
    }
    auto new_block = [&](uint32_t f, uint32_t sz) {
      first.push_back(f);
      size.push_back(sz);
      marked.push_back(0);
      in_work.push_back(0);
      for (uint32_t i = f; i < f + sz; i++) blk[elems[i]] = (uint32_t)first.size() - 1;
      return (uint32_t)first.size() - 1;
    };
    if (n_acc) new_block(0, n_acc);
    if (n_acc < n) new_block(n_acc, n - n_acc);
    for (uint32_t b2 = 0; b2 < first.size(); b2++) {
      work.push_back(b2);
      in_work[b2] = 1;
    }
    while (!work.empty()) {
      const uint32_t a = work.back();
      work.pop_back();
      in_work[a] = 0;
      members.assign(elems.begin() + first[a], elems.begin() + first[a] + size[a]);   // the splitter as it is now
      if (!spend(members.size() + B)) return false;
      for (uint32_t c = 0; c < B; c++) {
        touched.clear();
        for (uint32_t t : members) {
          const size_t i0 = inv_off[(size_t)c * n + t], i1 = inv_off[(size_t)c * n + t + 1];
          if (!spend(1 + (i1 - i0))) return false;
          for (size_t i = i0; i < i1; i++) {
            const uint32_t p = inv[i], bp = blk[p];                 // a state is a predecessor of one t only: marked once
            if (marked[bp] == 0) touched.push_back(bp);
            const uint32_t to = first[bp] + marked[bp]++, from = loc[p], q = elems[to];
            elems[to] = p;
            loc[p] = to;
            elems[from] = q;
            loc[q] = from;
          }
        }
        for (uint32_t bp : touched) {
          const uint32_t m = marked[bp];
          marked[bp] = 0;
          if (m == size[bp]) continue;                               // every member steps into the splitter
          const uint32_t f = first[bp];
          first[bp] += m;
          size[bp] -= m;
          const uint32_t nb2 = new_block(f, m);                      // the marked part
          const uint32_t add = in_work[bp] ? nb2 : (size[nb2] <= size[bp] ? nb2 : bp);
          work.push_back(add);
          in_work[add] = 1;
        }
      }
    }
    *block = blk;
    *n_blocks = (uint32_t)first.size();
    return true;
  }

  // ---- the whole compilation ----
  // out: the table's words; empty for a pattern that matches nothing without being an error
  int compile(const uint8_t *s, uint64_t n, std::vector<uint32_t> *out) {
    out->clear();
    uint64_t i = 0;
    while (i < n) {
      uint32_t l;
      const uint32_t cp = utf8_decode(s, n, i, &l);
      if (cp == kUcBad) return kRxOk;               // not strict UTF-8: matches nothing
      cps.push_back(cp);
      at.push_back(i);
      i += l;
    }
    at.push_back(n);
    const int root = cps.empty() ? (int)add(RxNode::EPS) : parse_union();   // the empty pattern: the empty string
    if (ok() && more()) fail(kRxSyntax);            // an unbalanced ')'
    if (!ok()) return status;
    // base classes: every range end cuts [0, 0x10FFFF]
    cuts.push_back(0);
    for (const RxNode &nd : nodes)
      for (const RxRange &r : nd.set) {
        cuts.push_back(r.lo);
        if (r.hi < kRxMaxCp) cuts.push_back(r.hi + 1);
      }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    cuts.push_back(kRxMaxCp + 1);
    if (nb() > kRxMaxBaseClasses) return fail(kRxUnsupported), status;
    RxDfa work, d;
    std::vector<uint32_t> cmap, cmap2, block;
    uint32_t n_blocks = 0;
    if (!dfa_of((uint32_t)root, &work) || !merge_classes(work, &cmap, &d) || !minimise(d, &block, &n_blocks))
      return status;
    // the quotient, then classes again: merged states can make columns equal
    RxDfa q;
    q.nb = d.nb;
    q.acc.assign(n_blocks, 0);
    q.t.assign((size_t)n_blocks * d.nb, 0);
    for (uint32_t st = 0; st < d.n(); st++) {
      q.acc[block[st]] = d.acc[st];
      for (uint32_t c = 0; c < d.nb; c++) q.t[(size_t)block[st] * d.nb + c] = block[d.t[(size_t)st * d.nb + c]];
    }
    RxDfa m;
    if (!merge_classes(q, &cmap2, &m)) return status;
    const uint32_t C = m.nb, S = m.n(), start = block[0];
    // the dead block: no accepting state ahead (at most one after minimisation)
    std::vector<uint8_t> live(S, 0);
    for (bool grew = true; grew;) {
      grew = false;
      if (!spend((uint64_t)S * C)) return status;
      for (uint32_t st = 0; st < S; st++) {
        if (live[st]) continue;
        bool l = m.acc[st];
        for (uint32_t c = 0; c < C && !l; c++) l = live[m.t[(size_t)st * C + c]];
        if (l) live[st] = 1, grew = true;
      }
    }
    // canonical numbers: dead = 0, live states breadth-first from the start by class order
    std::vector<uint32_t> num(S, 0), order;
    if (live[start]) {
      num[start] = 1;
      order.push_back(start);
      for (size_t k = 0; k < order.size(); k++)
        for (uint32_t c = 0; c < C; c++) {
          const uint32_t t = m.t[(size_t)order[k] * C + c];
          if (live[t] && !num[t]) {
            order.push_back(t);
            num[t] = (uint32_t)order.size();
          }
        }
    }
    const uint32_t NS = (uint32_t)order.size() + 1;
    if (C > kRxMaxClasses || NS > 0xFFFFu) return fail(kRxUnsupported), status;
    std::vector<uint16_t> trans((size_t)NS * C, 0);
    std::vector<uint32_t> accept((NS + 31) / 32, 0);
    for (size_t k = 0; k < order.size(); k++) {
      const uint32_t st = order[k], id = (uint32_t)k + 1;
      if (m.acc[st]) accept[id >> 5] |= 1u << (id & 31u);
      for (uint32_t c = 0; c < C; c++) {
        const uint32_t t = m.t[(size_t)st * C + c];
        trans[(size_t)id * C + c] = (uint16_t)(live[t] ? num[t] : 0);
      }
    }
    // the shortest member, and the longest where the live states have no cycle
    uint32_t min_cps = kRxNoMax, max_cps = 0;
    if (NS > 1) {
      std::vector<uint32_t> dist(NS, kRxNoMax), bfs{1};
      dist[1] = 0;
      for (size_t k = 0; k < bfs.size(); k++) {
        const uint32_t st = bfs[k];
        if (((accept[st >> 5] >> (st & 31u)) & 1u) && dist[st] < min_cps) min_cps = dist[st];
        for (uint32_t c = 0; c < C; c++) {
          const uint32_t t = trans[(size_t)st * C + c];
          if (t && dist[t] == kRxNoMax) {
            dist[t] = dist[st] + 1;
            bfs.push_back(t);
          }
        }
      }
      // longest path by depth-first search, iterative: colour 1 = on the path (a cycle when met again)
      std::vector<uint32_t> longest(NS, 0), it(NS, 0), path{1};
      std::vector<uint8_t> colour(NS, 0);
      colour[1] = 1;
      bool cyclic = false;
      if (!spend((uint64_t)NS * C)) return status;
      while (!path.empty() && !cyclic) {
        const uint32_t st = path.back();
        if (it[st] < C) {
          const uint32_t t = trans[(size_t)st * C + it[st]++];
          if (!t) continue;
          if (colour[t] == 1) cyclic = true;
          else if (colour[t] == 0) {
            colour[t] = 1;
            path.push_back(t);
          }
        } else {
          uint32_t best = 0;
          for (uint32_t c = 0; c < C; c++) {
            const uint32_t t = trans[(size_t)st * C + c];
            if (t) best = std::max(best, longest[t] + 1);
          }
          longest[st] = best;
          colour[st] = 2;
          path.pop_back();
        }
      }
      max_cps = cyclic ? kRxNoMax : longest[1];
    }
    // the class maps: merged class of a base class, then ASCII and the merged non-ASCII intervals
    auto final_class = [&](uint32_t base_class) { return cmap2[cmap[base_class]]; };
    uint8_t ascii[128];
    for (uint32_t cp = 0; cp < 128; cp++) ascii[cp] = (uint8_t)final_class(class_of(cp));
    std::vector<uint32_t> iv_start;
    std::vector<uint8_t> iv_class;
    for (uint32_t b = class_of(128); b < nb(); b++) {
      const uint8_t c = (uint8_t)final_class(b);
      if (!iv_class.empty() && iv_class.back() == c) continue;
      iv_start.push_back(std::max<uint32_t>(cuts[b], 128));
      iv_class.push_back(c);
    }
    // a language's classes are numbered by their first code point whatever the pattern cut: renumber
    std::vector<int> ren(C, -1);
    uint32_t next = 0;
    for (uint32_t cp = 0; cp < 128; cp++)
      if (ren[ascii[cp]] < 0) ren[ascii[cp]] = (int)next++;
    for (uint8_t c : iv_class)
      if (ren[c] < 0) ren[c] = (int)next++;
    const uint32_t n_iv = (uint32_t)iv_start.size();
    const size_t words = kRxHeaderWords + 32 + n_iv + ((n_iv + 3) >> 2) + (((size_t)NS * C + 1) >> 1) + accept.size();
    if (words * 4 > kRxMaxTableBytes) return fail(kRxUnsupported), status;
    out->assign(words, 0);
    uint32_t *w = out->data();
    w[0] = (uint32_t)words;
    w[1] = NS | (C << 16);
    w[2] = n_iv;
    w[3] = NS > 1 ? 1u : 0u;
    w[4] = min_cps;
    w[5] = max_cps;
    uint8_t *b8 = reinterpret_cast<uint8_t *>(w + kRxHeaderWords);
    for (uint32_t cp = 0; cp < 128; cp++) b8[cp] = (uint8_t)ren[ascii[cp]];
    uint32_t *pw = w + kRxHeaderWords + 32;
    for (uint32_t k = 0; k < n_iv; k++) pw[k] = iv_start[k];
    pw += n_iv;
    b8 = reinterpret_cast<uint8_t *>(pw);
    for (uint32_t k = 0; k < n_iv; k++) b8[k] = (uint8_t)ren[iv_class[k]];
    pw += (n_iv + 3) >> 2;
    uint16_t *t16 = reinterpret_cast<uint16_t *>(pw);
    for (uint32_t st = 0; st < NS; st++)
      for (uint32_t c = 0; c < C; c++) t16[(size_t)st * C + ren[c]] = trans[(size_t)st * C + c];
    pw += ((size_t)NS * C + 1) >> 1;
    for (size_t k = 0; k < accept.size(); k++) pw[k] = accept[k];
    return kRxOk;
  }
};

// Pattern -> table.  kRxOk with an empty table: a pattern that is not strict
// UTF-8 (it matches nothing).  The empty language compiles to a table whose
// start state is 0, the empty pattern to the table of the empty string.
// *err_at (may be NULL): the byte offset of an error.
inline int rx_compile(const uint8_t *s, uint64_t n, std::vector<uint32_t> *table, uint64_t *err_at) {
  RxCompiler c;
  const int rc = c.compile(s, n, table);
  if (rc != kRxOk) table->clear();
  if (err_at) *err_at = c.err_at;
  return rc;
}

// is a compiled table staged nowhere?  (no table, the empty language, or the empty string alone: a term has a code point)
inline bool rx_table_matches_nothing(const std::vector<uint32_t> &table) {
  return table.empty() || table[3] == 0 || table[5] == 0;
}

}  // namespace tfidf
