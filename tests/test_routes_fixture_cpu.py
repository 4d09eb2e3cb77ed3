"""The route corpus reaches the cases it was built for (routes_ref.py), checked
against the references alone: what keeps the sweeps of
test_gpu_routes_incremental.py from passing vacuously.  The states are the
document lists those tests commit: 8300 documents and 200 more (shape A: block
0 is kept), the same with 50 new words in the 200, and 16 500 documents grown
to 3 * 8192 + 1 (shape B: blocks 0 and 1 are kept)."""
import functools

import fuzzy_ref as F
import routes_ref as RR
from routes_ref import BASE, BLOCK, END_B, FIRST_A, FIRST_B, APPEND_A


@functools.lru_cache(maxsize=None)
def state(name):
    return RR.expected({"a0": BASE[:FIRST_A], "a1": BASE[:FIRST_A + APPEND_A], "c1": BASE[:FIRST_A] + RR.new_batch(),
                        "b0": BASE[:FIRST_B], "b1": BASE[:END_B]}[name])


# (state after the append, its state before, documents of the kept blocks, documents of the appended batch)
SHAPES = [("a1", "a0", range(0, BLOCK), range(FIRST_A, FIRST_A + APPEND_A)),
          ("b1", "b0", range(0, 2 * BLOCK), range(FIRST_B, END_B))]


def both_sides(docs, kept, appended):
    docs = set(docs)
    return any(d in docs for d in kept) and any(d in docs for d in appended)


def test_every_probe_hits_a_kept_block_and_the_appended_batch():
    for after, _, kept, appended in SHAPES:
        w = state(after).want
        for p in RR.PHRASES:
            docs = [d for d, _, _ in w["phrase", p]] + [d for s in RR.SLOPS for d, _, _ in w["slop", p, s]]
            assert both_sides(docs, kept, appended), (after, p)
        for p in RR.WILDCARDS:
            assert both_sides(w["wild_docs", p][0], kept, appended), (after, p)
        for p in RR.REGEXES:
            assert both_sides(w["regex_docs", p][0], kept, appended), (after, p)
        for t in RR.FUZZY:
            for e, p in RR.FUZZY_PARAMS:
                assert both_sides([d for d, _ in w["fuzzy_hits", t, e, p][0]], kept, appended), (after, t, e, p)
        seeds = state(after).seeds
        for d in seeds:                                                        # every seed selects terms and has hits
            assert any(w["mlt_terms", d, i][0] and w["mlt_hits", d, i] for i in range(len(RR.MLT_PARAMS))), (after, d)
        assert any(d in kept for d in seeds) and any(d in appended for d in seeds)
        assert any(d in range(BLOCK, FIRST_A) for d in seeds)                  # shape A's tail


def test_the_append_changes_the_fuzzy_order_and_the_expansions_largest_df():
    for after, before, _, _ in SHAPES:
        a, b = state(after).want, state(before).want
        order = [[t for t, _, _ in w["fuzzy_terms", RR.FUZ[0], 2, 0, 10][0]] for w in (b, a)]
        assert sorted(order[0]) == sorted(order[1]) == sorted(RR.FUZ) and order[0] != order[1], after
        assert order[0][:3] != order[1][:3]                                    # ... within the first max_out = 3 too
        top = [max(df for _, df, _, _ in w["fuzzy_expand", RR.FUZ[0], 2, 0][0]) for w in (b, a)]
        assert top[0] != top[1]                                                # the idf every clause is weighted with
        assert b["fuzzy_hits", RR.FUZ[0], 2, 0] != a["fuzzy_hits", RR.FUZ[0], 2, 0]


def test_the_append_moves_a_pivot_across_the_mlt_filters():
    for after, before, _, _ in SHAPES:
        a, b = state(after), state(before)
        seed = b.seeds[0]
        assert a.texts[seed] == b.texts[seed] == RR.SEEDS[0]
        for i in (0, 1):                                                       # the defaults, and max_df = 4
            sel = [[t for t, _, _, _ in x.want["mlt_terms", seed, i][0]] for x in (b, a)]
            assert set(sel[0]) != set(sel[1]), (after, i)                      # a pivot word came or went
            assert (set(sel[0]) ^ set(sel[1])) <= {RR.PIV_A, RR.PIV_B}
            assert b.want["mlt_hits", seed, i] != a.want["mlt_hits", seed, i]
    assert (state("a0").vocab[RR.PIV_A], state("a1").vocab[RR.PIV_A]) == (3, 5)
    assert (state("b0").vocab[RR.PIV_B], state("b1").vocab[RR.PIV_B]) == (4, 6)


def test_a_wildcard_and_two_regexes_match_old_and_new_words():
    w = state("c1").want
    old, new = {RR.c(i) for i in range(1, 401)}, set(RR.NEW_WORDS)
    assert new <= set(state("c1").vocab) and not new & set(state("a1").vocab)
    for key in (("wild_terms", RR.OLD_AND_NEW, 1024), ("regex_terms", RR.REGEXES[1], 1024),
                ("regex_terms", RR.REGEXES[-1], 1024)):
        terms = {t for t, _ in w[key][0]}
        assert terms & old and terms & new, key
    near = {t for t, _, _ in F.expected(state("c1").vocab, RR.c(7), 2, 0, 1 << 20)[0]}
    assert near & old and near & new


def test_the_hashed_terms_and_the_phrases():
    for t in (RR.LONG_TERM, RR.N1, RR.N2):
        assert len(t) > 16 and t.isascii()
    assert F.osa(RR.LONG_TERM, RR.N1) == F.osa(RR.LONG_TERM, RR.N2) == 1 and F.osa(RR.N1, RR.N2) == 2
    a0, a1, b1, c1 = state("a0"), state("a1"), state("b1"), state("c1")
    first = lambda x, t: min(d for d, ts in enumerate(x.term_sets) if t in ts)      # noqa: E731
    assert first(a1, RR.LONG_TERM) < BLOCK and RR.N1 not in a1.vocab and first(c1, RR.N1) >= FIRST_A
    assert set(b1.vocab) - set(state("b0").vocab) == {RR.N2} and first(b1, RR.N2) >= FIRST_B
    for x in (a1, b1):
        w = x.want
        assert any(f > 1 for _, _, f in w["phrase", RR.M1 + b" " + RR.M2])
        exact = {d for d, _, _ in w["slop", RR.M1 + b" " + RR.M2, 0]}
        assert exact == {d for d, _, _ in w["phrase", RR.M1 + b" " + RR.M2]}
        for s in (1, 2):
            assert {d for d, _, _ in w["slop", RR.M1 + b" " + RR.M2, s]} - exact                  # slop-only matches
        assert not w["phrase", RR.M1 + b" " + RR.M3] and w["slop", RR.M1 + b" " + RR.M3, 1]
    # no word is new in documents 8300..8499 or in the 100 behind them: such a commit moves no column
    assert set(a0.vocab) == set(a1.vocab) and set(F.oracle_vocab(c1.texts + BASE[FIRST_A + APPEND_A:][:100])) == set(c1.vocab)
    assert set(F.oracle_vocab([t for i, t in enumerate(BASE[:FIRST_A]) if i not in (0, 4, 13)])) == \
        set(a0.vocab)                                                          # ... nor goes one with the deleted three
    # the positions the route documents were put at
    assert [BASE[i] in RR.ROUTE for i in (3, BLOCK - 1, BLOCK, FIRST_A - 1, FIRST_A, FIRST_A + APPEND_A - 1, 12000,
                                          FIRST_B - 1, FIRST_B, END_B - 1)] == [True] * 10
    assert BASE[END_B - 1] == RR.P_FULL and END_B - 1 == 3 * BLOCK


def test_every_probes_answer_differs_between_two_states():
    """A probe: a route and its pattern, term, query or seed, whatever the other parameters (a phrase with its
    slops).  The seed of the last batch of shape B exists in one state only; every other probe has two or more."""
    names = ("a0", "a1", "c1", "b1")
    probes, once = {}, set()
    for key in set().union(*(state(n).want for n in names)):
        answers = [state(n).want[key] for n in names if key in state(n).want]
        probe = ("phrase" if key[0] == "slop" else key[0], key[1])
        if len(answers) == 1:
            once.add(probe)
        probes.setdefault(probe, []).append(any(x != answers[0] for x in answers[1:]))
    last_seed = BASE.index(RR.SEEDS[3])
    assert once == {("mlt_terms", last_seed), ("mlt_hits", last_seed)} and len(probes) > 60
    for probe in once:
        del probes[probe]
    same = [p for p, differs in probes.items() if not any(differs)]
    assert not same, same
