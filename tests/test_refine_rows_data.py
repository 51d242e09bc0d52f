"""The case builders of tests/refine_rows_data.py, shown on the CPU to have teeth before they go to a GPU: the oracle's
scores of the constructed rows equal a closed form in numpy fp64, the lists the device form has to prove keep 1 % between
consecutive distinct scores, the order-sensitive rows of case B really change their float32 score when the additions are
reordered, and the BM25 rows of case D are long."""
import functools

import numpy as np
import pytest

import oracle
import refine_rows_data as R


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def get_case(name):
    if name == "A":
        return R.case_a()
    if name == "A_masked":
        return R.case_a(masked=True)
    if name == "B":
        return R.case_b()
    if name == "D":
        return R.case_d()
    return R.case_c(int(name[2:]))


CONSTRUCTED = ["A", "A_masked", "B"] + [f"C_{V}" for V in R.C_VOCABS]


@pytest.mark.parametrize("name", CONSTRUCTED)
def test_closed_form_scores_equal_the_oracle(name):
    case = get_case(name)
    for batch in case.batches:
        for qi, qv in batch.queries:
            got = oracle.sparse_scores(case.indptr, case.idx, case.val, qi, qv)
            want = R.closed_form_scores(case, qi, qv)
            bad = np.nonzero(bits(got) != bits(want))[0]
            assert bad.size == 0, (name, batch.name, bad[:5], got[bad[:5]], want[bad[:5]])


def test_a_scores_spell_out_the_positions():
    """multiplier * (sum of the bits of the row's matching positions), exactly, for every length and query."""
    case = get_case("A")
    for batch in case.batches:
        for qi, qv in batch.queries:
            got = oracle.sparse_scores(case.indptr, case.idx, case.val, qi, qv)
            for r, L in case.meta["layout"]:
                want = R.a_expected(L, case.meta["mult"][r], qi, qv) if L else np.float32(0)
                assert bits(got[r]) == bits(want), (batch.name, r, L, got[r], want)
                if L:     # and the sum is exact: every position is a bit of its own in the float32 score
                    q = dict(zip(qi.tolist(), qv.astype(np.float64).tolist()))
                    exact = case.meta["mult"][r] * sum(q.get(R.a_term(L, p), 0.0) for p in R.a_positions(L))
                    assert float(want) == exact
    # the placements the case promises
    rows = dict(case.meta["layout"])
    assert all(rows[640 + i] > 128 for i in range(16)) and 640 % 64 == 0
    assert all(rows[r] > 128 for r in range(1021, 1030)) and 1024 % 64 == 0
    assert rows[R.N_DOCS - 1] == 2500 and rows[16384 + 13] == 2500
    assert (rows[5000], rows[5001], rows[5002], rows[5003], rows[5004]) == (0, 1000, 0, 2500, 0)
    assert {L for _, L in case.meta["layout"]} == set(R.A_LENGTHS)
    assert R.N_DOCS % 64 != 0 and R.N_DOCS % 16 != 0


@pytest.mark.parametrize("name", CONSTRUCTED)
def test_one_percent_between_consecutive_distinct_scores(name):
    """On the oracle's scores alone: the top k + 1 of every list the device form must prove."""
    case = get_case(name)
    alive = None if case.mask is None else np.unpackbits(case.mask, bitorder="little")[:R.N_DOCS].astype(bool)
    for batch in case.batches:
        for j, (qi, qv) in enumerate(batch.queries):
            if j in batch.signed:
                continue
            sc = oracle.sparse_scores(case.indptr, case.idx, case.val, qi, qv).astype(np.float64)
            if alive is not None:
                sc = sc[alive]
            sc = np.sort(sc[sc > 0])[::-1]
            for k in batch.ks:
                top = sc[:k + 1]
                if top.size > k:
                    assert top[k - 1] != top[k], (name, batch.name, j, k, "a tie at the cut")
                for hi, lo in zip(top[:-1], top[1:]):
                    if hi == lo:
                        continue
                    if batch.near_ties and batch.near_ties[0] <= lo and hi <= batch.near_ties[1]:
                        continue          # case B's rows, an ulp apart on purpose and strictly inside the list
                    assert hi - lo >= 0.01 * hi, (name, batch.name, j, k, hi, lo)
                if batch.near_ties:       # ... strictly inside: neither the last place nor the first one out
                    for s in top[max(k - 1, 0):k + 1]:
                        assert not (batch.near_ties[0] <= s <= batch.near_ties[1])


def test_b_rows_depend_on_the_order_of_the_additions():
    """With numpy alone: every row's float32 score changes when the matches of a segment are summed pairwise, and every
    row whose four entries span two segments changes when the segments are summed in another order.  (Four entries
    inside ONE segment cannot depend on the order of the segments; the assertion for them is that they do not.)"""
    seen_across = 0
    for name, first, roles, want in R.b_blocks():
        pos, prod = R.b_matches(first, roles)
        canon = R.score_canonical(prod)
        assert bits(canon) == bits(want), name
        assert bits(R.score_pairwise(pos, prod)) != bits(canon), name
        if len(set((pos // 64).tolist())) > 1:
            seen_across += 1
            assert bits(R.score_segments_reversed(pos, prod)) != bits(canon), name
        else:
            assert bits(R.score_segments_reversed(pos, prod)) == bits(canon), name
        # each product is the product of the two float32 weights the row and the query hold
        for role in roles:
            assert float(np.float32(R.B_DOC_W[role])) * float(np.float32(R.B_QUERY_W[role])) == R.B_PRODUCT[role]
    assert seen_across == 9
    # both orientations at every placement, and the block in the order the issue states it
    names = [n for n, *_ in R.b_blocks()]
    for where in ("inside_20", "inside_200", "across_64", "across_128", "across_192"):
        assert f"down_{where}" in names and f"up_{where}" in names
    # the rows as stored give the same scores through the closed form
    case = get_case("B")
    qi, qv = case.batches[0].queries[0]
    by_name = {n: w for n, _, _, w in case.meta["blocks"]}
    for r, n in case.meta["names"].items():
        assert bits(R.closed_form(*case.rows[r], qi, qv)) == bits(by_name[n]), (r, n)


@pytest.mark.parametrize("V", R.C_VOCABS)
def test_c_aliases_are_presented(V):
    case = get_case(f"C_{V}")
    base = case.meta["base"]
    assert 0 in base
    held = set(np.concatenate([t for t, _ in case.rows.values()]).tolist())
    assert {0, V - 1, V - 2} <= held
    q_base, q_alias, q_ends, q_signed, q_pairs = case.batches[0].queries
    assert {0, V - 1, V - 2} <= set(q_ends[0].tolist())
    assert (q_signed[1] < 0).sum() == 1
    if V > 32768:
        # rows that hold only an alias of a query term: same filter bit, score 0; and the rows that hold the term score
        alias_only = [r for r, terms in case.meta["specs"].items() if all(t >= 32768 for t in terms)]
        assert alias_only
        sc = R.closed_form_scores(case, *q_base)
        assert all(sc[r] == 0 for r in alias_only)
        assert all(sc[r] > 0 for r, terms in case.meta["specs"].items() if any(t in base for t in terms))
        assert any((t - 32768) in set(q_base[0].tolist()) for r in alias_only for t in case.meta["specs"][r])
    if V >= 65536:
        for form, batch in zip(R.FORM_TERMS, case.batches):
            ti = batch.queries[4][0]
            assert ti.size == {"hash512": 128, "hash1024": 256, "sorted": 300}[form]
            low = ti[ti < 32768]
            assert np.isin(low + 32768, ti).all() and 2 * low.size == ti.size    # congruent modulo 32768 in pairs
    for form, batch in zip(R.FORM_TERMS.values(), case.batches):
        assert all(len(q[0]) >= form for q in batch.queries[:4])


@pytest.mark.parametrize("V", [65536 + 3, 1 << 20])
def test_c_aliases_reach_every_lookup_form(V):
    """A lookup that lost its final equality test would score a row that holds no query term: under every lookup form,
    for some query whose list the device form must prove, at the k that leaves room for such a row."""
    case = get_case(f"C_{V}")
    for form, batch in zip(R.FORM_TERMS, case.batches):
        caught = 0
        for j, (qi, qv) in enumerate(batch.queries):
            if j in batch.signed:
                continue
            assert (qv > 0).all()
            held = set(qi.tolist())
            scoring = sum(1 for t, _ in case.rows.values() if held & set(t.tolist()))
            assert scoring < max(batch.ks)        # a row that wrongly scores above 0 enters the longer list
            for t, w in case.rows.values():
                if not held & set(t.tolist()) and any(R.c_taken_for_present(qi, form, x) for x in t.tolist()):
                    assert (w > 0).all()
                    caught += 1
        assert caught >= 1, (V, form)


def test_forms_and_batch_sizes_straddle_the_thresholds():
    assert R.FORM_TERMS["hash512"] <= 128 < R.FORM_TERMS["hash1024"] <= 256 < R.FORM_TERMS["sorted"]
    # the batches lie on either side of the threshold finish_fused_ok holds today, read from its source
    assert R.FUSED_MIN_QUERIES == R.fused_threshold_in_source()
    assert R.BATCH_SIZES == (R.FUSED_MIN_QUERIES - 1, R.FUSED_MIN_QUERIES)
    qs, pick = R.batch_of(get_case("A").batches[0], 63)
    assert len(qs) == 63 and set(pick) == {0, 1, 2, 3}


def test_d_rows_are_long():
    case = get_case("D")
    lens = np.diff(case.indptr)
    assert lens.size == R.D_DOCS
    assert (lens > 128).sum() * 3 >= lens.size, lens[:10]
    assert lens.max() <= 600 and case.idx.max() < R.D_V
    assert [len(q[0]) > 256 for q in case.batches[0].queries] == [True] * 5 + [False] * 2
