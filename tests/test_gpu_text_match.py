"""TEXT_MATCH on the device: the keyword leaf of hr_filter_eval_expr_dev (filter_expr_kernel<true>, csrc/filter.h).

Part 1 calls the C ABI on synthetic word CSRs, against numpy: an entry is a hit iff its id is a set member, a hit belongs to
the row whose span holds it, a row passes iff it is below tok_rows and owns at least m hits.  Garbage-filled outputs with a
canary word behind each, every word of `mask` and `undecided`, the bits at and beyond n_rows and both counts are compared.

Part 2 goes through DeviceFilters and MilvusIndexManager on a small collection appended in three pieces, against
filters.evaluate (held to the written-out restatement by tests/test_text_match_host.py) and the oracle."""
import asyncio
import functools

import numpy as np
import pytest

import oracle
from advanced_rag import MilvusIndexManager
from advanced_rag import _native as nat
from advanced_rag import filters as F
from test_text_match_host import make_contents, restated

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOKENS, MATCH, OP_IN = nat.HR_COL_TOKENS, nat.HR_OP_MATCH, nat.HR_OP_IN
I64, STR = nat.HR_COL_I64, nat.HR_COL_STR16
EQ, LT = nat.FILTER_OPS["=="], nat.FILTER_OPS["<"]
P_AND, P_OR, P_NOT = nat.HR_FILTER_AND, nat.HR_FILTER_OR, nat.HR_FILTER_NOT
GARBAGE, CANARY = 0xA5A5A5A5A5A5A5A5, 0x5EEDC0DE0DDBA115
DEVICE = "cuda:0"
TOP_ID = (1 << 31) - 2
UNIVERSE = 3000                      # ordinary words are ids 1 .. UNIVERSE - 1; 0 and TOP_ID are planted or drawn on purpose
LONG = 5000


# ---- sets: n_set in {0, 1, 2, 1000, 16384}, members 0 and 2^31 - 2 ----------------------------------------------------------------
def _sets():
    rng = np.random.default_rng(41)
    s1000 = np.sort(np.concatenate([[0, TOP_ID], rng.choice(np.arange(1, UNIVERSE), 998, replace=False)]))
    s16384 = np.sort(np.concatenate([[0, TOP_ID], np.arange(1, UNIVERSE), np.arange(UNIVERSE, UNIVERSE + 16384 - 2 - (UNIVERSE - 1))]))
    s1025 = np.sort(np.concatenate([[0, TOP_ID], rng.choice(np.arange(1, UNIVERSE), 1023, replace=False)]))
    sets = {"empty": [], "zero": [0], "top": [TOP_ID], "ends": [0, TOP_ID], "pair": [7, 11], "s1000": s1000, "s16384": s16384,
            "s1025": s1025, "few": [3, 5, 7, 11, 13, 17, 19]}
    return {k: np.asarray(v, dtype=np.int32) for k, v in sets.items()}


SETS = _sets()
# every n_set with m in {1, 2, n_set, n_set + 1}
COMBOS = [("empty", 1), ("empty", 2), ("zero", 1), ("zero", 2), ("top", 1), ("ends", 1), ("ends", 2), ("ends", 3), ("pair", 2),
          ("s1000", 1), ("s1000", 2), ("s1000", 1000), ("s1000", 1001), ("s16384", 1), ("s16384", 2), ("s16384", 16384),
          ("s16384", 16385)]


def test_the_sets_are_what_the_contract_asks_for():
    assert sorted({len(m) for m in SETS.values()}) == [0, 1, 2, 7, 1000, 1025, 16384]
    for m in SETS.values():
        assert m.dtype == np.int32 and (np.diff(m.astype(np.int64)) > 0).all()
    for name in ("s1000", "s16384", "s1025", "ends"):
        assert SETS[name][0] == 0 and SETS[name][-1] == TOP_ID


# ---- word CSRs ------------------------------------------------------------------------------------------------------------------------
def _row(rng, k):
    """k draws -> ascending unique ids: mostly ordinary words, now and then 0 or TOP_ID."""
    ids = rng.integers(1, UNIVERSE, k)
    kind = rng.random(k)
    ids = np.where(kind < 0.1, 0, np.where(kind < 0.2, TOP_ID, ids))
    return np.unique(ids)


def _long_row(rng):
    """5 000 ids that hold every member of s1000 (m = n_set can be met) beside 4 000 words no set holds."""
    row = np.union1d(SETS["s1000"], rng.choice(np.arange(UNIVERSE + 20000, UNIVERSE + 30000), LONG - 1000, replace=False))
    assert row.shape[0] == LONG
    return row


def make_csr(pattern, tok_rows, seed):
    """-> (indptr int64 [tok_rows + 1], ids int32, planted rows or None)."""
    rng = np.random.default_rng(seed)
    rows, planted = [], None
    empty = np.zeros(0, dtype=np.int64)
    if pattern == "empty":
        rows = [empty] * tok_rows
    elif pattern == "ones":
        rows = [_row(rng, 1) for _ in range(tok_rows)]
    elif pattern == "alternating":
        rows = [_row(rng, 1) if r % 2 else empty for r in range(tok_rows)]
    elif pattern == "gaps":           # >= 130 consecutive empty rows between non-empty ones
        rows = [_row(rng, 1 + int(rng.integers(0, 7))) if r % 131 == 0 or r == tok_rows - 1 else empty for r in range(tok_rows)]
    elif pattern.startswith("long@"):
        at = tok_rows - 1 if pattern == "long@last" else int(pattern[5:])
        rows = [_long_row(rng) if r == at else _row(rng, int(rng.integers(0, 4))) for r in range(tok_rows)]
    elif pattern == "random":
        rows = [_row(rng, int(rng.integers(0, 8))) for _ in range(tok_rows)]
    elif pattern == "planted":
        # ordinary words only, rows 1 .. 135 empty; then 0 (always a row's FIRST entry) and TOP_ID (always its LAST) are planted:
        # the first entry after the run of empty rows, the last entry of row 63 (tok_rows > 140: that row is empty, so the last
        # entry of the row before the run, row 0), the first entry of row 64 is in the run too -> rows 191 / 192 carry the pair
        # at the next 64-row edge; and the very last entry of the array
        rows = [np.unique(rng.integers(1, UNIVERSE, 1 + int(rng.integers(0, 7)))) for _ in range(tok_rows)]
        planted = {}
        if tok_rows > 140:
            for r in range(1, 136):
                rows[r] = empty
            planted[136] = 0
        lo_edge, hi_edge = (63, 64) if tok_rows <= 140 else (191, 192)
        if tok_rows > hi_edge:
            planted[lo_edge], planted[hi_edge] = TOP_ID, 0
        if tok_rows:
            planted[tok_rows - 1] = TOP_ID if planted.get(tok_rows - 1) is None else planted[tok_rows - 1]
        for r, word in planted.items():
            rows[r] = np.union1d(rows[r], [word])
        if tok_rows:
            assert planted[tok_rows - 1] == 0 or rows[tok_rows - 1][-1] == TOP_ID
    else:
        raise AssertionError(pattern)
    lens = np.asarray([len(r) for r in rows], dtype=np.int64)
    indptr = np.zeros(tok_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    ids = np.concatenate(rows).astype(np.int32) if tok_rows and indptr[-1] else np.zeros(0, dtype=np.int32)
    return indptr, ids, planted


def match_ref(indptr, ids, n_rows, members, m):
    """The contract in numpy: hits per row, counted; a row at or beyond tok_rows holds nothing."""
    tok_rows = indptr.shape[0] - 1
    owner = np.repeat(np.arange(tok_rows), np.diff(indptr))
    hits = np.bincount(owner[np.isin(ids, members)], minlength=max(tok_rows, 1))[:tok_rows]
    out = np.zeros(n_rows, dtype=bool)
    k = min(n_rows, tok_rows)
    out[:k] = hits[:k] >= m
    return out


class Buffers:
    """[mask words | canary | undecided words | canary] and [counts[2] | canary[2]], refilled with garbage before every call;
    a tombstone mask, an int64 column and a key column for the leaves beside the keyword leaf."""

    def __init__(self, n):
        rng = np.random.default_rng(7000 + n)
        dev = torch.device(DEVICE)
        self.n, self.n_words = n, (n + 63) // 64
        w = self.n_words
        tmpl = np.full(2 * (w + 1), GARBAGE, dtype=np.uint64)
        tmpl[w] = tmpl[2 * w + 1] = CANARY
        self.tmpl = torch.from_numpy(tmpl.view(np.int64)).to(dev)
        self.out = torch.empty_like(self.tmpl)
        self.ctmpl = torch.tensor([0x5A5A5A5A, -7, 0x0DDBA115, -0x0DDBA115], dtype=torch.int32, device=dev)
        self.counts = torch.empty_like(self.ctmpl)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.dead = rng.random(n) < 0.3
        bits = np.ones(((n + 7) // 8) * 8, dtype=bool)
        bits[:n] = self.dead
        self.d_dead = torch.from_numpy(np.packbits(bits, bitorder="little")).to(dev)
        self.i64 = rng.integers(0, 6, max(n, 1)).astype(np.int64)
        self.d_i64 = torch.from_numpy(self.i64).to(dev)
        self.key = np.where((rng.random(max(n, 1)) < 0.4)[:, None], np.array([[5, 9]], dtype=np.uint64),
                            rng.integers(0, 1 << 62, (max(n, 1), 2)).astype(np.uint64))
        self.d_key = torch.from_numpy(np.ascontiguousarray(self.key).view(np.int64)).to(dev)
        self.d_in_set = torch.tensor([1, 3, 4], dtype=torch.int64, device=dev)

    def pointers(self):
        base = self.out.data_ptr()
        return base, base + 8 * (self.n_words + 1), self.counts.data_ptr()

    def refill(self):
        self.out.copy_(self.tmpl)
        self.counts.copy_(self.ctmpl)

    def read(self):
        o, w = self.out.cpu().numpy().view(np.uint64), self.n_words
        return o[:w].copy(), o[w], o[w + 1:2 * w + 1].copy(), o[2 * w + 1], self.counts.cpu().numpy()

    def words(self, rows):
        bits = np.zeros(self.n_words * 64, dtype=bool)
        bits[:self.n] = rows
        return np.packbits(bits, bitorder="little").view("<u8")

    def untouched(self):
        return torch.equal(self.out, self.tmpl) and torch.equal(self.counts, self.ctmpl)

    # leaves beside the keyword leaf: (leaf, lo, hi)
    def in_leaf(self):
        leaf = nat.FilterLeaf()
        leaf.term.kind, leaf.term.op, leaf.term.col = I64, OP_IN, self.d_i64.data_ptr()
        leaf.set, leaf.n_set = self.d_in_set.data_ptr(), 3
        has = np.isin(self.i64[:self.n], [1, 3, 4])
        return leaf, has, has

    def tie_leaf(self):
        """key == (5, 9): unknown for the rows that hold that key, false for the others."""
        leaf = nat.FilterLeaf()
        leaf.term.kind, leaf.term.op, leaf.term.col = STR, EQ, self.d_key.data_ptr()
        leaf.term.key[0], leaf.term.key[1] = 5, 9
        tie = (self.key[:self.n, 0] == 5) & (self.key[:self.n, 1] == 9)
        return leaf, np.zeros(self.n, bool), tie


class Csr:
    def __init__(self, indptr, ids):
        dev = torch.device(DEVICE)
        self.indptr, self.ids, self.tok_rows = indptr, ids, indptr.shape[0] - 1
        self.d_indptr = torch.from_numpy(indptr).to(dev)
        # the word pointer may be 0 only without rows: rows that are all empty still get an array (of one unused word)
        self.d_ids = torch.from_numpy(ids if ids.shape[0] else np.full(1, 12345, np.int32)).to(dev) if self.tok_rows else None
        self._hits = {}

    def leaf(self, set_name, m):
        leaf = nat.FilterLeaf()
        t = leaf.term
        t.kind, t.op, t.col, t.ival = TOKENS, MATCH, self.d_indptr.data_ptr(), m
        t.key[0], t.key[1] = (self.d_ids.data_ptr() if self.d_ids is not None else 0), self.tok_rows
        t.dval, t.fval = float("nan"), float("nan")               # fields the leaf does not read
        leaf.n_set = len(SETS[set_name])
        leaf.set = d_set(set_name).data_ptr() if leaf.n_set else None
        return leaf

    def ref(self, n_rows, set_name, m):
        return match_ref(self.indptr, self.ids, n_rows, SETS[set_name], m)


@functools.lru_cache(maxsize=None)
def d_set(name):
    return torch.from_numpy(SETS[name]).to(torch.device(DEVICE))


def kleene(program, pairs):
    stack = []
    for code in program:
        if code >= 0:
            stack.append(pairs[code])
        elif code == P_NOT:
            lo, hi = stack.pop()
            stack.append((~hi, ~lo))
        else:
            (lo_b, hi_b), (lo_a, hi_a) = stack.pop(), stack.pop()
            stack.append((lo_a & lo_b, hi_a & hi_b) if code == P_AND else (lo_a | lo_b, hi_a | hi_b))
    (lo, hi), = stack
    return lo, hi


def check(b, leaves, program, pairs, tombstones=False, what=""):
    """One launch, held to the Kleene evaluation of the leaves' (lo, hi) pairs; -> the raw read-back."""
    b.refill()
    mask, und, counts = b.pointers()
    nat.filter_eval_expr_dev(leaves, program, b.n, b.d_dead.data_ptr() if tombstones else 0, mask, und, counts, b.stream)
    got = b.read()
    lo, hi = kleene(program, pairs)
    alive = ~b.dead if tombstones else np.ones(b.n, bool)
    keep, undecided = alive & lo, alive & hi & ~lo
    for name, words, rows in (("mask", got[0], keep), ("undecided", got[2], undecided)):
        want = b.words(rows)
        if not np.array_equal(words, want):
            w = int(np.nonzero(words != want)[0][0])
            bit = int(words[w] ^ want[w])
            bit = (bit & -bit).bit_length() - 1
            pytest.fail(f"{name}: {what}: row {64 * w + bit} (n_rows {b.n}): expected {int(want[w]) >> bit & 1}")
        if b.n % 64:
            assert int(words[-1]) >> (b.n % 64) == 0, f"{name}: bits at or beyond n_rows are set: {what}"
    assert got[1] == CANARY and got[3] == CANARY, f"a word behind an output buffer was written: {what}"
    assert got[4].tolist() == [int(keep.sum()), int(undecided.sum())] + b.ctmpl.cpu().tolist()[2:], f"counts: {what}"
    return got, keep


# ---- part 1: the kernel through the C ABI ------------------------------------------------------------------------------------------
N_ROWS = [1, 63, 64, 65, 130, 4099]
PATTERNS = ["empty", "ones", "alternating", "gaps", "long@0", "long@63", "long@64", "long@last", "random", "planted"]
FULL = ("random", "long@63", "planted")          # every (set, m) on these; five of them, rotating, on the others


def _tok_rows(n):
    return [t for t in (0, n - 70, n, n + 5) if t >= 0]


@pytest.mark.parametrize("n", N_ROWS)
def test_one_keyword_leaf_equals_numpy(gpu, n):
    b = Buffers(n)
    launches = kept_some = 0
    for tok_rows in _tok_rows(n):
        for p, pattern in enumerate(PATTERNS):
            if pattern.startswith("long@") and pattern != "long@last" and int(pattern[5:]) >= tok_rows:
                continue
            if pattern == "long@last" and tok_rows == 0:
                continue
            indptr, ids, planted = make_csr(pattern, tok_rows, seed=1000 * n + 10 * tok_rows + p)
            csr = Csr(indptr, ids)
            combos = COMBOS if pattern in FULL else [COMBOS[(p * 7 + tok_rows + 5 * j) % len(COMBOS)] for j in range(5)]
            if pattern.startswith("long@"):
                combos = list(combos) + [("s1000", 1000), ("s1000", 1001)]
            for set_name, m in combos:
                want = csr.ref(n, set_name, m)
                what = f"{pattern}, tok_rows {tok_rows}, set {set_name}, m {m}"
                _, keep = check(b, [csr.leaf(set_name, m)], [0], [(want, want)], what=what)
                launches += 1
                kept_some += bool(keep.any())
                if pattern.startswith("long@") and (set_name, m) == ("s1000", 1000):      # the long row holds the whole set
                    at = tok_rows - 1 if pattern == "long@last" else int(pattern[5:])
                    assert keep.tolist() == [r == at for r in range(n)], what
                if pattern.startswith("long@") and (set_name, m) == ("s1000", 1001):
                    assert not keep.any(), what
            if pattern == "planted":
                rows0 = {r for r, word in planted.items() if word == 0 and r < n}
                rows_top = {r for r, word in planted.items() if word == TOP_ID and r < n}
                assert set(np.flatnonzero(csr.ref(n, "zero", 1))) == rows0
                assert set(np.flatnonzero(csr.ref(n, "top", 1))) == rows_top
                assert set(np.flatnonzero(csr.ref(n, "ends", 1))) == rows0 | rows_top
                if tok_rows > 192 and n > 192:
                    assert {136, 192} <= rows0 and {191, tok_rows - 1} & rows_top
    assert launches > 50 and (kept_some > 10 or n == 1)


def test_planted_rows_are_where_the_comment_says():
    indptr, ids, planted = make_csr("planted", 4099, 3)
    assert planted == {136: 0, 191: TOP_ID, 192: 0, 4098: TOP_ID}
    assert (np.diff(indptr)[1:136] == 0).all() and ids[indptr[136]] == 0 and ids[indptr[192]] == 0
    assert ids[indptr[192] - 1] == TOP_ID and ids[-1] == TOP_ID
    indptr, ids, planted = make_csr("planted", 130, 3)
    assert planted == {63: TOP_ID, 64: 0, 129: TOP_ID} and ids[indptr[64] - 1] == TOP_ID and ids[indptr[64]] == 0


@pytest.mark.parametrize("n", [65, 4099])
def test_programs_with_two_keyword_leaves_and_other_leaves(gpu, n):
    b = Buffers(n)
    a_csr = Csr(*make_csr("random", n, seed=n + 1)[:2])
    b_csr = Csr(*make_csr("gaps", n + 5, seed=n + 2)[:2])             # another CSR with another tok_rows in the same program
    specs = [(a_csr, "s1000", 2), (a_csr, "few", 1), (b_csr, "s1025", 1), (a_csr, "ends", 1)]      # all sets share 64 KiB
    leaves = [c.leaf(s, m) for c, s, m in specs]
    pairs = [(c.ref(n, s, m),) * 2 for c, s, m in specs]
    in_leaf, in_lo, in_hi = b.in_leaf()
    tie_leaf, tie_lo, tie_hi = b.tie_leaf()
    leaves += [in_leaf, tie_leaf]
    pairs += [(in_lo, in_hi), (tie_lo, tie_hi)]
    programs = {
        "a and b": [0, 1, P_AND], "a or b": [0, 1, P_OR], "not a": [0, P_NOT], "a and not b": [0, 1, P_NOT, P_AND],
        "not (a or c)": [0, 2, P_OR, P_NOT], "b and a (counters are reset between the leaves)": [1, 0, P_AND],
        "(a or d) and (b or c)": [0, 3, P_OR, 1, 2, P_OR, P_AND],
        "a and in": [0, 4, P_AND], "in or a": [4, 0, P_OR], "not in and not a": [4, P_NOT, 0, P_NOT, P_AND],
        "a or tie": [0, 5, P_OR], "a and tie": [0, 5, P_AND], "not (tie and b) or d": [5, 1, P_AND, P_NOT, 3, P_OR],
        "tie or (in and a)": [5, 4, 0, P_AND, P_OR],
    }
    for name, program in programs.items():
        for tombstones in (False, True):
            got, keep = check(b, leaves, program, pairs, tombstones, what=f"{name}, tombstones {tombstones}")
            again, _ = check(b, leaves, program, pairs, tombstones, what=name)
            for x, y in zip(got, again):                               # two runs are byte-identical
                assert np.array_equal(x, y), name
    # the undecided bits appear only where Kleene says so: under `or`, a row the keyword leaf passes is decided
    a_rows, tie = pairs[0][0], tie_hi
    b.refill()
    mask, und, counts = b.pointers()
    nat.filter_eval_expr_dev(leaves, programs["a or tie"], n, 0, mask, und, counts, b.stream)
    got = b.read()
    assert np.array_equal(got[2], b.words(tie & ~a_rows)) and np.array_equal(got[0], b.words(a_rows))
    assert (tie & a_rows).any() and (tie & ~a_rows).any()
    nat.filter_eval_expr_dev(leaves, programs["a and tie"], n, 0, mask, und, counts, b.stream)
    got = b.read()
    assert np.array_equal(got[2], b.words(tie & a_rows)) and not got[0].any()


def test_every_wave_makes_two_trips(gpu):
    """300 032 rows are 4 688 words; 1 025 members are more than 4 KiB of sets, so the grid is capped at 1 024 blocks of 4
    waves: every wave takes at least two words, and ends and counters are rewritten between them."""
    n = 300_032
    rng = np.random.default_rng(300)
    lens = rng.integers(0, 8, n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    # ids ascending and unique within a row: a sorted random base per row plus the position inside the row
    base = np.repeat(rng.integers(0, UNIVERSE - 8, n), lens)
    ids = (base + (np.arange(indptr[-1]) - np.repeat(indptr[:-1], lens))).astype(np.int32)
    csr, b = Csr(indptr, ids), Buffers(n)
    assert (n + 63) // 64 > 1024 * 4 and len(SETS["s1025"]) * 4 > 4096
    for m in (1, 3):
        want = csr.ref(n, "s1025", m)
        assert 1000 < want.sum() < n - 1000
        got, _ = check(b, [csr.leaf("s1025", m)], [0], [(want, want)], tombstones=(m == 3), what=f"multi-trip, m {m}")
        again, _ = check(b, [csr.leaf("s1025", m)], [0], [(want, want)], tombstones=(m == 3), what="multi-trip again")
        for x, y in zip(got, again):
            assert np.array_equal(x, y)


def test_refusals_leave_the_buffers_alone(gpu):
    n = 65
    b = Buffers(n)
    csr = Csr(*make_csr("random", n, seed=5)[:2])
    mask, und, counts = b.pointers()
    good = lambda: csr.leaf("few", 1)

    def changed(**fields):
        leaf = good()
        for k, v in fields.items():
            if k in ("set", "n_set"):
                setattr(leaf, k, v)
            elif k in ("key0", "key1"):
                leaf.term.key[int(k[3])] = v
            else:
                setattr(leaf.term, k, v)
        return leaf

    over = changed(n_set=16385)
    cap_a, cap_b = csr.leaf("s16384", 1), csr.leaf("few", 1)
    in_leaf = b.in_leaf()[0]
    bad_calls = {
        "tokens with op in": ([changed(op=OP_IN)], [0], ValueError, "bad filter term 0"),
        "tokens with op ==": ([changed(op=EQ)], [0], ValueError, "bad filter term 0"),
        "int64 with op match": ([changed(kind=I64)], [0], ValueError, "bad filter term 0"),
        "string key with op match": ([good(), changed(kind=STR)], [0, 1, P_AND], ValueError, "bad filter term 1"),
        "m = 0": ([changed(ival=0)], [0], ValueError, "bad filter term 0"),
        "m = -1": ([changed(ival=-1)], [0], ValueError, "bad filter term 0"),
        "null indptr": ([changed(col=None)], [0], ValueError, "bad filter term 0"),
        "misaligned indptr": ([changed(col=csr.d_indptr.data_ptr() + 4)], [0], ValueError, "bad filter term 0"),
        "misaligned words": ([changed(key0=csr.d_ids.data_ptr() + 2)], [0], ValueError, "bad filter term 0"),
        "no words but rows": ([changed(key0=0)], [0], ValueError, "bad filter term 0"),
        "negative tok_rows": ([changed(key1=(1 << 64) - 1)], [0], ValueError, "bad filter term 0"),
        "members without a set": ([changed(set=None)], [0], ValueError, "bad filter term 0"),
        "a set without members": ([changed(n_set=0)], [0], ValueError, "bad filter term 0"),
        "negative n_set": ([changed(n_set=-1)], [0], ValueError, "bad filter term 0"),
        "misaligned set": ([changed(set=d_set("few").data_ptr() + 2)], [0], ValueError, "bad filter term 0"),
        "one id over the budget": ([over], [0], nat.HbmRagError, "up to 65536 bytes"),
        "two keyword sets over the budget together": ([cap_a, cap_b], [0, 1, P_OR], nat.HbmRagError, "up to 65536 bytes"),
        "a keyword set and an in set over the budget together": ([cap_a, in_leaf], [0, 1, P_OR], nat.HbmRagError, "up to 65536 bytes"),
        "the in set first": ([in_leaf, cap_a], [0, 1, P_OR], nat.HbmRagError, "up to 65536 bytes"),
    }
    for name, (leaves, program, error, message) in bad_calls.items():
        b.refill()
        with pytest.raises(error, match=message):
            nat.filter_eval_expr_dev(leaves, program, n, 0, mask, und, counts, b.stream)
        assert b.untouched(), name
    # the conjunction entry point keeps refusing the kind
    b.refill()
    with pytest.raises(ValueError, match="bad filter term 0"):
        nat.filter_eval_dev([good().term], n, 0, mask, und, counts, b.stream)
    assert b.untouched()
    want = csr.ref(n, "few", 1)
    check(b, [good()], [0], [(want, want)], what="a good call after the refusals")
    # no rows and no words: the word pointer may be 0
    none = Csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    check(b, [none.leaf("few", 1)], [0], [(np.zeros(n, bool),) * 2], what="tok_rows 0, word pointer 0")
    assert nat.load_library().hr_version() >= 11400


# ---- part 2: through DeviceFilters and the manager -----------------------------------------------------------------------------------
N, D, V, NNZ = 3011, 8, 500, 8
APPENDS = (700, 800, 1511)
P16 = "0123456789abcdef"
DOCS = [P16 + "-tail-A", P16 + "-tail-B", P16, "doc7", "zzz", ""]
EXPRS = [
    'TEXT_MATCH(content, "timeout")',
    'text_match(content, "TIMEOUT, Retry!")',
    'TEXT_MATCH(content, "timeout retry disk", minimum_should_match=2)',
    'TEXT_MATCH(content, "timeout retry disk", minimum_should_match=3)',
    'TEXT_MATCH(content, "timeout retry disk", minimum_should_match=4)',
    'TEXT_MATCH(content, "")',
    'TEXT_MATCH(content, "nosuchword")',
    'TEXT_MATCH(content, "nosuchword disk", minimum_should_match=2)',
    'not TEXT_MATCH(content, "confidential")',
    'TEXT_MATCH(content, "über 日本語") or chunk_index == 3',
    'TEXT_MATCH(content, "don\'t") and entropy >= 0.5',
    'TEXT_MATCH(content, "raft") and not (text_match(content, "leader quorum", minimum_should_match=2) or doc_id in ["doc7", "zzz"])',
    f'doc_id == "{P16}-tail-A" or TEXT_MATCH(content, "snapshot index")',
    f'doc_id != "{P16}-tail-B" and not TEXT_MATCH(content, "vote follower heartbeat", minimum_should_match=2)',
]


def _bits(mask_u8):
    return np.unpackbits(mask_u8.cpu().numpy(), bitorder="little").astype(bool)


@pytest.fixture(scope="module")
def collection():
    rng = np.random.default_rng(3011)
    X = rng.standard_normal((N, D)).astype(np.float32)
    idx = np.sort(np.argpartition(rng.random((N, V)), NNZ - 1, axis=1)[:, :NNZ], axis=1).astype(np.int32).reshape(-1)
    val = np.abs(rng.standard_normal(N * NNZ)).astype(np.float32)
    ptr = np.arange(N + 1, dtype=np.int64) * NNZ
    ids = [f"c{r}" for r in range(N)]
    cols = dict(doc_id=[DOCS[p] for p in rng.integers(0, len(DOCS), N).tolist()],
                entropy=(rng.integers(0, 11, N) / 10).astype(np.float32).tolist(), chunk_index=rng.integers(0, 6, N).tolist())
    return X, (ptr, idx, val), ids, cols, make_contents(N, 77)


def _host_columns(cols, contents, rows):
    return {"content": [contents[r] for r in rows], "doc_id": np.asarray([cols["doc_id"][r] for r in rows]),
            "entropy": np.asarray([cols["entropy"][r] for r in rows], dtype=np.float32),
            "chunk_index": np.asarray([cols["chunk_index"][r] for r in rows], dtype=np.int64)}


def test_masks_follow_appends_deletes_and_compaction(gpu, collection):
    X, (ptr, idx, val), ids, cols, contents = collection
    m = MilvusIndexManager(semantic_dim=D, sparse_dim=V, dtype="float32", enable_domain=False)
    try:
        def check_all(rows, deleted=None):
            n = len(rows)
            host = _host_columns(cols, contents, rows)
            for expr in EXPRS:
                want = F.evaluate(expr, host, n)
                if deleted is not None:
                    want = want & ~deleted
                got = m._global_device_mask(expr)
                got = np.ones(n, bool) if got is None else _bits(got)
                assert np.array_equal(got[:n], want) and not got[n:].any(), (expr, n)

        lo = 0
        for step in APPENDS:
            hi = lo + step
            m.add_rows(X[lo:hi], (ptr[lo:hi + 1], idx, val), ids=ids[lo:hi], contents=contents[lo:hi],
                       **{k: v[lo:hi] for k, v in cols.items()})
            m.finalize()
            check_all(list(range(hi)))                       # the word mirror grows under the expressions
            lo = hi
        dev = m._dev_filters
        assert dev.stats["match_leaves"] == 3 * sum(e.lower().count("text_match(") for e in EXPRS)
        assert dev.word_mirror_bytes > 0
        # the written-out restatement, once, beside filters.evaluate
        got = _bits(m._global_device_mask(EXPRS[2]))[:N]
        assert np.array_equal(got, restated(contents, "timeout retry disk", 2)) and 0 < got.sum() < N

        # a repeated expression uploads nothing: the manager keeps the mask, and the evaluator has every row already
        before = dict(dev.stats)
        m._global_device_mask(EXPRS[0])
        assert dev.stats == before
        dev.evaluate(EXPRS[0], N)
        assert dev.stats["uploaded_bytes"] == before["uploaded_bytes"] and dev.stats["match_leaves"] == before["match_leaves"] + 1

        # the tie under `or`: the rows that share 16 bytes with the literal are settled on the full strings
        before = dev.stats["undecided_rows"]
        mask, kept = dev.evaluate(EXPRS[12], N)
        want = F.evaluate(EXPRS[12], _host_columns(cols, contents, range(N)), N)
        assert np.array_equal(_bits(mask)[:N], want) and kept == int(want.sum())
        shares = np.asarray([d.startswith(P16) for d in cols["doc_id"]])
        hit = restated(contents, "snapshot index")
        assert dev.stats["undecided_rows"] - before == int((shares & ~hit).sum()) > 0     # decided where the keyword leaf is true

        # delete by keyword, then compact: the survivors are renumbered and the mirror is rebuilt
        gone = restated(contents, "confidential")
        assert 0 < gone.sum() < N
        asyncio.run(m.delete_by_filter("semantic_index", 'TEXT_MATCH(content, "Confidential!")'))
        check_all(list(range(N)), deleted=gone)
        m.compact()
        assert m._dev_filters is None
        left = np.flatnonzero(~gone).tolist()
        check_all(left)
        assert m._dev_filters.stats["match_leaves"] > 0
    finally:
        asyncio.run(m.close())


def test_searches_under_a_keyword_filter_equal_the_oracle(gpu, collection):
    X, (ptr, idx, val), ids, cols, contents = collection
    rng = np.random.default_rng(78)
    m = MilvusIndexManager(semantic_dim=D, sparse_dim=V, dtype="float32", enable_domain=False)
    try:
        lo = 0
        for step in APPENDS:
            hi = lo + step
            m.add_rows(X[lo:hi], (ptr[lo:hi + 1], idx, val), ids=ids[lo:hi], contents=contents[lo:hi],
                       **{k: v[lo:hi] for k, v in cols.items()})
            m.finalize()
            lo = hi
        expr = 'TEXT_MATCH(content, "raft leader quorum", minimum_should_match=2) or (text_match(content, "disk") and chunk_index < 3)'
        keep = restated(contents, "raft leader quorum", 2) | (restated(contents, "disk") & (np.asarray(cols["chunk_index"]) < 3))
        assert 100 < keep.sum() < N - 100
        m8 = np.packbits(keep, bitorder="little")
        k, top_k = 20, 10
        Q = rng.standard_normal((2, D)).astype(np.float32)
        SQ = [(np.sort(rng.choice(V, 12, replace=False)).astype(np.int32), np.abs(rng.standard_normal(12)).astype(np.float32))
              for _ in range(2)]
        sp = {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}
        di, ds = oracle.dense_search(X, Q, k, oracle.COSINE, m8)
        si, ss = oracle.sparse_search(ptr, idx, val, SQ, k, 0.2, m8)
        for b in range(2):
            hits = asyncio.run(m.search(Q[b], "semantic_index", k, expr))
            assert [h["_row"] for h in hits] == di[b].tolist() and [h["score"] for h in hits] == [float(x) for x in ds[b]]
            sq = {"indices": SQ[b][0].tolist(), "values": SQ[b][1].tolist()}
            hits = asyncio.run(m.search(sq, "sparse_index", k, expr, sp))
            live = si[b] >= 0
            assert live.any() and [h["_row"] for h in hits] == si[b][live].tolist()
            assert [h["score"] for h in hits] == [float(x) for x in ss[b][live]]
            res = asyncio.run(m.hybrid_search(Q[b], sq, top_k, expr, (0.7, 0.3), sparse_params=sp))
            assert res is not None, "the hybrid round did not answer"
            fi, fs, _ = oracle.rrf(di[b][di[b] >= 0], si[b][si[b] >= 0], (), 0.7, 0.3, 0.0, 60)
            assert [hit["_row"] for hit, _, _ in res] == fi[:top_k].tolist()
        assert m._dev_filters.stats["match_leaves"] == 2              # one evaluation: the mask is kept per expression
        # query: the rows in ascending order, and their count
        assert [h["id"] for h in asyncio.run(m.query("semantic_index", expr))] == [ids[r] for r in np.flatnonzero(keep)]
        assert asyncio.run(m.query("semantic_index", expr, ["count(*)"])) == [{"count(*)": int(keep.sum())}]
        # search by primary key: the ranking of the entity's own vector under the same mask
        seeds = [5, 1234, N - 1]
        lists = asyncio.run(m.search_by_ids([ids[r] for r in seeds], "semantic_index", top_k, expr))
        ri, rs = oracle.dense_search(X, X[seeds], top_k, oracle.COSINE, m8)
        for got, want_rows in zip(lists, ri):
            assert [h["_row"] for h in got] == want_rows.tolist() and all(keep[h["_row"]] for h in got)
    finally:
        asyncio.run(m.close())


def test_caps_and_refusals_upload_nothing(gpu, collection):
    X, (ptr, idx, val), ids, cols, contents = collection
    m = MilvusIndexManager(semantic_dim=D, sparse_dim=V, dtype="float32", enable_domain=False)
    try:
        m.add_rows(X[:700], (ptr[:701], idx, val), ids=ids[:700], contents=[f"w{r} common" for r in range(700)],
                   **{k: v[:700] for k, v in cols.items()})
        m.finalize()
        dev = m._filters_on_device()
        ok = 'TEXT_MATCH(content, "' + " ".join(f"w{r}" for r in range(0, 700, 2)) + '", minimum_should_match=1)'
        got = _bits(m._global_device_mask(ok))[:700]
        assert got.tolist() == [r % 2 == 0 for r in range(700)]
        before = dict(dev.stats)
        many_leaves = " or ".join(f'TEXT_MATCH(content, "w{i}")' for i in range(17))
        many_words = " or ".join('TEXT_MATCH(content, "' + " ".join(f"w{r}" for r in range(700)) + '")' for _ in range(15)) \
            + ' or chunk_index in [' + ", ".join(str(i) for i in range(3000)) + "]"      # 15 * 2 800 + 24 000 bytes > 64 KiB
        for bad, message in ((many_leaves, "up to 16 terms"), (many_words, "16384 words"),
                             ('TEXT_MATCH(doc_id, "a")', "TEXT_MATCH"), ('TEXT_MATCH(content, "a", minimum_should_match=0)', "minimum_should_match")):
            with pytest.raises(ValueError, match=message):
                m._global_device_mask(bad)
        assert dev.stats == before
    finally:
        asyncio.run(m.close())
