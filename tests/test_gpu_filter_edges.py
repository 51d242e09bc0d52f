"""The device filter (filter_eval_kernel, entry point hr_filter_eval_dev) off the 64-row grid and at the value edges.

Part 1 calls the C ABI with synthetic device columns and holds every word of `mask` and `undecided`, the bits at and beyond
n_rows, the two counts and a canary word behind each buffer to a plain numpy restatement of the contract of
include/hbmrag.h / csrc/filter.h: int64 against an integer as int64, int64 against a float as float64, float32 against
the float32 literal, string keys as unsigned lexicographic order on two words; keep = not deleted, no term failed, no
term tied; undecided = not deleted, no term failed, some string term tied.  Row counts sit on, one off and between the
64-row words, plus one shape two words (the last ragged) beyond a full trip of the capped grid.  Column values are the
ones a wrong comparison gets wrong: +-2^53 +- 1 and the int64 extremes, NaN / +-inf / +-0 / the smallest denormal / one
ulp either side of a literal, keys and literal keys with the top bit of either word set (a signed compare inverts those).

Part 2 takes the same edges through MilvusIndexManager: a 4133-row collection filled in three appends (the HBM copies of
the columns start at 1024 rows and grow twice, with a filter evaluated in between), non-ASCII / 16-byte-straddling /
NUL-holding strings, NaN and infinities in a FLOAT payload, tombstones whose count is no multiple of 8 -- the device mask,
filters.evaluate and oracle.filter_mask agree bit for bit, and the dense, sparse and hybrid searches under such a mask
return the oracle's ids and scores."""
import asyncio
import functools

import numpy as np
import pytest

import oracle
from advanced_rag import MilvusIndexManager
from advanced_rag import _native as nat
from advanced_rag import filters as F

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I64, I64F, F32, STR = nat.HR_COL_I64, nat.HR_COL_I64_VS_F64, nat.HR_COL_F32, nat.HR_COL_STR16
KIND_NAME = {I64: "int64 vs int", I64F: "int64 vs float64", F32: "float32", STR: "key16"}
OP_NAME = {v: k for k, v in nat.FILTER_OPS.items()}
EQ, NE, LT, LE, GT, GE = (nat.FILTER_OPS[o] for o in ("==", "!=", "<", "<=", ">", ">="))
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
TOP = 1 << 63
GRID_ROWS = 4096 * 4 * 64          # rows of one trip of the capped launch (hr_filter_eval_dev: 4096 blocks x 4 waves)
N_ROWS = [0, 1, 7, 8, 63, 64, 65, 127, 129, 255, 257, 1000, GRID_ROWS + 69]
GARBAGE, CANARY = 0xA5A5A5A5A5A5A5A5, 0x5EEDC0DE0DDBA115
DEVICE = "cuda:0"

# ---- literals ------------------------------------------------------------------------------------------------------------
LIT32 = np.float32(0.30000001192092896)
LITERALS = {
    I64: [0, 2, -1, 2**53, 2**53 + 1, -(2**53 + 1), INT64_MIN, INT64_MAX],
    # 2.5 / -0.0: between and on integers; 2^53: where the column's conversion starts to round; +-1e19, +-inf: beyond every
    # int64; 2^63 = (double)INT64_MAX; nan: only != passes
    I64F: [2.5, -0.0, 9007199254740992.0, 1e19, -1e19, float("inf"), float("nan"), 9223372036854775808.0, float("-inf")],
    F32: [0.30000001192092896, 0.0, float("inf"), float("nan"), 1e-45],
    # (word 0, word 1): top bit of word 0 set; top bit of word 1 set; plain ASCII ("doc123"); the empty string
    STR: [(TOP | 0x1234567890ABCDEF, 0x0FEDCBA987654321), (0x6162636465666768, TOP | 0x0000000000000001),
          (int.from_bytes(b"doc123\0\0", "big"), 0), (0, 0)],
}
I64_VALUES = [0, 1, -1, 2, 3, 2**53 - 1, -(2**53 - 1), 2**53, -(2**53), 2**53 + 1, -(2**53 + 1), INT64_MIN, INT64_MAX,
              INT64_MIN + 1, INT64_MAX - 1, 2**53 + 2, -(2**53 + 2)]
F32_VALUES = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, LIT32, np.nextafter(LIT32, np.float32(1)),
              np.nextafter(LIT32, np.float32(0)), 1.0, -1.0, np.finfo(np.float32).max, np.finfo(np.float32).tiny]


def _key_values():
    """Per literal key: the key itself (a tie), one that differs only in word 1 (below and above), one that differs from it
    only in the top bit of word 1, and one only in the top bit of word 0."""
    out = []
    for k0, k1 in LITERALS[STR]:
        out += [(k0, k1), (k0, (k1 + 1) % (1 << 64)), (k0, (k1 - 1) % (1 << 64)), (k0, k1 ^ TOP), (k0 ^ TOP, k1)]
    return out


def _spread(rng, n, values, random_rows, dtype):
    """A column of n rows: 70 % of the rows draw one of `values`, the others are random; the LAST rows hold every value
    once (as many as fit), so that the ragged last word of every shape holds the edge values too."""
    values = np.asarray(values, dtype=dtype)
    col = np.where((rng.random(n) < 0.7).reshape((n,) + (1,) * (values.ndim - 1)), values[rng.integers(0, len(values), n)],
                   random_rows)
    m = min(n, len(values))
    if m:
        col[n - m:] = values[:m]
    return np.ascontiguousarray(col.astype(dtype))


class Case:
    """Host and device columns of one row count, and the output buffers: [mask words | canary | undecided words | canary]
    in one tensor, [counts[2] | canary[2]] in another, refilled with garbage before every call."""

    def __init__(self, n):
        rng = np.random.default_rng(1000 + n % 9973)
        self.n, self.n_words = n, (n + 63) // 64
        small = rng.integers(-4, 5, n)
        wide = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
        self.i64 = _spread(rng, n, I64_VALUES, np.where(rng.random(n) < 0.5, small, wide), np.int64)
        self.f32 = _spread(rng, n, F32_VALUES, rng.standard_normal(n).astype(np.float32), np.float32)
        self.key = _spread(rng, n, _key_values(), rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64), np.uint64)
        self.k0, self.k1 = np.ascontiguousarray(self.key[:, 0]), np.ascontiguousarray(self.key[:, 1])
        dead = rng.random(n) < 0.3
        bits = np.ones(((n + 7) // 8) * 8, dtype=bool)          # the pad bits of the last byte are set: they are no rows
        bits[:n] = dead
        self.dead, self.dead_bytes = dead, np.packbits(bits, bitorder="little")
        assert self.dead_bytes.size == (n + 7) // 8
        dev = torch.device(DEVICE)

        def up(a, dtype):    # at least one element: a column pointer may not be null, even for 0 rows
            t = torch.zeros(max(a.size, 1), dtype=dtype, device=dev)
            if a.size:
                t[:a.size] = torch.from_numpy(a.reshape(-1).view(np.int64 if a.dtype == np.uint64 else a.dtype)).to(dev)
            return t
        self.d_cols = {I64: up(self.i64, torch.int64), F32: up(self.f32, torch.float32), STR: up(self.key, torch.int64)}
        self.d_cols[I64F] = self.d_cols[I64]
        self.d_dead = torch.from_numpy(self.dead_bytes).to(dev)
        w = self.n_words
        tmpl = np.full(2 * (w + 1), GARBAGE, dtype=np.uint64)
        tmpl[w] = tmpl[2 * w + 1] = CANARY
        self.tmpl = torch.from_numpy(tmpl.view(np.int64)).to(dev)
        self.out = torch.empty_like(self.tmpl)
        self.ctmpl = torch.tensor([0x5A5A5A5A, -7, 0x0DDBA115, -0x0DDBA115], dtype=torch.int32, device=dev)
        self.counts = torch.empty_like(self.ctmpl)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    # -- the kernel ---------------------------------------------------------------------------------------------------------
    def term(self, kind, op, lit, col_ptr=None):
        t = nat.FilterTerm()
        t.kind, t.op = kind, op
        t.col = self.d_cols[kind].data_ptr() if col_ptr is None else col_ptr
        # the literal fields this kind does not read hold values that would change the verdict if it did read them
        t.ival, t.dval, t.fval, t.key[0], t.key[1] = -1, float("nan"), float("nan"), (1 << 64) - 1, (1 << 64) - 1
        if kind == I64:
            t.ival = lit
        elif kind == I64F:
            t.dval = lit
        elif kind == F32:
            t.fval = float(np.float32(lit))
        elif kind == STR:
            t.key[0], t.key[1] = lit
        return t

    def pointers(self):
        base = self.out.data_ptr()
        return base, base + 8 * (self.n_words + 1), self.counts.data_ptr()

    def refill(self):
        self.out.copy_(self.tmpl)
        self.counts.copy_(self.ctmpl)

    def read(self):
        o, w = self.out.cpu().numpy().view(np.uint64), self.n_words
        return o[:w], o[w], o[w + 1:2 * w + 1], o[2 * w + 1], self.counts.cpu().numpy()

    def launch(self, terms, tombstones):
        self.refill()
        mask, und, counts = self.pointers()
        nat.filter_eval_dev([self.term(*t) for t in terms], self.n, self.d_dead.data_ptr() if tombstones else 0, mask, und,
                            counts, self.stream)
        return self.read()

    # -- the contract, in numpy ---------------------------------------------------------------------------------------------
    def ref_term(self, kind, op, lit):
        """-> (verdict per row where the term decides, tie per row)."""
        n = self.n
        if kind == STR:
            k0, k1, l0, l1 = self.k0, self.k1, np.uint64(lit[0]), np.uint64(lit[1])
            tie = (k0 == l0) & (k1 == l1)
            less = (k0 < l0) | ((k0 == l0) & (k1 < l1))           # unsigned, word 0 first
            verdict = {EQ: np.zeros(n, bool), NE: np.ones(n, bool), LT: less, LE: less, GT: ~less, GE: ~less}[op]
            return verdict, tie
        if kind == I64:
            a, b = self.i64, np.int64(lit)
        elif kind == I64F:
            a, b = self.i64.astype(np.float64), np.float64(lit)
        else:
            with np.errstate(over="ignore"):
                a, b = self.f32, np.float32(lit)
        with np.errstate(invalid="ignore"):
            verdict = {EQ: a == b, NE: a != b, LT: a < b, LE: a <= b, GT: a > b, GE: a >= b}[op]
        return verdict, np.zeros(n, bool)

    def ref(self, terms, tombstones):
        """-> (keep, undecided) per row."""
        fail = self.dead.copy() if tombstones else np.zeros(self.n, bool)
        maybe = np.zeros(self.n, bool)
        for t in terms:
            verdict, tie = self.ref_term(*t)
            maybe |= tie
            fail |= ~tie & ~verdict
        return ~fail & ~maybe, ~fail & maybe

    def words(self, rows):
        bits = np.zeros(self.n_words * 64, dtype=bool)
        bits[:self.n] = rows
        return np.packbits(bits, bitorder="little").view("<u8")

    def check(self, terms, tombstones):
        what = " and ".join(f"[{KIND_NAME[k]}] col {OP_NAME[o]} {lit!r}" for k, o, lit in terms) + \
            f" (n_rows={self.n}, tombstones={tombstones})"
        mask, canary_m, und, canary_u, counts = self.launch(terms, tombstones)
        keep, undecided = self.ref(terms, tombstones)
        for name, got, rows in (("mask", mask, keep), ("undecided", und, undecided)):
            want = self.words(rows)
            if not np.array_equal(got, want):
                w = int(np.nonzero(got != want)[0][0])
                bit = int(got[w] ^ want[w])
                bit = (bit & -bit).bit_length() - 1
                row = 64 * w + bit
                pytest.fail(f"{name}: {what}: row {row} (word {w}, bit {bit}{', beyond n_rows' if row >= self.n else ''}): "
                            f"expected {int(want[w]) >> bit & 1}, got {int(got[w]) >> bit & 1}; "
                            f"{int(np.unpackbits(got.view(np.uint8)).sum())} bits set, reference {int(rows.sum())}")
            if self.n % 64:      # follows from the words being equal; stated because the scans read these bits
                assert int(got[-1]) >> (self.n % 64) == 0, f"{name}: bits at or beyond n_rows are set: {what}"
        assert canary_m == CANARY and canary_u == CANARY, f"a word behind an output buffer was written: {what}"
        assert counts.tolist() == [int(keep.sum()), int(undecided.sum())] + self.ctmpl.cpu().tolist()[2:], f"counts: {what}"
        return keep, undecided


@functools.lru_cache(maxsize=2)
def case(n):
    return Case(n)


def _ops_that_must_have_rows(kind, lit):
    """Where the column's type has values below / above / equal to a numeric literal, the test columns must hold some."""
    if lit != lit:
        return []          # nan
    if kind == I64:
        below, above, equal = lit > INT64_MIN, lit < INT64_MAX, True
    elif kind == I64F:     # 2^63 is (double)INT64_MAX: equal to a row, above none
        below, above, equal = lit > -2.0**63, lit < 2.0**63, float(lit).is_integer() and abs(lit) <= 2.0**63
    else:
        below, above, equal = lit > float("-inf"), lit < float("inf"), True
    return [op for op, needed in ((LT, below), (GT, above), (EQ, equal)) if needed]


# ---- part 1: the kernel through the C ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_ROWS)
def test_every_kind_and_op_as_a_single_term(gpu, n):
    c = case(n)
    mixed = set()
    for kind, literals in LITERALS.items():
        for lit in literals:
            for op in OP_NAME:
                keep, undecided = c.check([(kind, op, lit)], False)
                if (keep | undecided).any() and not (keep | undecided).all():
                    mixed.add((kind, op))
    if n >= 255:
        # the inputs are not vacuous: every kind x op cell has a literal with rows on both sides; every literal but nan and
        # the ones beyond the type's range has rows equal to it; every literal key has ties and rows that differ in word 1 only
        # (a key's != fails no row: a row either differs, and passes, or ties, and is undecided)
        assert mixed == {(k, o) for k in LITERALS for o in OP_NAME} - {(STR, NE)}, sorted(mixed)
        for kind in (I64, I64F, F32):
            for lit in LITERALS[kind]:
                for op in _ops_that_must_have_rows(kind, lit):
                    assert c.ref_term(kind, op, lit)[0].any(), (KIND_NAME[kind], OP_NAME[op], lit)
        for lit in LITERALS[STR]:
            assert c.ref_term(STR, EQ, lit)[1].any()
            assert ((c.k0 == np.uint64(lit[0])) & (c.k1 != np.uint64(lit[1]))).any()
        assert (c.k0 >= np.uint64(TOP)).any() and (c.k1 >= np.uint64(TOP)).any()


def _draw_terms(c, rng, n_terms, retain):
    """n_terms random (kind, op, literal) triples; with `retain`, a draw is taken again (up to 30 times) while it would leave
    less than that share of the rows the terms so far have left, so that a long conjunction still keeps rows."""
    terms, alive = [], np.ones(c.n, bool)
    for _ in range(n_terms):
        for _attempt in range(30):
            kind = int(rng.integers(0, 4))
            t = (kind, int(rng.integers(0, 6)), LITERALS[kind][int(rng.integers(0, len(LITERALS[kind])))])
            verdict, tie = c.ref_term(*t)
            left = alive & (verdict | tie)
            if retain is None or left.sum() >= retain * alive.sum():
                break
        terms.append(t)
        alive = left
    return terms


@pytest.mark.parametrize("n", N_ROWS)
def test_conjunctions_of_mixed_terms_with_and_without_tombstones(gpu, n):
    c = case(n)
    for n_terms, retain in ((2, None), (5, 0.7), (16, 0.88)):
        for seed in (0, 1):
            rng = np.random.default_rng([n, n_terms, seed])
            terms = _draw_terms(c, rng, n_terms, retain)
            for tombstones in (False, True):
                keep, undecided = c.check(terms, tombstones)
                if n >= 255 and retain is not None:
                    assert (keep | undecided).any(), terms      # the conjunction is not vacuous
    # no term at all: the mask is the tombstones' complement
    c.check([], True)
    c.check([], False)


def test_zero_rows_zero_the_counts_and_write_nothing(gpu):
    c = case(0)
    mask, canary_m, und, canary_u, counts = c.launch([(I64, LT, 5), (STR, GE, LITERALS[STR][0])], False)
    assert mask.size == 0 and und.size == 0          # both pointers point AT the canaries
    assert canary_m == CANARY and canary_u == CANARY
    assert counts.tolist() == [0, 0] + c.ctmpl.cpu().tolist()[2:]


def test_bad_arguments_are_refused_before_anything_is_written(gpu):
    """hr_filter_eval_dev checks the term count, every kind / op / column pointer and the alignment of the two outputs
    before its memset of the counts and before the launch: each refusal leaves the buffers, the canaries and the
    (garbage) counts as they were."""
    c = case(65)
    mask, und, counts = c.pointers()
    good = (I64, LT, 5)
    null_col = c.term(*good)
    null_col.col = None
    # the binding raises HbmRagError for HR_ELIMIT and, like every entry point, ValueError for HR_EINVAL (include/hbmrag.h)
    bad_calls = {
        "17 terms": ([c.term(*good)] * 17, mask, und, nat.HbmRagError, "up to 16 terms"),
        "op 6": ([c.term(I64, 6, 5)], mask, und, ValueError, "bad filter term 0"),
        "op -1": ([c.term(*good), c.term(F32, -1, 0.5)], mask, und, ValueError, "bad filter term 1"),
        "kind 4": ([c.term(4, LT, 5, c.d_cols[I64].data_ptr())], mask, und, ValueError, "bad filter term 0"),
        "kind -1": ([c.term(-1, LT, 5, c.d_cols[I64].data_ptr())], mask, und, ValueError, "bad filter term 0"),
        "null column": ([c.term(*good), null_col], mask, und, ValueError, "bad filter term 1"),
        "mask not 8-byte aligned": ([c.term(*good)], mask + 4, und, ValueError, "8-byte aligned"),
        "undecided not 8-byte aligned": ([c.term(*good)], mask, und + 4, ValueError, "8-byte aligned"),
    }
    for name, (terms, m, u, error, message) in bad_calls.items():
        c.refill()
        with pytest.raises(error, match=message):
            nat.filter_eval_dev(terms, c.n, 0, m, u, counts, c.stream)
        assert torch.equal(c.out, c.tmpl) and torch.equal(c.counts, c.ctmpl), name
    c.check([good], False)      # and the same buffers still take a good call


# ---- part 2: the same edges through the index manager ------------------------------------------------------------------------
N, D, V, NNZ = 4133, 8, 500, 8
APPENDS = (700, 800, 2633)
STRADDLE = "0123456789abcde"            # 15 bytes: a two-byte character after it straddles byte 16
DOC_POOL = ["émile", "日本語テキスト", "\U0001F600 smile", "zzz", "ÿ", STRADDLE + "é", STRADDLE + "è", STRADDLE + "é-tail",
            "0123456789abcdef-tail-A", "0123456789abcdef-tail-B", "0123456789abcdef", "abc", "abc\0x", "", "doc7", "Zebra"]
ENTROPY_POOL = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 0.30000001192092896, 0.2, 0.5, 0.9]
CHUNK_POOL = [0, 1, 2, 3, -1, 2**53 - 1, 2**53, 2**53 + 1, -(2**53 + 1), INT64_MIN, INT64_MAX]
STAGED = 'doc_id >= "0123456789abcdeé" and entropy <= inf and chunk_index < 9007199254740993 and token_count != 7'
STAGED_BYTES_PER_ROW = 16 + 4 + 8 + 8     # the doc_id key, entropy, chunk_index, token_count
MANAGER_EXPRS = [
    'doc_id >= "é"',                                   # first byte 0xC3: a signed key compare puts it below every ASCII row
    'doc_id < "日本語テキスト"',
    'doc_id == "émile"',
    'doc_id > "zzz"',
    'doc_id >= "\U0001F600"',
    f'doc_id == "{STRADDLE}é"',                        # ties with the è row on the 16-byte prefix: settled on the full strings
    f'doc_id < "{STRADDLE}é"',
    f'doc_id > "{STRADDLE}é" and doc_id <= "{STRADDLE}é-tail"',
    'doc_id != "0123456789abcdef-tail-A"',
    'doc_id == "abc"',
    'doc_id > "abc"',
    'doc_id <= "abc\0x" and doc_id >= "abc"',
    'doc_id == ""',
    "entropy != nan",
    "entropy == nan",
    "entropy < inf",
    "entropy >= -inf and entropy <= -0.0",
    "entropy > 0 and entropy < 0.2",                   # the denormal alone
    "entropy < 1e39",
    "chunk_index >= 9007199254740992.0",
    "chunk_index == 9007199254740993",
    "chunk_index > 9007199254740992",
    "chunk_index < 1e19 and chunk_index > -1e19",
    "chunk_index <= -0.0",
    "chunk_index >= 2.5 and chunk_index != nan",
    "chunk_index >= -9223372036854775808 and chunk_index < 9223372036854775807",
    'doc_id >= "é" and entropy <= inf and chunk_index < 2.5 and token_count > 100',
    STAGED,
]
SEARCH_EXPR = f'doc_id >= "{STRADDLE}é" and entropy >= -inf and chunk_index <= 9007199254740992.0'


def _bits(mask_u8):
    return np.unpackbits(mask_u8.cpu().numpy(), bitorder="little").astype(bool)


def _collection(rng):
    """Dense rows, CSR sparse rows, ids and payload columns of the 4133-row collection."""
    X = rng.standard_normal((N, D)).astype(np.float32)
    idx = np.sort(np.argpartition(rng.random((N, V)), NNZ - 1, axis=1)[:, :NNZ], axis=1).astype(np.int32).reshape(-1)
    val = np.abs(rng.standard_normal(N * NNZ)).astype(np.float32)
    ptr = np.arange(N + 1, dtype=np.int64) * NNZ
    ids = [f"c{r}" for r in range(N)]
    pick = rng.integers(0, len(DOC_POOL) + 4, N)
    cols = dict(doc_id=[DOC_POOL[p] if p < len(DOC_POOL) else f"doc{r % 13}" for r, p in enumerate(pick.tolist())],
                # columns.py takes non-finite FLOAT payloads as they are (only dense vectors are refused): NaN and the
                # infinities are rows of this collection
                entropy=np.asarray(ENTROPY_POOL, np.float32)[rng.integers(0, len(ENTROPY_POOL), N)].tolist(),
                chunk_index=[CHUNK_POOL[p] for p in rng.integers(0, len(CHUNK_POOL), N).tolist()],
                token_count=rng.integers(0, 2000, N).tolist(),
                timestamp=[f"202{r % 6}-0{1 + r % 9}-1{r % 9}" for r in range(N)])
    return X, (ptr, idx, val), ids, cols


def test_manager_filters_at_4133_rows_in_three_appends(gpu):
    rng = np.random.default_rng(4133)
    X, (ptr, idx, val), ids, cols = _collection(rng)
    m = MilvusIndexManager(semantic_dim=D, sparse_dim=V, dtype="float32", enable_domain=False)
    try:
        # ---- three appends, a filter after each: the HBM columns hold 1024, then 1536, then 4133 rows
        lo, caps = 0, []
        for step in APPENDS:
            hi = lo + step
            m.add_rows(X[lo:hi], (ptr[lo:hi + 1], idx, val), ids=ids[lo:hi], **{k: v[lo:hi] for k, v in cols.items()})
            m.finalize()
            host_cols = m._columns()
            got = _bits(m._global_device_mask(STAGED))
            assert got.size == 64 * ((hi + 63) // 64) and not got[hi:].any(), f"bits beyond row {hi} are set"
            assert np.array_equal(got[:hi], oracle.filter_mask(STAGED, host_cols, hi)), f"after {hi} rows"
            caps.append(sorted((name, t.shape[0]) for name, (t, _) in m._dev_filters._dev.items()))
            assert m._dev_filters.stats["uploaded_bytes"] == hi * STAGED_BYTES_PER_ROW      # every row of every column: once
            lo = hi
        assert lo == N
        assert [sorted({cap for _, cap in c}) for c in caps] == [[1024], [1536], [N]], caps   # grown twice, with a copy
        assert [name for name, _ in caps[-1]] == ["chunk_index", "entropy", "key:doc_id", "token_count"]

        # ---- the expressions: device == oracle, host evaluator == oracle, nothing set beyond the last row
        host_cols = m._columns()
        for expr in MANAGER_EXPRS:
            want = oracle.filter_mask(expr, host_cols, N)
            got = _bits(m._global_device_mask(expr))
            if not np.array_equal(got[:N], want):
                row = int(np.nonzero(got[:N] != want)[0][0])
                pytest.fail(f"{expr!r}: n_rows={N}, row {row} (doc_id {cols['doc_id'][row]!r}, entropy {cols['entropy'][row]!r}, "
                            f"chunk_index {cols['chunk_index'][row]}): expected {int(want[row])}, got {int(got[row])}")
            assert not got[N:].any(), expr
            assert np.array_equal(F.evaluate(expr, host_cols, N), want), expr
            # rows on both sides, but for the three expressions that nan and the float64 range decide for every row
            assert want.sum() == {"entropy == nan": 0, "entropy != nan": N, "chunk_index < 1e19 and chunk_index > -1e19": N}.get(expr) \
                or 0 < want.sum() < N, expr
        assert m._dev_filters.stats["undecided_rows"] > 0
        assert m._dev_filters.stats["uploaded_bytes"] == N * STAGED_BYTES_PER_ROW          # nothing went up a second time

        # ---- a literal no int64 holds: refused before its column (or any other) is uploaded
        before = dict(m._dev_filters.stats)
        for bad in ('timestamp >= "2024" and chunk_index < 9223372036854775808', "token_count >= -9223372036854775809"):
            with pytest.raises(ValueError) as ei:
                m._global_device_mask(bad)
            assert bad.split(" and ")[-1] in str(ei.value)
        assert m._dev_filters.stats == before and "key:timestamp" not in m._dev_filters._dev

        # ---- tombstones: a number of rows that is no multiple of 8, in a collection whose size is none either
        gone = oracle.filter_mask('doc_id == "ÿ"', host_cols, N) | oracle.filter_mask("entropy == -inf", host_cols, N)
        asyncio.run(m.delete_by_filter("semantic_index", 'doc_id == "ÿ"'))
        asyncio.run(m.delete_by_filter("semantic_index", "entropy == -inf"))
        assert gone.sum() % 8 != 0 and np.array_equal(m._deleted[:N], gone)
        keep = ~gone & oracle.filter_mask(SEARCH_EXPR, host_cols, N)
        got = _bits(m._global_device_mask(SEARCH_EXPR))
        assert np.array_equal(got[:N], keep) and not got[N:].any()
        assert 100 < keep.sum() < N - 100
        und0 = m._dev_filters.stats["undecided_rows"]

        # ---- dense, sparse and hybrid search under that mask: the oracle's ids and scores
        m8 = np.packbits(keep, bitorder="little")
        k, top_k = 20, 10
        Q = rng.standard_normal((3, D)).astype(np.float32)
        SQ = [(np.sort(rng.choice(V, 12, replace=False)).astype(np.int32), np.abs(rng.standard_normal(12)).astype(np.float32))
              for _ in range(3)]
        sp = {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}
        di, ds = oracle.dense_search(X, Q, k, oracle.COSINE, m8)
        si, ss = oracle.sparse_search(ptr, idx, val, SQ, k, 0.2, m8)
        for b in range(3):
            hits = asyncio.run(m.search(Q[b], "semantic_index", k, SEARCH_EXPR))
            live = di[b] >= 0
            assert [h["_row"] for h in hits] == di[b][live].tolist() and [h["id"] for h in hits] == [ids[r] for r in di[b][live]]
            assert [h["score"] for h in hits] == [float(x) for x in ds[b][live]]
            assert all(keep[h["_row"]] for h in hits)
            sq = {"indices": SQ[b][0].tolist(), "values": SQ[b][1].tolist()}
            hits = asyncio.run(m.search(sq, "sparse_index", k, SEARCH_EXPR, sp))
            live = si[b] >= 0
            assert live.any()
            assert [h["_row"] for h in hits] == si[b][live].tolist() and [h["id"] for h in hits] == [ids[r] for r in si[b][live]]
            assert [h["score"] for h in hits] == [float(x) for x in ss[b][live]]
            # the engine's hybrid form: both searches (2 x top_k wide) and their rank fusion in one round
            res = asyncio.run(m.hybrid_search(Q[b], sq, top_k, SEARCH_EXPR, (0.7, 0.3), sparse_params=sp))
            assert res is not None, "the hybrid round did not answer"
            fi, fs, _ = oracle.rrf(di[b][di[b] >= 0], si[b][si[b] >= 0], (), 0.7, 0.3, 0.0, 60)
            assert [hit["_row"] for hit, _, _ in res] == fi[:top_k].tolist()
            assert [hit["id"] for hit, _, _ in res] == [ids[r] for r in fi[:top_k]]
            assert [score for _, score, _ in res] == [float(x) for x in fs[:top_k]]
        assert m._dev_filters.stats["undecided_rows"] >= und0 > 0
    finally:
        asyncio.run(m.close())
