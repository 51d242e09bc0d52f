"""Filter expressions beyond the conjunction on the device (filter_expr_kernel, entry point hr_filter_eval_expr_dev): `in`
lists, or, not, parentheses.

Part 1 calls the C ABI with synthetic device columns, as test_gpu_filter_edges.py does for the conjunction: garbage-filled
outputs, a canary word behind each, every word of `mask` and `undecided`, the bits at and beyond n_rows and both counts held
to a plain numpy restatement of the contract of include/hbmrag.h -- a leaf is (lo, hi) = (certainly true, possibly true) per
row, a comparison as in hr_filter_eval_dev, a numeric membership leaf lo = hi = "some member == value", a string one lo = 0,
hi = "some member key == the row's key"; and / or / not are Kleene's on the pair; mask = alive & lo, undecided = alive & hi
& ~lo.  Sets of 0, 1, 2, 3, 64 members and the cap (8192 int64, 16384 float32, 4096 keys) whose first, middle and last
member are column values, beside values one below the first and one above the last member; programs from one leaf to 16-leaf
chains, depth-32 nesting and a mixed tree with two string leaves.

Part 2 takes ties through DeviceFilters.evaluate on a small collection: ids that share 16 bytes with list members (and list
members with each other), under not, under or beside a true numeric leaf, under and beside a false one.  Part 3 runs the
searches, a grouped search, delete + compact and the caps through MilvusIndexManager.  Expected masks are composed from the
oracle leaf by leaf (filter_expr_oracle.py)."""
import asyncio
import functools
import json

import numpy as np
import pytest

import oracle
from advanced_rag import MilvusIndexManager
from advanced_rag import _native as nat
from filter_expr_oracle import AND, C, IN, NOT, OR, expected

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I64, I64F, F32, STR = nat.HR_COL_I64, nat.HR_COL_I64_VS_F64, nat.HR_COL_F32, nat.HR_COL_STR16
EQ, NE, LT, LE, GT, GE = (nat.FILTER_OPS[o] for o in ("==", "!=", "<", "<=", ">", ">="))
OP_IN, P_AND, P_OR, P_NOT = nat.HR_OP_IN, nat.HR_FILTER_AND, nat.HR_FILTER_OR, nat.HR_FILTER_NOT
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
TOP = 1 << 63
U64 = 1 << 64
GRID_ROWS = 4096 * 4 * 64          # rows of one trip of the widest launch (4096 blocks x 4 waves)
N_ROWS = [0, 1, 63, 64, 65, 257, GRID_ROWS + 69]
GARBAGE, CANARY = 0xA5A5A5A5A5A5A5A5, 0x5EEDC0DE0DDBA115
DEVICE = "cuda:0"
CAP = {I64: 8192, F32: 16384, STR: 4096}
SIZES = (0, 1, 2, 3, 64)

# ---- comparison literals and column values: the edge sets of test_gpu_filter_edges.py ------------------------------------------
LIT32 = np.float32(0.30000001192092896)
KEY_LITERALS = [(TOP | 0x1234567890ABCDEF, 0x0FEDCBA987654321), (0x6162636465666768, TOP | 0x0000000000000001),
                (int.from_bytes(b"doc123\0\0", "big"), 0), (0, 0)]
I64_VALUES = [0, 1, -1, 2, 3, 2**53 - 1, -(2**53 - 1), 2**53, -(2**53), 2**53 + 1, -(2**53 + 1), INT64_MIN, INT64_MAX,
              INT64_MIN + 1, INT64_MAX - 1, 2**53 + 2, -(2**53 + 2)]
F32_VALUES = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, LIT32, np.nextafter(LIT32, np.float32(1)),
              np.nextafter(LIT32, np.float32(0)), 1.0, -1.0, np.finfo(np.float32).max, np.finfo(np.float32).tiny]


def _key_values(keys):
    """Per key: the key itself (a tie), one that differs only in word 1 (below and above), one that differs from it only in the
    top bit of word 1, and one only in the top bit of word 0."""
    out = []
    for k0, k1 in keys:
        out += [(k0, k1), (k0, (k1 + 1) % U64), (k0, (k1 - 1) % U64), (k0, k1 ^ TOP), (k0 ^ TOP, k1)]
    return out


# ---- membership sets -------------------------------------------------------------------------------------------------------------
def _int_sets():
    """name -> ascending int64 members.  "run": an arithmetic run of step 2 (the values between two members are none);
    "ends": INT64_MIN, a run from 2^53, INT64_MAX."""
    sets = {"int empty": []}
    for i, s in enumerate(SIZES[1:] + (CAP[I64],)):
        sets[f"int run {s}"] = [100_000 * (i + 1) + 2 * j for j in range(s)]
        if s >= 2:
            sets[f"int ends {s}"] = [INT64_MIN] + [2**53 + j for j in range(s - 2)] + [INT64_MAX]
    sets["int one min"], sets["int one max"] = [INT64_MIN], [INT64_MAX]
    return {k: np.asarray(v, dtype=np.int64) for k, v in sets.items()}


def _float_sets():
    """Ascending float32 members, no NaN: -inf, a run of quarters from 0 (0.0 and 1.0 are column values), +inf."""
    sets = {"float empty": [], "float one zero": [0.0], "float one -zero": [-0.0], "float one lit": [LIT32],
            "float infs": [-np.inf, np.inf], "float three": [-np.inf, -0.0, np.inf]}
    for s in (64, CAP[F32]):
        sets[f"float run {s}"] = [-np.inf] + [0.25 * j for j in range(s - 2)] + [np.inf]
    return {k: np.asarray(v, dtype=np.float32) for k, v in sets.items()}


def _key_run(s):
    return [(0x4000000000000000 + 7 * j, (3 * j) % U64 if j % 2 else TOP | j) for j in range(s)]


def _key_sets():
    """Ascending two-word keys (unsigned, word 0 first): the empty key first, a run in the middle, a top-bit key last."""
    lits = sorted(KEY_LITERALS)
    sets = {"key empty": [], "key one zero": [(0, 0)], "key one top": [lits[-1]], "key two": [lits[0], lits[-1]],
            "key three": [lits[0], lits[2], lits[-1]]}
    for s in (64, CAP[STR]):
        sets[f"key run {s}"] = [lits[0]] + _key_run(s - 2) + [lits[-1]]
    return {k: np.asarray(v, dtype=np.uint64).reshape(-1, 2) for k, v in sets.items()}


SETS = {I64: _int_sets(), F32: _float_sets(), STR: _key_sets()}


def _probes(members):
    """Of a set: its first, middle and last member and the values one below the first / one above the last."""
    if not len(members):
        return []
    picks = [members[0], members[len(members) // 2], members[-1]]
    if members.dtype == np.int64:
        return [int(p) for p in picks] + [v for v in (int(members[0]) - 1, int(members[0]) + 1, int(members[-1]) + 1)
                                          if INT64_MIN <= v <= INT64_MAX]
    if members.dtype == np.float32:
        finite = members[np.isfinite(members)]
        edge = [np.nextafter(finite[0], np.float32(-np.inf)), np.nextafter(finite[-1], np.float32(np.inf))] if len(finite) else []
        return picks + edge
    return _key_values([tuple(int(x) for x in p) for p in picks])


INT_POOL = I64_VALUES + [v for m in SETS[I64].values() for v in _probes(m)]
FLOAT_POOL = F32_VALUES + [v for m in SETS[F32].values() for v in _probes(m)]
KEY_POOL = _key_values(KEY_LITERALS) + [v for m in SETS[STR].values() for v in _probes(m)]


def _spread(rng, n, values, random_rows, dtype):
    """A column of n rows: 70 % of the rows draw one of `values`, the others are random; the LAST rows hold every value once (as
    many as fit), so that the ragged last word of every shape holds edge values too."""
    values = np.asarray(values, dtype=dtype)
    col = np.where((rng.random(n) < 0.7).reshape((n,) + (1,) * (values.ndim - 1)), values[rng.integers(0, len(values), n)],
                   random_rows)
    m = min(n, len(values))
    if m:
        col[n - m:] = values[:m]
    return np.ascontiguousarray(col.astype(dtype))


def _s16(keys):
    """[n, 2] uint64 keys as 16-byte strings: equal bytes <=> equal keys (all are 16 bytes long before numpy strips NULs)."""
    return np.ascontiguousarray(keys.astype(">u8")).view("S16").reshape(-1)


class Case:
    """Host and device columns of one row count, the device sets, and the output buffers: [mask words | canary | undecided
    words | canary] in one tensor, [counts[2] | canary[2]] in another, refilled with garbage before every call."""

    def __init__(self, n):
        rng = np.random.default_rng(2000 + n % 9973)
        self.n, self.n_words = n, (n + 63) // 64
        small = rng.integers(-4, 5, n)
        wide = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
        self.i64 = _spread(rng, n, INT_POOL, np.where(rng.random(n) < 0.5, small, wide), np.int64)
        self.f32 = _spread(rng, n, FLOAT_POOL, rng.standard_normal(n).astype(np.float32), np.float32)
        self.key = _spread(rng, n, KEY_POOL, rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64), np.uint64)
        self.k0, self.k1 = np.ascontiguousarray(self.key[:, 0]), np.ascontiguousarray(self.key[:, 1])
        dead = rng.random(n) < 0.3
        if n >= 63 and dead.sum() % 8 == 0:
            dead[np.nonzero(~dead)[0][0]] = True                 # a number of tombstones that is no multiple of 8
        bits = np.ones(((n + 7) // 8) * 8, dtype=bool)          # the pad bits of the last byte are set: they are no rows
        bits[:n] = dead
        self.dead, self.dead_bytes = dead, np.packbits(bits, bitorder="little")
        dev = torch.device(DEVICE)

        def up(a, dtype):    # at least one element: a column pointer may not be null, even for 0 rows
            t = torch.zeros(max(a.size, 1), dtype=dtype, device=dev)
            if a.size:
                t[:a.size] = torch.from_numpy(a.reshape(-1).view(np.int64 if a.dtype == np.uint64 else a.dtype)).to(dev)
            return t
        self.d_cols = {I64: up(self.i64, torch.int64), F32: up(self.f32, torch.float32), STR: up(self.key, torch.int64)}
        self.d_cols[I64F] = self.d_cols[I64]
        self.d_sets = {(kind, name): up(m, torch.float32 if kind == F32 else torch.int64)
                       for kind, sets in SETS.items() for name, m in sets.items() if len(m)}
        self.d_dead = torch.from_numpy(self.dead_bytes).to(dev)
        w = self.n_words
        tmpl = np.full(2 * (w + 1), GARBAGE, dtype=np.uint64)
        tmpl[w] = tmpl[2 * w + 1] = CANARY
        self.tmpl = torch.from_numpy(tmpl.view(np.int64)).to(dev)
        self.out = torch.empty_like(self.tmpl)
        self.ctmpl = torch.tensor([0x5A5A5A5A, -7, 0x0DDBA115, -0x0DDBA115], dtype=torch.int32, device=dev)
        self.counts = torch.empty_like(self.ctmpl)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self._leaf_ref = {}

    # -- leaves: ("cmp", kind, op, literal) or ("in", kind, set name) ------------------------------------------------------------
    def term(self, kind, op, lit):
        t = nat.FilterTerm()
        t.kind, t.op, t.col = kind, op, self.d_cols[kind].data_ptr()
        # the literal fields this kind does not read hold values that would change the verdict if it did read them
        t.ival, t.dval, t.fval, t.key[0], t.key[1] = -1, float("nan"), float("nan"), U64 - 1, U64 - 1
        if lit is None:          # a membership leaf: no literal
            pass
        elif kind == I64:
            t.ival = lit
        elif kind == I64F:
            t.dval = lit
        elif kind == F32:
            t.fval = float(np.float32(lit))
        elif kind == STR:
            t.key[0], t.key[1] = lit
        return t

    def leaf(self, spec):
        leaf = nat.FilterLeaf()
        if spec[0] == "cmp":
            leaf.term = self.term(*spec[1:])
            leaf.set, leaf.n_set = 0xDEAD0000, 12345            # a comparison leaf reads neither
        else:
            _, kind, name = spec
            leaf.term = self.term(kind, OP_IN, None)
            leaf.n_set = len(SETS[kind][name])
            leaf.set = self.d_sets[(kind, name)].data_ptr() if leaf.n_set else None
        return leaf

    def pointers(self):
        base = self.out.data_ptr()
        return base, base + 8 * (self.n_words + 1), self.counts.data_ptr()

    def refill(self):
        self.out.copy_(self.tmpl)
        self.counts.copy_(self.ctmpl)

    def read(self):
        o, w = self.out.cpu().numpy().view(np.uint64), self.n_words
        return o[:w].copy(), o[w], o[w + 1:2 * w + 1].copy(), o[2 * w + 1], self.counts.cpu().numpy()

    def launch(self, leaves, program, tombstones):
        self.refill()
        mask, und, counts = self.pointers()
        nat.filter_eval_expr_dev([self.leaf(s) for s in leaves], program, self.n, self.d_dead.data_ptr() if tombstones else 0,
                                 mask, und, counts, self.stream)
        return self.read()

    # -- the contract, in numpy ---------------------------------------------------------------------------------------------------
    def ref_cmp(self, kind, op, lit):
        """-> (verdict per row where the term decides, tie per row): as in test_gpu_filter_edges.py."""
        n = self.n
        if kind == STR:
            k0, k1, l0, l1 = self.k0, self.k1, np.uint64(lit[0]), np.uint64(lit[1])
            tie = (k0 == l0) & (k1 == l1)
            less = (k0 < l0) | ((k0 == l0) & (k1 < l1))           # unsigned, word 0 first
            return {EQ: np.zeros(n, bool), NE: np.ones(n, bool), LT: less, LE: less, GT: ~less, GE: ~less}[op], tie
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

    def ref_leaf(self, spec):
        """-> (lo, hi) per row: certainly true, possibly true."""
        if spec not in self._leaf_ref:
            if spec[0] == "cmp":
                verdict, tie = self.ref_cmp(*spec[1:])
                pair = verdict & ~tie, verdict | tie
            else:
                _, kind, name = spec
                members = SETS[kind][name]
                if kind == STR:
                    pair = np.zeros(self.n, bool), np.isin(_s16(self.key), _s16(members))
                else:
                    col = self.i64 if kind == I64 else self.f32
                    has = np.zeros(self.n, bool)
                    if len(members) and self.n:
                        # the ascending set holds a value == the row's iff the first member that is not below it is one
                        at = np.minimum(np.searchsorted(members, col, side="left"), len(members) - 1)
                        has = members[at] == col
                        if kind == F32 and len(members) <= 64 and self.n <= 4096:   # and, spelled out where it is cheap: any member == value
                            assert np.array_equal(has, (col[:, None] == members[None, :]).any(axis=1))
                    pair = has, has
            self._leaf_ref[spec] = pair
        return self._leaf_ref[spec]

    def ref(self, leaves, program, tombstones):
        stack = []
        for code in program:
            if code >= 0:
                stack.append(self.ref_leaf(leaves[code]))
            elif code == P_NOT:
                lo, hi = stack.pop()
                stack.append((~hi, ~lo))
            else:
                (lo_b, hi_b), (lo_a, hi_a) = stack.pop(), stack.pop()
                stack.append((lo_a & lo_b, hi_a & hi_b) if code == P_AND else (lo_a | lo_b, hi_a | hi_b))
        (lo, hi), = stack
        alive = ~self.dead if tombstones else np.ones(self.n, bool)
        return alive & lo, alive & hi & ~lo

    def words(self, rows):
        bits = np.zeros(self.n_words * 64, dtype=bool)
        bits[:self.n] = rows
        return np.packbits(bits, bitorder="little").view("<u8")

    def check(self, leaves, program, tombstones):
        what = f"leaves {leaves} program {program} (n_rows={self.n}, tombstones={tombstones})"
        mask, canary_m, und, canary_u, counts = self.launch(leaves, program, tombstones)
        keep, undecided = self.ref(leaves, program, tombstones)
        for name, got, rows in (("mask", mask, keep), ("undecided", und, undecided)):
            want = self.words(rows)
            if not np.array_equal(got, want):
                w = int(np.nonzero(got != want)[0][0])
                bit = int(got[w] ^ want[w])
                bit = (bit & -bit).bit_length() - 1
                row = 64 * w + bit
                pytest.fail(f"{name}: {what}: row {row} (word {w}, bit {bit}{', beyond n_rows' if row >= self.n else ''}): "
                            f"expected {int(want[w]) >> bit & 1}, got {int(got[w]) >> bit & 1}; i64 {self.i64[min(row, self.n - 1)]}, "
                            f"f32 {self.f32[min(row, self.n - 1)]!r}, key {self.key[min(row, self.n - 1)].tolist()}")
            if self.n % 64:
                assert int(got[-1]) >> (self.n % 64) == 0, f"{name}: bits at or beyond n_rows are set: {what}"
        assert canary_m == CANARY and canary_u == CANARY, f"a word behind an output buffer was written: {what}"
        assert counts.tolist() == [int(keep.sum()), int(undecided.sum())] + self.ctmpl.cpu().tolist()[2:], f"counts: {what}"
        return keep, undecided


@functools.lru_cache(maxsize=2)
def case(n):
    return Case(n)


ALL_SET_LEAVES = [("in", kind, name) for kind, sets in SETS.items() for name in sets]


# ---- part 1: the kernel through the C ABI ------------------------------------------------------------------------------------------
def test_the_sets_are_what_the_contract_asks_for():
    for kind, sets in SETS.items():
        assert sorted({len(m) for m in sets.values()}) == sorted(SIZES + (CAP[kind],)), kind
        for name, m in sets.items():
            if kind == STR:
                assert [tuple(r) for r in m.tolist()] == sorted({tuple(r) for r in m.tolist()}), name
            else:
                assert (m[1:] > m[:-1]).all() and not (m != m).any(), name
            assert m.nbytes <= nat.HR_MAX_FILTER_SET_BYTES
        assert max(m.nbytes for m in sets.values()) == nat.HR_MAX_FILTER_SET_BYTES     # the cap itself is a case
    assert any(int(k0) >= TOP for m in SETS[STR].values() for k0, _ in m.tolist())
    assert any(int(k1) >= TOP for m in SETS[STR].values() for _, k1 in m.tolist())


@pytest.mark.parametrize("n", N_ROWS)
def test_every_set_as_a_single_leaf_and_under_not(gpu, n):
    c = case(n)
    for spec in ALL_SET_LEAVES:
        for program in ([0], [0, P_NOT]):
            for tombstones in (False, True):
                c.check([spec], program, tombstones)
    if n >= 257:
        # the inputs are not vacuous: every set but the empty ones has a row equal to its first, its middle and its last
        # member, and rows one below the first / one above the last (where the type has such a value) that are no members
        for kind, sets in SETS.items():
            col = {I64: c.i64, F32: c.f32}.get(kind)
            for name, m in sets.items():
                if not len(m):
                    assert not c.ref_leaf(("in", kind, name))[1].any()
                    continue
                for member in (m[0], m[len(m) // 2], m[-1]):
                    at = _s16(c.key) == _s16(member[None, :])[0] if kind == STR else col == member
                    assert at.any() and c.ref_leaf(("in", kind, name))[1][at].all(), (name, member)
                if kind == I64 and m[0] > INT64_MIN:
                    assert (col == m[0] - 1).any() and not c.ref_leaf(("in", kind, name))[1][col == m[0] - 1].any(), name
                if kind == I64 and m[-1] < INT64_MAX:
                    assert (col == m[-1] + 1).any() and not c.ref_leaf(("in", kind, name))[1][col == m[-1] + 1].any(), name
        with np.errstate(invalid="ignore"):
            nan, zero = c.f32 != c.f32, c.f32 == 0
        assert nan.any() and (np.signbit(c.f32) & zero).any() and (~np.signbit(c.f32) & zero).any() and np.isinf(c.f32).any()
        for name in SETS[F32]:
            assert not c.ref_leaf(("in", F32, name))[1][nan].any()                  # a NaN row is a member of nothing
        for name in ("float one zero", "float one -zero", "float three"):
            assert c.ref_leaf(("in", F32, name))[1][zero].all()                     # -0.0 and 0.0 are one member
        assert (c.k0 >= np.uint64(TOP)).any() and (c.k1 >= np.uint64(TOP)).any()
        und = c.check([("in", STR, "key three")], [0], False)[1]
        assert und.any() and not c.check([("in", STR, "key three")], [0], False)[0].any()   # a string leaf never says true


CHAIN = [("in", I64, "int run 64"), ("cmp", I64, GE, 0), ("in", F32, "float run 64"), ("cmp", F32, LT, 1.0),
         ("in", STR, "key run 64"), ("cmp", STR, GE, KEY_LITERALS[2]), ("cmp", I64F, LT, 2.5), ("in", I64, "int ends 3"),
         ("cmp", STR, EQ, KEY_LITERALS[0]), ("in", F32, "float three"), ("cmp", F32, NE, float("nan")), ("in", STR, "key two"),
         ("in", I64, "int empty"), ("cmp", I64, NE, 2), ("in", F32, "float one lit"), ("cmp", STR, NE, KEY_LITERALS[3])]


def _chain(op, n_leaves=16, negate=()):
    program = []
    for i in range(n_leaves):
        program.append(i)
        if i in negate:
            program.append(P_NOT)
        if i:
            program.append(op)
    return program


def _nested():
    """32 pushes, then 31 operators from the inside out, alternately and / or, and one not: 64 codes, depth 32."""
    return [i % 16 for i in range(32)] + [P_AND if i % 2 else P_OR for i in range(31)] + [P_NOT]


MIXED = [("in", STR, "key run 64"), ("cmp", I64, GT, 0), ("cmp", STR, LE, KEY_LITERALS[1]), ("in", F32, "float run 64"),
         ("in", I64, "int run 3")]
# (key in S or i64 > 0) and not (key <= L and f32 in R) or i64 in T
MIXED_PROGRAM = [0, 1, P_OR, 2, 3, P_AND, P_NOT, P_AND, 4, P_OR]


@pytest.mark.parametrize("n", N_ROWS)
def test_programs(gpu, n):
    c = case(n)
    assert len(CHAIN) == 16 and len(_nested()) == nat.HR_MAX_FILTER_PROGRAM
    programs = [(CHAIN, _chain(P_AND)), (CHAIN, _chain(P_OR)), (CHAIN, _chain(P_AND, negate=(0, 4, 8, 12, 14))),
                (CHAIN, _chain(P_OR, negate=(1, 4, 5, 13))), (CHAIN, _nested()), (MIXED, MIXED_PROGRAM),
                (MIXED, MIXED_PROGRAM + [P_NOT]), (CHAIN, [4, 4, P_NOT, P_OR]),       # `a or not a` stays undecided on a tie
                (CHAIN, _chain(P_OR, n_leaves=3) + _chain(P_OR, n_leaves=2) + [P_AND])]
    seen = set()
    for leaves, program in programs:
        for tombstones in (False, True):
            keep, undecided = c.check(leaves, program, tombstones)
            seen |= {("keep", bool(keep.any())), ("undecided", bool(undecided.any())), ("drop", bool((~keep & ~undecided).any()))}
    if n >= 257:
        assert seen >= {("keep", True), ("undecided", True), ("drop", True)}
        for leaves, program in programs[5:7]:
            keep, undecided = c.ref(leaves, program, False)
            assert keep.any() and undecided.any() and (~keep & ~undecided).any(), program


def _draw_terms(c, rng, n_terms, retain):
    literals = {I64: [0, 2, -1, 2**53, INT64_MIN, INT64_MAX], I64F: [2.5, -0.0, 1e19, float("nan"), 9223372036854775808.0],
                F32: [float(LIT32), 0.0, float("inf"), float("nan"), 1e-45], STR: KEY_LITERALS}
    terms, alive = [], np.ones(c.n, bool)
    for _ in range(n_terms):
        for _attempt in range(30):
            kind = int(rng.integers(0, 4))
            t = ("cmp", kind, int(rng.integers(0, 6)), literals[kind][int(rng.integers(0, len(literals[kind])))])
            verdict, tie = c.ref_cmp(*t[1:])
            left = alive & (verdict | tie)
            if retain is None or left.sum() >= retain * alive.sum():
                break
        terms.append(t)
        alive = left
    return terms


@pytest.mark.parametrize("n", N_ROWS)
def test_a_conjunction_of_comparisons_equals_hr_filter_eval_dev(gpu, n):
    c = case(n)
    for n_terms, retain in ((1, None), (2, None), (5, 0.7), (16, 0.88)):
        terms = _draw_terms(c, np.random.default_rng([n, n_terms]), n_terms, retain)
        for tombstones in (False, True):
            keep, undecided = c.check(terms, _chain(P_AND, n_terms), tombstones)
            new = c.read()
            c.refill()
            mask, und, counts = c.pointers()
            nat.filter_eval_dev([c.term(*t[1:]) for t in terms], c.n, c.d_dead.data_ptr() if tombstones else 0, mask, und, counts,
                                c.stream)
            old = c.read()
            for a, b in zip(new, old):           # mask words, canary, undecided words, canary, counts + their canaries
                assert np.array_equal(a, b), (terms, tombstones)
            if n >= 257 and retain is not None:
                assert (keep | undecided).any()


def test_zero_rows_zero_the_counts_and_write_nothing(gpu):
    c = case(0)
    mask, canary_m, und, canary_u, counts = c.launch(MIXED, MIXED_PROGRAM, False)
    assert mask.size == 0 and und.size == 0
    assert canary_m == CANARY and canary_u == CANARY
    assert counts.tolist() == [0, 0] + c.ctmpl.cpu().tolist()[2:]


def test_bad_programs_and_leaves_are_refused_before_anything_is_written(gpu):
    """hr_filter_eval_expr_dev checks the leaves, the sets' sizes and the whole program on the host, before its memset of the
    counts and before the launch: every refusal is a status, and leaves the buffers, the canaries and the (garbage) counts as
    they were."""
    c = case(65)
    mask, und, counts = c.pointers()
    a, b = ("cmp", I64, LT, 5), ("in", I64, "int run 3")
    over = c.leaf(("in", I64, f"int run {CAP[I64]}"))
    over.n_set += 1                                              # one member over the cap (the pointer is never read)
    two_caps = [c.leaf(("in", I64, f"int run {CAP[I64]}")), c.leaf(("in", F32, "float one lit"))]
    mixed_kind = c.leaf(b)
    mixed_kind.term.kind = I64F
    null_set, set_of_none = c.leaf(b), c.leaf(("in", I64, "int empty"))
    null_set.set, set_of_none.set = None, c.d_sets[(I64, "int run 3")].data_ptr()
    null_col = c.leaf(a)
    null_col.term.col = None
    good = [c.leaf(a), c.leaf(b)]
    # the binding raises HbmRagError for HR_ELIMIT and, like every entry point, ValueError for HR_EINVAL (include/hbmrag.h)
    bad_calls = {
        "stack underflow (and)": (good, [0, P_AND], mask, ValueError, "empty stack"),
        "stack underflow (not)": (good, [P_NOT, 0], mask, ValueError, "empty stack"),
        "final depth 2": (good, [0, 1], mask, ValueError, "2 values left"),
        "final depth 0": (good, [], mask, ValueError, "bad filter arguments"),
        "depth 33": (good, [0] * 33, mask, ValueError, "deeper than 32"),
        "leaf index out of range": (good, [0, 2, P_OR], mask, ValueError, "names leaf 2 of 2"),
        "unknown code": (good, [0, -4], mask, ValueError, "unknown code"),
        "65 codes": (good, [0] + [P_NOT] * 64, mask, nat.HbmRagError, "up to 64 codes"),
        "17 leaves": ([c.leaf(a)] * 17, [0], mask, nat.HbmRagError, "up to 16 terms"),
        "no leaf": ([], [0], mask, ValueError, "bad filter arguments"),
        "int64-vs-float64 membership": ([mixed_kind], [0], mask, ValueError, "bad filter term 0"),
        "one member over the cap": ([over], [0], mask, nat.HbmRagError, "up to 65536 bytes"),
        "two sets over the cap together": (two_caps, [0, 1, P_OR], mask, nat.HbmRagError, "up to 65536 bytes"),
        "members without a set": ([c.leaf(a), null_set], [0, 1, P_OR], mask, ValueError, "bad filter term 1"),
        "a set without members": ([set_of_none], [0], mask, ValueError, "bad filter term 0"),
        "op 7": ([c.leaf(("cmp", I64, 7, 5))], [0], mask, ValueError, "bad filter term 0"),
        "null column": ([c.leaf(a), null_col], [0, 1, P_AND], mask, ValueError, "bad filter term 1"),
        "mask not 8-byte aligned": (good, [0, 1, P_AND], mask + 4, ValueError, "8-byte aligned"),
    }
    for name, (leaves, program, m, error, message) in bad_calls.items():
        c.refill()
        with pytest.raises(error, match=message):
            nat.filter_eval_expr_dev(leaves, program, c.n, 0, m, und, counts, c.stream)
        assert torch.equal(c.out, c.tmpl) and torch.equal(c.counts, c.ctmpl), name
    c.check([a, b], [0, 1, P_OR], False)      # and the same buffers still take a good call
    assert nat.load_library().hr_version() >= 10900


# ---- parts 2 and 3: through DeviceFilters and the index manager ----------------------------------------------------------------------
N, D, V, NNZ = 3011, 8, 500, 8
APPENDS = (700, 800, 1511)
P16 = "0123456789abcdef"                # 16 bytes: every id that starts with it has the same prefix key
STRADDLE = "0123456789abcde"            # 15 bytes: a two-byte character after it straddles byte 16
DOC_POOL = [P16 + "-tail-A", P16 + "-tail-B", P16 + "-tail-C", P16, STRADDLE + "é", STRADDLE + "è", "émile", "日本語テキスト", "zzz",
            "abc", "abc\0x", "", "doc7", "Zebra", 'q"uo\\te', "a, b"]


def _bits(mask_u8):
    return np.unpackbits(mask_u8.cpu().numpy(), bitorder="little").astype(bool)


def _q(s):
    return '"' + s.replace("\\", "\\\\").replace('"', '\\"') + '"'


@pytest.fixture(scope="module")
def collection():
    rng = np.random.default_rng(3011)
    X = rng.standard_normal((N, D)).astype(np.float32)
    idx = np.sort(np.argpartition(rng.random((N, V)), NNZ - 1, axis=1)[:, :NNZ], axis=1).astype(np.int32).reshape(-1)
    val = np.abs(rng.standard_normal(N * NNZ)).astype(np.float32)
    ptr = np.arange(N + 1, dtype=np.int64) * NNZ
    ids = [f"c{r}" for r in range(N)]
    pick = rng.integers(0, len(DOC_POOL) + 6, N)
    cols = dict(doc_id=[DOC_POOL[p] if p < len(DOC_POOL) else f"doc{r % 13}" for r, p in enumerate(pick.tolist())],
                entropy=(rng.integers(0, 11, N) / 10).astype(np.float32).tolist(),
                chunk_index=rng.integers(0, 6, N).tolist(), token_count=rng.integers(0, 2000, N).tolist(),
                timestamp=[f"202{r % 6}-0{1 + r % 9}-1{r % 9}" for r in range(N)])
    return X, (ptr, idx, val), ids, cols


def _manager(collection):
    X, (ptr, idx, val), ids, cols = collection
    m = MilvusIndexManager(semantic_dim=D, sparse_dim=V, dtype="float32", enable_domain=False)
    lo = 0
    for step in APPENDS:
        hi = lo + step
        m.add_rows(X[lo:hi], (ptr[lo:hi + 1], idx, val), ids=ids[lo:hi], **{k: v[lo:hi] for k, v in cols.items()})
        m.finalize()
        if hi < N:           # a list evaluated between the appends: the HBM columns grow under it
            spec = IN("doc_id", _q("zzz"), _q("doc7"))
            got = _bits(m._global_device_mask('doc_id in ["zzz", "doc7"]'))
            assert np.array_equal(got[:hi], expected(spec, m._columns(), hi)) and not got[hi:].any()
        lo = hi
    return m


TAIL_A, TAIL_B, TAIL_Z = _q(P16 + "-tail-A"), _q(P16 + "-tail-B"), _q(P16 + "-tail-Z")
TIES = [
    # two members share their 16 bytes with each other and with the -tail-C and the bare rows; the tie sits under not
    (f"not (doc_id in [{TAIL_A}, {TAIL_B}, \"zzz\"])", NOT(IN("doc_id", TAIL_A, TAIL_B, '"zzz"'))),
    (f"doc_id not in [{TAIL_Z}] and chunk_index < 4", AND(NOT(IN("doc_id", TAIL_Z)), C("chunk_index < 4"))),   # ties, equals none
    # under or beside a numeric leaf: where that one is true the kernel decides, elsewhere the tie stays
    (f"doc_id in [{TAIL_A}, {TAIL_Z}, \"abc\"] or entropy > 0.5", OR(IN("doc_id", TAIL_A, TAIL_Z, '"abc"'), C("entropy > 0.5"))),
    # under and beside a numeric leaf: where that one is false the kernel decides
    (f"doc_id in [{TAIL_B}, \"{STRADDLE}é\"] and chunk_index < 2", AND(IN("doc_id", TAIL_B, f'"{STRADDLE}é"'), C("chunk_index < 2"))),
    (f"not doc_id == {TAIL_A} and (chunk_index in [0, 1, 2] or doc_id > {TAIL_B})",
     AND(NOT(C(f"doc_id == {TAIL_A}")), OR(IN("chunk_index", "0", "1", "2"), C(f"doc_id > {TAIL_B}")))),
    (f"!(doc_id in [{TAIL_A}] || doc_id in [{TAIL_B}, \"\"]) && entropy in [0.1, 0.5, 0.9]",
     AND(NOT(OR(IN("doc_id", TAIL_A), IN("doc_id", TAIL_B, '""'))), IN("entropy", "0.1", "0.5", "0.9"))),
]


def _string_members(spec):
    if spec[0] == "in":
        return [oracle_literal for oracle_literal in spec[2] if oracle_literal.startswith('"')]
    if spec[0] == "cmp":
        lit = spec[1].split(" ", 2)[2]
        return [lit] if lit.startswith('"') else []
    return [m for child in spec[1:] for m in _string_members(child)]


def test_ties_are_settled_on_the_full_strings(gpu, collection):
    m = _manager(collection)
    try:
        dev, host_cols = m._dev_filters, m._columns()
        doc16 = np.array([d.encode("utf-8")[:16].ljust(16, b"\0") for d in collection[3]["doc_id"]], dtype=object)
        for expr, spec in TIES:
            want = expected(spec, host_cols, N)
            assert 0 < want.sum() < N, expr
            before = dict(dev.stats)
            mask, kept = dev.evaluate(expr, N)
            got = _bits(mask)
            assert np.array_equal(got[:N], want) and not got[N:].any() and kept == int(want.sum()), expr
            assert dev.stats["expr_evaluations"] == before["expr_evaluations"] + 1
            assert dev.stats["undecided_rows"] > before["undecided_rows"], expr          # the settle path ran
            # the kernel's own answer, before the host settles anything
            leaves, program = dev._terms(expr, N)
            raw = torch.empty(2 * mask.shape[0], dtype=torch.uint8, device=mask.device)
            counts = torch.zeros(2, dtype=torch.int32, device=mask.device)
            nat.filter_eval_expr_dev(leaves, program.codes, N, 0, raw.data_ptr(), raw.data_ptr() + mask.shape[0], counts.data_ptr(),
                                     torch.cuda.current_stream(mask.device).cuda_stream)
            torch.cuda.synchronize()
            sure, und = _bits(raw[:mask.shape[0]])[:N], _bits(raw[mask.shape[0]:])[:N]
            assert und.any() and not (sure & und).any(), expr
            assert counts.tolist() == [int(sure.sum()), int(und.sum())]
            assert not (sure & ~want).any(), expr                                       # decided true: true
            assert not (~sure & ~und & want).any(), expr                                # decided false: false
            member16 = {json.loads(lit).encode("utf-8")[:16].ljust(16, b"\0") for lit in _string_members(spec)}
            tied = np.array([d in member16 for d in doc16])
            assert not (und & ~tied).any(), expr                     # only a row whose 16 bytes equal a member's is undecided
            assert dev.stats["undecided_rows"] - before["undecided_rows"] == int(und.sum())
    finally:
        asyncio.run(m.close())


SEARCH_EXPR = f'doc_id in ["zzz", {TAIL_A}, "émile", "doc3", "nope"] or entropy > 0.8'
SEARCH_SPEC = OR(IN("doc_id", '"zzz"', TAIL_A, '"émile"', '"doc3"'), C("entropy > 0.8"))
GROUP_EXPR = f'doc_id in ["zzz", {TAIL_B}, "doc3", "doc4", "doc5", "abc", ""] and chunk_index not in [5]'
GROUP_SPEC = AND(IN("doc_id", '"zzz"', TAIL_B, '"doc3"', '"doc4"', '"doc5"', '"abc"', '""'), NOT(IN("chunk_index", "5")))


def test_manager_searches_groups_and_deletes_under_lists(gpu, collection):
    X, (ptr, idx, val), ids, cols = collection
    rng = np.random.default_rng(77)
    m = _manager(collection)
    try:
        dev, host_cols = m._dev_filters, m._columns()
        # ---- a conjunction, however it is spelled, still takes hr_filter_eval_dev
        base = dev.stats["expr_evaluations"]
        for expr, spec in (('doc_id >= "abc" and entropy <= 0.5', AND(C('doc_id >= "abc"'), C("entropy <= 0.5"))),
                           ('(doc_id >= "abc") AND entropy <= 0.5 && (chunk_index != 2)',
                            AND(C('doc_id >= "abc"'), C("entropy <= 0.5"), C("chunk_index != 2")))):
            got = _bits(m._global_device_mask(expr))
            assert np.array_equal(got[:N], expected(spec, host_cols, N)), expr
        assert dev.stats["expr_evaluations"] == base and dev.stats["evaluations"] >= 2

        # ---- dense, sparse and hybrid search under a list-or-comparison mask: the oracle's ids and scores
        keep = expected(SEARCH_SPEC, host_cols, N)
        assert 100 < keep.sum() < N - 100
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
            sq = {"indices": SQ[b][0].tolist(), "values": SQ[b][1].tolist()}
            hits = asyncio.run(m.search(sq, "sparse_index", k, SEARCH_EXPR, sp))
            live = si[b] >= 0
            assert live.any()
            assert [h["_row"] for h in hits] == si[b][live].tolist() and [h["score"] for h in hits] == [float(x) for x in ss[b][live]]
            res = asyncio.run(m.hybrid_search(Q[b], sq, top_k, SEARCH_EXPR, (0.7, 0.3), sparse_params=sp))
            assert res is not None, "the hybrid round did not answer"
            fi, fs, _ = oracle.rrf(di[b][di[b] >= 0], si[b][si[b] >= 0], (), 0.7, 0.3, 0.0, 60)
            assert [hit["_row"] for hit, _, _ in res] == fi[:top_k].tolist()
            assert [score for _, score, _ in res] == [float(x) for x in fs[:top_k]]
        assert dev.stats["expr_evaluations"] == base + 1          # one evaluation: the mask is kept per expression

        # ---- a grouped search under a list: the first chunk of every document of the oracle's ranking
        gkeep = expected(GROUP_SPEC, host_cols, N)
        assert 50 < gkeep.sum() < N
        gi, gs = oracle.dense_search(X, Q[:1], 256, oracle.COSINE, np.packbits(gkeep, bitorder="little"))
        seen, want = set(), []
        for r, s in zip(gi[0].tolist(), gs[0].tolist()):
            if r >= 0 and cols["doc_id"][r] not in seen:
                seen.add(cols["doc_id"][r])
                want.append((r, float(s)))
        assert (gi[0] >= 0).sum() == min(256, gkeep.sum()) and len(want) >= 5
        got = asyncio.run(m.search(Q[0], "semantic_index", 5, GROUP_EXPR, group_by_field="doc_id"))
        assert [(h["_row"], h["score"]) for h in got] == want[:5]

        # ---- the caps: refused in the user's terms, before a column or a set goes up
        before = dict(dev.stats)
        many_strings = "doc_id in [" + ", ".join(f'"k{i}"' for i in range(4097)) + "]"
        many_ints = "redundancy > 2 or token_count in [" + ", ".join(str(i) for i in range(8193)) + "]"
        many_terms = " or ".join(f"domain_density > {i}" for i in range(17))
        many_codes = "not " * 64 + "redundancy > 0.5"
        for bad, message in ((many_strings, "4096 strings or 8192 integers"), (many_ints, "4096 strings or 8192 integers"),
                             (many_terms, "up to 16 terms"), (many_codes, "up to 64 terms and operators")):
            with pytest.raises(ValueError, match=message):
                m._global_device_mask(bad)
        assert dev.stats == before and not {"redundancy", "domain_density"} & set(dev._dev)
        full = "token_count in [" + ", ".join(str(i) for i in range(8192)) + "]"            # the cap itself is taken
        assert np.array_equal(_bits(m._global_device_mask(full))[:N], np.ones(N, bool))

        # ---- one delete for a list of documents, then compact
        gone = expected(IN("doc_id", '"zzz"', TAIL_A, '"doc1"'), host_cols, N)
        assert 0 < gone.sum() < N and gone.sum() % 8 != 0
        epoch = m._delete_epoch
        asyncio.run(m.delete_by_filter("semantic_index", f'doc_id in ["zzz", {TAIL_A}, "doc1"]'))
        assert m._delete_epoch == epoch + 1 and np.array_equal(m._deleted[:N], gone)
        got = _bits(m._global_device_mask(SEARCH_EXPR))
        assert np.array_equal(got[:N], keep & ~gone) and not got[N:].any()
        stats = m.compact()
        survivors = N - int(gone.sum())
        assert stats["rows_after"] == survivors
        assert m.collections["semantic_index"].num_entities == survivors
        after = _bits(m._global_device_mask(SEARCH_EXPR))
        assert np.array_equal(after[:survivors], keep[~gone]) and not after[survivors:].any()
    finally:
        asyncio.run(m.close())
