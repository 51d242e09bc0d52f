"""The filter language beyond the flat conjunction, without a GPU: `in` lists, `or`, `not`, parentheses.

The parser (precedence, spellings, what a quoted string may hold, every refusal with the term in its message);
filters.evaluate against the oracle composed leaf by leaf (filter_expr_oracle.py) on the 4000-row column set of
test_host_logic.test_filter_expression_evaluates_to_row_mask; what parsed before parses to the same thing; the manager in
its host form (search, delete_by_filter, a synthetic collection); the retriever's `$in` / `$nin` option."""
import asyncio
import json
import os

import numpy as np
import pytest

import oracle
from advanced_rag import filters as F
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.retrieval import HybridRetriever, RetrievalConfig
from filter_expr_oracle import AND, C, IN, NOT, OR, expected

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def cmp(field, op, value):
    return ("cmp", field, op, value)


A, B, Cc, D = cmp("a", "==", 1), cmp("b", "==", 2), cmp("c", "==", 3), cmp("d", "<", 4)


# ---- the parser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expr,tree", [
    ("a == 1 or b == 2 and c == 3", ("or", A, ("and", B, Cc))),                       # and binds tighter than or
    ("a == 1 and b == 2 or c == 3", ("or", ("and", A, B), Cc)),
    ("not a == 1 and b == 2", ("and", ("not", A), B)),                                # not binds tighter than and
    ("not (a == 1 or b == 2)", ("not", ("or", A, B))),
    ("not not a == 1", ("not", ("not", A))),
    ("a == 1 or b == 2 or c == 3", ("or", ("or", A, B), Cc)),                         # left to right
    ("((a == 1))", A),
    ("(a == 1 or (b == 2 and (c == 3 or d < 4))) and a == 1", ("and", ("or", A, ("and", B, ("or", Cc, D))), A)),
    ("a == 1 && b == 2 || !c == 3", ("or", ("and", A, B), ("not", Cc))),
    ("a == 1 AND b == 2 OR NOT c == 3", ("or", ("and", A, B), ("not", Cc))),
    ("!(a == 1)", ("not", A)),
    ("!(a==1)&&b==2", ("and", ("not", A), B)),
    ("a != 1", cmp("a", "!=", 1)),
    ("a!=1", cmp("a", "!=", 1)),
    ("!a != 1", ("not", cmp("a", "!=", 1))),
    ("d<4", D),
    ("d < -4.5e-3", cmp("d", "<", -4.5e-3)),
    ("a == true or a == False", ("or", cmp("a", "==", True), cmp("a", "==", False))),
    ('doc_id == "x and y" or doc_id == "p or q"', ("or", cmp("doc_id", "==", "x and y"), cmp("doc_id", "==", "p or q"))),
    ('doc_id == "in [" and doc_id != "]"', ("and", cmp("doc_id", "==", "in ["), cmp("doc_id", "!=", "]"))),
    ('doc_id == "a, b" or doc_id == "q\\"x) or (\\\\"', ("or", cmp("doc_id", "==", "a, b"), cmp("doc_id", "==", 'q"x) or (\\'))),
    ('doc_id in ["a, b", "x\\" or \\"y"]', ("in", "doc_id", ["a, b", 'x" or "y'])),
    ('doc_id in [" and ", " or ", "in [", "]", ",", "not"]', ("in", "doc_id", [" and ", " or ", "in [", "]", ",", "not"])),
    ('doc_id not in ["a"]', ("not", ("in", "doc_id", ["a"]))),
    ('doc_id NOT IN ["a"]', ("not", ("in", "doc_id", ["a"]))),
    ('not doc_id in ["a"]', ("not", ("in", "doc_id", ["a"]))),
    ("chunk_index in []", ("in", "chunk_index", [])),
    ("chunk_index in [ ]", ("in", "chunk_index", [])),
    ('doc_id in[]', ("in", "doc_id", [])),
    ("chunk_index in[1,2 ,3 , 4]", ("in", "chunk_index", [1, 2, 3, 4])),
    ("  chunk_index   not   in   [ 1 ]  ", ("not", ("in", "chunk_index", [1]))),
    ("chunk_index in [true, False, 7]", ("in", "chunk_index", [True, False, 7])),
    ("entropy in [1, 0.5, -inf, 1e-3]", ("in", "entropy", [1, 0.5, float("-inf"), 1e-3])),
    ("chunk_index in [-9223372036854775808, 9223372036854775807]", ("in", "chunk_index", [-(1 << 63), (1 << 63) - 1])),
    ('doc_id in ["a"] and not (chunk_index in [0, 1])',
     ("and", ("in", "doc_id", ["a"]), ("not", ("in", "chunk_index", [0, 1])))),
])
def test_parse_tree(expr, tree):
    assert F.parse_tree(expr) == tree


@pytest.mark.parametrize("expr,named", [
    ('doc_id in ["a", 1]', 'doc_id in ["a", 1]'),                                     # strings and numbers mixed
    ('chunk_index == 1 or entropy in [0.5, "x"]', 'entropy in [0.5, "x"]'),
    ("chunk_index in [1, 2.5]", "chunk_index in [1, 2.5]"),                           # a float in an INT64 field's list
    ("token_count in [1e3]", "token_count in [1000.0]"),
    ("chunk_index in [9223372036854775808]", "9223372036854775808"),                  # outside int64
    ("entropy > 0.5 and token_count not in [1, -9223372036854775809]", "-9223372036854775809"),
    ('chunk_index in ["1"]', 'chunk_index in ["1"]'),                                 # a string in a numeric field's list
    ('entropy in ["0.5"]', 'entropy in ["0.5"]'),
    ("doc_id in [1, 2]", "doc_id in [1, 2]"),                                         # a number in a string field's list
    ("timestamp in [2024]", "timestamp in [2024]"),
    ("chunk_index in [1, 2,]", "chunk_index in [1, 2,]"),                             # a trailing comma
    ('entropy < 1 or doc_id in ["a",]', 'doc_id in ["a",]'),
    ("chunk_index in [,]", "chunk_index in [,]"),
    ("chunk_index in [1 2]", "chunk_index in [1 2]"),
    ("chunk_index in [1, 2", "chunk_index in [1, 2"),
    ("chunk_index in 1", "chunk_index in 1"),
    ("(chunk_index == 1", "(chunk_index == 1"),                                       # unbalanced parentheses
    ("chunk_index == 1)", "chunk_index == 1)"),
    ("((chunk_index == 1) or entropy > 1", "((chunk_index == 1) or entropy > 1"),
    ("()", ")"),
    ('doc_id like "a%"', "doc_id like"),                                              # the rest of Milvus' language
    ('doc_id LIKE "a%"', "doc_id LIKE"),
    ("chunk_index + 1 > 2", "chunk_index +"),
    ("chunk_index * 2 == 4", "chunk_index *"),
    ("chunk_index % 2 == 0", "chunk_index %"),
    ("1 < chunk_index < 5", "1 < chunk_index"),
    ("0 < chunk_index", "0 < chunk_index"),
    ("chunk_index < 5 < 6", "chunk_index < 5 < 6"),
    ("chunk_index < token_count", "chunk_index < token_count"),
    ("chunk_index == token_count or entropy > 1", "chunk_index == token_count"),
    ('json_contains(metadata_json, "a")', "json_contains("),
    ('metadata_json["k"] == 1', 'metadata_json['),
    ("array_length(tags) > 1", "array_length("),
    ("chunk_index", "chunk_index"),
    ("chunk_index ==", "chunk_index =="),
    ("chunk_index == 1 or", "chunk_index == 1 or"),
    ("chunk_index == 1 and and entropy > 1", "and entropy"),
    ("not", "not"),
    ("chunk_index = 1", "chunk_index ="),
    ("chunk_index == 'a'", "'a'"),
    ('doc_id == "open', '"open'),
])
def test_parse_tree_refuses_and_names_the_term(expr, named):
    with pytest.raises(ValueError) as ei:
        F.parse_tree(expr)
    assert named in str(ei.value), str(ei.value)
    with pytest.raises(ValueError):
        F.evaluate(expr, BIG, N)
    with pytest.raises(ValueError):
        F.fields(expr)


def test_the_empty_expression_is_no_tree():
    with pytest.raises(ValueError, match="empty filter expression"):
        F.parse_tree("  ")
    assert F.parse("") == [] and F.evaluate("", BIG, N).all()        # as before: no term, every row


def test_fields():
    assert F.fields('doc_id == "a" and entropy >= 0.2') == {"doc_id", "entropy"}
    assert F.fields('doc_id in ["x"] or not (chunk_index in [1] and chunk_index > 5)') == {"doc_id", "chunk_index"}
    assert F.fields("a == 1 AND (b == 2)") == {"a", "b"}


# ---- filters.evaluate against the composed oracle -------------------------------------------------------------------------------
N = 4000
POOL = ['doc"123', "a\\b", "a >= b", "x and y", 'q"uo\\te', "", "0123456789abcdef-tail-A", "0123456789abcdef-tail-B", "doc9",
        "doc95", "ünï"]


def _big():
    rng = np.random.default_rng(3)
    return {"chunk_index": rng.integers(0, 12, N), "token_count": rng.integers(0, 2000, N),
            "entropy": (rng.integers(0, 11, N) / 10).astype(np.float32), "redundancy": (rng.integers(0, 11, N) / 10).astype(np.float32),
            "domain_density": rng.random(N).astype(np.float32), "doc_id": np.array([POOL[i] for i in rng.integers(0, len(POOL), N)]),
            "chunk_id": np.array([f"d::{i % 3}::abcd123{i % 10}" for i in range(N)]),
            "timestamp": np.array([f"202{i % 6}-0{1 + i % 9}-1{i % 9}" for i in range(N)])}


BIG = _big()
EXPRESSIONS = [
    ('doc_id in ["doc9", "doc95"]', IN("doc_id", '"doc9"', '"doc95"')),
    ('doc_id not in ["doc9", "", "ünï"]', NOT(IN("doc_id", '"doc9"', '""', '"ünï"'))),
    ('doc_id in ["0123456789abcdef-tail-A"]', IN("doc_id", '"0123456789abcdef-tail-A"')),     # -tail-B shares its 16 bytes
    ('doc_id in ["0123456789abcdef-tail-A", "0123456789abcdef-tail-B", "0123456789abcdef"]',
     IN("doc_id", '"0123456789abcdef-tail-A"', '"0123456789abcdef-tail-B"')),
    (r'doc_id in ["x and y", "a >= b", "doc\"123", "a\\b"]', IN("doc_id", '"x and y"', '"a >= b"', r'"doc\"123"', r'"a\\b"')),
    ("chunk_index in [0, 1, 11]", IN("chunk_index", "0", "1", "11")),
    ("chunk_index not in [3]", NOT(IN("chunk_index", "3"))),
    ("chunk_index in [true, False, 40]", IN("chunk_index", "1", "0")),
    ("entropy in [0.3, 0.7, 1]", IN("entropy", "0.3", "0.7", "1")),
    ("entropy not in [0.30000001192092896, 0, nan]", NOT(IN("entropy", "0.3", "0"))),
    ("redundancy in [0.1, 0.1, 0.10000000149011612, -0.0]", IN("redundancy", "0.1", "0")),
    ("token_count in [5, 1999, 12345678] or chunk_index == 4", OR(IN("token_count", "5", "1999"), C("chunk_index == 4"))),
    ('timestamp < "2023" or entropy > 0.8', OR(C('timestamp < "2023"'), C("entropy > 0.8"))),
    ("not entropy > 0.8", NOT(C("entropy > 0.8"))),
    ('not (chunk_index in [0, 1] or doc_id == "doc9")', NOT(OR(IN("chunk_index", "0", "1"), C('doc_id == "doc9"')))),
    ("chunk_index == 1 or chunk_index == 2 and entropy >= 0.5",
     OR(C("chunk_index == 1"), AND(C("chunk_index == 2"), C("entropy >= 0.5")))),
    ("not chunk_index == 1 and entropy >= 0.5", AND(NOT(C("chunk_index == 1")), C("entropy >= 0.5"))),
    ("(chunk_index == 1 or chunk_index == 2) and entropy >= 0.5",
     AND(OR(C("chunk_index == 1"), C("chunk_index == 2")), C("entropy >= 0.5"))),
    ('doc_id in ["doc9"] && !(chunk_index in [0, 1]) || redundancy <= 0.1',
     OR(AND(IN("doc_id", '"doc9"'), NOT(IN("chunk_index", "0", "1"))), C("redundancy <= 0.1"))),
    ('chunk_id in ["d::0::abcd1230", "d::2::abcd1235"] OR NOT timestamp >= "2021"',
     OR(IN("chunk_id", '"d::0::abcd1230"', '"d::2::abcd1235"'), NOT(C('timestamp >= "2021"')))),
    ("doc_id in [] or chunk_index == 5", C("chunk_index == 5")),
    ("token_count not in [] and chunk_index >= 2.5", C("chunk_index >= 2.5")),
    (r'((entropy in [0.5] or (domain_density < 0.25 and not (doc_id in ["a\\b"]))) and token_count >= 1e3)',
     AND(OR(IN("entropy", "0.5"), AND(C("domain_density < 0.25"), NOT(IN("doc_id", r'"a\\b"')))), C("token_count >= 1e3"))),
    ('doc_id != "doc9" and not doc_id in ["doc95"]', AND(C('doc_id != "doc9"'), NOT(IN("doc_id", '"doc95"')))),
    (r'redundancy in [0.1, 0.2] and doc_id in ["q\"uo\\te", "ünï"] or token_count in [7]',
     OR(AND(IN("redundancy", "0.1", "0.2"), IN("doc_id", r'"q\"uo\\te"', '"ünï"')), IN("token_count", "7"))),
    ('domain_density > 0.5 and (timestamp in ["2020-01-10", "2021-02-11"] or chunk_index not in [0,1,2,3,4,5,6,7,8])',
     AND(C("domain_density > 0.5"), OR(IN("timestamp", '"2020-01-10"', '"2021-02-11"'),
                                       NOT(IN("chunk_index", *"012345678"))))),
    ('timestamp < "2023" AND (entropy > 0.8)', AND(C('timestamp < "2023"'), C("entropy > 0.8"))),   # a conjunction, respelled
]


def test_evaluate_equals_the_composed_oracle():
    assert len(EXPRESSIONS) >= 20
    for expr, spec in EXPRESSIONS:
        want = expected(spec, BIG, N)
        assert 0 < want.sum() < N, expr          # the expression keeps a row and drops a row
        got = F.evaluate(expr, BIG, N)
        assert got.dtype == bool and np.array_equal(got, want), (expr, int(got.sum()), int(want.sum()))
    # a list names rows only through its members: no member, no row; every row of the pool, every row
    assert not F.evaluate("doc_id in []", BIG, N).any() and F.evaluate("entropy not in []", BIG, N).all()
    assert not F.evaluate("entropy in [nan]", BIG, N).any()
    for bad in ("nofield in [1]", 'nofield in ["a"] or chunk_index == 1'):
        with pytest.raises(ValueError, match="unknown filter field"):
            F.evaluate(bad, BIG, N)


def test_float_membership_is_float32_equality():
    cols = {"entropy": np.array([0.0, -0.0, np.nan, np.inf, 0.3, 0.1 + 0.2, 1e-45], np.float32)}
    assert F.evaluate("entropy in [0]", cols, 7).tolist() == [True, True, False, False, False, False, False]
    assert F.evaluate("entropy in [-0.0, nan, inf]", cols, 7).tolist() == [True, True, False, True, False, False, False]
    assert F.evaluate("entropy in [0.30000001192092896]", cols, 7).tolist() == [False, False, False, False, True, True, False]
    assert F.evaluate("entropy not in [0.3, 1e39]", cols, 7).tolist() == [True, True, True, False, False, False, True]


# ---- what parsed before -------------------------------------------------------------------------------------------------------------
PARSED_TODAY = {
    'doc_id == "doc\\"123" and entropy >= 0.2': [("doc_id", "==", 'doc"123'), ("entropy", ">=", 0.2)],
    "redundancy < 0.5 and redundancy > 0.1 and redundancy == 0.2 and redundancy != 0.3 and chunk_index == 1":
        [("redundancy", "<", 0.5), ("redundancy", ">", 0.1), ("redundancy", "==", 0.2), ("redundancy", "!=", 0.3),
         ("chunk_index", "==", 1)],
    'doc_id == "a\\\\b"': [("doc_id", "==", "a\\b")],
    'timestamp >= "2024-01-01" and timestamp < "2025-01-01"': [("timestamp", ">=", "2024-01-01"), ("timestamp", "<", "2025-01-01")],
    'token_count <= 512 and domain_density == 0.5 and chunk_id == "d::0::abcd1234"':
        [("token_count", "<=", 512), ("domain_density", "==", 0.5), ("chunk_id", "==", "d::0::abcd1234")],
    "chunk_index == True": [("chunk_index", "==", True)],
    "entropy >= 1": [("entropy", ">=", 1)],
    'doc_id == "ünï"': [("doc_id", "==", "ünï")],
    "chunk_index == true and entropy != 0.30000001192092896": [("chunk_index", "==", True), ("entropy", "!=", 0.30000001192092896)],
    "token_count >= 1e3": [("token_count", ">=", 1000.0)],
    "chunk_index >= 2.5": [("chunk_index", ">=", 2.5)],
    'doc_id < "0123456789abcdef-tail-B" and doc_id >= "0123456789abcdef"':
        [("doc_id", "<", "0123456789abcdef-tail-B"), ("doc_id", ">=", "0123456789abcdef")],
}


def test_what_parsed_before_parses_to_the_same():
    with open(os.path.join(GOLD, "g4_filters.json")) as f:
        golden = [c["expr"] for c in json.load(f) if c.get("expr")]
    assert set(golden) <= set(PARSED_TODAY)
    for expr, terms in PARSED_TODAY.items():
        got = F.parse(expr)
        assert got == terms and [type(v) for _, _, v in got] == [type(v) for _, _, v in terms], expr
        assert F.lower(expr) == (terms, None), expr
        assert np.array_equal(F.evaluate(expr, BIG, N), oracle.filter_mask(expr, BIG, N)), expr
    # parse keeps to the flat conjunction
    for expr in ('doc_id in ["a"]', 'doc_id == "a" or doc_id == "b"', "not chunk_index == 1", "(chunk_index == 1)",
                 "chunk_index == 1 AND entropy > 1", "chunk_index == 1 && entropy > 1", 'doc_id == "a" || doc_id == "b"'):
        with pytest.raises(ValueError):
            F.parse(expr)
    # ... and a conjunction spelled the new way is still one: the device takes today's entry point for it
    assert F.lower("chunk_index == 1 AND (entropy > 1)") == ([("chunk_index", "==", 1), ("entropy", ">", 1)], None)
    assert F.lower("chunk_index == 1 or entropy > 1")[0] is None


# ---- the manager in its host form ---------------------------------------------------------------------------------------------------------
class _OracleShard:
    """Stands in for a ShardHandle: the oracle over the rows it was given (as in test_group_host.py)."""

    def __init__(self, sparse_dim):
        self.X = None
        self.ptr, self.idx, self.val = np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
        self.device, self.sparse_dim = 0, sparse_dim

    num_rows = property(lambda self: 0 if self.X is None else self.X.shape[0])
    num_sparse_rows = property(lambda self: len(self.ptr) - 1)

    def add_dense(self, rows):
        self.X = rows.copy() if self.X is None else np.concatenate([self.X, rows])

    def add_sparse(self, ptr, idx, val):
        self.idx = np.concatenate([self.idx, idx[ptr[0]:ptr[-1]]])
        self.val = np.concatenate([self.val, val[ptr[0]:ptr[-1]]])
        self.ptr = np.concatenate([self.ptr, ptr[1:] - ptr[0] + self.ptr[-1]])

    def search_dense(self, q, k, mask=None):
        return oracle.dense_search(self.X, q, k, oracle.COSINE, mask)

    def search_sparse(self, queries, k, drop, mask=None):
        return oracle.sparse_search(self.ptr, self.idx, self.val, queries, k, drop, mask)

    def finalize(self):
        pass

    def close(self):
        pass


M_ROWS, DIM, V = 150, 8, 32


def test_manager_host_form_searches_and_deletes_under_in_lists():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((M_ROWS, DIM)).astype(np.float32)
    idx = np.sort(rng.integers(0, V // 4, size=(M_ROWS, 4)) + np.arange(4) * (V // 4), axis=1).astype(np.int32)
    csr = (np.arange(M_ROWS + 1, dtype=np.int64) * 4, idx.reshape(-1), np.ones(M_ROWS * 4, np.float32))
    docs = [("a", "b", "c", "d, e", 'q"x')[r % 5] for r in range(M_ROWS)]
    chunk = [r % 4 for r in range(M_ROWS)]
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, connect=False, enable_domain=False)
    mgr.attach_shards([_OracleShard(V), _OracleShard(V)])
    try:
        for lo in range(0, M_ROWS, 60):
            hi = min(M_ROWS, lo + 60)
            mgr.add_rows(X[lo:hi], (csr[0][lo:hi + 1], csr[1], csr[2]), ids=[f"c{r}" for r in range(lo, hi)],
                         doc_id=docs[lo:hi], chunk_index=chunk[lo:hi])
        assert mgr._filters_on_device() is None
        expr = r'doc_id in ["a", "d, e", "q\"x", "nope"] and not (chunk_index in [0, 1])'
        want = {r for r in range(M_ROWS) if docs[r] in ("a", "d, e", 'q"x') and chunk[r] not in (0, 1)}
        assert 0 < len(want) < M_ROWS
        sq = {"indices": list(range(V)), "values": [1.0] * V}
        for query, collection in ((X[:9].sum(axis=0), "semantic_index"), (sq, "sparse_index")):
            hits = asyncio.run(mgr.search(query, collection, top_k=M_ROWS, filters=expr))
            assert {h["_row"] for h in hits} == want, collection
            ranking = asyncio.run(mgr.search(query, collection, top_k=M_ROWS))
            assert [h["_row"] for h in hits] == [h["_row"] for h in ranking if h["_row"] in want], collection   # in rank order
        epoch = mgr._delete_epoch
        asyncio.run(mgr.delete_by_filter("semantic_index", 'doc_id in ["a", "b"]'))
        assert mgr._delete_epoch == epoch + 1                                       # one call, one pass
        assert mgr._deleted[:M_ROWS].tolist() == [d in ("a", "b") for d in docs]
        hits = asyncio.run(mgr.search(X[:9].sum(axis=0), "semantic_index", top_k=M_ROWS, filters=expr))
        assert {h["_row"] for h in hits} == {r for r in want if docs[r] != "a"}
    finally:
        asyncio.run(mgr.close())


def test_synthetic_collection_takes_lists_on_chunk_index_only():
    rng = np.random.default_rng(9)
    X = rng.standard_normal((95, DIM)).astype(np.float32)
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=0, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard(0)])
    try:
        mgr.add_rows_synthetic(X)
        q = X[:30].sum(axis=0)
        hits = asyncio.run(mgr.search(q, "semantic_index", top_k=95, filters="chunk_index in [1, 3] or chunk_index == 7"))
        assert {h["_row"] for h in hits} == {r for r in range(95) if r % 10 in (1, 3, 7)}
        with pytest.raises(ValueError, match=r"bulk-ingested without payload columns: only chunk_index \(= row % 10\) can be "
                                             r"filtered on, not \['doc_id'\]"):
            asyncio.run(mgr.search(q, "semantic_index", top_k=5, filters='doc_id in ["x"]'))
    finally:
        asyncio.run(mgr.close())


# ---- the retriever's dict form ------------------------------------------------------------------------------------------------------------
def test_retriever_list_operators_are_an_option():
    on = HybridRetriever(index_manager=None, config=RetrievalConfig(extended_filter_operators=True))
    expr = on._build_filter_expression({"doc_id": {"$in": ["a", 'q"x', "b\\c"]}, "chunk_index": {"$nin": [1, 2], "$gte": 0},
                                        "entropy": {"$in": [0.5, 1, True]}})
    assert expr == r'doc_id in ["a", "q\"x", "b\\c"] and chunk_index not in [1, 2] and chunk_index >= 0 and entropy in [0.5, 1, True]'
    assert F.parse_tree(expr) == ("and", ("and", ("and", ("in", "doc_id", ["a", 'q"x', "b\\c"]), ("not", ("in", "chunk_index", [1, 2]))),
                                          cmp("chunk_index", ">=", 0)), ("in", "entropy", [0.5, 1, True]))
    assert on._build_filter_expression({"doc_id": {"$in": []}}) == "doc_id in []"
    assert all(p.extended_filter_operators for p in on.profiles.values())         # the request's profile keeps the option
    for bad in ({"doc_id": {"$in": "a"}}, {"doc_id": {"$in": ["a", 1]}}, {"doc_id": {"$nin": [None]}}, {"domain": {"$in": ["a"]}},
                {"doc_id": {"$all": ["a"]}}):
        with pytest.raises(ValueError):
            on._build_filter_expression(bad)
    off = HybridRetriever(index_manager=None)
    assert RetrievalConfig().extended_filter_operators is False
    for refused in ({"doc_id": {"$in": ["a"]}}, {"chunk_index": {"$nin": [1]}}):
        with pytest.raises(ValueError, match="Invalid operator"):
            off._build_filter_expression(refused)
    with open(os.path.join(GOLD, "g4_filters.json")) as f:
        for c in json.load(f):
            if "error" in c:
                with pytest.raises(Exception) as ei:
                    off._build_filter_expression(c["filters"])
                assert type(ei.value).__name__ == c["error"], c
            else:
                assert off._build_filter_expression(c["filters"]) == c["expr"], c
                if c["expr"]:
                    assert on._build_filter_expression(c["filters"]) == c["expr"], c
