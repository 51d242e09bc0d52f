"""TEXT_MATCH(content, "words"[, minimum_should_match=m]) without a GPU: the grammar, the analyzer, filters.evaluate, the
word-set column, a CPU manager and the dict form of the retriever.

Every expected row set is the restatement `len(set(analyze(content)) & set(analyze(text))) >= m` (no row when the query has
no word), written out below; the analyzer itself is held to the BM25 tokenizer."""
import asyncio
import re

import numpy as np
import pytest

import oracle
from advanced_rag import bm25
from advanced_rag import filters as F
from advanced_rag.columns import PayloadColumns
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.retrieval import HybridRetriever, RetrievalConfig


def words_of(text):
    return set(re.findall(r"\w+", text.lower()))


def restated(contents, text, m=1):
    """The match rule, restated: at least m distinct query words among the row's words; a query without a word matches nothing."""
    q = words_of(text)
    return np.array([bool(q) and len(words_of(c) & q) >= m for c in contents], dtype=bool)


# ---- grammar ----------------------------------------------------------------------------------------------------------------------
M = lambda text, m=1: ("match", "content", text, m)


@pytest.mark.parametrize("expr, tree", [
    ('TEXT_MATCH(content, "disk failure")', M("disk failure")),
    ('text_match(content, "disk failure")', M("disk failure")),
    ('TEXT_MATCH ( content , "a b c" , minimum_should_match = 2 )', M("a b c", 2)),
    ('text_match(content,"a",minimum_should_match=16384)', M("a", 16384)),
    ('TEXT_MATCH(content, "")', M("")),
    # what stands inside the quotes belongs to the string
    ('TEXT_MATCH(content, "a) or (b")', M("a) or (b")),
    ('TEXT_MATCH(content, "x, minimum_should_match=3")', M("x, minimum_should_match=3")),
    (r'TEXT_MATCH(content, "say \"hi\", then)")', M('say "hi", then)')),
    # precedence: not > and > or, as for every other leaf
    ('not TEXT_MATCH(content, "a") and chunk_index == 1 or text_match(content, "b", minimum_should_match=2)',
     ("or", ("and", ("not", M("a")), ("cmp", "chunk_index", "==", 1)), M("b", 2))),
    ('chunk_index in [1, 2] && (TEXT_MATCH(content, "a") || !text_match(content, "b"))',
     ("and", ("in", "chunk_index", [1, 2]), ("or", M("a"), ("not", M("b"))))),
    ('TEXT_MATCH(content, "a") and TEXT_MATCH(content, "b") and entropy > 0.5',
     ("and", ("and", M("a"), M("b")), ("cmp", "entropy", ">", 0.5))),
])
def test_trees(expr, tree):
    assert F.parse_tree(expr) == tree
    assert "content" in F.fields(expr)
    assert F.conjunction_terms(tree) is None and F.lower(expr) == (None, tree)       # always the expression path
    assert [leaf for leaf in F.leaves(tree) if leaf[0] == "match"]
    with pytest.raises(ValueError):
        F.parse(expr)                                                                  # the flat form keeps refusing it


@pytest.mark.parametrize("expr, named", [
    ('TEXT_MATCH(doc_id, "a")', 'TEXT_MATCH(doc_id, "a")'),                           # only content is analysed
    ('TEXT_MATCH(metadata_json, "a")', 'TEXT_MATCH(metadata_json, "a")'),
    ('TEXT_MATCH(content)', "TEXT_MATCH(content)"),                                   # missing text
    ('TEXT_MATCH(content,)', "TEXT_MATCH(content,)"),
    ('TEXT_MATCH(content, 5)', "TEXT_MATCH(content, 5)"),                             # non-string text
    ('TEXT_MATCH(content, disk)', "TEXT_MATCH(content, disk)"),
    ('TEXT_MATCH("content", "a")', 'TEXT_MATCH("content", "a")'),
    ('TEXT_MATCH(content, "a", minimum_should_match=0)', "minimum_should_match=0)"),
    ('TEXT_MATCH(content, "a", minimum_should_match=1.5)', "minimum_should_match=1.5)"),
    ('TEXT_MATCH(content, "a", minimum_should_match=true)', "minimum_should_match=true)"),
    ('TEXT_MATCH(content, "a", minimum_should_match=16385)', "minimum_should_match=16385)"),
    ('TEXT_MATCH(content, "a", minimum_should_match=-1)', "minimum_should_match=-1)"),
    ('TEXT_MATCH(content, "a", minimum_should_match="2")', 'minimum_should_match="2")'),
    ('TEXT_MATCH(content, "a", minimum_should_match)', "minimum_should_match)"),
    ('TEXT_MATCH(content, "a", slop=1)', "slop"),                                     # unknown option
    ('TEXT_MATCH(content, "a", minimum_should_match=1, minimum_should_match=1)', "minimum_should_match=1, minimum_should_match=1)"),
    ('TEXT_MATCH(content, "a"', 'TEXT_MATCH(content, "a"'),                           # missing )
    ('TEXT_MATCH(content, "a" and chunk_index == 1', 'TEXT_MATCH(content, "a" and chunk_index == 1'),
    ('TEXT_MATCH content, "a")', "TEXT_MATCH content"),
    ('PHRASE_MATCH(content, "a b")', "PHRASE_MATCH("),
    ('phrase_match(content, "a b", 1)', "phrase_match("),
    ('content like "%a%"', "content like"),
    ("chunk_index = 1", "chunk_index ="),                                             # a bare = stays an error outside the leaf
    ("chunk_index == 1 and token_count = 2", "token_count ="),
])
def test_refusals_name_the_term(expr, named):
    with pytest.raises(ValueError) as ei:
        F.parse_tree(expr)
    assert named in str(ei.value), str(ei.value)
    with pytest.raises(ValueError):
        F.evaluate(expr, {"content": ["a"], "chunk_index": np.zeros(1, np.int64), "token_count": np.zeros(1, np.int64)}, 1)
    with pytest.raises(ValueError):
        F.fields(expr)


# ---- analyzer ---------------------------------------------------------------------------------------------------------------------
POOL = ["Timeout, then RETRY; timeout.", "error 0x80070057 (E_INVALIDARG)", "don't panic", "snake_case and kebab-case", "v2.5.1 / 42",
        "Ünïcode Straße ǅ", "İstanbul'da", "日本語 テキスト と english", "tabs\tand\nnewlines\r\n", "", "!!!", "  ", "a_b__c 9lives _x_",
        "é é", "x²+y³"]


def test_the_analyzer_is_the_bm25_tokenizer():
    for text in POOL + [" ".join(POOL)]:
        assert F.analyze(text) == bm25._WORD.findall(text.lower()), text
    assert F.analyze("Timeout, then RETRY; timeout.") == ["timeout", "then", "retry", "timeout"]
    assert F.analyze("don't snake_case 0x80070057") == ["don", "t", "snake_case", "0x80070057"]
    assert F.analyze("!!!") == [] and F.analyze("") == []


# ---- filters.evaluate against the restatement ---------------------------------------------------------------------------------
VOCAB = ["timeout", "retry", "disk", "failure", "confidential", "0x80070057", "snake_case", "über", "日本語", "don", "t", "error",
         "node", "raft", "leader", "quorum", "log", "commit", "apply", "snapshot", "index", "term", "vote", "follower", "heartbeat",
         "election", "append", "entries", "client", "state"]
GLUE = [" ", ", ", ". ", "; ", " (", ") ", "! ", "\n", " - ", ": "]


def make_contents(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n):
        k = int(rng.integers(0, 9)) if r % 37 else 0                     # some rows have no word at all
        ws = [VOCAB[i] for i in rng.integers(0, len(VOCAB), k)]
        ws = [w.upper() if rng.random() < 0.3 else w.capitalize() if rng.random() < 0.3 else w for w in ws]
        out.append("".join(w + GLUE[int(rng.integers(0, len(GLUE)))] for w in ws) if ws else ("" if r % 2 else "?! ..."))
    return out


N = 509
CONTENTS = make_contents(N, 5)
COLS = {"content": CONTENTS, "chunk_index": np.arange(N, dtype=np.int64) % 7,
        "entropy": (np.arange(N) % 11 / 10).astype(np.float32), "doc_id": np.asarray([f"doc{r % 9}" for r in range(N)])}
R = lambda text, m=1: restated(CONTENTS, text, m)
CASES = [
    ('TEXT_MATCH(content, "timeout")', R("timeout")),
    ('text_match(content, "TIMEOUT, Retry!")', R("timeout retry")),
    ('TEXT_MATCH(content, "timeout retry disk", minimum_should_match=2)', R("timeout retry disk", 2)),
    ('TEXT_MATCH(content, "timeout retry disk", minimum_should_match=3)', R("timeout retry disk", 3)),          # all of them
    ('TEXT_MATCH(content, "timeout retry disk", minimum_should_match=4)', np.zeros(N, bool)),                     # all + 1
    ('TEXT_MATCH(content, "timeout timeout Timeout", minimum_should_match=2)', np.zeros(N, bool)),                # one distinct word
    ('TEXT_MATCH(content, "")', np.zeros(N, bool)),
    ('TEXT_MATCH(content, "!!! ...")', np.zeros(N, bool)),
    ('TEXT_MATCH(content, "nosuchword")', np.zeros(N, bool)),
    ('TEXT_MATCH(content, "nosuchword disk")', R("disk")),
    ('TEXT_MATCH(content, "nosuchword disk", minimum_should_match=2)', np.zeros(N, bool)),
    ('not TEXT_MATCH(content, "confidential")', ~R("confidential")),
    ('TEXT_MATCH(content, "über 日本語") or chunk_index == 3', R("über 日本語") | (COLS["chunk_index"] == 3)),
    ('TEXT_MATCH(content, "don\'t") and entropy >= 0.5', R("don t") & (COLS["entropy"] >= np.float32(0.5))),
    ('TEXT_MATCH(content, "raft") and not (text_match(content, "leader quorum", minimum_should_match=2) or doc_id in ["doc1", "doc2"])',
     R("raft") & ~(R("leader quorum", 2) | np.isin(COLS["doc_id"], ["doc1", "doc2"]))),
    ('TEXT_MATCH(content, "0x80070057 snake_case")', R("0x80070057 snake_case")),
]


@pytest.mark.parametrize("expr, want", CASES)
def test_evaluate_equals_the_restatement(expr, want):
    got = F.evaluate(expr, COLS, N)
    assert got.dtype == bool and np.array_equal(got, want), expr


def test_the_cases_cover_both_outcomes():
    assert 0 < R("timeout").sum() < N and 0 < R("timeout retry disk", 3).sum() < R("timeout retry disk", 2).sum()
    assert R("über 日本語").any() and R("don t").any()


# ---- the word-set column --------------------------------------------------------------------------------------------------------------
def _payload(cols, contents, base=0):
    n = len(contents)
    cols["id"].extend(f"c{base + r}" for r in range(n))
    cols["doc_id"].extend(f"doc{(base + r) % 9}" for r in range(n))
    cols["content"].extend(contents)
    cols["timestamp"].extend("2024" for _ in range(n))
    cols["metadata_json"].extend("{}" for _ in range(n))
    for k in ("chunk_index", "token_count"):
        cols[k].extend([0] * n)
    for k in ("entropy", "redundancy", "domain_density"):
        cols[k].extend([0.0] * n)


def _check_word_sets(ws, contents):
    assert len(ws) == len(contents)
    by_id = {i: w for w, i in ws.ids.items()}
    indptr, tok = ws.indptr(), ws.tokens()
    assert indptr.dtype == np.int64 and tok.dtype == np.int32 and indptr[0] == 0 and indptr[-1] == tok.shape[0]
    for r, text in enumerate(contents):
        row = ws.row(r)
        assert np.array_equal(row, tok[indptr[r]:indptr[r + 1]])
        assert (np.diff(row) > 0).all()                                               # ascending, each id once
        assert {by_id[i] for i in row.tolist()} == words_of(text)


def test_word_sets_build_extend_and_compact():
    cols = PayloadColumns()
    first, second = CONTENTS[:200], CONTENTS[200:330]
    _payload(cols, first)
    mmr = cols.token_sets()
    mmr_ids, mmr_tok = dict(mmr.ids), mmr.tokens().copy()
    ws = cols.word_sets()
    _check_word_sets(ws, first)
    # first-seen order: the ids are 0, 1, 2, ... in the order in which the words first occur, row after row
    seen = []
    for text in first:
        for w in F.analyze(text):
            if w not in seen:
                seen.append(w)
    assert list(ws.ids) == seen and list(ws.ids.values()) == list(range(len(seen)))
    before = dict(ws.ids)
    # an append extends it; ids given once stay
    _payload(cols, second, 200)
    assert cols.word_sets() is ws
    _check_word_sets(ws, first + second)
    assert all(ws.ids[w] == i for w, i in before.items())
    # compact gathers the rows and keeps the dictionary
    keep = np.ones(330, dtype=bool)
    keep[::3] = False
    before = dict(ws.ids)
    cols.compact(keep)
    assert cols.word_sets() is ws and ws.ids == before
    _check_word_sets(ws, [c for c, k in zip(first + second, keep) if k])
    # the MMR tokens are another column with another dictionary: "timeout," stays a token of its own there
    assert cols.token_sets() is mmr and mmr is not ws
    assert all(mmr.ids[t] == i for t, i in mmr_ids.items())
    assert any(not t.isalnum() and t not in ws.ids for t in mmr.ids)
    assert np.array_equal(cols.token_sets().tokens()[:0], mmr_tok[:0]) and len(mmr) == int(keep.sum())


def test_word_sets_are_built_on_first_use_only():
    cols = PayloadColumns()
    _payload(cols, CONTENTS[:10])
    assert cols._word_sets is None
    cols.token_sets()
    assert cols._word_sets is None                     # MMR does not build them
    cols.word_sets()
    assert cols._word_sets is not None and cols._token_sets is not cols._word_sets


# ---- a CPU manager ------------------------------------------------------------------------------------------------------------------
class _OracleShard:
    """Stands in for a ShardHandle: the oracle over the rows it was given."""

    def __init__(self):
        self.X = None
        self.device, self.sparse_dim = 0, 0

    num_rows = property(lambda self: 0 if self.X is None else self.X.shape[0])
    num_sparse_rows = 0
    device_bytes = property(lambda self: 0 if self.X is None else self.X.nbytes)
    dim = property(lambda self: self.X.shape[1])

    def add_dense(self, rows):
        self.X = rows.copy() if self.X is None else np.concatenate([self.X, rows])

    def compact(self, keep=None, d_keep=0):
        self.X = self.X[np.asarray(keep, dtype=bool)]
        return self.X.shape[0], 0

    def search_dense(self, q, k, mask=None):
        return oracle.dense_search(self.X, q, k, oracle.COSINE, mask)

    def get_dense_rows(self, rows):
        return self.X[np.asarray(rows, dtype=np.int64)].astype(np.float32)

    def finalize(self):
        pass

    def close(self):
        pass


MN, DIM = 203, 12


def _manager():
    rng = np.random.default_rng(23)
    X = rng.standard_normal((MN, DIM)).astype(np.float32)
    contents = make_contents(MN, 9)
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=0, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard() for _ in range(2)])
    for lo in range(0, MN, 80):
        hi = min(MN, lo + 80)
        mgr.add_rows(X[lo:hi], None, ids=[f"c{r}" for r in range(lo, hi)], contents=contents[lo:hi],
                     doc_id=[f"doc{r // 10}" for r in range(lo, hi)], chunk_index=[r % 10 for r in range(lo, hi)])
    assert mgr._filters_on_device() is None
    return mgr, X, contents


def test_cpu_manager_search_query_and_delete():
    mgr, X, contents = _manager()
    try:
        chunk = np.arange(MN) % 10
        expr = 'TEXT_MATCH(content, "raft LEADER, quorum", minimum_should_match=2) or (text_match(content, "disk") and chunk_index < 5)'
        keep = restated(contents, "raft leader quorum", 2) | (restated(contents, "disk") & (chunk < 5))
        assert 5 < keep.sum() < MN - 5
        q = X[:7].sum(axis=0)
        di, ds = oracle.dense_search(X, q[None, :], MN, oracle.COSINE, np.packbits(keep, bitorder="little"))
        hits = asyncio.run(mgr.search(q, "semantic_index", top_k=MN, filters=expr))
        assert [h["id"] for h in hits] == [f"c{r}" for r in di[0][di[0] >= 0]] and len(hits) == int(keep.sum())
        assert asyncio.run(mgr.query("semantic_index", expr, ["count(*)"])) == [{"count(*)": int(keep.sum())}]
        assert [h["id"] for h in asyncio.run(mgr.query("semantic_index", expr))] == [f"c{r}" for r in np.flatnonzero(keep)]
        # delete every row that mentions a word: those rows are gone from every later answer
        gone = restated(contents, "confidential")
        assert 0 < gone.sum() < MN
        asyncio.run(mgr.delete_by_filter("semantic_index", 'TEXT_MATCH(content, "Confidential.")'))
        assert asyncio.run(mgr.query("semantic_index", "chunk_index >= 0", ["count(*)"])) == [{"count(*)": int((~gone).sum())}]
        assert asyncio.run(mgr.query("semantic_index", expr, ["count(*)"])) == [{"count(*)": int((keep & ~gone).sum())}]
        assert asyncio.run(mgr.query("semantic_index", 'TEXT_MATCH(content, "confidential")', ["count(*)"])) == [{"count(*)": 0}]
        mgr.compact()
        left = [c for c, g in zip(contents, gone) if not g]
        want = [f"c{r}" for r in np.flatnonzero(~gone)[restated(left, "timeout retry")]]
        assert [h["id"] for h in asyncio.run(mgr.query("semantic_index", 'TEXT_MATCH(content, "timeout retry")'))] == want
    finally:
        asyncio.run(mgr.close())


def test_a_synthetic_collection_refuses_the_leaf():
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=0, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard()])
    try:
        mgr.add_rows_synthetic(np.random.default_rng(1).standard_normal((30, DIM)).astype(np.float32))
        with pytest.raises(ValueError, match="only chunk_index"):
            asyncio.run(mgr.query("semantic_index", 'TEXT_MATCH(content, "a")', ["count(*)"]))
    finally:
        asyncio.run(mgr.close())


# ---- the dict form ------------------------------------------------------------------------------------------------------------------
def test_the_dict_form():
    on = HybridRetriever(index_manager=None, config=RetrievalConfig(extended_filter_operators=True))
    assert on._build_filter_expression({"content": {"$text_match": "disk failure"}}) == 'TEXT_MATCH(content, "disk failure")'
    expr = on._build_filter_expression({"content": {"$text_match": {"query": 'say "hi") \\ ok', "minimum_should_match": 2}},
                                        "chunk_index": {"$gte": 1}})
    assert expr == r'TEXT_MATCH(content, "say \"hi\") \\ ok", minimum_should_match=2) and chunk_index >= 1'
    assert F.parse_tree(expr) == ("and", ("match", "content", 'say "hi") \\ ok', 2), ("cmp", "chunk_index", ">=", 1))
    for bad in ({"content": {"$text_match": 5}}, {"content": {"$text_match": {"query": "a", "minimum_should_match": 0}}},
                {"content": {"$text_match": {"query": "a", "minimum_should_match": True}}},
                {"content": {"$text_match": {"query": "a", "minimum_should_match": 1.5}}},
                {"content": {"$text_match": {"query": "a", "slop": 1}}}, {"content": {"$text_match": {"minimum_should_match": 1}}},
                {"content": {"$eq": "a"}}, {"content": "a"}, {"content": {"$text_match": "a", "$eq": "b"}},
                {"doc_id": {"$text_match": "a"}}):
        with pytest.raises(ValueError):
            on._build_filter_expression(bad)
    off = HybridRetriever(index_manager=None)
    with pytest.raises(ValueError, match="Invalid filter field: content"):
        off._build_filter_expression({"content": {"$text_match": "disk failure"}})
