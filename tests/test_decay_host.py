"""The decay ranker without a GPU: the canonical exponential, the factor, the spec object, the ISO parse, the host
restatement of hr_decay_rerank_dev, the epoch column, and search(ranker=...) / retrieve(decay=...) on the manager over
oracle-backed stand-ins for the shard handles (the setup of test_sparse_query_host.py)."""
import asyncio
import math
import random
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import range_yardstick as ry
import test_sparse_query_host as sq
from advanced_rag import HybridRetriever, RetrievalConfig
from advanced_rag import _native as nat
from advanced_rag import decay as D
from advanced_rag.columns import PayloadColumns
from advanced_rag.constants import RetrievalConstants
from advanced_rag.decay import DecayRanker
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.pipeline import PipelineConfig
from advanced_rag.retrieval import canonical_atan, rrf_rank_lists

NAN = float("nan")
PI = float.fromhex("0x1.921fb54442d18p+1")


def ulps(a, b):
    return abs(a - b) / math.ulp(b)


def operands(function, origin, scale, offset=0.0, decay=0.5):
    return DecayRanker("chunk_index", function, origin, scale, offset, decay).operands()


# ---- canonical_exp ---------------------------------------------------------------------------------------------------
def test_codes_match_the_header():
    assert (nat.HR_DECAY_GAUSS, nat.HR_DECAY_EXP, nat.HR_DECAY_LINEAR, nat.HR_COL_F64, nat.HR_NORM_NONE) == (0, 1, 2, 5, -1)
    assert nat.DECAY_QUERY_DTYPE.itemsize == 32 and "hr_decay_rerank_dev" in nat.EXPORTED_SYMBOLS


def test_canonical_exp_edge_values():
    for x in (0.0, -0.0, 1e-300, 1.0, 709.0, float("inf")):
        assert D.canonical_exp(x) == 1.0
    for x in (NAN, -708.0000000000001, -1e9, float("-inf")):
        assert D.canonical_exp(x) == 0.0 and math.copysign(1.0, D.canonical_exp(x)) == 1.0
    low = D.canonical_exp(-708.0)
    assert low >= 2.0 ** -1022 and ulps(low, math.exp(-708.0)) <= 2       # a normal number


def test_canonical_exp_is_monotone_and_within_2_ulp_of_math_exp():
    grid = [-50.0 + 50.0 * i / 20000 for i in range(20001)] + [-708.0 + 658.0 * i / 5000 for i in range(5001)]
    grid.sort()
    vals = [D.canonical_exp(x) for x in grid]
    assert all(a <= b for a, b in zip(vals, vals[1:]))
    rnd = random.Random(708)
    worst = max(ulps(D.canonical_exp(x), math.exp(x)) for x in (-rnd.uniform(1e-6, 708.0) for _ in range(40000)))
    print("canonical_exp: worst error", worst, "ulp")
    assert worst <= 2.0


# ---- decay_factor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("function", ["gauss", "exp", "linear"])
def test_decay_factor_shape(function):
    scale, offset, decay, origin = 37.5, 4.0, 0.3, 100.0
    ops = operands(function, origin, scale, offset, decay)
    for v in (origin, origin + offset, origin - offset, origin + 1.25, origin - 3.999):
        assert D.decay_factor(ops, v) == 1.0                     # anywhere inside offset: exactly 1
    for v in (origin + offset + scale, origin - offset - scale):  # d == scale
        f = D.decay_factor(ops, v)
        print(function, "f(d = scale) =", f)
        assert abs(f - decay) <= 1e-15 if function == "linear" else ulps(f, decay) <= 4
    fs = [D.decay_factor(ops, origin + offset + 0.37 * i) for i in range(2000)]
    assert all(a >= b for a, b in zip(fs, fs[1:])) and fs[0] == 1.0 and fs[-1] < fs[0]
    for v in (NAN, float("inf"), float("-inf")):
        assert D.decay_factor(ops, v) == 0.0
    if function == "linear":
        cut = scale / (1.0 - decay)
        assert D.decay_factor(ops, origin + offset + cut * 1.0000001) == 0.0 and D.decay_factor(ops, origin - offset - 2 * cut) == 0.0
        assert D.decay_factor(ops, origin + offset + cut * 0.999) > 0.0
    assert D.decay_factor(ops[:3] + (7,), origin) == 0.0         # an unknown function code: factor 0
    assert ops[2] > 0 if function == "linear" else ops[2] < 0


# ---- DecayRanker -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, name", [
    (dict(field="content", scale=1.0, origin=0.0), "field"), (dict(field=3, scale=1.0, origin=0.0), "field"),
    (dict(field="entropy", function="cubic", scale=1.0, origin=0.0), "function"),
    (dict(field="entropy", scale=0.0, origin=0.0), "scale"), (dict(field="entropy", scale=-1.0, origin=0.0), "scale"),
    (dict(field="entropy", origin=0.0), "scale"), (dict(field="entropy", scale=NAN, origin=0.0), "scale"),
    (dict(field="entropy", scale=True, origin=0.0), "scale"), (dict(field="entropy", scale="1", origin=0.0), "scale"),
    (dict(field="entropy", scale=1.0, origin=0.0, offset=-0.5), "offset"),
    (dict(field="entropy", scale=1.0, origin=0.0, offset=float("inf")), "offset"),
    (dict(field="entropy", scale=1.0, origin=0.0, offset=False), "offset"),
    (dict(field="entropy", scale=1.0, origin=0.0, decay=0.0), "decay"), (dict(field="entropy", scale=1.0, origin=0.0, decay=1.0), "decay"),
    (dict(field="entropy", scale=1.0, origin=0.0, decay=True), "decay"), (dict(field="entropy", scale=1.0, origin=0.0, decay=NAN), "decay"),
    (dict(field="entropy", scale=1.0), "origin"), (dict(field="entropy", scale=1.0, origin=NAN), "origin"),
    (dict(field="entropy", scale=1.0, origin=True), "origin"), (dict(field="entropy", scale=1.0, origin="2024-01-01"), "origin"),
    (dict(field="timestamp", scale=1.0, origin="yesterday"), "origin"),
    (dict(field="entropy", scale=1.0, origin=0.0, normalization="softmax"), "normalization"),
    (dict(field="entropy", scale=1.0, origin=0.0, candidates=0), "candidates"),
    (dict(field="entropy", scale=1.0, origin=0.0, candidates=2.5), "candidates"),
])
def test_decay_ranker_refusals_name_their_argument(kw, name):
    with pytest.raises(ValueError, match=name):
        DecayRanker(**kw)


def test_decay_ranker_operands_and_norm_codes():
    r = DecayRanker("timestamp", scale=86400.0)
    now = r.operands()[0]
    assert abs(now - datetime.now(timezone.utc).timestamp()) < 5.0 and r.operands()[1:] == (0.0, math.log(0.5) / (86400.0 * 86400.0), 0)
    assert DecayRanker("timestamp", "exp", "2024-03-01T00:00:00+00:00", 3600).operands() == (1709251200.0, 0.0, math.log(0.5) / 3600.0, 1)
    assert DecayRanker("timestamp", "exp", datetime(2024, 3, 1), 3600).operands()[0] == 1709251200.0
    assert DecayRanker("timestamp", "exp", datetime(2024, 3, 1, 2, tzinfo=timezone(timedelta(hours=2))), 3600).operands()[0] == 1709251200.0
    assert DecayRanker("token_count", "linear", 5, 10, 2, 0.25).operands() == (5.0, 2.0, 0.75 / 10.0, 2)
    act = DecayRanker("entropy", origin=0.0, scale=1.0)
    assert [act.norm_code(m) for m in ("COSINE", "IP", "L2")] == [0, 1, 2] and act.norm_code("L2", fused=True) == -1
    mm = DecayRanker("entropy", origin=0.0, scale=1.0, normalization="minmax")
    assert [mm.norm_code(m) for m in ("COSINE", "IP", "L2")] == [3, 3, 4] and mm.norm_code("L2", fused=True) == 3
    none = DecayRanker("entropy", origin=0.0, scale=1.0, normalization="none")
    assert none.norm_code("COSINE") == -1 and none.norm_code("IP") == -1
    with pytest.raises(ValueError, match="L2"):
        none.norm_code("L2")
    assert act.window(10) == 10 and DecayRanker("entropy", origin=0.0, scale=1.0, candidates=40).window(10) == 40
    assert DecayRanker("entropy", origin=0.0, scale=1.0, candidates=4).window(10) == 10
    with pytest.raises(Exception):
        act.scale = 2.0                                           # frozen


def test_configs_carry_the_decay_field():
    r = DecayRanker("timestamp", scale=86400.0)
    assert RetrievalConfig().decay is None and PipelineConfig().decay is None and PipelineConfig(decay=r).decay is r
    retr = HybridRetriever(object(), RetrievalConfig(decay=r))
    assert all(p.decay is r for p in retr.profiles.values())
    with pytest.raises(ValueError, match="decay"):
        RetrievalConfig(decay="gauss")


# ---- epoch_seconds -----------------------------------------------------------------------------------------------------
def test_epoch_seconds():
    assert D.epoch_seconds("2024-03-01T12:30:00") == 1709296200.0                       # naive: UTC
    assert D.epoch_seconds("2024-03-01T12:30:00+02:00") == 1709296200.0 - 7200.0        # aware: converted
    assert D.epoch_seconds("2024-03-01") == 1709251200.0                                # a date only
    assert D.epoch_seconds("2024-03-01T12:30:00.250000") == 1709296200.25               # microseconds
    assert D.epoch_seconds("1969-12-31T23:59:59") == -1.0
    for text in ("", "yesterday", "2024-13-01", None, 17):
        assert math.isnan(D.epoch_seconds(text))


# ---- decay_rerank ------------------------------------------------------------------------------------------------------
def test_decay_rerank_ties_cut_and_zero_factors():
    ids, scores = [10, 11, 12, 13, 14], [0.5] * 5
    ops = operands("exp", 0.0, 10.0)
    pos, oid, fin = D.decay_rerank(ids, scores, [3.0, 1.0, 3.0, 1.0, 3.0], ops, -1, 5)
    assert pos == [1, 3, 0, 2, 4] and oid == [11, 13, 10, 12, 14] and fin[0] == fin[1] > fin[2] == fin[3] == fin[4]
    assert D.decay_rerank(ids, scores, [3.0, 1.0, 3.0, 1.0, 3.0], ops, -1, 2)[:2] == ([1, 3], [11, 13])      # the cut
    pos, oid, fin = D.decay_rerank(ids, [0.9, 0.8, 0.7, 0.6, 0.5], [NAN] * 5, ops, 0, 9)      # no row has the field
    assert pos == [0, 1, 2, 3, 4] and oid == ids and fin == [0.0] * 5                     # order kept, nothing padded here
    assert D.decay_rerank([], [], [], ops, 3, 4) == ([], [], [])


def test_decay_rerank_every_norm_code():
    rng = np.random.default_rng(4)
    s32 = np.round(rng.uniform(-1, 1, 30) * 64).astype(np.float32) / 64
    scores = [float(x) for x in s32]
    values = [float(v) for v in rng.integers(0, 50, 30)]
    ops = operands("gauss", 20.0, 8.0, 2.0, 0.4)
    f = [D.decay_factor(ops, v) for v in values]
    lo, hi = min(scores), max(scores)
    want = {-1: scores, 0: [(1.0 + s) * 0.5 for s in scores], 1: [0.5 + canonical_atan(s) / PI for s in scores],
            2: [1.0 - (2.0 * canonical_atan(s)) / PI for s in scores], 3: [(s - lo) / (hi - lo) for s in scores],
            4: [(hi - s) / (hi - lo) for s in scores]}
    for code, ns in want.items():
        final = [a * b for a, b in zip(ns, f)]
        order = sorted(range(30), key=lambda i: (-final[i], i))
        pos, oid, fin = D.decay_rerank(list(range(100, 130)), scores, values, ops, code, 30)
        assert pos == order and oid == [100 + i for i in order] and fin == [final[i] for i in order], code
    for code in (3, 4):      # hi == lo: 1.0 for every entry, so final == the factor
        pos, _, fin = D.decay_rerank([1, 2, 3], [0.25] * 3, [20.0, 40.0, 21.0], ops, code, 3)
        assert pos == [0, 2, 1] and fin == [1.0, D.decay_factor(ops, 21.0), D.decay_factor(ops, 40.0)]
    with pytest.raises(ValueError):
        D.decay_rerank([1], [0.5], [1.0], ops, 5, 1)


# ---- the epoch column ----------------------------------------------------------------------------------------------------
def _fill(cols, stamps, base=0):
    n = len(stamps)
    cols["id"].extend(f"c{base + i}" for i in range(n))
    for name in ("doc_id", "content", "metadata_json"):
        cols[name].extend("" for _ in range(n))
    for name in ("chunk_index", "token_count", "entropy", "redundancy", "domain_density"):
        cols[name].extend([0] * n)
    cols["timestamp"].extend(stamps)


def test_epoch_column_is_extended_by_appends_and_gathered_by_compact():
    cols = PayloadColumns()
    first = ["2024-03-01T00:00:00", "", "2024-03-02", "garbage", "2024-03-03T00:00:00+01:00"]
    _fill(cols, first)
    assert cols._epoch is None                                                    # built on first use
    a = cols.epoch_seconds()
    assert a.dtype == np.float64 and a.shape == (5,)
    assert a[[0, 2, 4]].tolist() == [1709251200.0, 1709337600.0, 1709424000.0 - 3600.0] and np.isnan(a[[1, 3]]).all()
    _fill(cols, ["2024-03-04", "2024-03-05"], base=5)
    assert len(cols._epoch) == 5
    a = cols.epoch_seconds()
    assert len(cols._epoch) == 7 and a[5:].tolist() == [1709510400.0, 1709596800.0]
    _fill(cols, ["2024-03-06"], base=7)                                           # one row the column has not parsed yet
    keep = np.array([True, False, True, True, False, True, False, True])
    cols.compact(keep)
    got = cols.epoch_seconds()
    want = [D.epoch_seconds(t) for t in cols["timestamp"]]
    assert len(want) == 5 and np.array_equal(got, np.array(want), equal_nan=True)
    assert np.array_equal(np.isnan(got), [False, False, True, False, False])


# ---- search(ranker=...) on the stand-in manager ------------------------------------------------------------------------------
class _L2Shard(sq._OracleShard):
    metric = nat.HR_METRIC_L2

    def search_dense(self, q, k, mask=None):
        if mask is not None:       # the handle's packed row mask -> one bool per row
            mask = np.unpackbits(np.asarray(mask, np.uint8), bitorder="little")[:self.X.shape[0]].astype(bool)
        return ry.range_search(self.X, q, k, ry.L2, None, None, mask)


T0 = datetime(2024, 3, 1)


def _stamps(n):
    out = [(T0 - timedelta(hours=7 * r % 1440)).isoformat() for r in range(n)]
    for r in range(0, n, 17):
        out[r] = "" if r % 2 else "not a time"
    return out


def _manager(shard_cls, shards):
    X, csr = sq._corpus()
    n = sq.N
    mgr = MilvusIndexManager(semantic_dim=sq.DIM, sparse_dim=sq.V, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([shard_cls(sq.V) for _ in range(shards)])
    mgr.add_rows(X[:n], csr, ids=[f"c{r}" for r in range(n)], doc_id=[f"doc{r // 5}" for r in range(n)],
                 chunk_index=[r % 9 for r in range(n)], token_count=[30 + r % 41 for r in range(n)],
                 entropy=[(r % 13) / 13.0 for r in range(n)], timestamp=_stamps(n),
                 contents=[f"topic{r % 5} word{r % 7} text{r % 3} common" for r in range(n)])
    return mgr, X, csr


@pytest.fixture(scope="module", params=[("COSINE", 1), ("L2", 3)], ids=["cosine-1", "l2-3"])
def host(request):
    metric, shards = request.param
    mgr, X, csr = _manager(sq._OracleShard if metric == "COSINE" else _L2Shard, shards)
    assert mgr.semantic_metric == metric and mgr._filters_on_device() is None
    yield mgr, X, csr, metric
    asyncio.run(mgr.close())


def _values(mgr, field, rows):
    if field == "timestamp":
        return [D.epoch_seconds(mgr._cols["timestamp"][r]) for r in rows]
    return [float(mgr._cols[field][r]) for r in rows]


def _check_search(mgr, query, coll, metric, ranker, top_k, **kw):
    W = max(top_k, ranker.candidates or top_k)
    plain = asyncio.run(mgr.search(query, coll, W, **kw))
    got = asyncio.run(mgr.search(query, coll, top_k, ranker=ranker, **kw))
    rows = [h["_row"] for h in plain]
    norm = ranker.norm_code(metric)
    pos, _, fin = D.decay_rerank(rows, [h["score"] for h in plain], _values(mgr, ranker.field, rows), ranker.operands(), norm, W)
    assert [h["id"] for h in got] == [plain[p]["id"] for p in pos[:top_k]]
    assert [float(h["score"]).hex() for h in got] == [float(f).hex() for f in fin[:top_k]]
    assert [h["raw_score"] for h in got] == [plain[p]["score"] for p in pos[:top_k]]
    return got, plain


def test_search_with_a_ranker_equals_the_restatement_over_the_plain_search(host):
    mgr, X, csr, metric = host
    q = X[5] + 0.25 * X[40]
    origin = (T0 - timedelta(days=20)).isoformat()
    stamp = DecayRanker("timestamp", "gauss", origin, 5 * 86400.0, 3600.0, 0.5, candidates=40)
    got, plain = _check_search(mgr, q, "semantic_index", metric, stamp, 10)
    assert [h["id"] for h in got] != [h["id"] for h in plain[:10]]                        # the decay says something
    for ranker in (DecayRanker("timestamp", "exp", origin, 86400.0, normalization="minmax"),
                   DecayRanker("chunk_index", "linear", 4, 3, 1, 0.5, candidates=25),
                   DecayRanker("entropy", "gauss", 0.5, 0.2),
                   DecayRanker("token_count", "exp", 50, 10.0, normalization="minmax", candidates=12)):
        _check_search(mgr, q, "semantic_index", metric, ranker, 10)
    _check_search(mgr, q, "semantic_index", metric, stamp, 7, filters="chunk_index >= 3")
    if metric != "L2":
        _check_search(mgr, q, "semantic_index", metric, DecayRanker("chunk_index", "exp", 0, 4, normalization="none"), 10)
    # the sparse collection ranks by IP
    a, b = csr[0][12], csr[0][13]
    sparse_q = {"indices": csr[1][a:b].tolist(), "values": csr[2][a:b].tolist()}
    got, _ = _check_search(mgr, sparse_q, "sparse_index", "IP", stamp, 5)
    assert len(got) == 5
    # origin=None is "now", read once per request: far from every row, so gauss saturates to 0 and the order is kept
    hits = asyncio.run(mgr.search(q, "semantic_index", 5, ranker=DecayRanker("timestamp", scale=60.0)))
    assert [h["id"] for h in hits] == [h["id"] for h in plain[:5]] and all(h["score"] == 0.0 for h in hits)
    # search_by_ids passes the ranker through
    by_id = asyncio.run(mgr.search_by_ids(["c7"], "semantic_index", 6, ranker=stamp))[0]
    direct = asyncio.run(mgr.search(mgr.collections["semantic_index"].handle.get_dense_rows([7])[0], "semantic_index", 6, ranker=stamp))
    assert [(h["id"], h["score"]) for h in by_id] == [(h["id"], h["score"]) for h in direct] and len(by_id) == 6


def test_search_refusals(host):
    mgr, X, _, metric = host
    q, r = X[0], DecayRanker("chunk_index", "exp", 0, 4)
    run = lambda **kw: asyncio.run(mgr.search(q, "semantic_index", kw.pop("top_k", 5), **kw))
    with pytest.raises(ValueError, match="group_by_field"):
        run(ranker=r, group_by_field="doc_id")
    with pytest.raises(ValueError, match="offset"):
        run(ranker=r, offset=3)
    with pytest.raises(ValueError, match="deep window"):
        run(ranker=r, top_k=nat.HR_MAX_TOPK + 1)
    with pytest.raises(ValueError, match="deep window"):
        run(ranker=DecayRanker("chunk_index", "exp", 0, 4, candidates=nat.HR_MAX_TOPK + 1))
    with pytest.raises(ValueError, match="DecayRanker"):
        run(ranker="gauss")
    with pytest.raises(ValueError, match="not found"):
        asyncio.run(mgr.search(q, "nope", 5, ranker=r))
    if metric == "L2":
        with pytest.raises(ValueError, match="L2"):
            run(ranker=DecayRanker("chunk_index", "exp", 0, 4, normalization="none"))
    with pytest.raises(ValueError, match="group_by_field"):
        asyncio.run(mgr.search_by_ids(["c1"], "semantic_index", 5, ranker=r, group_by_field="doc_id"))
    assert len(run(ranker=None)) == 5                                                    # the default: the call it was


def test_synthetic_collection_has_no_timestamps():
    X, csr = sq._corpus()
    mgr = MilvusIndexManager(semantic_dim=sq.DIM, sparse_dim=sq.V, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([sq._OracleShard(sq.V)])
    mgr.add_rows_synthetic(X[:sq.N], csr)
    try:
        with pytest.raises(ValueError, match="timestamp"):
            asyncio.run(mgr.search(X[0], "semantic_index", 5, ranker=DecayRanker("timestamp", scale=60.0)))
        with pytest.raises(ValueError, match="entropy"):
            asyncio.run(mgr.search(X[0], "semantic_index", 5, ranker=DecayRanker("entropy", origin=0.0, scale=1.0)))
        r = DecayRanker("chunk_index", "linear", 9, 5, candidates=30)                      # chunk_index = row % 10 can be derived
        plain = asyncio.run(mgr.search(X[0], "semantic_index", 30))
        rows = [h["_row"] for h in plain]
        pos, _, fin = D.decay_rerank(rows, [h["score"] for h in plain], [float(x % 10) for x in rows], r.operands(), 0, 30)
        got = asyncio.run(mgr.search(X[0], "semantic_index", 8, ranker=r))
        assert [(h["_row"], h["score"]) for h in got] == [(rows[p], f) for p, f in zip(pos[:8], fin[:8])]
    finally:
        asyncio.run(mgr.close())


def test_torchrun_form_is_not_built(host):
    mgr, X, _, _ = host

    class Collective:
        round = None
    coll = mgr.collections["semantic_index"]
    real, coll.handle = coll.handle, Collective()
    try:
        with pytest.raises(NotImplementedError, match="torchrun"):
            asyncio.run(mgr.search(X[0], "semantic_index", 5, ranker=DecayRanker("chunk_index", "exp", 0, 4)))
    finally:
        coll.handle = real


# ---- retrieve(decay=...) on the general path ------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, X, csr):
        self.X, self.csr = X, csr

    def _n(self, text):
        return int(text.rsplit("q", 1)[1])

    def encode_semantic(self, text):
        return self.X[self._n(text)] + 0.5 * self.X[self._n(text) + 1]

    def encode_sparse(self, text):
        r = self._n(text) + 1
        a, b = self.csr[0][r], self.csr[0][r + 1]
        return {"indices": self.csr[1][a:b].tolist(), "values": self.csr[2][a:b].astype(float).tolist()}

    def encode_domain(self, text, domain=None):
        return np.zeros(8, np.float32)


@pytest.mark.parametrize("mmr", [False, True])
@pytest.mark.parametrize("normalization", ["activation", "minmax"])
def test_retrieve_with_decay_equals_the_restatement_over_the_fused_list(host, mmr, normalization):
    mgr, X, csr, metric = host
    mgr.embedding_generator = _Gen(X, csr)
    top_k = 6
    ranker = DecayRanker("timestamp", "exp", (T0 - timedelta(days=10)).isoformat(), 4 * 86400.0, normalization=normalization)
    params = {"metric_type": metric, "params": {"ef": 64}}
    old, RetrievalConstants.TIMEOUT_SECONDS = RetrievalConstants.TIMEOUT_SECONDS, 60.0
    try:
        for qn in (10, 30):
            initialize_caches()
            text = f"plain statement q{qn}"
            gen = mgr.embedding_generator
            sem = asyncio.run(mgr.search(gen.encode_semantic(text), "semantic_index", 2 * top_k, None, params))
            spa = asyncio.run(mgr.search(gen.encode_sparse(text), "sparse_index", 2 * top_k, None,
                                         {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}))
            assert len(sem) == 2 * top_k and len(spa) >= 2
            ranked = rrf_rank_lists([[h["id"] for h in sem], [h["id"] for h in spa]], (0.7, 0.3))
            row_of = {h["id"]: h["_row"] for h in sem + spa}
            rows = [row_of[i] for i, _, _ in ranked]
            norm = 3 if normalization == "minmax" else -1                  # "activation" on a fused list: identity
            pos, _, fin = D.decay_rerank(rows, [s for _, s, _ in ranked], _values(mgr, "timestamp", rows), ranker.operands(), norm,
                                         len(rows))
            want = [{"id": ranked[p][0], "score": f, "fused_score": ranked[p][1], "content": mgr._cols["content"][rows[p]]}
                    for p, f in zip(pos, fin)]
            assert [h["id"] for h in want] != [i for i, _, _ in ranked]    # the decay reorders the fused list
            if mmr:
                want = HybridRetriever._mmr_diversify(want, top_k, 0.6)
            cfg = RetrievalConfig(top_k=top_k, decay=ranker, enable_mmr=mmr, mmr_lambda=0.6, semantic_search_params=params)
            got = asyncio.run(HybridRetriever(mgr, cfg).retrieve(text, profile_hint="default"))
            assert [(h["id"], float(h["score"]).hex(), float(h["fused_score"]).hex()) for h in got] == \
                [(h["id"], float(h["score"]).hex(), float(h["fused_score"]).hex()) for h in want[:top_k]]
            plain = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=top_k, enable_mmr=mmr, mmr_lambda=0.6,
                                                                     semantic_search_params=params)).retrieve(text, profile_hint="default"))
            assert all("fused_score" not in h for h in plain)              # without decay: the hits they were
    finally:
        RetrievalConstants.TIMEOUT_SECONDS = old
        mgr.embedding_generator = None
