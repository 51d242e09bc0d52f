"""MilvusIndexManager.compact(): after delete_by_filter + compact() every search answers as before — the same hit dicts,
only "_row" renumbered — num_entities counts the survivors, the batching front is rebuilt, later appends take the new
row numbers, and a snapshot of the compacted collection loads into a new manager."""
import asyncio

import numpy as np
import pytest

from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, V, NQ = 3000, 64, 2000, 8
WORDS = [f"w{i}" for i in range(60)]


@pytest.fixture()
def long_timeout():
    old = RetrievalConstants.TIMEOUT_SECONDS
    RetrievalConstants.TIMEOUT_SECONDS = 60.0
    yield
    RetrievalConstants.TIMEOUT_SECONDS = old


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(23)
    X = rng.standard_normal((N, D)).astype(np.float32)
    idx = (np.arange(20) * 100 + rng.integers(0, 100, size=(N, 20))).astype(np.int32).reshape(-1)
    val = (np.abs(rng.standard_normal(N * 20)) + 0.01).astype(np.float32)
    csr = (np.arange(N + 1, dtype=np.int64) * 20, idx, val)
    payload = dict(
        ids=[f"doc{r // 10}::{r % 10}::{r:08x}" for r in range(N)],
        contents=[" ".join(rng.choice(WORDS, size=10).tolist()) + f" topic{r % 7}" for r in range(N)],
        doc_id=[f"doc{r // 10}" for r in range(N)], chunk_index=[r % 10 for r in range(N)],
        token_count=[5 + r % 3 for r in range(N)], entropy=[(r % 8) / 8.0 for r in range(N)],
        redundancy=[(r % 4) / 4.0 for r in range(N)], domain_density=[(r % 16) / 16.0 for r in range(N)],
        timestamp=[f"2024-0{1 + r % 9}-1{r % 9}T00:00:00" for r in range(N)], metadata_json=["{}"] * N)
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    SQ = [((np.arange(20) * 100 + rng.integers(0, 100, size=20)).astype(np.int32),
           (np.abs(rng.standard_normal(20)) + 0.01).astype(np.float32)) for _ in range(NQ)]
    return X, csr, payload, Q, SQ


class _KeyedGen:
    """Embeddings keyed by the trailing query number of the text ("... q<i>")."""

    def __init__(self, Q, SQ):
        self.Q, self.SQ = Q, SQ

    def encode_semantic(self, text):
        return self.Q[int(text.rsplit("q", 1)[1])]

    def encode_sparse(self, text):
        qi, qv = self.SQ[int(text.rsplit("q", 1)[1])]
        return {"indices": qi.tolist(), "values": qv.astype(float).tolist()}

    def encode_domain(self, text, domain=None):
        return np.zeros(8, np.float32)


def _sparse_q(SQ, i):
    return {"indices": SQ[i][0].tolist(), "values": SQ[i][1].astype(float).tolist()}


def _timeless(hits):
    out = []
    for h in hits:
        h = dict(h, metadata=dict(h["metadata"]))
        h["metadata"].pop("recency", None)     # 1 / (1 + age in days) at the moment of the call
        out.append(h)
    return out


FILTERS = ['chunk_index >= 5', 'entropy < 0.5 and token_count >= 6', 'doc_id == "doc20"', 'chunk_index != 0 and redundancy <= 0.5']


def _answers(mgr, retr, Q, SQ):
    """Every kind of call of the test, in a fixed order -> list of results."""
    out = []
    for i in range(NQ):
        out.append(asyncio.run(mgr.search(Q[i], "semantic_index", top_k=10)))
        out.append(asyncio.run(mgr.search(_sparse_q(SQ, i), "sparse_index", top_k=10)))
    for i, expr in enumerate(FILTERS):
        if i % 2 == 0:
            out.append(asyncio.run(mgr.search(Q[i], "semantic_index", top_k=10, filters=expr)))
        else:
            out.append(asyncio.run(mgr.search(_sparse_q(SQ, i), "sparse_index", top_k=10, filters=expr)))
    for i in range(2):
        res = asyncio.run(mgr.hybrid_search(Q[i], _sparse_q(SQ, i), 10, None, (0.7, 0.3)))
        out.append(None if res is None else [(hit, score, methods) for hit, score, methods in res])
    initialize_caches()
    out.append(_timeless(asyncio.run(retr.retrieve("plain statement q2"))))
    out.append(_timeless(asyncio.run(retr.retrieve("plain statement q3", profile_hint="troubleshooting"))))
    return out


def _hit_lists(answer):
    """The manager-level hit dicts (with "_row") inside one answer."""
    if answer is None:
        return []
    if answer and isinstance(answer[0], tuple):
        return [h for h, _, _ in answer]
    return [h for h in answer if "_row" in h]


def _without_rows(answer):
    if answer is None:
        return None
    if answer and isinstance(answer[0], tuple):
        return [({k: v for k, v in h.items() if k != "_row"}, s, m) for h, s, m in answer]
    return [{k: v for k, v in h.items() if k != "_row"} for h in answer]


@pytest.mark.parametrize("variant", ["plain", "mmr_on_device", "two_shards"])
def test_compact_keeps_every_answer(gpu, long_timeout, tmp_path, corpus, variant):
    X, csr, payload, Q, SQ = corpus
    kw = dict(semantic_dim=D, sparse_dim=V, enable_domain=False)
    if variant == "mmr_on_device":
        kw["mmr_on_device"] = True
    if variant == "two_shards":
        kw["devices"] = [0, 0]
    mgr = MilvusIndexManager(**kw)
    other = None
    try:
        mgr.add_rows(X, csr, **payload)
        mgr.finalize()
        mgr.embedding_generator = _KeyedGen(Q, SQ)
        retr = HybridRetriever(mgr, RetrievalConfig(top_k=10))
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 3"))
        asyncio.run(mgr.delete_by_filter("semantic_index", 'doc_id == "doc17"'))
        dead = np.array([r % 10 == 3 or r // 10 == 17 for r in range(N)])
        survivors = int((~dead).sum())
        before = _answers(mgr, retr, Q, SQ)
        assert any(_hit_lists(a) for a in before)
        assert mgr.collections["semantic_index"].num_entities == N

        stats = mgr.collections["semantic_index"].compact()
        print(variant, stats)
        assert (stats["rows_before"], stats["rows_after"]) == (N, survivors)
        assert stats["device_bytes_after"] < stats["device_bytes_before"]
        assert mgr._front is None and mgr._deleted is None
        for name in ("semantic_index", "sparse_index"):
            assert mgr.collections[name].num_entities == survivors
        ids_now = payload["ids"]
        assert mgr._cols["id"].tolist() == [ids_now[r] for r in range(N) if not dead[r]]

        after = _answers(mgr, retr, Q, SQ)
        new_row_of = np.cumsum(~dead) - 1
        for n, (a, b) in enumerate(zip(before, after)):
            assert _without_rows(a) == _without_rows(b), n
            for ha, hb in zip(_hit_lists(a), _hit_lists(b)):
                assert hb["_row"] == new_row_of[ha["_row"]] and mgr._cols["id"][hb["_row"]] == hb["id"], n
        if variant != "two_shards":
            assert before[-3] is not None and mgr._front is not None     # the one-round path answered, through a new front

        # a second compact() finds nothing to do
        again = mgr.compact()
        assert again["rows_after"] == again["rows_before"] == survivors
        assert again["device_bytes_after"] == again["device_bytes_before"] == stats["device_bytes_after"]

        # 16 concurrent searches through the rebuilt front equal the sequential ones
        async def burst():
            return await asyncio.gather(*(mgr.search(Q[i % NQ], "semantic_index", top_k=10) for i in range(16)))
        together = asyncio.run(burst())
        assert together == [after[2 * (i % NQ)] for i in range(16)]

        # later appends take the new row numbers
        rng = np.random.default_rng(5)
        target = rng.standard_normal(D).astype(np.float32)
        newX = (target[None, :] + 0.01 * rng.standard_normal((10, D))).astype(np.float32)
        new_csr = (np.arange(11, dtype=np.int64) * 20, np.tile((np.arange(20) * 100 + 7).astype(np.int32), 10),
                   np.ones(200, np.float32))
        mgr.add_rows(newX, new_csr, ids=[f"new{j}" for j in range(10)], contents=[f"fresh row {j}" for j in range(10)])
        mgr.finalize()
        hits = asyncio.run(mgr.search(target, "semantic_index", top_k=10))
        assert sorted(h["_row"] for h in hits) == list(range(survivors, survivors + 10))
        assert all(h["id"] == f"new{h['_row'] - survivors}" for h in hits)
        assert mgr.collections["semantic_index"].num_entities == survivors + 10

        # the compacted collection's snapshot needs nothing new
        want = _answers(mgr, retr, Q, SQ)
        mgr.save_snapshot(str(tmp_path / "snap"))
        other = MilvusIndexManager(**kw)
        other.load_snapshot(str(tmp_path / "snap"))
        other.embedding_generator = _KeyedGen(Q, SQ)
        got = _answers(other, HybridRetriever(other, RetrievalConfig(top_k=10)), Q, SQ)
        assert got == want
    finally:
        asyncio.run(mgr.close())
        if other is not None:
            asyncio.run(other.close())


def test_synthetic_payload_collection_is_refused(gpu, corpus):
    X, csr, _, _, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, enable_domain=False)
    try:
        mgr.add_rows_synthetic(X[:500], (csr[0][:501], csr[1], csr[2]))
        mgr.finalize()
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 3"))
        with pytest.raises(ValueError):
            mgr.compact()
        assert mgr.collections["semantic_index"].num_entities == 500
    finally:
        asyncio.run(mgr.close())
