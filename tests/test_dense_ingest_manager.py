"""The index manager refuses a dense batch with a NaN / infinite element (as the shard stores it) BEFORE any shard, sparse
collection or payload column is touched: the row number is the only join key between them.  Driven without a GPU through
the growing oracle shard of test_distributed_cpu.py."""
import asyncio

import numpy as np
import pytest

from advanced_rag import AdvancedRAGPipeline, MilvusIndexManager, PipelineConfig
from advanced_rag.indexing import ShardCollection
from advanced_rag.shards import ShardSet

from test_distributed_cpu import _GrowingOracleShard

DIM, V, DOM = 8, 50, 4


def _manager(dtype="float16"):
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, domain_dim=DOM, connect=False, dtype=dtype)
    mgr._native = None
    mgr.attach_shards([_GrowingOracleShard(DIM, V)])
    mgr._domain = ShardSet([_GrowingOracleShard(DOM, 0)])
    mgr.collections["domain_index"] = ShardCollection(mgr, "domain_index", "dense", mgr._domain, DOM, "COSINE")
    return mgr


def _counts(mgr):
    main, dom = mgr._main.handles[0], mgr._domain.handles[0]
    return (main.num_rows, main.num_sparse_rows, dom.num_rows, mgr._main.num_rows, len(mgr._main.rows_of[0]),
            tuple(len(mgr._cols[k]) for k in mgr._cols))


def _batch(rng, n):
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    ptr = np.arange(n + 1, dtype=np.int64) * 2
    idx = np.tile(np.array([3, 17], np.int32), n)
    val = np.abs(rng.standard_normal(2 * n)).astype(np.float32) + 0.1
    return X, (ptr, idx, val)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 65520.0, -1e5])
def test_add_rows_refuses_a_non_finite_row_before_anything_is_touched(bad):
    rng = np.random.default_rng(1)
    mgr = _manager()
    X, csr = _batch(rng, 10)
    mgr.add_rows(X, csr, ids=[f"a{r}" for r in range(10)])
    before = _counts(mgr)
    assert before[:2] == (10, 10) and set(before[5]) == {10}
    Y, csr_y = _batch(rng, 7)
    Y[3, 5] = bad
    with pytest.raises(ValueError, match=r"row 3\b"):
        mgr.add_rows(Y, csr_y, ids=[f"b{r}" for r in range(7)])
    with np.errstate(over="ignore"):
        Y16 = Y.astype(np.float16)                           # rows already in the store's type
    with pytest.raises(ValueError, match=r"row 3\b"):
        mgr.add_rows(Y16, csr_y)
    assert _counts(mgr) == before
    Z, csr_z = _batch(rng, 5)
    mgr.add_rows(Z, csr_z, ids=[f"c{r}" for r in range(5)])
    after = _counts(mgr)
    assert after[:2] == (15, 15) and set(after[5]) == {15}
    assert [mgr._cols["id"][r] for r in (9, 10, 14)] == ["a9", "c0", "c4"]
    assert np.array_equal(mgr._main.handles[0].X[10:], Z.astype(np.float16))
    assert np.array_equal(mgr._main.rows_of[0], np.arange(15))
    asyncio.run(mgr.close())


def test_fp32_store_takes_what_overflows_fp16_and_the_edge_is_fine():
    rng = np.random.default_rng(2)
    X, csr = _batch(rng, 6)
    X[2, 0], X[4, 7] = 1e5, np.nextafter(np.float32(65520.0), np.float32(0))
    mgr = _manager("float32")
    with np.errstate(over="ignore"):                         # the oracle shard keeps fp16 whatever the manager stores
        mgr.add_rows(X, csr)
    assert mgr.num_rows == 6
    asyncio.run(mgr.close())
    mgr = _manager("float16")
    with pytest.raises(ValueError, match=r"row 2\b"):
        mgr.add_rows(X, csr)
    X[2, 0] = -65519.9
    mgr.add_rows(X, csr)
    assert mgr.num_rows == 6
    asyncio.run(mgr.close())
    mgr = _manager()
    with pytest.raises(ValueError, match=r"row 0\b"):
        mgr.add_rows_synthetic(np.full((1, DIM), np.nan, np.float32))
    assert mgr.num_rows == 0 and mgr._main.handles[0].num_rows == 0
    asyncio.run(mgr.close())


def test_ingest_documents_refuses_a_batch_whose_encoder_returned_an_inf():
    class Gen:
        poison = None

        def encode_semantic_batch(self, texts):
            out = np.ones((len(texts), DIM), np.float32)
            for i, t in enumerate(texts):
                out[i, 0] = len(t)
                if self.poison is not None and i == self.poison:
                    out[i, DIM - 1] = np.inf
            return list(out)

        def encode_semantic(self, text):
            return self.encode_semantic_batch([text])[0]

        def encode_sparse(self, text):
            return {"indices": [1, 9], "values": [1.0, 0.5]}

        def encode_domain(self, text, domain=""):
            return np.ones(DOM, np.float32)

    p = AdvancedRAGPipeline(connect_to_milvus=False, config=PipelineConfig(enable_audit_logging=False))
    mgr = p.index_manager = p.retriever.index_manager = _manager()
    mgr.embedding_generator = gen = Gen()
    docs = [{"id": f"d{i}", "text": f"document number {i} speaks of retrieval " * (3 + i)} for i in range(3)]
    rep = asyncio.run(p.ingest_documents(docs))
    n = rep["chunks_created"]
    assert n >= 3 and rep["indexing_summary"]["indexed_semantic"] == n and not rep["indexing_summary"]["errors"]
    before = _counts(mgr)
    assert before[:3] == (n, n, n) and set(before[5]) == {n}

    gen.poison = 1
    more = [{"id": f"e{i}", "text": f"a later document {i} on another matter entirely " * (4 + i)} for i in range(3)]
    rep = asyncio.run(p.ingest_documents(more))
    summary = rep["indexing_summary"]
    assert summary["indexed_semantic"] == summary["indexed_sparse"] == summary["indexed_domain"] == 0
    assert len(summary["errors"]) == 1 and "row 1 " in summary["errors"][0]["insert_error"]
    assert _counts(mgr) == before

    gen.poison = None           # other texts: the host embedding cache holds what the encoder returned for these
    fresh = [{"id": f"f{i}", "text": f"a third batch, document {i}, nothing wrong with it " * (4 + i)} for i in range(3)]
    rep = asyncio.run(p.ingest_documents(fresh))
    m = rep["chunks_created"]
    after = _counts(mgr)
    assert rep["indexing_summary"]["indexed_semantic"] == m and after[:3] == (n + m, n + m, n + m)
    assert set(after[5]) == {n + m}
    asyncio.run(p.close())


def test_appending_rows_keeps_the_device_filter_columns_and_replacing_the_row_space_drops_them():
    """Every ingest forgets the cached row masks (they cover the old rows).  The device filter columns grow in place when
    rows are appended (add_rows), so that object stays; a row space that is replaced (add_rows_synthetic) drops it."""
    rng = np.random.default_rng(3)
    X, csr = _batch(rng, 6)

    def prime(mgr):
        mgr._mask_cache[("e", 0, 0)] = np.ones(0, bool)
        mgr._dev_masks[("global", "e", 0, 0)] = object()
        mgr._dev_filters = object()
        return mgr._dev_filters

    mgr = _manager()
    filters = prime(mgr)
    mgr.add_rows(X, csr)
    assert mgr._mask_cache == {} and mgr._dev_masks == {} and mgr._dev_filters is filters
    asyncio.run(mgr.close())
    mgr = _manager()
    prime(mgr)
    mgr.add_rows_synthetic(X, csr)
    assert mgr._mask_cache == {} and mgr._dev_masks == {} and mgr._dev_filters is None
    asyncio.run(mgr.close())
