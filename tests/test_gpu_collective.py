"""The torchrun form on real shards: two processes (gloo between them; on an 8-GPU node the same code runs over RCCL) each
own a libhbmrag shard on the card, the collection is INGESTED through rank 0 (collective add / finalize), searched and
retrieved from rank 0, saved (every rank writes its own shard file) and resumed rank by rank.  Every answer is checked
against the oracle over the whole corpus: bit-exact ids, scores within the fp16-row tolerance of the other parity tests."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _corpus(n=20011, d=64, V=500, nnz=9, B=5, tie=(300, 15000)):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, d)).astype(np.float16)
    if tie:
        X[tie[0]] = X[tie[1]]               # an exact tie across the ranks
    idx = np.sort(np.argpartition(rng.random((n, V)), nnz - 1, axis=1)[:, :nnz], axis=1).astype(np.int32).reshape(-1)
    val = np.abs(rng.standard_normal(n * nnz)).astype(np.float32)
    ptr = np.arange(n + 1, dtype=np.int64) * nnz
    Q = rng.standard_normal((B, d)).astype(np.float32)
    if tie:
        Q[0] = X[tie[0]].astype(np.float32)
    SQ = [(np.sort(rng.choice(V, 30, replace=False)).astype(np.int32), np.abs(rng.standard_normal(30)).astype(np.float32))
          for _ in range(B)]
    return X, ptr, idx, val, Q, SQ


def _worker(rank, world, port, ret, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))
    import asyncio

    import torch.distributed as dist

    import oracle
    from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig, _native
    from advanced_rag.constants import RetrievalConstants
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, ptr, idx, val, Q, SQ = _corpus()
        n, d, V = X.shape[0], X.shape[1], 500
        _native.load_library()

        def manager():
            m = MilvusIndexManager(semantic_dim=d, sparse_dim=V, connect=False, dtype="float16")
            m._connect()
            return m

        def same(got, want):
            gi, gs = got
            wi, ws = want
            assert np.array_equal(gi, wi), (gi[0, :8], wi[0, :8])
            assert np.allclose(gs, ws, rtol=2e-6, atol=2e-6)

        mgr = manager()
        h = _native.ShardHandle(d, _native.HR_F16, _native.HR_METRIC_COSINE, V, 0)
        mgr.attach_shards([h], rows_of=[np.zeros(0, np.int64)], process_group=True, local_ids=True)
        if rank != 0:
            mgr.serve()
        else:
            cs = mgr._main
            cuts = [0, 7001, 7002, 16000, n]
            for a, b in zip(cuts[:-1], cuts[1:]):
                mgr.add_rows(X[a:b], (ptr[a:b + 1], idx, val), chunk_index=[r % 10 for r in range(a, b)])
            mgr.finalize()
            assert (cs.num_rows, cs.num_sparse_rows, mgr.num_rows) == (n, n, n)
            keep = (np.arange(n) % 10) < 5
            packed = np.packbits(keep, bitorder="little")
            same(cs.search_dense(Q, 40), oracle.dense_search(X, Q, 40, oracle.COSINE))
            same(cs.search_dense(Q, 40, keep), oracle.dense_search(X, Q, 40, oracle.COSINE, packed))
            same(cs.search_sparse(SQ, 40, 0.2), oracle.sparse_search(ptr, idx, val, SQ, 40, 0.2))
            same(cs.search_sparse(SQ, 40, 0.0, keep), oracle.sparse_search(ptr, idx, val, SQ, 40, 0.0, packed))
            assert cs.search_dense(Q[:1], 40)[0][0, :2].tolist() == [300, 15000]

            class Gen:
                def encode_semantic(self, text):
                    return Q[int(text)]

                def encode_sparse(self, text):
                    qi, qv = SQ[int(text)]
                    return {"indices": qi.tolist(), "values": qv.tolist()}

            mgr.embedding_generator = Gen()
            RetrievalConstants.TIMEOUT_SECONDS = 60.0
            retr = HybridRetriever(mgr, RetrievalConfig(top_k=20))
            flt = {"chunk_index": {"$lt": 5}}
            out = asyncio.run(retr.retrieve("2", filters=flt, profile_hint="default"))
            di, _ = oracle.dense_search(X, Q[2:3], 40, oracle.COSINE, packed)
            si, _ = oracle.sparse_search(ptr, idx, val, SQ[2:3], 40, 0.2, packed)
            fi, fs, _ = oracle.rrf(di[0], si[0][si[0] >= 0], (), 0.7, 0.3, 0.2, 60)
            assert [o["id"] for o in out] == [MilvusIndexManager.synthetic_id(int(r)) for r in fi[:20]]
            assert np.allclose([o["score"] for o in out], fs[:20], rtol=1e-12)
            mgr.save_snapshot(tmp)
            maps = cs.row_maps()
            assert sorted(np.concatenate(maps).tolist()) == list(range(n))
            mgr.stop_workers()
        dist.barrier()

        # ---- resume: every rank loads its own shard file and row map
        m2 = manager()
        m2.load_snapshot_rank(tmp, process_group=True, device=0)
        if rank != 0:
            m2.serve()
        else:
            cs2 = m2._main
            assert cs2.num_rows == n and m2.num_rows == n
            same(cs2.search_dense(Q, 40), oracle.dense_search(X, Q, 40, oracle.COSINE))
            same(cs2.search_sparse(SQ, 40, 0.2, keep), oracle.sparse_search(ptr, idx, val, SQ, 40, 0.2, packed))
            m2.embedding_generator = mgr.embedding_generator
            out2 = asyncio.run(HybridRetriever(m2, RetrievalConfig(top_k=20)).retrieve("2", filters=flt, profile_hint="default"))
            assert [o["id"] for o in out2] == [o["id"] for o in out]
            m2.stop_workers()
        ret[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(420)
def test_collective_ingest_search_snapshot_on_two_gpu_processes(gpu, tmp_path):
    import torch.multiprocessing as mp
    world = 2
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, ret, str(tmp_path)), nprocs=world, join=True)
    assert dict(ret) == {0: True, 1: True}


def _hybrid_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))
    import asyncio

    import torch.distributed as dist

    import oracle
    from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig, _native
    from advanced_rag.constants import RetrievalConstants
    from advanced_rag.engine import shard_range
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, ptr, idx, val, Q, SQ = _corpus()
        n, d, V = X.shape[0], X.shape[1], 500
        lo, hi = shard_range(n, rank, world, align=64)
        h = _native.ShardHandle(d, _native.HR_F16, _native.HR_METRIC_COSINE, V, 0)
        h.set_row_offset(lo)
        h.add_dense(X[lo:hi])
        h.add_sparse(ptr[lo:hi + 1] - ptr[lo], idx[ptr[lo]:ptr[hi]], val[ptr[lo]:ptr[hi]])
        h.finalize()
        mgr = MilvusIndexManager(semantic_dim=d, sparse_dim=V, connect=False, dtype="float16")
        mgr._connect()
        mgr.attach_shards([h], rows_of=[np.arange(hi - lo)], synthetic_rows=n, process_group=True, first_row=lo)
        cs = mgr._main
        assert cs.supports_hybrid_round
        if rank != 0:
            mgr.serve()
            ret[rank] = True
            return

        class Gen:
            def encode_semantic(self, text):
                return Q[int(text)]

            def encode_sparse(self, text):
                qi, qv = SQ[int(text)]
                return {"indices": qi.tolist(), "values": qv.tolist()}

        mgr.embedding_generator = Gen()
        RetrievalConstants.TIMEOUT_SECONDS = 60.0
        retr = HybridRetriever(mgr, RetrievalConfig(top_k=20))

        def want(q, packed=None, w=(0.7, 0.3)):
            di, _ = oracle.dense_search(X, Q[q:q + 1], 40, oracle.COSINE, packed)
            si, _ = oracle.sparse_search(ptr, idx, val, SQ[q:q + 1], 40, 0.2, packed)
            fi, fs, _ = oracle.rrf(di[0], si[0][si[0] >= 0], (), w[0], w[1], 0.2, 60)
            return [MilvusIndexManager.synthetic_id(int(r)) for r in fi[:20]], fs[:20]

        # a lone retrieve(): ONE packet broadcast of the shard set (the lists travel in the engine's all-gather)
        c0 = cs.n_collectives
        out = asyncio.run(retr.retrieve("1", profile_hint="default"))
        front = mgr._coalescer(mgr.collections["semantic_index"])
        assert cs.n_collectives - c0 == 1 and front.stats["hybrid_launches"] == 1
        ids, fs = want(1)
        assert [o["id"] for o in out] == ids
        assert np.allclose([o["score"] for o in out], fs, rtol=1e-12)
        # with a filter: the mask travels once, and the ranks keep their slices in HBM
        flt = {"chunk_index": {"$lt": 5}}
        packed = np.packbits((np.arange(n) % 10) < 5, bitorder="little")
        for expect in (2, 1):
            c0 = cs.n_collectives
            out = asyncio.run(retr.retrieve("2", filters=flt, profile_hint="default"))
            assert cs.n_collectives - c0 == expect
            assert [o["id"] for o in out] == want(2, packed)[0] and all(o["metadata"]["chunk_index"] < 5 for o in out)

        # concurrent callers share rounds; per-request fusion weights ride in the packet
        async def many():
            return await asyncio.gather(*[retr.retrieve(str(q), profile_hint="default") for q in range(5)])
        c0, l0 = cs.n_collectives, front.stats["hybrid_launches"]
        outs = asyncio.run(many())
        assert cs.n_collectives - c0 < 5 and front.stats["hybrid_launches"] - l0 < 5
        for q, o in enumerate(outs):
            assert [x["id"] for x in o] == want(q)[0]
        res = asyncio.run(mgr.hybrid_search(Q[3], {"indices": SQ[3][0].tolist(), "values": SQ[3][1].tolist()}, 20, None, (0.2, 0.8),
                                            sparse_params={"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}))
        assert [hit["id"] for hit, _, _ in res] == want(3, None, (0.2, 0.8))[0]
        mgr.stop_workers()
        ret[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(420)
def test_hybrid_rounds_on_the_device_across_two_gpu_processes(gpu):
    """retrieve() on rank 0 of a two-rank collection of pre-built shards: the two searches and the fusion of a request are
    ONE collective round on the device (CollectiveShardSet.round_hybrid: packet broadcast, hr_search_hybrid_dev per rank on
    views of the packet, the engine's all-gather + merge/fuse launch) — checked against the oracle chain over the whole
    corpus, with filters, concurrent callers and per-request weights."""
    import torch.multiprocessing as mp
    world = 2
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_hybrid_worker, args=(world, port, ret), nprocs=world, join=True)
    assert dict(ret) == {0: True, 1: True}


def _hybrid_rounds_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))
    import torch.distributed as dist

    import oracle
    from advanced_rag import MilvusIndexManager, _native
    from advanced_rag.engine import pack_sparse_queries, shard_range
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        top_k, kp, drop, rrf_k, w = 20, 40, 0.2, 60, (0.7, 0.3)
        X, ptr, idx, val, Q, SQ = _corpus(n=1500, B=3, tie=None)
        n, d, V = X.shape[0], X.shape[1], 500
        # 31 terms in the first query: 25 + 24 + 24 survive the drop, so the packet's idx / val sections have an odd length
        # for B = 1 and for B = 3
        SQ[0] = (np.arange(0, 31 * 16, 16, dtype=np.int32), np.linspace(0.5, 2.0, 31).astype(np.float32))
        assert all(pack_sparse_queries(SQ[:B], drop, V)[1].size % 2 == 1 for B in (1, 3))
        lo, hi = shard_range(n, rank, world, align=64)
        h = _native.ShardHandle(d, _native.HR_F16, _native.HR_METRIC_COSINE, V, 0)
        h.set_row_offset(lo)
        h.add_dense(X[lo:hi])
        h.add_sparse(ptr[lo:hi + 1] - ptr[lo], idx[ptr[lo]:ptr[hi]], val[ptr[lo]:ptr[hi]])
        h.finalize()
        mgr = MilvusIndexManager(semantic_dim=d, sparse_dim=V, connect=False, dtype="float16")
        mgr._connect()
        mgr.attach_shards([h], rows_of=[np.arange(hi - lo)], synthetic_rows=n, process_group=True, first_row=lo)
        cs = mgr._main
        assert cs.supports_hybrid_round
        if rank != 0:
            mgr.serve()
            ret[rank] = True
            return

        def check(B, keep, collectives):
            packed = None if keep is None else np.packbits(keep, bitorder="little")
            c0 = cs.n_collectives
            res = cs.round_hybrid(Q[:B], SQ[:B], top_k, drop, rrf_k, np.tile(w, (B, 1)), keep)
            assert cs.n_collectives - c0 == collectives, (cs.n_collectives - c0, collectives)
            # one entry past the lists: no tie at the cut and no short list, so the oracle alone says every list is provable
            di, ds = oracle.dense_search(X, Q[:B], kp + 1, oracle.COSINE, packed)
            si, ss = oracle.sparse_search(ptr, idx, val, SQ[:B], kp + 1, drop, packed)
            for li, ls in ((di, ds), (si, ss)):
                assert (li[:, kp] >= 0).all() and (ls[:, kp - 1] != ls[:, kp]).all()
            assert res["proven"].shape == (B,) and res["proven"].all()
            assert np.array_equal(res["list_ids"][0], di[:, :kp]) and np.array_equal(res["list_ids"][1], si[:, :kp])
            for q in range(B):
                fi, fs, _ = oracle.rrf(di[q, :kp], si[q, :kp], (), w[0], w[1], 0.2, rrf_k)
                assert res["fused_n"][q] == top_k and np.array_equal(res["fused_ids"][q], fi[:top_k]), (B, q)
                assert np.allclose(res["fused_scores"][q], fs[:top_k], rtol=1e-12)

        rng = np.random.default_rng(11)
        keeps = [rng.random(n) < 0.5 for _ in range(cs.MAX_MASKS + 2)]
        check(3, None, 1)
        check(1, None, 1)
        for i, keep in enumerate(keeps):
            check((1, 3)[i % 2], keep, 2)           # the packet + the new mask
        check(3, keeps[0], 2)                       # rolled out of every rank's cache (slice and device copy): travels again
        check(1, keeps[-1], 1)                      # still there
        check(3, keeps[-1], 1)
        mgr.stop_workers()
        ret[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_hybrid_rounds_read_the_packet_and_roll_masks_over_on_the_device(gpu):
    """round_hybrid() on two processes sharing the card: the operands of hr_search_hybrid_dev are typed views of the packet
    where it was uploaded (B = 1 and 3, idx / val sections of odd length), more distinct filters pass than the mask cache
    keeps and the first comes back.  Every fused list and both modality lists equal the oracle chain (dense 2k, sparse 2k,
    RRF) over the whole corpus, every list is proven, a new mask costs one extra collective and a known one none."""
    import torch.multiprocessing as mp
    world = 2
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_hybrid_rounds_worker, args=(world, port, ret), nprocs=world, join=True)
    assert dict(ret) == {0: True, 1: True}


def _nccl_worker(rank, world, port, ret, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))
    import asyncio

    import torch
    import torch.distributed as dist

    import oracle
    from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig, _native
    from advanced_rag.constants import RetrievalConstants
    from advanced_rag.shards import CollectiveShardSet
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    try:
        dist.init_process_group("nccl", rank=rank, world_size=world)
        dist.all_reduce(torch.ones(1, device="cuda:0"))          # the communicator really exists
        torch.cuda.synchronize()
    except Exception as e:   # no RCCL on this box: say so instead of failing what the gloo tests already cover
        ret["skip"] = f"{type(e).__name__}: {e}"
        return
    try:
        X, ptr, idx, val, Q, SQ = _corpus()
        n, d, V = X.shape[0], X.shape[1], 500
        h = _native.ShardHandle(d, _native.HR_F16, _native.HR_METRIC_COSINE, V, 0)
        h.add_dense(X)
        h.add_sparse(ptr, idx, val)
        h.finalize()
        mgr = MilvusIndexManager(semantic_dim=d, sparse_dim=V, connect=False, dtype="float16")
        mgr._connect()
        mgr.attach_shards([h], rows_of=[np.arange(n)], synthetic_rows=n, process_group=True, first_row=0)
        cs = mgr._main
        assert cs.dev.type == "cuda" and cs._packet.is_cuda and cs.supports_hybrid_round

        class Gen:
            def encode_semantic(self, text):
                return Q[int(text)]

            def encode_sparse(self, text):
                qi, qv = SQ[int(text)]
                return {"indices": qi.tolist(), "values": qv.tolist()}

        mgr.embedding_generator = Gen()
        RetrievalConstants.TIMEOUT_SECONDS = 60.0
        retr = HybridRetriever(mgr, RetrievalConfig(top_k=20))
        packed = np.packbits((np.arange(n) % 10) < 5, bitorder="little")

        def want(q, p=None):
            di, _ = oracle.dense_search(X, Q[q:q + 1], 40, oracle.COSINE, p)
            si, _ = oracle.sparse_search(ptr, idx, val, SQ[q:q + 1], 40, 0.2, p)
            fi, _, _ = oracle.rrf(di[0], si[0][si[0] >= 0], (), 0.7, 0.3, 0.2, 60)
            return [MilvusIndexManager.synthetic_id(int(r)) for r in fi[:20]]

        for on_device in (True, False):      # the packet's device views, then the host-form rounds with a device gather
            CollectiveShardSet.hybrid_on_device = on_device
            assert [o["id"] for o in asyncio.run(retr.retrieve("1", profile_hint="default"))] == want(1)
            out = asyncio.run(retr.retrieve("2", filters={"chunk_index": {"$lt": 5}}, profile_hint="default"))
            assert [o["id"] for o in out] == want(2, packed)
        CollectiveShardSet.hybrid_on_device = True
        same_i, same_s = cs.search_dense(Q, 40)
        oi, os_ = oracle.dense_search(X, Q, 40, oracle.COSINE)
        assert np.array_equal(same_i, oi) and np.allclose(same_s, os_, atol=2e-6)
        mgr.stop_workers()

        # collective ingest over nccl: the batch travels as device tensors
        m2 = MilvusIndexManager(semantic_dim=d, sparse_dim=V, connect=False, dtype="float16")
        m2._connect()
        h2 = _native.ShardHandle(d, _native.HR_F16, _native.HR_METRIC_COSINE, V, 0)
        m2.attach_shards([h2], rows_of=[np.zeros(0, np.int64)], process_group=True, local_ids=True)
        for a, b in ((0, 9000), (9000, n)):
            m2.add_rows(X[a:b], (ptr[a:b + 1], idx, val))
        m2.finalize()
        gi, gs = m2._main.search_dense(Q, 40)
        assert np.array_equal(gi, oi) and np.allclose(gs, os_, atol=2e-6)
        m2.save_snapshot(tmp)
        assert m2._main.row_maps()[0].tolist() == list(range(n))
        m2.stop_workers()
        ret[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(420)
def test_the_nccl_branches_run_on_one_rank(gpu, tmp_path):
    """What a one-GPU box can prove about `backend="nccl"`: with a group of ONE rank the collectives are trivial, but every
    line that differs from the gloo path runs — the packet lives on the device and the hybrid round's operands are VIEWS of
    it (alignment, dtypes), the gather / all-gather / status all-reduce take CUDA tensors, collective ingest broadcasts the
    batch as device tensors.  Answers against the oracle.  Skipped (not failed) where RCCL cannot create a communicator."""
    import torch.multiprocessing as mp
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_nccl_worker, args=(1, port, ret, str(tmp_path)), nprocs=1, join=True)
    if "skip" in ret:
        pytest.skip(f"RCCL not usable on this box: {ret['skip']}")
    assert dict(ret) == {0: True}
