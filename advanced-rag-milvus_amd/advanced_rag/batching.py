"""Coalescing of concurrent `MilvusIndexManager.search` calls into batched device searches.

The reference serves up to 64 in-flight `retrieve()` calls on one event loop (service.py:136,149); each of them
gathers its two or three `index_manager.search` calls (retrieval.py:293-306), and every such call is one RPC that the
Milvus server is free to batch with the others (indexing.py:503-506 runs it in a worker thread).  Here a search is a
scan of the whole shard, so the counterpart of the server's request queue is this front: calls that arrive while a
round of scans is in flight — or within a short window of the first call of a round — are packed per
(collection, top_k, filter expression, search params) into ONE `hr_search_dense_dev` / `hr_search_sparse_dev` batch
(and the rank fusions of the same callers into one `hr_fuse_rrf_dev`, or — weighted score fusions, a kind of their own —
into one `hr_fuse_scores_dev`; fusions of up to 16 lists, kind "fuse_n", into one `hr_fuse_lists_dev`), run on the front's own stream with one
synchronisation per round, and the per-query lists are handed back to the awaiting coroutines.  Lists the device form
could not prove exact are redone through the host form, which widens the candidate set by itself.

Range searches (search_params {"params": {"radius": r, "range_filter": f}} on a dense collection) coalesce too: the two
numbers are per-query operands of `hr_search_dense_range_dev` (the request carries them beside its query, RangedQuery),
the request key only says "ranged" — ranged requests with different bounds share a launch, and never one with unranged
requests.

Grouping searches (search(..., group_by_field=F)) coalesce the same way; the field is part of the request key, so grouped and
ungrouped requests never share a launch.  Their batch searches the window K' (MilvusIndexManager.group_window) and runs ONE
`hr_group_select_dev` for all of its queries behind the search on the same stream; a query whose window ended before its
top_k-th group is redone through the manager's blocking loop, which continues the ranking exactly.  The group size is part of
the key too: a batch with group_size > 1 runs ONE `hr_group_select_n_dev`, and a query is answered from it only when both of its
flag bits are set (the groups are final and so are their members); any other is redone through the blocking loop's two phases.

A caller that has BOTH embeddings of a request in hand (HybridRetriever._retrieve_inner via
MilvusIndexManager.hybrid_search) submits one "hybrid" request instead of two searches and a fusion: the batch runs as
one `hr_search_hybrid_dev` (both scans, the fused finishing kernel) + one `hr_post_lists_dev` (RRF) — the engine's own
step — and the caller gets the fused top-k with the per-modality scores in ONE round instead of two.  A request of a
diversifying profile (MMR; only from a manager created with mmr_on_device=True) takes the same round with the WHOLE fused
list kept (4 x top_k entries) and one `hr_mmr_select_dev` behind it on the same stream; lambda is a per-query operand, so
profiles that differ only in lambda share the round.  A request with fusion="weighted" carries the fusion mode and its two norm
codes in the key: it gets an engine whose post kernel fuses by weighted scores, and never shares a launch with an RRF request.

Decay rerankings (search(..., ranker=DecayRanker(...)) behind its plain search, retrieve() with RetrievalConfig(decay=...)
behind its fusion) are a kind of their own: the field, the norm code, the padded list length and the score type are the key;
origin, offset, coefficient and function travel per query (hr_decay_query), so requests with different curves share ONE
`hr_decay_rerank_dev` launch (stats["decay_launches"]).  In the one-round path the same kernel runs behind `hr_post_lists_dev`
on the hybrid stream, over the whole fused list, before MMR or the cut.

Vector MMR selections (search(..., ranker=MMRRanker(...)) behind its plain search, retrieve() with
RetrievalConfig(mmr_similarity="embedding") behind its fusion) are wired the same way, kind "mmr": the collection, the padded
list length, the norm code and the score type are the key, lambda travels per query, and the requests of a round share ONE
`hr_mmr_select_vec_dev` launch (counted in stats["mmr_launches"] beside the token-Jaccard launches).

Boost rerankings (search(..., ranker=BoostRanker | FunctionScore) behind its plain search, retrieve() with
RetrievalConfig(boost=...) behind its fusion) are kind "boost": both modes, the norm code, the direction, the padded list
length and the score type are the key; the functions travel per query (hr_boost_func: the cached device mask of the
function's filter, the group-key tensor of a keyed draw, weight, seed), padded to the chunk's largest number with inactive
slots, so requests with different filters, weights and seeds share ONE `hr_boost_rerank_dev` launch
(stats["boost_launches"]).  The launch state holds the mask and key tensors until the stream has been synchronised: the
32-entry mask cache may evict one meanwhile.  In the one-round path the kernel runs behind `hr_post_lists_dev`, before the
decay ranker when both are set.

Late-interaction rerankings (search(..., ranker=MaxSimRanker(...)) behind its plain search, retrieve() with
RetrievalConfig(late_interaction=True) behind its fusion) are kind "maxsim": the collection, the padded list length and the
token dim are the key; the query tokens are padded to the batch's largest Tq and the token count travels per query, so
requests with different token counts share ONE `hr_maxsim_rerank_dev` launch (stats["maxsim_launches"]).

One worker thread per manager; the event loop never blocks on the GPU.
"""
from __future__ import annotations

import queue
import threading
import time
from concurrent.futures import Future
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .engine import EngineConfig, HybridSearchEngine, pack_sparse_queries
from .staging import dense_rows_device, dense_rows_host, list_buffers, upload_sparse


def _deliver(fut: Future, value) -> None:
    """Hand a result to a caller that may be gone: a request whose awaiting coroutine timed out or was cancelled has a
    cancelled Future (asyncio.wrap_future propagates it), and set_result on it raises InvalidStateError — which must
    never reach the other requests of the batch."""
    try:
        if not fut.done():
            fut.set_result(value)
    except Exception:   # InvalidStateError: cancelled between the check and the call
        pass


def _fail(fut: Future, exc: BaseException) -> None:
    try:
        if not fut.done():
            fut.set_exception(exc)
    except Exception:
        pass


def _answer(fut: Future, fn, *args) -> None:
    """Answer a request with the value of fn(*args), or fail it with what the call raised."""
    try:
        _deliver(fut, fn(*args))
    except Exception as e:
        _fail(fut, e)


def _set_many(items) -> None:
    """On the event loop: the answers of one round, in one callback."""
    for fut, ok, value in items:
        if not fut.done():          # a caller that timed out or was cancelled is simply skipped
            if ok:
                fut.set_result(value)
            else:
                fut.set_exception(value)


class _LoopFuture:
    """What a coroutine's request carries instead of a concurrent Future: the asyncio future it awaits.  Answers are
    collected in the front's outbox and handed to the loop with ONE call_soon_threadsafe per round (asyncio.wrap_future
    costs a concurrent future, a chained callback and a loop wake-up per request)."""
    __slots__ = ("loop", "afut", "outbox", "_done")

    def __init__(self, loop, afut, outbox):
        self.loop, self.afut, self.outbox, self._done = loop, afut, outbox, False

    def done(self) -> bool:
        return self._done or self.afut.cancelled()     # a benign cross-thread read: worst case one unread answer

    def set_running_or_notify_cancel(self) -> bool:
        return not self.afut.cancelled()

    def set_result(self, value) -> None:
        self._done = True
        self.outbox.setdefault(self.loop, []).append((self.afut, True, value))

    def set_exception(self, exc) -> None:
        self._done = True
        self.outbox.setdefault(self.loop, []).append((self.afut, False, exc))


@dataclass
class RangedQuery:
    """The payload of a dense range-search request: the query and its (radius, range_filter)."""
    query: Any
    bounds: Tuple[float, float]


@dataclass
class _Request:
    kind: str                 # "dense" | "sparse" | "fuse" | "fuse_scores" | "fuse_n" | "decay" | "boost" | "mmr" | "maxsim" | "hybrid" | "encode"
    key: Tuple                # requests with equal (kind, key) share a launch
    payload: Any
    future: Future = field(default_factory=Future)


class SearchCoalescer:
    """Batches requests of one MilvusIndexManager.  `max_batch` bounds the queries per launch (256 = the largest single
    dense pass); `window_s` is how long a round keeps waiting for the next request after the last one
    arrived (the sibling searches of one retrieve() are microseconds apart; under load the queue is never empty and the
    window never runs)."""

    def __init__(self, manager, max_batch: int = 256, window_s: float = 40e-6):
        self.mgr = manager
        self.max_batch = int(max_batch)
        self.window_s = float(window_s)
        self._q: "queue.SimpleQueue[Optional[_Request]]" = queue.SimpleQueue()
        self._thread: Optional[threading.Thread] = None
        self._lock = threading.Lock()
        self._closed = False
        # torchrun form (shards.CollectiveShardSet): a round of the front = one round of the shard set, i.e. ONE
        # broadcast + ONE gather for all the dense and sparse searches that share (top_k, filter, drop ratio)
        self.collective = hasattr(getattr(manager, "_main", None), "round")
        if self.collective:
            # a round of the torchrun form costs a broadcast + a gather over every rank whatever it carries: waiting a few
            # hundred microseconds for the other search of the same retrieve() (and for other callers) halves the collectives
            self.window_s = max(self.window_s, 250e-6)
        self.stats = {"rounds": 0, "requests": 0, "dense_launches": 0, "sparse_launches": 0, "fuse_launches": 0,
                      "hybrid_launches": 0, "mmr_launches": 0, "encode_launches": 0, "encoded_texts": 0, "max_batch_seen": 0, "redone_unproven": 0,
                      "group_launches": 0, "redone_grouped": 0, "range_launches": 0, "score_fuse_launches": 0, "decay_launches": 0, "fuse_n_launches": 0, "boost_launches": 0, "maxsim_launches": 0, "busy_s": 0.0}
        self._engines: Dict[Tuple, Any] = {}   # hybrid engines per (top_k, rrf_k, mmr)
        self._inflight: List[_Request] = []    # the requests of the round in progress (failed as a whole if the worker dies)
        self._outbox: Dict[Any, list] = {}     # event loop -> [(asyncio future, ok, value)] of the round in progress

    # ------------------------------------------------------------------ front
    def _put(self, req: _Request) -> None:
        with self._lock:
            if self._closed:
                raise RuntimeError("search front is closed")
            if self._thread is None or not self._thread.is_alive():   # first request, or the worker died: start one
                self._thread = threading.Thread(target=self._guarded, name="search-coalescer", daemon=True)
                self._thread.start()
        self._q.put(req)

    def submit(self, kind: str, key: Tuple, payload: Any) -> Future:
        req = _Request(kind, key, payload)
        self._put(req)
        return req.future

    def _guarded(self):
        """The worker loop with a last line of defence: whatever escapes a round (a HIP error from a stream
        synchronisation, a bug) fails every request that is still waiting — nobody hangs — and ends this thread; the
        next submit() starts a fresh one."""
        self._inflight: List[_Request] = []
        try:
            (self._run_collective if self.collective else self._run)()
        except BaseException as e:   # noqa: BLE001 - the callers must hear about it, whatever it was
            self.stats["worker_failures"] = self.stats.get("worker_failures", 0) + 1
            err = RuntimeError(f"search front worker failed: {type(e).__name__}: {e}")
            for r in self._inflight:
                _fail(r.future, err)
            while True:
                try:
                    r = self._q.get_nowait()
                except queue.Empty:
                    break
                if r is not None:
                    _fail(r.future, err)
            self._flush()
            with self._lock:
                if self._thread is threading.current_thread():
                    self._thread = None

    def submit_async(self, kind: str, key: Tuple, payload: Any):
        """submit() for a caller on an event loop: returns an asyncio future of that loop (await it directly)."""
        import asyncio
        loop = asyncio.get_running_loop()
        afut = loop.create_future()
        self._put(_Request(kind, key, payload, _LoopFuture(loop, afut, self._outbox)))
        return afut

    def _flush(self):
        """Hand the collected answers to their event loops: one wake-up per loop and round."""
        if not self._outbox:
            return
        out = list(self._outbox.items())
        self._outbox.clear()
        for loop, items in out:
            try:
                loop.call_soon_threadsafe(_set_many, items)
            except RuntimeError:      # the loop is closed: nobody is waiting any more
                pass

    def close(self):
        with self._lock:
            self._closed = True
            t = self._thread
        if t is not None:
            self._q.put(None)
            t.join(timeout=30)

    # ------------------------------------------------------------------ worker
    def _collect(self) -> Optional[List[_Request]]:
        """The requests of one round: everything already queued (what piled up while the previous round ran), plus what
        arrives within `window_s` of the LAST arrival, at most 4 windows after the first request.  The wait is a blocking
        get with a timeout — it releases the GIL, so the event loop can go on submitting, and returns the moment a request
        arrives; a lone retrieve() pays the expiry of one window per round (search round, fusion round)."""
        first = self._q.get()
        if first is None:
            return None
        reqs = [first]
        t_first = time.perf_counter()
        while len(reqs) < 4 * self.max_batch:
            try:
                r = self._q.get_nowait()
            except queue.Empty:
                if time.perf_counter() - t_first >= 4 * self.window_s:
                    break
                try:
                    r = self._q.get(timeout=self.window_s)
                except queue.Empty:
                    break
            if r is None:
                self._q.put(None)  # close() arrived behind real work: finish this round first
                break
            reqs.append(r)
        # claim the futures: a request cancelled while it waited in the queue is dropped here, and one that is claimed
        # can no longer be cancelled under the worker's feet (Future.cancel() fails on a running future)
        live = [r for r in reqs if r.future.set_running_or_notify_cancel()]
        self.stats["cancelled_before_launch"] = self.stats.get("cancelled_before_launch", 0) + len(reqs) - len(live)
        self._inflight = live
        return live

    def _rounds(self):
        """The frame both worker loops share: yields each non-empty round's requests until close() and keeps the books around
        it (stats, `_inflight`, the answers for the event loops).  A round that raises leaves `_inflight` to _guarded."""
        while True:
            reqs = self._collect()
            if reqs is None:
                return
            if not reqs:
                continue
            t0 = time.perf_counter()
            self.stats["rounds"] += 1
            self.stats["requests"] += len(reqs)
            yield reqs
            self._inflight = []
            self._flush()
            self.stats["busy_s"] += time.perf_counter() - t0

    def _run(self):
        import torch
        dev = torch.device("cuda", self.mgr.device)
        # one stream per kind of work: the dense and the sparse searches of a round run side by side (a lone retrieve()
        # overlaps its two scans, as its two worker threads did before the front existed)
        streams = {k: torch.cuda.Stream(dev) for k in ("dense", "sparse", "fuse", "fuse_scores", "fuse_n", "decay", "boost", "mmr", "maxsim", "hybrid", "encode")}
        for reqs in self._rounds():
            groups: Dict[Tuple, List[_Request]] = {}
            for r in reqs:
                groups.setdefault((r.kind, r.key), []).append(r)
            launched = []
            for (kind, key), rs in groups.items():
                stream = streams[kind]
                with torch.cuda.stream(stream):
                    step = min(self.max_batch, 128) if kind == "hybrid" else self.max_batch
                    for c0 in range(0, len(rs), step):
                        chunk = rs[c0:c0 + step]
                        self.stats["max_batch_seen"] = max(self.stats["max_batch_seen"], len(chunk))
                        try:
                            launched.append((kind, key, chunk, getattr(self, "_enqueue_" + kind)(torch, dev, stream, key, chunk)))
                        except Exception as e:   # a bad batch must not take the other groups down: one by one
                            launched.append((kind, key, chunk, e))
            for kind in {kind for kind, _ in groups}:
                streams[kind].synchronize()
            for kind, key, chunk, state in launched:
                if isinstance(state, Exception):
                    self._one_by_one(kind, key, chunk)
                    continue
                try:
                    getattr(self, "_scatter_" + kind)(key, chunk, state)
                except Exception as e:  # never leave a caller waiting
                    for r in chunk:
                        _fail(r.future, e)

    def _run_collective(self):
        """Rounds of the torchrun form: the dense and the sparse searches of the callers that share (top_k, filter
        expression, drop ratio) travel in one packet; other combinations take a round of their own."""
        cs = self.mgr._main
        if getattr(cs.dev, "type", "cpu") == "cuda":   # the current device is a per-thread setting: the collectives of this
            import torch                                # thread must run on the rank's GPU
            torch.cuda.set_device(cs.dev)
        for reqs in self._rounds():
            groups: Dict[Tuple, Dict[str, List[_Request]]] = {}
            hybrid: Dict[Tuple, List[_Request]] = {}
            for r in reqs:
                if r.kind == "hybrid":
                    hybrid.setdefault(r.key, []).append(r)
                    continue
                if r.kind == "fuse":
                    _answer(r.future, self.mgr._fuse_rows_blocking, r.payload, r.key)
                    continue
                if r.kind == "fuse_scores":
                    _answer(r.future, self.mgr._fuse_scores_blocking, r.payload, r.key)
                    continue
                if r.kind == "fuse_n":
                    _answer(r.future, self.mgr._fuse_lists_blocking, r.payload, r.key)
                    continue
                coll_name, top_k, expr, params_key, group_field, _ = r.key
                if group_field is not None or self.mgr.collections[coll_name].handle is not cs:
                    # two cases for the manager's blocking path.  A grouping search: its loop searches window after window,
                    # each a round of the shard set.  Or a collection that is NOT spread over the ranks (the local domain
                    # shard): its searches have nothing to do with the shard set's rounds
                    _answer(r.future, self._lists_blocking, r, r.key)
                    continue
                drop = float(dict(params_key).get("drop_ratio_search", 0.0)) if r.kind == "sparse" else None
                groups.setdefault((top_k, expr), {}).setdefault((r.kind, drop), []).append(r)
            for (top_k, expr, drop, rrf_k, _mmr), rs in hybrid.items():   # (MMR requests never get here: hybrid_search declines)
                # both searches and the fusion of these requests as ONE collective round on the device (shards.round_hybrid)
                for c0 in range(0, len(rs), 64):
                    chunk = rs[c0:c0 + 64]
                    try:
                        keep = self.mgr._row_mask(expr)
                        q = dense_rows_host([r.payload[0] for r in chunk])
                        res = cs.round_hybrid(q, [r.payload[1] for r in chunk], top_k, drop, rrf_k,
                                              np.array([[r.payload[2], r.payload[3]] for r in chunk], dtype=np.float64), keep)
                        self.stats["hybrid_launches"] += 1
                        self.stats["max_batch_seen"] = max(self.stats["max_batch_seen"], len(chunk))
                        self._scatter_hybrid_lists(chunk, res["fused_ids"], res["fused_scores"], res["fused_methods"], res["fused_n"],
                                                   res["list_ids"], res["list_scores"], res["proven"])
                    except Exception as e:
                        for r in chunk:
                            _fail(r.future, e)
            for (top_k, expr), by_kind in groups.items():
                dense = next((v for (kind, _), v in by_kind.items() if kind == "dense"), [])
                sparse_sets = [(d, v) for (kind, d), v in by_kind.items() if kind == "sparse"] or [(0.0, [])]
                for n_round, (drop, sparse) in enumerate(sparse_sets):
                    dn = dense if n_round == 0 else []
                    for c0 in range(0, max(len(dn), len(sparse), 1), 64):
                        d_chunk, s_chunk = dn[c0:c0 + 64], sparse[c0:c0 + 64]
                        if not d_chunk and not s_chunk:
                            continue
                        try:
                            keep = self.mgr._row_mask(expr)
                            q = dense_rows_host([r.payload for r in d_chunk]) if d_chunk else None
                            res = cs.round(q, [r.payload for r in s_chunk] if s_chunk else None, top_k, drop or 0.0, keep)
                            self.stats["dense_launches"] += 1 if d_chunk else 0
                            self.stats["sparse_launches"] += 1 if s_chunk else 0
                            self.stats["max_batch_seen"] = max(self.stats["max_batch_seen"], len(d_chunk), len(s_chunk))
                            for chunk, lists in ((d_chunk, res[0]), (s_chunk, res[1])):
                                for i, r in enumerate(chunk):
                                    _deliver(r.future, (lists[0][i], lists[1][i]))
                        except Exception as e:
                            for r in d_chunk + s_chunk:
                                _fail(r.future, e)

    def _lists_blocking(self, r: _Request, key: Tuple):
        """The lists of one dense or sparse request through the manager's blocking single-query path."""
        coll_name, top_k, expr, params_key, group_field, group_size = key
        if isinstance(r.payload, RangedQuery):
            return self.mgr._search_lists_blocking(r.payload.query, coll_name, top_k, expr, dict(params_key), group_field,
                                                   r.payload.bounds)
        return self.mgr._search_lists_blocking(r.payload, coll_name, top_k, expr, dict(params_key), group_field,
                                               group_size=group_size)

    def _one_by_one(self, kind: str, key: Tuple, chunk: List[_Request]):
        """Fallback when a batched launch was refused: each request through the blocking single-query path, so that
        only the request that is actually at fault fails."""
        for r in chunk:
            if kind == "fuse":
                _answer(r.future, self.mgr._fuse_rows_blocking, r.payload, key)
            elif kind == "fuse_scores":
                _answer(r.future, self.mgr._fuse_scores_blocking, r.payload, key)
            elif kind == "fuse_n":
                _answer(r.future, self.mgr._fuse_lists_blocking, r.payload, key)
            elif kind == "decay":
                _answer(r.future, self.mgr._decay_rows_blocking, r.payload, key)
            elif kind == "boost":
                _answer(r.future, self.mgr._boost_rows_blocking, r.payload, key)
            elif kind == "mmr":
                _answer(r.future, self.mgr._mmr_rows_blocking, r.payload, key)
            elif kind == "maxsim":
                _answer(r.future, self.mgr._maxsim_rows_blocking, r.payload, key)
            elif kind == "hybrid":
                _deliver(r.future, None)   # the caller falls back to two searches + a fusion
            elif kind == "encode":
                _answer(r.future, lambda: self.mgr.embedding_generator.encode_to_device([r.payload[1]])[0])
            else:
                _answer(r.future, self._lists_blocking, r, key)

    # ------------------------------------------------------------------ dense
    def _enqueue_dense(self, torch, dev, stream, key, chunk):
        coll_name, top_k, expr, _, group_field, group_size = key
        handle = self.mgr.collections[coll_name].handle.first
        B = len(chunk)
        if isinstance(chunk[0].payload, RangedQuery):   # the key's "ranged" marker: every request of the chunk is one
            return self._enqueue_dense_range(torch, dev, stream, handle, top_k, expr, chunk)
        k = self.mgr.group_window(top_k, group_size) if group_field is not None else top_k
        q = dense_rows_device([r.payload for r in chunk], dev, handle.dim)
        ids, sc, fl = list_buffers(B, k, dev)
        mask = self.mgr._device_row_mask(expr, "dense")
        handle.search_dense_dev(q.data_ptr(), B, k, ids.data_ptr(), sc.data_ptr(), fl.data_ptr(),
                                mask.data_ptr() if mask is not None else 0, stream.cuda_stream)
        self.stats["dense_launches"] += 1
        st = {"ids": ids, "sc": sc, "fl": fl, "keep": (q, mask)}
        if group_field is not None:
            self._group_select(torch, dev, stream, top_k, group_field, group_size, st)
        return st

    def _enqueue_dense_range(self, torch, dev, stream, handle, top_k, expr, chunk):
        """The ranged requests of a round in ONE hr_search_dense_range_dev: the bounds are a [2, B] float64 operand."""
        B = len(chunk)
        q = dense_rows_device([r.payload.query for r in chunk], dev, handle.dim)
        rb = torch.from_numpy(np.array([r.payload.bounds for r in chunk], dtype=np.float64).T.copy()).to(dev)
        ids, sc, fl = list_buffers(B, top_k, dev)
        mask = self.mgr._device_row_mask(expr, "dense")
        handle.search_dense_range_dev(q.data_ptr(), B, top_k, rb[0].data_ptr(), rb[1].data_ptr(), ids.data_ptr(),
                                      sc.data_ptr(), fl.data_ptr(), mask.data_ptr() if mask is not None else 0,
                                      stream.cuda_stream)
        self.stats["dense_launches"] += 1
        self.stats["range_launches"] += 1
        return {"ids": ids, "sc": sc, "fl": fl, "keep": (q, rb, mask)}

    def _group_select(self, torch, dev, stream, top_k, group_field, group_size, st):
        """The first top_k groups of every window of the batch (hr_group_select_dev, same stream, behind the search) -> st["group"]
        = (positions [B, top_k], groups selected [B], flags [B]).  With group_size > 1: hr_group_select_n_dev, positions
        [B, top_k * group_size] (-1 where a group has fewer members), flags 3 = groups and members are final."""
        from . import _native as nat
        ids = st["ids"]
        B, window = int(ids.shape[0]), int(ids.shape[1])
        n = self.mgr.num_rows
        keys = self.mgr._group_keys_on_device().tensor(group_field, n)
        pos = torch.empty((B, top_k * group_size), dtype=torch.int32, device=dev)
        n_sel = torch.empty((B,), dtype=torch.int32, device=dev)
        gfl = torch.empty((B,), dtype=torch.int32, device=dev)
        if group_size > 1:
            cnt = torch.empty((B, top_k), dtype=torch.int32, device=dev)
            nat.group_select_n_dev(ids.data_ptr(), 0, B, window, keys.data_ptr(), n, 0, top_k, group_size, pos.data_ptr(), 0,
                                   cnt.data_ptr(), n_sel.data_ptr(), gfl.data_ptr(), stream.cuda_stream)
            st["keep"] = st["keep"] + (cnt,)
        else:
            nat.group_select_dev(ids.data_ptr(), 0, B, window, keys.data_ptr(), n, 0, top_k, pos.data_ptr(), 0, n_sel.data_ptr(),
                                 gfl.data_ptr(), stream.cuda_stream)
        self.stats["group_launches"] += 1
        st["group"] = (pos, n_sel, gfl)
        st["keep"] = st["keep"] + (keys,)

    # ------------------------------------------------------------------ sparse
    def _enqueue_sparse(self, torch, dev, stream, key, chunk):
        coll_name, top_k, expr, params_key, group_field, group_size = key
        handle = self.mgr.collections[coll_name].handle.first
        drop = float(dict(params_key).get("drop_ratio_search", 0.0))
        B = len(chunk)
        k = self.mgr.group_window(top_k, group_size) if group_field is not None else top_k
        d_ptr, d_idx, d_val, max_nnz = upload_sparse(
            pack_sparse_queries([r.payload for r in chunk], drop, handle.sparse_dim), dev)
        nnz = int(d_idx.shape[0])
        ids, sc, fl = list_buffers(B, k, dev)
        mask = self.mgr._device_row_mask(expr, "sparse")
        handle.search_sparse_dev(d_ptr.data_ptr(), d_idx.data_ptr() if nnz else 0, d_val.data_ptr() if nnz else 0, B,
                                 nnz, int(max_nnz), k, ids.data_ptr(), sc.data_ptr(), fl.data_ptr(),
                                 mask.data_ptr() if mask is not None else 0, stream.cuda_stream)
        self.stats["sparse_launches"] += 1
        st = {"ids": ids, "sc": sc, "fl": fl, "keep": (d_ptr, d_idx, d_val, mask)}
        if group_field is not None:
            self._group_select(torch, dev, stream, top_k, group_field, group_size, st)
        return st

    def _scatter_lists(self, key, chunk, st):
        ids, sc, fl = st["ids"].cpu().numpy(), st["sc"].cpu().numpy(), st["fl"].cpu().numpy()
        group = [t.cpu().numpy() for t in st["group"]] if "group" in st else None
        members = key[5] > 1 if group is not None else False      # group_size > 1: both flag bits must be set
        for i, r in enumerate(chunk):
            if fl[i] != 1:  # ties at the candidate cut: the host form widens the candidate set until the proof holds
                self.stats["redone_unproven"] += 1
                _answer(r.future, self._lists_blocking, r, key)
            elif group is None:
                _deliver(r.future, (ids[i], sc[i]))
            elif group[2][i] != (3 if members else 1):
                # the window ended before the top_k-th group (or, with group_size > 1, before a group's last member was
                # proven): the blocking loop continues the ranking
                self.stats["redone_grouped"] += 1
                _answer(r.future, self._lists_blocking, r, key)
            elif members:
                at = group[0][i][group[0][i] >= 0]          # slot order = group order, members in list order
                _deliver(r.future, (ids[i][at], sc[i][at]))
            else:
                at = group[0][i, :int(group[1][i])]
                _deliver(r.future, (ids[i][at], sc[i][at]))

    _scatter_dense = _scatter_sparse = _scatter_lists     # what _run looks up as "_scatter_" + kind

    # ------------------------------------------------------------------ hybrid (both searches + RRF of a request)
    def _enqueue_hybrid(self, torch, dev, stream, key, chunk):
        top_k, expr, drop, rrf_k, mmr = key[:5]
        fuse, decay = key[5:], ()   # fuse: () = RRF, or ("weighted", norm code of the semantic list, of the sparse list)
        if "decay" in fuse:         # then ("decay", field, norm code): the fused list is kept whole and reranked before MMR / the cut
            fuse, decay = fuse[:fuse.index("decay")], fuse[fuse.index("decay") + 1:]
        boost = ()
        if "boost" in fuse:         # before it ("boost", function mode, boost mode, norm code, direction): reranked before the decay ranker
            fuse, boost = fuse[:fuse.index("boost")], fuse[fuse.index("boost") + 1:]
        whole = mmr or bool(decay) or bool(boost)
        handle = self.mgr.collections["semantic_index"].handle.first
        ekey = (top_k, rrf_k, whole) + fuse
        eng = self._engines.get(ekey)
        if eng is None:
            if len(self._engines) >= 16:
                self._engines.clear()
            weighted = {"fusion": "weighted", "norms": (fuse[1], fuse[2], 0)} if fuse else {}
            eng = self._engines[ekey] = HybridSearchEngine(
                handle, EngineConfig(top_k=top_k, rrf_k=rrf_k, enable_reranking=False,
                                     fused_k=4 * top_k if whole else None, **weighted), device=str(dev))   # MMR, decay: two 2 * top_k lists, whole
        # the fusion weights are per REQUEST (a weight_adapter may pick them per query, reference retrieval.py:251-262):
        # they travel as a [B, 3] operand of the post kernel, so requests with different weights still share the round
        wq = torch.from_numpy(np.array([[r.payload[2], r.payload[3], 0.0] for r in chunk], dtype=np.float64)).to(dev)
        q = dense_rows_device([r.payload[0] for r in chunk], dev, handle.dim)
        packed = pack_sparse_queries([r.payload[1] for r in chunk], drop, handle.sparse_dim)
        if not packed[1].size:
            raise ValueError("no sparse terms in the batch")   # -> one by one through the general path
        d_sparse = upload_sparse(packed, dev)
        mask = self.mgr._device_row_mask(expr, "dense")
        b = eng.search(q, d_sparse, rowmask=mask, weights=wq)
        self.stats["hybrid_launches"] += 1
        self.stats["dense_launches"] += 1
        self.stats["sparse_launches"] += 1
        # the engine reuses ONE buffer set per batch size: another group (or the next chunk of this one) with the same B
        # is enqueued before this round is read back, so the results are copied out here, in stream order
        if boost:       # (the functions are the request's last operand, behind the decay ranker's)
            b = self._boost_fused(torch, dev, stream, boost, chunk, b)
        if decay:
            b = self._decay_fused(torch, dev, stream, decay, chunk, b)
        if mmr:
            return {"b": self._mmr_select(torch, dev, stream, top_k, chunk, b), "keep": (q, d_sparse, mask, wq)}
        if decay or boost:       # the cut: the first top_k of the reranked list
            out = {k: b[k][:, :top_k].clone() for k in ("fused_ids", "fused_scores", "fused_methods", "fused_raw")}
            out.update(fused_n=b["fused_n"].clamp(max=top_k), keep=b["keep"], **{k: b[k].clone() for k in ("ids", "scores", "flags")})
            return {"b": out, "keep": (q, d_sparse, mask, wq)}
        out = {k: b[k].clone() for k in ("fused_ids", "fused_scores", "fused_methods", "fused_n", "ids", "scores", "flags")}
        return {"b": out, "keep": (q, d_sparse, mask, wq)}

    def _decay_fused(self, torch, dev, stream, decay, chunk, b):
        """The decay ranker over the whole fused lists of the batch (hr_decay_rerank_dev, same stream, behind the post kernel)
        -> the engine's buffers with fused_ids / fused_scores in decayed order (scores = the final ones), the method bits
        following through the positions, fused_raw = the fusion's scores in the same order."""
        field, norm = decay
        B, fk = len(chunk), int(b["fused_ids"].shape[1])
        pos, oi, os_, on, keep = self._decay_launch(torch, dev, stream, field, norm, [r.payload[5] for r in chunk], b["fused_ids"],
                                                    b["fused_scores"], True, b["fused_n"], B, fk)
        at = pos.clamp(min=0).to(torch.int64)      # (-1 padding lies beyond fused_n: never read)
        return {"fused_ids": oi, "fused_scores": os_, "fused_methods": b["fused_methods"].gather(1, at),
                "fused_raw": b.get("fused_raw", b["fused_scores"]).gather(1, at), "fused_n": on, "ids": b["ids"],
                "scores": b["scores"], "flags": b["flags"], "keep": (keep, pos, b.get("keep"))}

    def _boost_fused(self, torch, dev, stream, boost, chunk, b):
        """The boost ranker over the whole fused lists of the batch (hr_boost_rerank_dev, same stream, behind the post kernel)
        -> the engine's buffers in boosted order, as _decay_fused returns them."""
        B, fk = len(chunk), int(b["fused_ids"].shape[1])
        pos, oi, os_, _, on, keep = self._boost_launch(torch, dev, stream, boost, [r.payload[-1] for r in chunk], b["fused_ids"],
                                                       b["fused_scores"], True, b["fused_n"], B, fk)
        at = pos.clamp(min=0).to(torch.int64)      # (-1 padding lies beyond fused_n: never read)
        return {"fused_ids": oi, "fused_scores": os_, "fused_methods": b["fused_methods"].gather(1, at),
                "fused_raw": b["fused_scores"].gather(1, at), "fused_n": on, "ids": b["ids"], "scores": b["scores"],
                "flags": b["flags"], "keep": (keep, pos)}

    def _mmr_select(self, torch, dev, stream, top_k, chunk, b):
        """HybridRetriever._mmr_diversify over the whole fused lists of the batch (hr_mmr_select_dev, same stream) -> the
        buffers _scatter_hybrid reads, with fused_* = the selected entries in selection order and fused_n = their number."""
        from . import _native as nat
        B = len(chunk)
        lam = torch.from_numpy(np.array([r.payload[4] for r in chunk], dtype=np.float64)).to(dev)
        indptr, tok, rows = self.mgr._token_sets_on_device().tensors()
        pos = torch.empty((B, top_k), dtype=torch.int32, device=dev)
        n_sel = torch.empty((B,), dtype=torch.int32, device=dev)
        nat.mmr_select_dev(b["fused_ids"].data_ptr(), b["fused_scores"].data_ptr(), b["fused_n"].data_ptr(), B,
                           int(b["fused_ids"].shape[1]), indptr.data_ptr() if rows else 0, tok.data_ptr() if rows else 0,
                           rows, 0, lam.data_ptr(), top_k, pos.data_ptr(), n_sel.data_ptr(), stream.cuda_stream)
        self.stats["mmr_launches"] += 1
        at = pos.clamp(min=0).to(torch.int64)      # (-1 padding lies beyond fused_n: never read)
        out = {k: b[k].gather(1, at) for k in ("fused_ids", "fused_scores", "fused_methods", "fused_raw") if k in b}
        out.update(fused_n=n_sel, **{k: b[k].clone() for k in ("ids", "scores", "flags")})
        out["keep"] = (lam, indptr, tok, pos, b.get("keep"))
        return out

    def _scatter_hybrid(self, key, chunk, st):
        b = st["b"]
        fi, fs = b["fused_ids"].cpu().numpy(), b["fused_scores"].cpu().numpy()
        fm, fn = b["fused_methods"].cpu().numpy(), b["fused_n"].cpu().numpy()
        ids, sc, fl = b["ids"].cpu().numpy(), b["scores"].cpu().numpy(), b["flags"].cpu().numpy()
        self._scatter_hybrid_lists(chunk, fi, fs, fm, fn, ids, sc, fl.min(axis=0) == 1,
                                   b["fused_raw"].cpu().numpy() if "fused_raw" in b else None)

    def _scatter_hybrid_lists(self, chunk, fi, fs, fm, fn, ids, sc, proven, raw=None):
        # score of a fused row in the list its payload comes from: the dense list if the row is in it, else the sparse one
        # (HybridRetriever._assemble_fused); rows are unique within a list
        in_d = fi[:, :, None] == ids[0][:, None, :]
        in_s = fi[:, :, None] == ids[1][:, None, :]
        orig = np.where(in_d.any(axis=2), np.take_along_axis(sc[0], in_d.argmax(axis=2), axis=1),
                        np.take_along_axis(sc[1], in_s.argmax(axis=2), axis=1))
        for i, r in enumerate(chunk):
            if not proven[i]:   # ties at a candidate cut: the general path redoes the searches through the host forms
                self.stats["redone_unproven"] += 1
                _deliver(r.future, None)
                continue
            n = int(fn[i])
            res = (fi[i, :n].copy(), fs[i, :n].copy(), fm[i, :n].copy(), orig[i, :n].copy())
            _deliver(r.future, res + (raw[i, :n].copy(),) if raw is not None else res)   # decay: the fusion's scores beside the final ones

    # ------------------------------------------------------------------ query encoder
    def _enqueue_encode(self, torch, dev, stream, key, chunk):
        """The query texts of a round's cache misses in ONE forward of the sentence encoder (the reference embeds each
        request alone, indexing.py:601-627; its batch form loops per text, :580-587): payload = (cache key, text).  The rows
        go into the manager's device-resident embedding table (when it has one) and are handed to the callers as device
        tensors — the search round that follows reads them in place, no host hop."""
        gen = self.mgr.embedding_generator
        texts: Dict[str, str] = {}
        for r in chunk:
            texts.setdefault(r.payload[0], r.payload[1])
        vecs = gen.encode_to_device(list(texts.values()), batch_size=len(texts))
        table = getattr(self.mgr, "_dev_cache", None)
        rows = {k: (table.store(k, vecs[i]) if table is not None else vecs[i]) for i, k in enumerate(texts)}
        self.stats["encode_launches"] += 1
        self.stats["encoded_texts"] += len(texts)
        return {"rows": rows, "keep": vecs}

    def _scatter_encode(self, key, chunk, st):
        for r in chunk:
            _deliver(r.future, st["rows"][r.payload[0]])

    # ------------------------------------------------------------------ fuse
    def _enqueue_fuse(self, torch, dev, stream, key, chunk):
        from . import _native as nat
        wa, wb, wc, rrf_k = key
        B = len(chunk)
        ka = max(1, max(len(r.payload[0]) for r in chunk))
        kb = max(len(r.payload[1]) for r in chunk)
        kc = max(len(r.payload[2]) for r in chunk)
        host = np.full((B, ka + kb + kc), -1, dtype=np.int64)
        for i, r in enumerate(chunk):
            a, b, c = r.payload
            host[i, :len(a)] = a
            host[i, ka:ka + len(b)] = b
            host[i, ka + kb:ka + kb + len(c)] = c
        d = torch.from_numpy(host).to(dev)
        la = d[:, :ka].contiguous()
        lb = d[:, ka:ka + kb].contiguous() if kb else None
        lc = d[:, ka + kb:].contiguous() if kc else None
        total = ka + kb + kc
        oi = torch.empty((B, total), dtype=torch.int64, device=dev)
        os_ = torch.empty((B, total), dtype=torch.float64, device=dev)
        om = torch.empty((B, total), dtype=torch.int32, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        nat.fuse_rrf_dev(la.data_ptr(), ka, lb.data_ptr() if kb else 0, kb, lc.data_ptr() if kc else 0, kc, B, wa, wb, wc,
                         rrf_k, total, oi.data_ptr(), os_.data_ptr(), om.data_ptr(), on.data_ptr(), stream.cuda_stream)
        self.stats["fuse_launches"] += 1
        return {"oi": oi, "os": os_, "om": om, "on": on, "keep": (la, lb, lc)}

    def _scatter_fuse(self, key, chunk, st):
        oi, os_, om, on = st["oi"].cpu().numpy(), st["os"].cpu().numpy(), st["om"].cpu().numpy(), st["on"].cpu().numpy()
        for i, r in enumerate(chunk):
            n = int(on[i])
            _deliver(r.future, (oi[i, :n].copy(), os_[i, :n].copy(), om[i, :n].copy()))

    # ------------------------------------------------------------------ weighted score fusion
    def _enqueue_fuse_scores(self, torch, dev, stream, key, chunk):
        """The weighted score fusions of a round in ONE hr_fuse_scores_dev: key = the three norm codes, payload =
        (((rows, scores) x 3), (wa, wb, wc)); the weights travel as the [B, 3] per-query operand."""
        from . import _native as nat
        B = len(chunk)
        k = [max(len(r.payload[0][m][0]) for r in chunk) for m in range(3)]
        k[0] = max(1, k[0])
        total = sum(k)
        ids = np.full((B, total), -1, dtype=np.int64)
        sc = np.zeros((B, total), dtype=np.float32)
        off = (0, k[0], k[0] + k[1])
        for i, r in enumerate(chunk):
            for m, (rows, scores) in enumerate(r.payload[0]):
                ids[i, off[m]:off[m] + len(rows)] = rows
                sc[i, off[m]:off[m] + len(rows)] = scores
        d_ids, d_sc = torch.from_numpy(ids).to(dev), torch.from_numpy(sc).to(dev)
        wq = torch.from_numpy(np.array([r.payload[1] for r in chunk], dtype=np.float64)).to(dev)
        li = [d_ids[:, off[m]:off[m] + k[m]].contiguous() if k[m] else None for m in range(3)]
        ls = [d_sc[:, off[m]:off[m] + k[m]].contiguous() if k[m] else None for m in range(3)]
        oi = torch.empty((B, total), dtype=torch.int64, device=dev)
        os_ = torch.empty((B, total), dtype=torch.float64, device=dev)
        om = torch.empty((B, total), dtype=torch.int32, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        args = []
        for m in range(3):
            args += [li[m].data_ptr() if k[m] else 0, ls[m].data_ptr() if k[m] else 0, k[m], int(key[m])]
        nat.fuse_scores_dev(*args, B, 0.0, 0.0, 0.0, wq.data_ptr(), total, oi.data_ptr(), os_.data_ptr(), om.data_ptr(),
                            on.data_ptr(), stream.cuda_stream)
        self.stats["score_fuse_launches"] += 1
        return {"oi": oi, "os": os_, "om": om, "on": on, "keep": (li, ls, wq)}

    _scatter_fuse_scores = _scatter_fuse

    # ------------------------------------------------------------------ multi-list fusion
    def _enqueue_fuse_n(self, torch, dev, stream, key, chunk):
        """The multi-list fusions of a round in ONE hr_fuse_lists_dev: key = (mode, n_lists, padded k_in, norm codes, rrf_k,
        top_k), payload = (((rows, scores) per list), weights); lists are padded with -1 and the weights travel as the
        [B, n_lists] per-query operand, so requests with different weights share the launch."""
        from . import _native as nat
        from .multi_search import stage_fuse_lists
        mode, n_lists, k_in, norms, rrf_k, top_k = key
        B = len(chunk)
        ids, sc, wq = stage_fuse_lists([r.payload for r in chunk], key)
        d_ids, d_wq = torch.from_numpy(ids).to(dev), torch.from_numpy(wq).to(dev)
        d_sc = torch.from_numpy(sc).to(dev) if sc is not None else None
        oi = torch.empty((B, top_k), dtype=torch.int64, device=dev)
        os_ = torch.empty((B, top_k), dtype=torch.float64, device=dev)
        om = torch.empty((B, top_k), dtype=torch.int32, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        nat.fuse_lists_dev(d_ids.data_ptr(), d_sc.data_ptr() if d_sc is not None else 0, n_lists, k_in, B, mode, rrf_k, norms,
                           None, d_wq.data_ptr(), top_k, oi.data_ptr(), os_.data_ptr(), om.data_ptr(), on.data_ptr(),
                           stream.cuda_stream)
        self.stats["fuse_n_launches"] += 1
        return {"oi": oi, "os": os_, "om": om, "on": on, "keep": (d_ids, d_sc, d_wq)}

    _scatter_fuse_n = _scatter_fuse

    # ------------------------------------------------------------------ decay ranker
    def _decay_launch(self, torch, dev, stream, field, norm, operands, d_ids, d_scores, f64, d_n, B, k_in):
        """ONE hr_decay_rerank_dev over B lists already in HBM, whole lists out (k_out = k_in), on `stream`
        -> (positions int32 [B, k_in], rows, float64 final scores, entries [B], what must stay alive)."""
        from . import _native as nat
        n_rows = self.mgr.num_rows
        col, kind = self.mgr._decay_columns_on_device().tensor(field, n_rows, self.mgr._filters_on_device())
        params = np.zeros(B, dtype=nat.DECAY_QUERY_DTYPE)
        for i, (origin, offset, coef, func) in enumerate(operands):
            params[i] = (origin, offset, coef, func, 0)
        d_params = torch.from_numpy(params.view(np.uint8).reshape(B, -1)).to(dev)
        pos = torch.empty((B, k_in), dtype=torch.int32, device=dev)
        oi = torch.empty((B, k_in), dtype=torch.int64, device=dev)
        os_ = torch.empty((B, k_in), dtype=torch.float64, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        nat.decay_rerank_dev(d_ids.data_ptr(), d_scores.data_ptr(), f64, d_n.data_ptr(), B, k_in, col.data_ptr(), kind, n_rows, 0,
                             d_params.data_ptr(), norm, k_in, pos.data_ptr(), oi.data_ptr(), os_.data_ptr(), on.data_ptr(),
                             stream.cuda_stream)
        self.stats["decay_launches"] += 1
        return pos, oi, os_, on, (col, d_params)

    def _enqueue_decay(self, torch, dev, stream, key, chunk):
        """The decay rerankings of a round in ONE launch: key = (field, norm code, padded list length, scores are float64),
        payload = (rows, scores, (origin, offset, coef, func))."""
        field, norm, width, f64 = key
        B = len(chunk)
        ids = np.full((B, width), -1, dtype=np.int64)
        sc = np.zeros((B, width), dtype=np.float64 if f64 else np.float32)
        n = np.zeros(B, dtype=np.int32)
        for i, r in enumerate(chunk):
            rows, scores, _ = r.payload
            n[i] = len(rows)
            ids[i, :n[i]] = rows
            sc[i, :n[i]] = scores
        d_ids, d_sc, d_n = torch.from_numpy(ids).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(n).to(dev)
        pos, oi, os_, on, keep = self._decay_launch(torch, dev, stream, field, norm, [r.payload[2] for r in chunk], d_ids, d_sc,
                                                    f64, d_n, B, width)
        return {"pos": pos, "oi": oi, "os": os_, "on": on, "keep": (d_ids, d_sc, d_n, keep)}

    def _scatter_decay(self, key, chunk, st):
        pos, oi, os_, on = (st[k].cpu().numpy() for k in ("pos", "oi", "os", "on"))
        for i, r in enumerate(chunk):
            n = int(on[i])
            _deliver(r.future, (pos[i, :n].copy(), oi[i, :n].copy(), os_[i, :n].copy()))

    # ------------------------------------------------------------------ boost ranker
    def _boost_launch(self, torch, dev, stream, modes, functions, d_ids, d_scores, f64, d_n, B, k_in):
        """ONE hr_boost_rerank_dev over B lists already in HBM, whole lists out (k_out = k_in), on `stream`: modes =
        (function mode, boost mode, norm code, direction), functions = per query the (filter, weight, seed or None, key field
        or None) of its functions -> (positions int32 [B, k_in], rows, float64 final scores, matched bits, entries [B], what
        must stay alive: the masks and key tensors among it)."""
        from . import _native as nat
        fmode, bmode, norm, asc = modes
        n_rows = self.mgr.num_rows
        n_funcs = max(len(f) for f in functions)
        rec = np.zeros((B, n_funcs), dtype=nat.BOOST_FUNC_DTYPE)       # flags 0: the inactive padding
        masks, keys = {}, {}
        for i, funcs in enumerate(functions):
            for j, (expr, weight, seed, field) in enumerate(funcs):
                m = k = None
                if expr is not None:
                    if expr not in masks:
                        masks[expr] = self.mgr._global_device_mask(expr)
                    m = masks[expr]
                if seed is not None and field is not None:
                    if field not in keys:
                        keys[field] = self.mgr._group_keys_on_device().tensor(field, n_rows)
                    k = keys[field]
                rec[i, j] = (m.data_ptr() if m is not None else 0, k.data_ptr() if k is not None else 0, n_rows,
                             n_rows if k is not None else 0, weight, seed or 0,
                             nat.HR_BOOST_ACTIVE | (nat.HR_BOOST_RANDOM if seed is not None else 0), 0)
        d_funcs = torch.from_numpy(rec.view(np.uint8).reshape(B, -1)).to(dev)
        pos = torch.empty((B, k_in), dtype=torch.int32, device=dev)
        oi = torch.empty((B, k_in), dtype=torch.int64, device=dev)
        os_ = torch.empty((B, k_in), dtype=torch.float64, device=dev)
        om = torch.empty((B, k_in), dtype=torch.int32, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        nat.boost_rerank_dev(d_ids.data_ptr(), d_scores.data_ptr(), f64, d_n.data_ptr(), B, k_in, d_funcs.data_ptr(), n_funcs, 0,
                             fmode, bmode, norm, bool(asc), k_in, pos.data_ptr(), oi.data_ptr(), os_.data_ptr(), om.data_ptr(),
                             on.data_ptr(), stream.cuda_stream)
        self.stats["boost_launches"] += 1
        return pos, oi, os_, om, on, (masks, keys, d_funcs)

    def _enqueue_boost(self, torch, dev, stream, key, chunk):
        """The boost rerankings of a round in ONE launch: key = (function mode, boost mode, norm code, direction, padded list
        length, scores are float64), payload = (rows, scores, functions)."""
        width, f64 = key[4:]
        B = len(chunk)
        ids = np.full((B, width), -1, dtype=np.int64)
        sc = np.zeros((B, width), dtype=np.float64 if f64 else np.float32)
        n = np.zeros(B, dtype=np.int32)
        for i, r in enumerate(chunk):
            rows, scores, _ = r.payload
            n[i] = len(rows)
            ids[i, :n[i]] = rows
            sc[i, :n[i]] = scores
        d_ids, d_sc, d_n = torch.from_numpy(ids).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(n).to(dev)
        pos, oi, os_, om, on, keep = self._boost_launch(torch, dev, stream, key[:4], [r.payload[2] for r in chunk], d_ids, d_sc,
                                                        f64, d_n, B, width)
        return {"pos": pos, "oi": oi, "os": os_, "om": om, "on": on, "keep": (d_ids, d_sc, d_n, keep)}

    def _scatter_boost(self, key, chunk, st):
        pos, oi, os_, om, on = (st[k].cpu().numpy() for k in ("pos", "oi", "os", "om", "on"))
        for i, r in enumerate(chunk):
            n = int(on[i])
            _deliver(r.future, (pos[i, :n].copy(), oi[i, :n].copy(), os_[i, :n].copy(), om[i, :n].copy()))

    # ------------------------------------------------------------------ vector MMR
    def _enqueue_mmr(self, torch, dev, stream, key, chunk):
        """The vector MMR selections of a round in ONE hr_mmr_select_vec_dev launch: key = (collection, padded list length,
        norm code, scores are float64), payload = (rows, scores, lambda, k_out).  lambda travels per query; the launch
        selects the largest k_out asked for, and a greedy selection's shorter answers are prefixes of its longer ones."""
        coll_name, width, norm, f64 = key
        handle = self.mgr.collections[coll_name].handle.first
        B = len(chunk)
        k_out = min(width, max(int(r.payload[3]) for r in chunk))
        ids = np.full((B, width), -1, dtype=np.int64)
        sc = np.zeros((B, width), dtype=np.float64 if f64 else np.float32)
        n = np.zeros(B, dtype=np.int32)
        lam = np.zeros(B, dtype=np.float64)
        for i, r in enumerate(chunk):
            rows, scores, lam[i], _ = r.payload
            n[i] = len(rows)
            ids[i, :n[i]] = rows
            sc[i, :n[i]] = scores
        d_ids, d_sc, d_n, d_lam = (torch.from_numpy(a).to(dev) for a in (ids, sc, n, lam))
        scratch = torch.empty(max(handle.mmr_vec_scratch_bytes(B, width), 16), dtype=torch.uint8, device=dev)
        pos = torch.empty((B, k_out), dtype=torch.int32, device=dev)
        val = torch.empty((B, k_out), dtype=torch.float64, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        handle.mmr_select_vec_dev(d_ids.data_ptr(), d_sc.data_ptr(), f64, norm, d_n.data_ptr(), B, width, d_lam.data_ptr(), k_out,
                                  scratch.data_ptr(), pos.data_ptr(), val.data_ptr(), on.data_ptr(), stream.cuda_stream)
        self.stats["mmr_launches"] += 1
        return {"pos": pos, "val": val, "on": on, "keep": (d_ids, d_sc, d_n, d_lam, scratch)}

    def _scatter_mmr(self, key, chunk, st):
        pos, val, on = (st[k].cpu().numpy() for k in ("pos", "val", "on"))
        for i, r in enumerate(chunk):
            n = min(int(on[i]), int(r.payload[3]))
            _deliver(r.future, (pos[i, :n].copy(), val[i, :n].copy()))

    # ------------------------------------------------------------------ late interaction (MaxSim)
    def _enqueue_maxsim(self, torch, dev, stream, key, chunk):
        """The late-interaction rerankings of a round in ONE hr_maxsim_rerank_dev launch: key = (collection, padded list
        length, token dim), payload = (rows, fp16 query tokens [Tq, dim]).  The query tokens are padded to the batch's
        largest Tq and d_qn travels per query, so requests with different token counts share the launch.  Whole lists out."""
        from . import _native as nat
        _, width, dim = key
        B = len(chunk)
        tq = max(int(r.payload[1].shape[0]) for r in chunk)
        ids = np.full((B, width), -1, dtype=np.int64)
        n = np.zeros(B, dtype=np.int32)
        qt = np.zeros((B, tq, dim), dtype=np.float16)
        qn = np.zeros(B, dtype=np.int32)
        for i, r in enumerate(chunk):
            rows, tokens = r.payload
            n[i], qn[i] = len(rows), tokens.shape[0]
            ids[i, :n[i]] = rows
            qt[i, :qn[i]] = tokens
        d_ids, d_n, d_qt, d_qn = (torch.from_numpy(a).to(dev) for a in (ids, n, qt, qn))
        indptr, val, tok_rows = self.mgr._token_vectors_on_device().tensors()
        pos = torch.empty((B, width), dtype=torch.int32, device=dev)
        oi = torch.empty((B, width), dtype=torch.int64, device=dev)
        os_ = torch.empty((B, width), dtype=torch.float64, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        nat.maxsim_rerank_dev(d_ids.data_ptr(), d_n.data_ptr(), B, width, d_qt.data_ptr(), d_qn.data_ptr(), tq, dim,
                              indptr.data_ptr() if tok_rows else 0, val.data_ptr() if tok_rows else 0, tok_rows, 0, width,
                              pos.data_ptr(), oi.data_ptr(), os_.data_ptr(), on.data_ptr(), stream.cuda_stream)
        self.stats["maxsim_launches"] += 1
        return {"pos": pos, "oi": oi, "os": os_, "on": on, "keep": (d_ids, d_n, d_qt, d_qn, indptr, val)}

    _scatter_maxsim = _scatter_decay
