"""In-HBM shard store behind the reference's index-manager protocol.

`MilvusIndexManager` here is a drop-in for the reference class of the same name
(reference src/advanced_rag/indexing.py:80-713) with the Milvus server replaced
by libhbmrag: the three collections ("semantic_index" dense/COSINE,
"sparse_index" sparse/IP, "domain_index" dense/COSINE; indexing.py:143-180)
live in HBM as a tiled fp16/fp32 matrix plus doc-range postings — on one GPU, or
spread over several (`devices=[0, 1, ...]`: one shard handle per device, searched in
parallel and merged, the counterpart of the reference's server-side `num_shards`,
indexing.py:234-239) — and `search` runs the HIP kernels instead of an RPC
(indexing.py:503-525).
Host and port are accepted and ignored.  Payload columns (content, ids, scalar
fields of the schema, indexing.py:191-225) stay on the host, keyed by row.

Protocol consumed by HybridRetriever (retrieval.py:348-354, :634-648):
  async _generate_semantic_embedding(text) -> float32[dim]
  async _generate_sparse_embedding(text)   -> {"indices","values"} | ndarray
  async _generate_domain_embedding(text, domain)
  async search(query_embedding, collection_name, top_k, filters, search_params)
        -> [{id, content, score, metadata{doc_id, chunk_index, entropy,
             redundancy, domain_density, timestamp}}]   (best first)
plus index_chunks / get_collection_stats / delete_by_filter / close.
"""
from __future__ import annotations

import asyncio
import threading
import logging
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from enum import Enum
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import filters as _filters
from .columns import TokenVectorColumn, FLOAT_COLUMNS, PayloadColumns, check_group_field
from .boost import BoostRanker, FunctionScore, boost_rerank, matched_functions
from .decay import DecayRanker, decay_rerank
from .maxsim import MaxSimRanker, as_fp16_tokens, check_token_dim, maxsim_rerank_csr, maxsim_search_csr
from .mmr import MMRRanker, vector_mmr
from .constants import GROUP_WINDOW_FACTOR, QUERY_MAX_WINDOW, IndexingConstants
from .embedding_cache import DeviceEmbeddingTable, EmbeddingCache, get_semantic_cache
from ._native import HR_MAX_TOPK   # importing the binding module does not load the library
from .shards import PartialAppend, ShardSet, cursor_key_interval, is_native_handle, ord_f32, rank_key  # noqa: F401 (re-exported)
from .staging import dense_rows_device, dense_rows_host, list_buffers

logger = logging.getLogger(__name__)


class IndexType(Enum):
    SEMANTIC = "semantic"
    SPARSE = "sparse"
    DOMAIN = "domain"
    HYBRID = "hybrid"


@dataclass
class IndexConfig:
    collection_name: str
    dimension: int
    index_type: str = "HNSW"   # accepted for compatibility; the store is always exact FLAT
    metric_type: str = "L2"
    index_params: Optional[Dict] = None
    enable_dynamic_field: bool = True

    def __post_init__(self):
        if self.index_params is None:
            self.index_params = {"M": 16, "efConstruction": 200}


METRIC_NAMES = ("L2", "IP", "COSINE")


def metric_code(name: str) -> int:
    """Milvus' dense metric_type ("L2" | "IP" | "COSINE") -> the HR_METRIC_* code of include/hbmrag.h."""
    from . import _native as nat
    codes = {"L2": nat.HR_METRIC_L2, "IP": nat.HR_METRIC_IP, "COSINE": nat.HR_METRIC_COSINE}
    if not isinstance(name, str) or name not in codes:
        raise ValueError(f"unknown metric_type {name!r}: expected one of {', '.join(METRIC_NAMES)}")
    return codes[name]


def metric_name(code) -> str:
    """The label of a shard handle's metric code; handles that carry none (stubs) are COSINE collections."""
    return {0: "IP", 1: "COSINE", 2: "L2"}.get(code, "COSINE")


RANGE_KEYS = ("radius", "range_filter")


def range_bounds(params: Optional[Dict], metric: str) -> Optional[Tuple[float, float]]:
    """Milvus' range search: (radius, range_filter) of search_params["params"], or None when neither is given.

    Kept are the rows with radius < score <= range_filter (COSINE, IP) or range_filter <= distance < radius (L2); an
    absent side is unbounded: radius = -inf and range_filter = +inf for COSINE and IP, the opposite for L2.  ValueError
    for a bound that is not a number or is NaN, and for an empty interval (radius >= range_filter; L2: range_filter >=
    radius)."""
    metric_code(metric)
    inner = (params or {}).get("params") or {}
    if not any(k in inner and inner[k] is not None for k in RANGE_KEYS):
        return None
    l2 = metric == "L2"
    fill = {"radius": float("inf") if l2 else float("-inf"), "range_filter": float("-inf") if l2 else float("inf")}
    out = []
    for k in RANGE_KEYS:
        v = inner.get(k)
        if v is None:
            out.append(fill[k])
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{k} must be a number, got {v!r}")
        v = float(v)
        if v != v:
            raise ValueError(f"{k} is NaN")
        out.append(v)
    radius, range_filter = out
    if (range_filter >= radius) if l2 else (radius >= range_filter):
        raise ValueError(f"empty range for {metric}: radius={radius}, range_filter={range_filter} "
                         + ("(kept are range_filter <= distance < radius)" if l2 else "(kept are radius < score <= range_filter)"))
    return radius, range_filter


def deep_window(top_k, offset=0) -> int:
    """W = offset + top_k of a search request, the depth of the ranking it reads.  top_k >= 1 and offset >= 0 are integers
    (bool and floats are refused, as group_size refuses them) and W <= QUERY_MAX_WINDOW, Milvus' cap on offset + limit.
    W <= HR_MAX_TOPK is served by the plain search, a deeper window by the deep search."""
    for name, v in (("top_k", top_k), ("offset", offset)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if top_k < 1:
        raise ValueError(f"top_k must be >= 1, got {top_k}")
    if offset < 0:
        raise ValueError(f"offset must be >= 0, got {offset}")
    if int(top_k) + int(offset) > QUERY_MAX_WINDOW:
        raise ValueError(f"a search takes offset + top_k <= {QUERY_MAX_WINDOW}, got offset={offset}, top_k={top_k}")
    return int(top_k) + int(offset)


def iterator_window(batch_size, limit=None) -> Tuple[int, Optional[int]]:
    """(batch_size, limit) of a search iterator: batch_size an integer in 1 .. QUERY_MAX_WINDOW (one page is one deep
    selection), limit None or an integer >= 1; bool and floats are refused, as deep_window refuses them."""
    for name, v in (("batch_size", batch_size),) + ((("limit", limit),) if limit is not None else ()):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not 1 <= batch_size <= QUERY_MAX_WINDOW:
        raise ValueError(f"batch_size must be in 1 .. {QUERY_MAX_WINDOW}, got {batch_size}")
    if limit is not None and limit < 1:
        raise ValueError(f"limit must be None or >= 1, got {limit}")
    return int(batch_size), None if limit is None else int(limit)


def iterate_ranking(ids, scores, batch_size, limit=None):
    """The pages a search iterator returns for a ranking that is already sorted: ids / scores [n] in ranking order (a -1 id
    ends the ranking) -> (ids, scores) slices of batch_size entries, the last one shorter, `limit` entries in all."""
    batch_size, limit = iterator_window(batch_size, limit)
    ids, scores = np.asarray(ids), np.asarray(scores)
    pad = np.flatnonzero(ids < 0)
    n = int(pad[0]) if len(pad) else len(ids)
    if limit is not None:
        n = min(n, limit)
    for lo in range(0, n, batch_size):
        yield ids[lo:min(lo + batch_size, n)], scores[lo:min(lo + batch_size, n)]


class SearchIterator:
    """pymilvus' search_iterator on one collection: the ranking of ONE query page by page, to any depth.

    A page is the first min(batch_size, remaining limit) rows of the collection's ranking (filter, tombstones and range
    applied as search() applies them) that come strictly after the last hit returned: one call of the cursor forms
    (hr_search_*_deep_after), i.e. one full refine of the shard, whatever the depth.  The iterator holds the last hit's
    (score, row), the count and the manager's row-space generation; nothing is kept on the device between pages, so a
    page sees the collection as it is when the page is asked for: a row deleted meanwhile and not yet returned does not
    appear, an appended row appears if its place is after the cursor, no hit is returned twice.  compact(), load_snapshot()
    and attach_shards() renumber or replace the rows a cursor speaks of: next() then raises RuntimeError."""

    def __init__(self, manager: "MilvusIndexManager", query_embedding, collection_name: str, batch_size=1000, limit=None,
                 filters: Optional[str] = None, search_params: Optional[Dict] = None):
        self.batch_size, self.limit = iterator_window(batch_size, limit)
        if collection_name not in manager.collections:
            raise ValueError(f"Collection {collection_name} not found")
        coll = manager.collections[collection_name]
        params = manager._search_params(coll, search_params)
        self._bounds = manager._range_request(coll, params, None)      # ValueError on the sparse collection, as search()
        if hasattr(coll.handle, "round"):
            raise NotImplementedError("search_iterator is not built for the torchrun form (CollectiveShardSet)")
        self._manager, self._name, self._filters = manager, collection_name, filters
        self._drop = float((params.get("params") or params).get("drop_ratio_search", 0.0))
        self._query = manager._as_sparse_payload(query_embedding) if coll.kind == "sparse" else query_embedding
        self._generation = manager._row_space_generation
        self._after: Optional[Tuple[float, int]] = None
        self.returned = 0
        self._done = False
        if self._bounds is not None:
            try:
                cursor_key_interval(None, self._bounds, coll.metric)
            except ValueError:          # the bounds differ as float64 but no fp32 score lies between them
                self._done = True

    def next_blocking(self) -> List[Dict[str, Any]]:
        """The next page as the usual hit dicts; [] once the ranking or `limit` is exhausted, and from then on."""
        if self._done:
            return []
        m = self._manager
        if m._row_space_generation != self._generation:
            raise RuntimeError(f"the row space of {self._name} was replaced by {m._row_space_reason} since this iterator was "
                               "created: its cursor names a row of the old numbering; create a new iterator")
        k = self.batch_size if self.limit is None else min(self.batch_size, self.limit - self.returned)
        hits = m._iterator_page_blocking(self._query, self._name, k, self._after, self._filters, self._bounds, self._drop)
        if hits:
            self._after = (hits[-1]["score"], hits[-1]["_row"])
            self.returned += len(hits)
        if len(hits) < k or (self.limit is not None and self.returned >= self.limit):
            self._done = True
        return hits

    async def next(self) -> List[Dict[str, Any]]:
        try:
            return await asyncio.wait_for(asyncio.to_thread(self.next_blocking), timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)
        except asyncio.TimeoutError:
            logging.error("shard search timeout for collection %s", self._name)
            raise Exception(f"Search timeout for collection {self._name}")

    def close(self) -> None:
        self._done = True

    def __aiter__(self):
        return self

    async def __anext__(self) -> List[Dict[str, Any]]:
        page = await self.next()
        if not page:
            raise StopAsyncIteration
        return page


class SearchPath:
    """ONE blocking request's way to its rows: one local GPU shard with the row mask in HBM (`shard` is its ShardHandle;
    masks are packed CUDA tensors), or a host mask over every shard of the set (`shard` is None: several shards, the
    torchrun form, stand-ins; masks are bool arrays).  query: the prepared query (a dense vector, or a sparse payload)."""

    def __init__(self, manager: "MilvusIndexManager", coll: "ShardCollection", query, drop: float):
        self.manager, self.coll, self.query, self.drop = manager, coll, query, drop
        self.sparse = coll.kind == "sparse"
        self.shard = manager._device_shard(coll.handle)
        self._q_host = None

    def base(self, filters: Optional[str]):
        """The row mask of a filter expression + tombstones (None = all rows): cached and shared, never written."""
        if self.shard is not None:
            return self.manager._device_row_mask(filters, self.coll.kind)
        return self.manager._row_mask(filters)

    def search(self, mask, k: int, bounds: Optional[Tuple[float, float]] = None, offset: Optional[int] = None):
        """(ids [k], scores [k]) under `mask` through the host forms, which are exact.  bounds: the range form (dense
        only); offset: entries offset .. offset + k - 1 through the deep forms."""
        on, m = (self.coll.handle, (mask,)) if self.shard is None else \
            (self.shard, (None, mask.data_ptr() if mask is not None else 0))       # a ShardHandle: (rowmask, d_rowmask)
        if self.sparse:
            if offset is None:
                ids, sc = on.search_sparse([self.query], k, self.drop, *m)
            else:
                ids, sc = on.search_sparse_deep([self.query], k, offset, self.drop, *m)
            return ids[0], sc[0]
        if self._q_host is None:
            self._q_host = dense_rows_host([self.query])
        if offset is not None:
            ids, sc = on.search_dense_deep(self._q_host, k, offset, *m)
        elif bounds is None:
            ids, sc = on.search_dense(self._q_host, k, *m)
        elif self.shard is not None:
            ids, sc = on.search_dense_range(self._q_host, k, bounds[0], bounds[1], *m)
        else:
            ids, sc = on.search_dense(self._q_host, k, *m, bounds=bounds)
        return ids[0], sc[0]

    def after(self, mask, k: int, after: Optional[Tuple[float, int]], bounds: Optional[Tuple[float, float]] = None):
        """(ids [k], scores [k]): the first k entries of the ranking under `mask` strictly after the cursor `after` =
        (score, row) (None: from the top) through the cursor forms; bounds: a range search's (dense only)."""
        on, m = (self.coll.handle, (mask,)) if self.shard is None else \
            (self.shard, (None, mask.data_ptr() if mask is not None else 0))
        cursor = None if after is None else ([after[0]], [after[1]])
        if self.sparse:
            ids, sc = on.search_sparse_deep_after([self.query], k, cursor, self.drop, *m)
            return ids[0], sc[0]
        if self._q_host is None:
            self._q_host = dense_rows_host([self.query])
        ids, sc = on.search_dense_deep_after(self._q_host, k, cursor, bounds, *m)
        return ids[0], sc[0]


class ShardCollection:
    """What `manager.collections[name]` holds: a named view of one ShardSet (the
    collection's shard handles, one per device) with the handful of Collection methods the reference calls
    (num_entities / flush / load / release / delete, indexing.py:259, :430, :683-701)."""

    def __init__(self, manager: "MilvusIndexManager", name: str, kind: str, handle, dim: int, metric: str):
        self.manager, self.name, self.kind, self.handle, self.dim, self.metric = manager, name, kind, handle, dim, metric

    @property
    def num_entities(self) -> int:
        return self.handle.num_sparse_rows if self.kind == "sparse" else self.handle.num_rows

    @property
    def schema(self) -> str:
        return (f"ShardCollection({self.name}, kind={self.kind}, dim={self.dim}, metric={self.metric}, "
                "fields=[id, chunk_id, doc_id, content, chunk_index, token_count, entropy, redundancy, "
                "domain_density, embedding, metadata_json, timestamp])")

    @property
    def indexes(self) -> List[str]:
        return [f"FLAT/{self.metric} (exact scan, gfx950)"]

    def flush(self):
        self.handle.finalize()

    load = flush

    def release(self):
        return None

    def delete(self, expr: str):
        self.manager._tombstone(expr)

    def compact(self) -> Dict[str, int]:
        """pymilvus' Collection.compact(): drop the deleted rows from the store for good (MilvusIndexManager.compact —
        the collections of a manager share their rows, so all of them are compacted)."""
        return self.manager.compact()

    def query(self, expr: Optional[str] = None, output_fields: Optional[Sequence[str]] = None, limit: Optional[int] = None,
              offset: int = 0) -> List[Dict[str, Any]]:
        """pymilvus' Collection.query(expr, output_fields, limit, offset), synchronous (MilvusIndexManager.query)."""
        return self.manager._query_blocking(self.name, expr, output_fields, limit, offset)

    def search_iterator(self, query_embedding, batch_size=1000, limit=None, filters: Optional[str] = None,
                        search_params: Optional[Dict] = None) -> SearchIterator:
        """pymilvus' Collection.search_iterator, synchronous: page with it.next_blocking() (MilvusIndexManager.search_iterator)."""
        return self.manager.search_iterator(query_embedding, self.name, batch_size, limit, filters, search_params)

    def search_by_ids(self, ids, top_k: int = 20, filters: Optional[str] = None, search_params: Optional[Dict] = None, *,
                      group_by_field: Optional[str] = None, group_size: int = 1,
                      strict_group_size: Optional[bool] = None) -> List[List[Dict[str, Any]]]:
        """Search with the stored vectors of the entities `ids`, synchronous (MilvusIndexManager.search_by_ids)."""
        return self.manager._search_by_ids_blocking(ids, self.name, top_k, filters, search_params, group_by_field, group_size,
                                                    strict_group_size)


class MilvusIndexManager:
    def __init__(self, host: str = "localhost", port: int = 19530, enable_sharding: bool = True, num_shards: int = 4,
                 semantic_dim: int = 1536, sparse_dim: int = 10000, domain_dim: int = 768, connect: bool = True,
                 *, dtype: str = "float16", device: int = 0, devices: Optional[Sequence[int]] = None,
                 enable_domain: bool = True, device_embedding_cache: int = 0, coalesce: bool = True,
                 semantic_metric: str = "COSINE", domain_metric: str = "COSINE", mmr_on_device: bool = False,
                 group_members: bool = False, token_dim: Optional[int] = None):
        self.host, self.port = host, port
        # late interaction: token_dim = elements per stored token vector (a multiple of 8 in 8..256); None = the collection
        # keeps no token vectors, MaxSimRanker is refused and every call is as before
        self.token_dim = check_token_dim(token_dim) if token_dim is not None else None
        # grouping searches with group_size > 1 (the best group_size rows of each of the top_k best groups): off = such a
        # request is refused, as before the fill phase of device_groups.grouped_search existed
        self.group_members = bool(group_members)
        # MMR profiles (troubleshooting, analysis) through the one-round path: the rows' token sets are mirrored into HBM
        # and hr_mmr_select_dev diversifies the fused lists there (hybrid_search(mmr_lambda=...)); off = the general path
        self.mmr_on_device = bool(mmr_on_device)
        metric_code(semantic_metric), metric_code(domain_metric)   # ValueError for anything but L2 / IP / COSINE
        self.semantic_metric, self.domain_metric = semantic_metric, domain_metric
        self.enable_sharding, self.num_shards = enable_sharding, num_shards
        self.semantic_dim, self.sparse_dim, self.domain_dim = semantic_dim, sparse_dim, domain_dim
        # devices = GPU of every shard (a device may be named more than once); default: one shard on `device`
        self.devices = [int(d) for d in devices] if devices else [int(device)]
        self.dtype, self.device, self.enable_domain = dtype, self.devices[0], enable_domain
        self.collections: Dict[str, ShardCollection] = {}
        self.embedding_generator = None
        self.embedding_executor = ThreadPoolExecutor(max_workers=IndexingConstants.THREAD_POOL_WORKERS,
                                                     thread_name_prefix="embedding-")
        self._main = None      # ShardSet: semantic + sparse
        self._domain = None    # ShardSet: domain
        # payload columns keyed by global row: append-only numeric arrays and offset-encoded strings (columns.py); the
        # filterable ones are mirrored into HBM on first use (device_filters.py)
        self._cols = PayloadColumns()
        self._dev_filters = None
        self._dev_tokens = None    # device_tokens.DeviceTokenSets: the token sets of "content" in HBM, on first use
        self._dev_groups = None    # device_groups.DeviceGroupKeys: the group keys of the fields grouped on, on first use
        self._dev_decay = None     # device_decay.DeviceDecayColumns: the epoch seconds a decay ranker reads, on first use
        self._dev_tokvec = None    # device_token_vectors.DeviceTokenVectors: the rows' token vectors in HBM, on first use
        if self.token_dim is not None:
            self._cols.enable_token_vectors(self.token_dim)
        # grouping searches answered by the blocking loop: searches, windows searched, windows that ended before the
        # top_k-th group and were continued without the groups they showed
        # group_fill_searches: grouping searches with group_size > 1 that needed the fill phase (a group's members were
        # not proven by the window that showed it); group_fill_rounds: the windows that phase searched
        # queries: query() calls answered; query_device: those whose page came from hr_mask_rows_dev (mask never left HBM)
        # search_by_ids: search_by_ids() calls whose ids were resolved and whose stored vectors were fetched
        # deep_searches: searches with offset + top_k > HR_MAX_TOPK, answered by the deep forms (a full refine of the shard)
        # iterator_pages: pages a SearchIterator fetched (each one call of the cursor forms: a full refine of the shard)
        # boost_host_reranks: the same for boost rerankings (hr_boost_rerank_dev)
        # decay_host_reranks: decay rerankings answered by the Python restatement instead of hr_decay_rerank_dev (sharded
        # managers, lists beyond 3 * HR_MAX_TOPK entries, the front's one-by-one fallback after a refused batch)
        # mmr_host_selects: vector MMR selections answered by the Python restatement instead of hr_mmr_select_vec_dev (the
        # same cases)
        # multi_searches: multi_search() calls that passed their checks
        # maxsim_host_reranks: late-interaction rerankings answered by the numpy restatement instead of hr_maxsim_rerank_dev
        # (sharded managers, stand-ins without a device, the front's one-by-one fallback)
        # maxsim_searches: maxsim_search() calls answered by hr_maxsim_scan_dev + hr_deep_topk_dev on one GPU shard;
        # maxsim_host_searches: those answered by the restatement over the host column (sharded managers, stand-ins)
        self.stats = {"group_searches": 0, "group_rounds": 0, "group_continuations": 0, "group_fill_searches": 0,
                      "group_fill_rounds": 0, "queries": 0, "query_device": 0, "search_by_ids": 0, "deep_searches": 0,
                      "decay_host_reranks": 0, "boost_host_reranks": 0, "iterator_pages": 0, "mmr_host_selects": 0, "multi_searches": 0,
                      "maxsim_host_reranks": 0, "maxsim_searches": 0, "maxsim_host_searches": 0}
        # bumped by what renumbers or replaces the rows (compact, load_snapshot, attach_shards): a SearchIterator's cursor
        # names a row, so an iterator created under another generation refuses to go on
        self._row_space_generation = 0
        self._row_space_reason = ""
        self._stats_lock = threading.Lock()    # the loop runs in worker threads and in the front's thread at once
        self._deleted: Optional[np.ndarray] = None
        self._mask_cache: Dict[Any, Optional[np.ndarray]] = {}   # (expr, rows, delete epoch) -> boolean row filter
        self._delete_epoch = 0
        self._synthetic_rows = 0   # rows whose payload is derived from the row number (bulk/benchmark ingest)
        # "embedding cache -> device-resident tensor": with device_embedding_cache=N > 0 the semantic QUERY
        # embeddings are kept in one [N, dim] HBM tensor; a hit hands the search kernel a device pointer
        # (no host hop), a miss encodes once (on the device when the generator offers encode_to_device).
        self._dev_cache_slots = int(device_embedding_cache)
        self._dev_cache = None
        # concurrent search() calls are packed into batched device searches (batching.SearchCoalescer): the counterpart
        # of the Milvus server's request queue (reference indexing.py:503-506 fires one RPC per call and the server
        # batches).  coalesce=False keeps the round-2 behaviour: every call its own scan of the shard.
        self.coalesce = bool(coalesce)
        self._front = None
        self._dev_masks: Dict[Any, Any] = {}   # (expr, rows, delete epoch, kind) -> packed row mask in HBM
        self._mask_lock = threading.RLock()
        if connect:
            self._connect()
            self._initialize_collections()

    # ------------------------------------------------------------------ lifecycle
    def _connect(self):
        from . import _native
        self._native = _native
        _native.load_library()

    @property
    def _store_half(self) -> bool:
        return self.dtype in ("float16", "fp16", "f16")

    @property
    def _store_code(self) -> int:
        return self._native.HR_F16 if self._store_half else self._native.HR_F32

    @staticmethod
    def _sparse_enabled() -> bool:
        return os.getenv("ENABLE_SPARSE", "1") == "1"

    def _shard_handle(self, kind: str, device: int, path: Optional[str] = None, sparse_on: Optional[bool] = None):
        """A shard handle of the "main" (semantic + sparse) or the "domain" collection on `device`: a new, empty one, or
        the one saved at `path`.  sparse_on: whether a main handle carries the sparse collection (default: the environment)."""
        if kind == "main":
            sparse_on = self._sparse_enabled() if sparse_on is None else sparse_on
            args = (self.semantic_dim, self._store_code, metric_code(self.semantic_metric),
                    self.sparse_dim if sparse_on else 0, device)
        else:
            args = (self.domain_dim, self._store_code, metric_code(self.domain_metric), 0, device)
        make = self._native.ShardHandle
        return make(*args) if path is None else make.load(path, *args)

    def _register_main_collections(self, sparse: bool):
        self.collections["semantic_index"] = ShardCollection(self, "semantic_index", "dense", self._main,
                                                             self.semantic_dim, self.semantic_metric)
        if sparse:
            self.collections["sparse_index"] = ShardCollection(self, "sparse_index", "sparse", self._main,
                                                               self.sparse_dim, "IP")

    def _new_row_space(self, reason: str) -> None:
        self._row_space_generation += 1
        self._row_space_reason = reason

    def _forget_masks(self, rebuild_filters: bool):
        """Drop every cached row mask, host and HBM: the rows changed.  After an APPEND (_append_payload, add_rows) the device
        filter columns, the token sets, the group keys and the epoch seconds stay: they grow in place, every row is uploaded once.  After the row
        space was REPLACED (attach_shards, add_rows_synthetic, load_snapshot, compact) they go too (rebuild_filters) and are
        rebuilt on first use.  close() drops HBM masks only."""
        self._mask_cache.clear()
        self._dev_masks.clear()
        if rebuild_filters:
            self._dev_filters = None
            self._dev_tokens = None
            self._dev_groups = None
            self._dev_decay = None
            self._dev_tokvec = None

    def _initialize_collections(self):
        self._main = ShardSet([self._shard_handle("main", d) for d in self.devices])
        self._register_main_collections(self._sparse_enabled())
        if self.enable_domain:
            self._domain = ShardSet([self._shard_handle("domain", d) for d in self.devices])
            self.collections["domain_index"] = ShardCollection(self, "domain_index", "dense", self._domain,
                                                               self.domain_dim, self.domain_metric)

    def attach_shards(self, handles, rows_of=None, synthetic_rows: int = 0, process_group=None, first_row: int = 0,
                      local_ids: bool = False):
        """Adopt already-built shard handles as the semantic (+ sparse) collection — e.g. the shard a benchmark has
        just filled.  rows_of[s] = global row of every local row of shard s (default: shard s follows shard s-1).

        With `process_group` (torch.distributed, one process per GPU) the collection spans the group's ranks: this
        rank's handle holds global rows [first_row, first_row + its rows) and must carry that offset
        (ShardHandle.set_row_offset); rank 0 answers `search`/`retrieve`, the other ranks call `serve()`.  With
        `local_ids=True` the handle numbers its rows from 0 (rows_of[0] = their global rows; empty at the start) and
        the collection is FILLED through rank 0: index_chunks / add_rows / add_rows_synthetic, finalize and
        save_snapshot on rank 0 become collective operations the serving ranks take part in (shards.py)."""
        if not hasattr(self, "_native"):
            self._connect()
        handles = list(handles)
        if rows_of is None:
            rows_of, base = [], 0
            for h in handles:
                rows_of.append(np.arange(base, base + h.num_rows, dtype=np.int64))
                base += h.num_rows
        local = ShardSet(handles)
        local.rows_of = [np.asarray(r, dtype=np.int64) for r in rows_of]
        local._n = int(sum(len(r) for r in rows_of))
        if process_group is not None:
            import torch.distributed as dist
            from .shards import CollectiveShardSet
            if len(handles) != 1:
                raise ValueError("the torchrun form takes one shard handle per process")
            group = None if process_group is True else process_group
            self._main = CollectiveShardSet(local, first_row, dist, group, local_ids=local_ids)
        else:
            self._main = local
        self.devices = [h.device for h in handles]
        # the collection's metric is the handles' own (COSINE for a handle that carries none)
        self.semantic_metric = metric_name(getattr(handles[0], "metric", None))
        self._register_main_collections(bool(handles[0].sparse_dim))
        self._synthetic_rows = int(synthetic_rows)
        self._forget_masks(rebuild_filters=True)
        self._new_row_space("attach_shards()")

    def serve(self):
        """Ranks > 0 of the torchrun form: answer rank 0's searches until it calls stop_workers()."""
        self._main.serve()

    def stop_workers(self):
        self._main.stop_workers()

    # ------------------------------------------------------------------ host columns
    def _columns(self) -> Dict[str, np.ndarray]:
        """numpy view of the filterable columns for the HOST restatement of the filter semantics (filters.evaluate): CPU
        tests and collections without a device; string fields are materialised as unicode arrays here."""
        if hasattr(self._cols, "filter_columns"):
            return self._cols.filter_columns()
        return {k: np.asarray(v) for k, v in self._cols.items()}

    @property
    def num_rows(self) -> int:
        return self._synthetic_rows or len(self._cols["id"])

    @staticmethod
    def synthetic_id(row: int) -> str:
        """String id of a bulk-ingested row: doc{row//10}::{row%10}::{row:08x}."""
        return f"doc{row // 10}::{row % 10}::{row:08x}"

    def _filters_on_device(self):
        """The device evaluator of this collection's filter expressions, or None (no GPU shard: CPU-only unit tests)."""
        main = getattr(self, "_main", None)
        if main is None or not hasattr(main, "first") or not hasattr(main.first, "_h"):
            return None
        if self._dev_filters is None:
            from .device_filters import DeviceFilters
            self._dev_filters = DeviceFilters(None if self._synthetic_rows else self._cols, main.first.device)
        return self._dev_filters

    def _device_shard(self, shard_set):
        """The ShardHandle of a shard set that is ONE local GPU shard whose filter masks live in HBM (the row mask of a
        search never leaves the device), or None: several shards, the torchrun form, stand-ins without a device — those
        take a host mask over every shard.  The evaluator asked for is the main collection's, for the domain set too."""
        if getattr(shard_set, "n_shards", 1) == 1 and hasattr(shard_set, "handles") and self._filters_on_device() is not None:
            return shard_set.first
        return None

    def _token_sets_on_device(self):
        """The HBM mirror of the rows' token sets (what hr_mmr_select_dev reads), on the main shard's device."""
        if self._dev_tokens is None:
            from .device_tokens import DeviceTokenSets
            self._dev_tokens = DeviceTokenSets(None if self._synthetic_rows else self._cols, self._main.first.device)
        return self._dev_tokens

    def _group_keys_on_device(self):
        """The HBM mirror of the rows' group keys (what hr_group_select_dev / hr_mask_drop_groups_dev read), on the main
        shard's device."""
        with self._mask_lock:
            if self._dev_groups is None:
                from .device_groups import DeviceGroupKeys
                self._dev_groups = DeviceGroupKeys(None if self._synthetic_rows else self._cols, self._main.first.device)
            return self._dev_groups

    def _decay_columns_on_device(self):
        """The HBM mirror of what a decay ranker reads (hr_decay_rerank_dev's d_col), on the main shard's device."""
        with self._mask_lock:
            if self._dev_decay is None:
                from .device_decay import DeviceDecayColumns
                self._dev_decay = DeviceDecayColumns(None if self._synthetic_rows else self._cols, self._main.first.device)
            return self._dev_decay

    def _token_vectors_on_device(self):
        """The HBM mirror of the rows' token vectors (what hr_maxsim_rerank_dev reads), on the main shard's device."""
        with self._mask_lock:
            if self._dev_tokvec is None:
                from .device_token_vectors import DeviceTokenVectors
                self._dev_tokvec = DeviceTokenVectors(self._cols, self._main.first.device)
            return self._dev_tokvec

    def _host_group_keys(self, field: str) -> np.ndarray:
        """int64 group key per global row on the host (collections whose masks are host arrays: several shards, the
        torchrun form, CPU tests)."""
        if self._synthetic_rows:
            from .device_groups import synthetic_group_keys
            return synthetic_group_keys(field, self._synthetic_rows)
        return self._cols.group_keys(field)

    def _count(self, name: str) -> None:
        with self._stats_lock:
            self.stats[name] += 1

    def _check_group_request(self, group_by_field, group_size, top_k=None, strict_group_size=None) -> None:
        """ValueError for what a grouping search does not serve, before anything is searched."""
        if not self.group_members:
            if group_size != 1:
                raise ValueError(f"group_size={group_size!r} is not supported: only group_size=1 (the best row of every group) is "
                                 "built — a window of the ranking cannot prove a group's later members exact")
        else:
            if isinstance(group_size, (bool, np.bool_)) or not isinstance(group_size, (int, np.integer)) or group_size < 1:
                raise ValueError(f"group_size must be an integer >= 1, got {group_size!r}")
            if strict_group_size is not None and not isinstance(strict_group_size, (bool, np.bool_)):
                raise ValueError(f"strict_group_size must be True, False or absent, got {strict_group_size!r}")
            if group_size > 1 and group_by_field is None:
                raise ValueError(f"group_size={group_size} needs group_by_field")
            if group_size > 1 and int(top_k) * int(group_size) > HR_MAX_TOPK:
                raise ValueError(f"a grouping search returns at most top_k * group_size <= HR_MAX_TOPK = {HR_MAX_TOPK} rows, "
                                 f"got {top_k} * {group_size}")
        if group_by_field is not None:
            if not isinstance(group_by_field, str):
                raise ValueError(f"unknown group_by_field: {group_by_field!r}")
            check_group_field(group_by_field)
            if self._synthetic_rows:
                from .device_groups import check_synthetic_group_field
                check_synthetic_group_field(group_by_field)

    def _global_device_mask(self, expr: Optional[str]):
        """Packed mask over GLOBAL rows of `expr` + tombstones as a CUDA tensor (None = all rows), evaluated on the
        device and kept per (expression, rows, tombstone epoch)."""
        n = self.num_rows
        dead = self._deleted is not None and bool(self._deleted[:n].any())
        if not expr and not dead:
            return None
        key = ("global", expr, n, self._delete_epoch)
        with self._mask_lock:   # searches of one request run in different threads and ask for the same new mask at once
            hit = self._dev_masks.get(key)
            if hit is None:
                if len(self._dev_masks) >= 32:
                    self._dev_masks.pop(next(iter(self._dev_masks)))
                hit = self._dev_masks[key] = self._filters_on_device().evaluate(expr, n, self._deleted if dead else None)[0]
        return hit

    def _row_mask(self, expr: Optional[str]) -> Optional[np.ndarray]:
        """Boolean filter over global rows for a filter expression plus the tombstones, or None for "all rows" — the
        host-side view of the mask (sharded / collective searches cut it up per shard).  With a GPU shard the
        predicate is evaluated on the device and read back once; without one (CPU-only tests) filters.evaluate runs on
        the host columns.  Kept per (expression, row count, tombstone epoch)."""
        n = self.num_rows
        if self._synthetic_rows and not expr and not (self._deleted is not None and self._deleted[:n].any()):
            return None
        key = (expr, n, self._delete_epoch)
        if key in self._mask_cache:
            return self._mask_cache[key]
        keep = None
        if self._filters_on_device() is not None:
            m = self._global_device_mask(expr)
            if m is not None:
                keep = np.unpackbits(m.cpu().numpy(), bitorder="little")[:n].astype(bool)
        else:
            if expr:
                keep = self._host_predicate(expr, n)
            if self._deleted is not None and self._deleted[:n].any():
                alive = np.ones(n, dtype=bool)
                alive[:self._deleted.shape[0]] = ~self._deleted[:n]
                keep = alive if keep is None else (keep & alive)
        if len(self._mask_cache) >= 64:
            self._mask_cache.pop(next(iter(self._mask_cache)))
        self._mask_cache[key] = keep
        return keep

    def _host_predicate(self, expr: str, n: int) -> np.ndarray:
        """filters.evaluate over the host columns (collections without a device: CPU tests, oracle-backed shards)."""
        if self._synthetic_rows:
            # bulk-ingested rows carry no payload columns; what their synthetic id encodes can still be filtered on:
            # chunk_index = row % 10 (synthetic_id), derived on the fly
            fields = _filters.fields(expr)
            if fields - {"chunk_index"}:
                raise ValueError("this shard was bulk-ingested without payload columns: only chunk_index (= row % 10) "
                                 f"can be filtered on, not {sorted(fields - {'chunk_index'})}")
            return _filters.evaluate(expr, {"chunk_index": np.arange(n, dtype=np.int64) % 10}, n)
        columns = self._columns()
        if "content" in _filters.fields(expr):    # TEXT_MATCH: the one leaf that reads a text field, any sequence of str
            columns = dict(columns, content=self._cols["content"])
        return _filters.evaluate(expr, columns, n)

    def _tombstone(self, expr: str):
        n = self.num_rows
        dev = self._filters_on_device()
        if dev is not None:
            hit = np.unpackbits(dev.evaluate(expr, n)[0].cpu().numpy(), bitorder="little")[:n].astype(bool)
        else:
            hit = self._host_predicate(expr, n)
        if self._deleted is None or self._deleted.shape[0] < n:
            grown = np.zeros(n, dtype=bool)
            if self._deleted is not None:
                grown[:self._deleted.shape[0]] = self._deleted
            self._deleted = grown
        self._deleted[:n] |= hit
        self._delete_epoch += 1

    # ------------------------------------------------------------------ compaction
    def compact(self) -> Dict[str, int]:
        """Remove every tombstoned row (delete_by_filter / Collection.delete) from the shards, the domain shards and the
        payload columns for good, and give the HBM back: hr_compact per shard (include/hbmrag.h).  The scans stop streaming
        the dead rows, num_entities counts the survivors, and the survivors are renumbered in order — a hit's "_row"
        changes, its "id" and everything else does not.

        A maintenance call like load_snapshot: it REPLACES the row space, nothing calls it by itself, and the caller
        issues no search while it runs.  It is out of place: until it returns, a shard's old and new store are in HBM
        together.  A collection whose payload is derived from the row number (add_rows_synthetic) cannot be compacted:
        its ids would change.  -> rows_before, rows_after, device_bytes_before, device_bytes_after."""
        if self._synthetic_rows:
            raise ValueError("a synthetic-payload collection cannot be compacted: its ids are a function of the row number")
        sets = [s for s in (self._main, self._domain) if s is not None]
        n = self.num_rows
        bytes_before = sum(int(getattr(s, "device_bytes", 0)) for s in sets)
        out = {"rows_before": n, "rows_after": n, "device_bytes_before": bytes_before, "device_bytes_after": bytes_before}
        if self._deleted is None or not self._deleted[:n].any():
            return out
        for s in sets:      # refuse before anything is touched
            if not hasattr(s, "handles"):
                s.compact(None)          # the torchrun form: NotImplementedError
        # the front's engines and buffers are sized for the old shard: the next search builds a new one
        if self._front is not None:
            self._front.close()
            self._front = None
        keep = np.ones(n, dtype=bool)
        keep[: self._deleted.shape[0]] = ~self._deleted[:n]
        d_keep = 0
        if self._device_shard(self._main) is not None:      # (every set left here has `handles`: the loop above)
            d_mask = self._global_device_mask(None)      # alive rows, packed, already in HBM
            d_keep = d_mask.data_ptr() if d_mask is not None else 0
        # the same mask over the rows each set has: row r of one stays row r of the other
        for s in sets:
            s.compact(keep, d_keep if s.device == self._main.device else 0)
        self._cols.compact(keep)     # only after every shard set succeeded
        self._deleted = None
        self._delete_epoch += 1
        self._forget_masks(rebuild_filters=True)
        self._new_row_space("compact()")
        out["rows_after"] = self.num_rows
        out["device_bytes_after"] = sum(int(getattr(s, "device_bytes", 0)) for s in sets)
        return out

    # ------------------------------------------------------------------ ingest
    async def index_chunks(self, chunks: List["Chunk"], domain: Optional[str] = None) -> Dict[str, Any]:
        """Embed and append chunks to every collection (reference indexing.py:264-437);
        same summary keys, same best-effort handling of sparse/domain failures.

        When the embedding generator offers `encode_to_device` (encoders.SentenceEncoder) the dense rows never leave
        the GPU: the encoder's output tensor is cast to the shard's storage type on the device and re-tiled into the
        shard by hr_add_dense_raw_dev on the encoder's stream; the host semantic cache is not
        consulted or filled on that path (it holds host arrays).  Sparse payloads of all chunks of a call travel as ONE
        CSR, and every collection is flushed once per call.  `timing_ms` in the summary is an addition to the
        reference's keys: encoder / append / flush wall time of this call."""
        import time as _time
        summary = {"total_chunks": len(chunks), "indexed_semantic": 0, "indexed_sparse": 0, "indexed_domain": 0,
                   "errors": []}
        timing = {"encode": 0.0, "append": 0.0, "flush": 0.0}
        use_sparse = "sparse_index" in self.collections and self._sparse_enabled()
        gen = self.embedding_generator
        on_device = gen is not None and hasattr(gen, "encode_to_device") and self._main is not None and \
            hasattr(self._main, "handles")
        t0 = _time.perf_counter()
        texts = [c.text for c in chunks]
        dense_dev = dom_dev = None
        if on_device and chunks:
            dense_dev = await self._run_encoder(gen.encode_to_device, texts)
            if dense_dev.dim() != 2 or dense_dev.shape[1] != self.semantic_dim:
                raise ValueError(f"semantic embedding has dim {tuple(dense_dev.shape)[1:]}, expected {self.semantic_dim}")
            if "domain_index" in self.collections and hasattr(gen, "encode_domain_to_device"):
                dom_dev = await self._run_encoder(gen.encode_domain_to_device, texts, domain)
                if dom_dev.shape[1] != self.domain_dim:
                    raise ValueError(f"domain embedding has dim {dom_dev.shape[1]}, expected {self.domain_dim}")
            dense_vecs = None
        else:
            dense_vecs = await self._generate_semantic_embeddings_batch(texts)
        # sparse payloads of the whole call from ONE hook call when the generator offers the batch form (SentenceEncoder:
        # hr_bm25_encode_dev on its GPU; the reference calls encode_sparse once per chunk, indexing.py:379-404); a batch the
        # hook or the checks below refuse goes chunk by chunk, where a bad payload costs only its own row
        sparse_batch = None
        if use_sparse and chunks and gen is not None and hasattr(gen, "encode_sparse_csr"):
            try:
                sparse_batch = self._checked_sparse_csr(await self._run_encoder(gen.encode_sparse_csr, texts), len(chunks))
            except Exception as e:
                logger.warning("batched sparse payloads failed (%s); encoding chunk by chunk", e)
        # token vectors of the whole call from ONE hook call; a failure costs the vectors (T_r = 0), never the rows
        token_batch = None
        if self.token_dim is not None and chunks and gen is not None and hasattr(gen, "encode_token_vectors"):
            try:
                token_batch = self._checked_token_vectors(await self._run_encoder(gen.encode_token_vectors, texts), len(chunks))
            except Exception as e:
                summary["errors"].append({"token_vectors_error": str(e)})
        rows_dense, rows_domain, sp_ptr, sp_idx, sp_val, kept, kept_idx = [], [], [0], [], [], [], []
        n_sparse_ok = 0
        for i, chunk in enumerate(chunks):
            try:
                dense = None
                if dense_vecs is not None:
                    dense = np.asarray(dense_vecs[i], dtype=np.float32).reshape(-1)
                    if dense.shape[0] != self.semantic_dim:
                        raise ValueError(f"semantic embedding has dim {dense.shape[0]}, expected {self.semantic_dim}")
                sp = None
                if sparse_batch is not None:
                    bp, bi, bv = sparse_batch
                    sp = (bi[bp[i]:bp[i + 1]], bv[bp[i]:bp[i + 1]])
                    n_sparse_ok += 1
                elif use_sparse:
                    try:
                        sp = self._clean_sparse_payload(await self._generate_sparse_embedding(chunk.text, role="document"))
                        n_sparse_ok += 1
                    except Exception as e:
                        summary["errors"].append({"chunk_id": chunk.metadata.chunk_id,
                                                  "error": f"sparse_embedding_failed: {e}"})
                dom = None
                if "domain_index" in self.collections and dom_dev is None:
                    dom = np.asarray(await self._generate_domain_embedding(chunk.text, domain),
                                     dtype=np.float32).reshape(-1)
                    if dom.shape[0] != self.domain_dim:
                        raise ValueError(f"domain embedding has dim {dom.shape[0]}, expected {self.domain_dim}")
            except Exception as e:
                summary["errors"].append({"chunk_id": chunk.metadata.chunk_id, "error": str(e)})
                continue
            if dense is not None:
                rows_dense.append(dense)
            if dom is not None:
                rows_domain.append(dom)
            if use_sparse:  # a row per chunk keeps row numbers aligned across collections
                si, sv = sp if sp is not None else (np.zeros(0, np.int32), np.zeros(0, np.float32))
                sp_idx.append(si)
                sp_val.append(sv)
                sp_ptr.append(sp_ptr[-1] + len(si))
            kept.append(chunk)
            kept_idx.append(i)
        timing["encode"] = (_time.perf_counter() - t0) * 1e3
        summary["timing_ms"] = timing
        if not kept:
            return summary

        def device_rows(t):
            """The kept rows of an encoder output, in the shard's storage type, still on the device."""
            import torch
            if len(kept_idx) != t.shape[0]:
                t = t.index_select(0, torch.as_tensor(kept_idx, device=t.device))
            return t.to(torch.float16 if self._store_half else torch.float32).contiguous()

        try:
            if "semantic_index" not in self.collections:
                raise KeyError("semantic_index")
            sparse_csr = None
            if use_sparse:
                sparse_csr = (np.asarray(sp_ptr, np.int64), np.concatenate(sp_idx) if sp_idx else np.zeros(0, np.int32),
                              np.concatenate(sp_val) if sp_val else np.zeros(0, np.float32))
            t1 = _time.perf_counter()
            # dense rows, sparse rows and payload columns of a chunk share one row number: the three are appended
            # together, and whatever fails afterwards is padded rather than left short
            dense_rows = device_rows(dense_dev) if dense_dev is not None else np.stack(rows_dense)
            self._check_dense_rows(dense_rows, self._main)    # refused whole, before anything is appended
            base_row = self.num_rows
            try:
                _, _, sparse_err = await asyncio.to_thread(self._main.add, dense_rows, sparse_csr)
            except PartialAppend as pa:
                # some shards took their piece before another refused: the payload of exactly those rows goes in, so
                # that later batches keep the row numbers the shards gave them
                self._append_payload(kept[: pa.end - pa.base])
                summary["indexed_semantic"] = pa.end - pa.base
                raise pa.cause
            self._append_payload(kept)
            if token_batch is not None:
                col = TokenVectorColumn(self.token_dim)
                col.extend(*token_batch)
                self._cols.extend_token_vectors(base_row, *col.gather(kept_idx))
            summary["indexed_semantic"] = len(kept)
            if use_sparse:
                if sparse_err is None:
                    summary["indexed_sparse"] = n_sparse_ok
                else:
                    logger.warning("Sparse insert failed; continuing without sparse index: %s", sparse_err)
                    summary["errors"].append({"insert_sparse_error": str(sparse_err)})
            if "domain_index" in self.collections:
                before = self._domain.num_rows
                try:
                    dom_rows = device_rows(dom_dev) if dom_dev is not None else np.stack(rows_domain)
                    self._check_dense_rows(dom_rows, self._domain)
                    await asyncio.to_thread(self._domain.add, dom_rows)
                    summary["indexed_domain"] = len(kept)
                except Exception as e:  # zero rows never match (cosine 0): the domain collection stays row-aligned
                    missing = len(kept) - (self._domain.num_rows - before)   # pad only what did not go in
                    if missing > 0:
                        await asyncio.to_thread(self._domain.add, np.zeros((missing, self.domain_dim), np.float32))
                    summary["errors"].append({"insert_domain_error": str(e)})
            timing["append"] = (_time.perf_counter() - t1) * 1e3
            t2 = _time.perf_counter()
            for coll in {id(c.handle): c for c in self.collections.values()}.values():
                await asyncio.to_thread(coll.flush)
            timing["flush"] = (_time.perf_counter() - t2) * 1e3
        except Exception as e:
            summary["errors"].append({"insert_error": str(e)})
        return summary

    def _append_payload(self, chunks):
        c = self._cols
        metas = [ch.metadata for ch in chunks]
        c["id"].extend(m.chunk_id for m in metas)
        c["doc_id"].extend(str(m.doc_id) for m in metas)
        c["content"].extend(ch.text[:65535] for ch in chunks)
        c["chunk_index"].extend([int(m.chunk_index) for m in metas])
        c["token_count"].extend([int(m.token_count) for m in metas])
        for name in FLOAT_COLUMNS:   # FLOAT fields hold float32 (reference schema, indexing.py:200-202)
            c[name].extend([getattr(m, name) for m in metas])
        c["timestamp"].extend(str(m.timestamp) for m in metas)
        c["metadata_json"].extend(str(m.to_dict())[:10000] for m in metas)
        self._forget_masks(rebuild_filters=False)

    def _add_to_main(self, dense, sparse_csr):
        """Append a bulk batch to the main shard set -> (rows the shards numbered, what stopped the append or None, the sparse
        collection's error or None).  Rows numbered before a shard refused (PartialAppend) still need their payload: the caller adds it."""
        self._check_dense_rows(dense, self._main)
        try:
            _, _, sparse_err = self._main.add(dense, sparse_csr if "sparse_index" in self.collections else None)
        except PartialAppend as pa:
            return pa.end - pa.base, pa.cause, None
        return dense.shape[0], None, sparse_err

    def add_rows(self, dense: np.ndarray, sparse_csr=None, ids: Optional[Sequence[str]] = None,
                 contents: Optional[Sequence[str]] = None, token_vectors=None, **scalar_columns):
        """Bulk ingest of pre-computed vectors (benchmarks, snapshots): dense [n, dim]
        float16/float32, optional CSR triple (indptr, indices, values).  token_vectors=(indptr, values): the rows' token
        vectors for the late-interaction rerank (a manager with token_dim), values [indptr[-1], token_dim] rounded to fp16
        by numpy's astype; refused whole, before any shard is touched, when the CSR is malformed or not finite as fp16."""
        if self._synthetic_rows:
            raise ValueError("shard is in synthetic-payload mode; use add_rows_synthetic")
        if token_vectors is not None:
            token_vectors = self._checked_token_vectors(token_vectors, len(dense))
        base = self.num_rows
        n, failed, sparse_err = self._add_to_main(dense, sparse_csr)
        if token_vectors is not None and n:
            self._cols.extend_token_vectors(base, token_vectors[0][: n + 1], token_vectors[1][: int(token_vectors[0][n])])
        c = self._cols
        defaults = {"doc_id": lambda r: f"doc{r // 10}", "chunk_index": lambda r: r % 10, "token_count": lambda r: 0,
                    "entropy": lambda r: 0.0, "redundancy": lambda r: 0.0, "domain_density": lambda r: 0.0,
                    "timestamp": lambda r: "", "metadata_json": lambda r: ""}
        step = 1 << 18   # bounded temporaries: the columns hold bytes and numbers, not Python objects
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            c["id"].extend(ids[lo:hi] if ids is not None else (self.synthetic_id(base + r) for r in range(lo, hi)))
            c["content"].extend(contents[lo:hi] if contents is not None else ("" for _ in range(lo, hi)))
            for name, fn in defaults.items():
                given = scalar_columns.get(name)
                c[name].extend(given[lo:hi] if given is not None else [fn(base + r) for r in range(lo, hi)])
        self._forget_masks(rebuild_filters=False)
        if failed is not None:
            raise failed
        if sparse_err is not None:  # the rows are in (with empty sparse rows); the caller still hears about it
            raise sparse_err

    def _checked_token_vectors(self, token_vectors, n_rows: int):
        """(indptr int64 [n_rows + 1], values fp16 [indptr[-1], token_dim]) of a batch, or ValueError: a manager without
        token_dim, an indptr that is not non-decreasing from 0 or names another row count, values of another shape or
        not finite as stored in fp16."""
        if self.token_dim is None:
            raise ValueError("token vectors need a manager created with token_dim=...")
        try:
            indptr, values = token_vectors
        except (TypeError, ValueError):
            raise ValueError("token_vectors must be a pair (indptr, values)") from None
        indptr = np.asarray(indptr)
        if indptr.ndim != 1 or indptr.dtype.kind not in "iu" or indptr.shape[0] != n_rows + 1:
            raise ValueError(f"token_vectors indptr must hold {n_rows + 1} integers (one row per appended row), got shape {indptr.shape}")
        indptr = indptr.astype(np.int64)
        if indptr[0] != 0 or (np.diff(indptr) < 0).any():
            raise ValueError("token_vectors indptr must be non-decreasing from 0")
        values = as_fp16_tokens("token_vectors values", values, self.token_dim)
        if values.shape[0] != int(indptr[-1]):
            raise ValueError(f"token_vectors values hold {values.shape[0]} vectors, indptr names {int(indptr[-1])}")
        return indptr, values

    def save_token_vectors(self, path: str) -> None:
        """Write the token vectors of every row to ONE .npz (indptr, values, token_dim): they are no part of a snapshot,
        whose layout is pinned."""
        col = self._token_vector_column()
        with open(path, "wb") as f:
            np.savez(f, indptr=col.indptr(), values=col.values(), token_dim=np.int64(col.dim))

    def load_token_vectors(self, path: str) -> None:
        """Replace the token vectors of every row by the ones save_token_vectors wrote.  ValueError when the file's row
        count or dim is not this manager's."""
        cur = self._token_vector_column()
        with np.load(path, allow_pickle=False) as z:
            indptr, values, dim = z["indptr"].astype(np.int64), z["values"], int(z["token_dim"])
        if dim != self.token_dim:
            raise ValueError(f"the file holds token vectors of dim {dim}, this manager was created with token_dim={self.token_dim}")
        if indptr.shape[0] - 1 != len(cur):
            raise ValueError(f"the file holds token vectors of {indptr.shape[0] - 1} rows, the collection holds {len(cur)}")
        indptr, values = self._checked_token_vectors((indptr, values), len(cur))
        self._cols.enable_token_vectors(self.token_dim, reset=True)
        self._cols.extend_token_vectors(0, indptr, values)
        with self._mask_lock:
            self._dev_tokvec = None

    def _token_vector_column(self):
        """The host token-vector column covering every row, or ValueError for a manager without token_dim."""
        if self.token_dim is None:
            raise ValueError("token vectors need a manager created with token_dim=...")
        if self._synthetic_rows:
            raise ValueError("a synthetic-payload collection keeps no token vectors")
        return self._cols.token_vectors()

    def add_rows_synthetic(self, dense: np.ndarray, sparse_csr=None):
        """Bulk ingest without host payload columns: ids/metadata are derived from the row
        number on demand (10M-row benchmarks would otherwise hold GBs of Python strings)."""
        if len(self._cols["id"]):
            raise ValueError("shard already holds payload columns")
        n, failed, sparse_err = self._add_to_main(dense, sparse_csr)
        self._synthetic_rows += n
        self._forget_masks(rebuild_filters=True)
        if failed is not None:
            raise failed
        if sparse_err is not None:
            raise sparse_err

    def finalize(self):
        for coll in {id(c.handle): c for c in self.collections.values()}.values():
            coll.flush()

    # ------------------------------------------------------------------ snapshot
    def save_snapshot(self, directory: str) -> None:
        """Write the shard(s) and the host payload columns to `directory` (resume without re-embedding)."""
        os.makedirs(directory, exist_ok=True)
        self.finalize()
        self._main.save(lambda s: os.path.join(directory, f"main.{s}.hbmrag"))
        if self._domain is not None:
            self._domain.save(lambda s: os.path.join(directory, f"domain.{s}.hbmrag"))
        cols = {k: (v.as_str_array() if hasattr(v, "as_str_array") else v.array()) for k, v in self._cols.items()}
        deleted = self._deleted if self._deleted is not None else np.zeros(0, dtype=bool)
        maps = {f"rows_main_{s}": r for s, r in enumerate(self._main.row_maps())}
        if self._domain is not None:
            maps.update({f"rows_domain_{s}": r for s, r in enumerate(self._domain.row_maps())})
        np.savez(os.path.join(directory, "payload.npz"), synthetic_rows=np.int64(self._synthetic_rows), deleted=deleted,
                 n_shards=np.int64(self._main.n_shards), **maps, **{f"col_{k}": v for k, v in cols.items()})

    def load_snapshot(self, directory: str) -> None:
        """Replace this manager's (empty) collections with the ones saved by `save_snapshot`; the manager must have
        been created with as many devices as the snapshot has shards."""
        sparse_on = "sparse_index" in self.collections     # what this manager was created with, not the environment of today
        path = lambda kind, s: os.path.join(directory, f"{kind}.{s}.hbmrag")
        with np.load(os.path.join(directory, "payload.npz"), allow_pickle=False) as z:
            n_shards = int(z["n_shards"])
            if n_shards != len(self.devices):
                raise ValueError(f"snapshot has {n_shards} shards, this manager was created with {len(self.devices)} devices")
            main = [self._shard_handle("main", d, path("main", s), sparse_on) for s, d in enumerate(self.devices)]
            self._main.adopt(main, [z[f"rows_main_{s}"] for s in range(n_shards)])
            if self._domain is not None and os.path.exists(path("domain", 0)):
                dom = [self._shard_handle("domain", d, path("domain", s)) for s, d in enumerate(self.devices)]
                self._domain.adopt(dom, [z[f"rows_domain_{s}"] for s in range(n_shards)])
            self._load_payload(z, with_columns=True)
        self._forget_masks(rebuild_filters=True)
        self._new_row_space("load_snapshot()")

    def _load_payload(self, z, with_columns: bool):
        """The host half of a snapshot (payload.npz): the synthetic-row count and, with_columns, the tombstones and the columns."""
        self._synthetic_rows = int(z["synthetic_rows"])
        if with_columns:
            self._deleted = z["deleted"].copy() if z["deleted"].size else None
            self._cols = PayloadColumns()
            if self.token_dim is not None:       # the token vectors are no part of a snapshot: load_token_vectors()
                self._cols.enable_token_vectors(self.token_dim)
            for k in self._cols:
                self._cols[k].extend(z[f"col_{k}"].tolist())

    def load_snapshot_rank(self, directory: str, process_group=True, device: Optional[int] = None) -> None:
        """Resume the torchrun form from a snapshot rank 0 wrote with save_snapshot(): EVERY rank calls this — it loads
        its own shard file main.<rank>.hbmrag and its row map, rank 0 also the payload columns — then ranks > 0 serve()."""
        import torch.distributed as dist
        if not hasattr(self, "_native"):
            self._connect()
        group = None if process_group is True else process_group
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        with np.load(os.path.join(directory, "payload.npz"), allow_pickle=False) as z:
            if int(z["n_shards"]) != world:
                raise ValueError(f"snapshot has {int(z['n_shards'])} shards, the process group has {world} ranks")
            rows = z[f"rows_main_{rank}"].astype(np.int64)
            h = self._shard_handle("main", self.devices[0] if device is None else device,
                                   os.path.join(directory, f"main.{rank}.hbmrag"))
            self._load_payload(z, with_columns=rank == 0)
        if self._main is not None:
            self._main.close()
        self.attach_shards([h], rows_of=[rows], synthetic_rows=self._synthetic_rows, process_group=process_group, local_ids=True)

    # ------------------------------------------------------------------ search
    @staticmethod
    def _as_sparse_payload(emb):
        if isinstance(emb, dict):
            idx = np.asarray(emb.get("indices", []), dtype=np.int32)
            val = np.asarray(emb.get("values", []), dtype=np.float32)
        elif hasattr(emb, "tocsr"):  # scipy sparse matrix (1, dim)
            m = emb.tocsr()
            idx, val = m.indices.astype(np.int32), m.data.astype(np.float32)
        else:
            raise ValueError("Sparse query embedding must be dict with indices/values or a scipy.sparse matrix")
        if idx.shape != val.shape:
            raise ValueError("sparse indices/values length mismatch")
        order = np.argsort(idx, kind="stable")
        return idx[order], val[order]

    def _check_dense_rows(self, rows, shard_set) -> None:
        """Refuse a dense batch before any shard, column or sparse collection is touched when some element, AS THE SHARD
        STORES IT, is NaN or infinite (an fp32 value of 65520 or more becomes an infinity in an fp16 store): the library
        refuses such a batch too (hr_add_dense, HR_EINVAL), but by then a multi-shard or collective append may have
        given other pieces their row numbers.  numpy rows are checked on the host in bounded blocks, a CUDA tensor (an
        encoder's output, already cast to the store's type) on its device.  ValueError names the first bad row."""
        h = getattr(shard_set, "local", shard_set).handles[0]
        code = getattr(h, "dtype", None)
        half = code == 1 if isinstance(code, int) else self._store_half
        bad = None
        if hasattr(rows, "is_cuda"):
            import torch
            ok = torch.isfinite(rows.to(torch.float16) if half else rows)
            if not bool(ok.all()):
                bad = int((~ok).reshape(ok.shape[0], -1).any(dim=1).nonzero()[0])
        else:
            a = np.asarray(rows)
            if a.ndim != 2 or a.dtype not in (np.float16, np.float32):
                return                      # the shard's own shape / dtype errors
            step = max(1, (1 << 22) // max(1, a.shape[1]))
            for lo in range(0, a.shape[0], step):
                blk = np.ascontiguousarray(a[lo:lo + step])
                if blk.dtype == np.float16:
                    ok = (blk.view(np.uint16) & 0x7C00) != 0x7C00      # exponent all ones: NaN or infinity
                elif half:
                    ok = np.abs(blk) < np.float32(65520.0)             # false for NaN; 65520 is the tie that rounds to inf
                else:
                    ok = np.isfinite(blk)
                if not ok.all():
                    bad = lo + int(np.flatnonzero(~ok.all(axis=1))[0])
                    break
        if bad is not None:
            raise ValueError(f"dense row {bad} of the batch holds a value that is NaN or infinite in the shard's "
                             f"{'fp16' if half else 'fp32'} store")

    def _checked_sparse_csr(self, csr, n: int):
        """A batch hook's CSR as (indptr int64, indices int32, values float32) if it is what the shard accepts as it stands —
        n rows, indices inside [0, sparse_dim) and strictly ascending within a row, finite values, rows of at most 60 000
        entries — else None (the per-chunk path then cleans or rejects payload by payload)."""
        ptr, idx, val = (np.asarray(csr[0], dtype=np.int64), np.asarray(csr[1], dtype=np.int32), np.asarray(csr[2], dtype=np.float32))
        if ptr.shape != (n + 1,) or ptr[0] != 0 or ptr[-1] != idx.shape[0] or idx.shape != val.shape or (np.diff(ptr) < 0).any():
            return None
        if idx.size:
            if idx.min() < 0 or idx.max() >= self.sparse_dim or not np.isfinite(val).all() or np.diff(ptr).max() > 60000:
                return None
            asc = np.ones(idx.size, dtype=bool)
            asc[1:] = idx[1:] > idx[:-1]
            asc[ptr[:-1][ptr[:-1] < idx.size]] = True          # the first entry of a row has no predecessor in its row
            if not asc.all():
                return None
        return ptr, idx, val

    def _clean_sparse_payload(self, emb):
        """A DOCUMENT's sparse payload, made acceptable to the shard or rejected here, chunk by chunk — a whole batch
        must not fail later because of one row: indices in range, values finite and within the fp16 posting range,
        duplicate indices merged by summing (what scipy's CSR arithmetic does with the reference's payload)."""
        idx, val = self._as_sparse_payload(emb)
        if idx.size:
            if idx[0] < 0 or idx[-1] >= self.sparse_dim:
                raise ValueError(f"sparse index out of range [0, {self.sparse_dim})")
            if not np.isfinite(val).all():
                raise ValueError("non-finite sparse value")
            if (idx[1:] == idx[:-1]).any():
                uniq, start = np.unique(idx, return_index=True)
                val = np.add.reduceat(val.astype(np.float64), start).astype(np.float32)
                idx = uniq.astype(np.int32)
            if np.abs(val).max() > 60000.0:
                raise ValueError("sparse weight exceeds the fp16 posting range (|w| <= 60000)")
        return idx, val

    def _format_hits(self, ids: np.ndarray, scores: np.ndarray) -> List[Dict[str, Any]]:
        c = self._cols
        out = []
        for row, score in zip(ids.tolist(), scores.tolist()):
            if row < 0:
                break
            if self._synthetic_rows:
                out.append({"id": self.synthetic_id(row), "content": "", "score": float(score),
                            "metadata": {"doc_id": f"doc{row // 10}", "chunk_index": row % 10, "entropy": 0.0,
                                         "redundancy": 0.0, "domain_density": 0.0, "timestamp": ""},
                            "_row": row})
                continue
            out.append({"id": c["id"][row], "content": c["content"][row], "score": float(score),
                        "metadata": {"doc_id": c["doc_id"][row], "chunk_index": c["chunk_index"][row],
                                     "entropy": c["entropy"][row], "redundancy": c["redundancy"][row],
                                     "domain_density": c["domain_density"][row], "timestamp": c["timestamp"][row]},
                        "_row": row})
        return out

    def _search_params(self, coll, search_params: Optional[Dict]) -> Dict:
        # no search_params: the collection's own metric (Milvus refuses a metric_type that differs from the index's)
        params = search_params or ({"metric_type": "IP"} if coll.kind == "sparse"
                                   else {"metric_type": coll.metric, "params": {"ef": 64}})
        metric = params.get("metric_type", coll.metric)
        if metric != coll.metric:
            raise ValueError(f"metric_type {metric} does not match collection {coll.name} ({coll.metric})")
        return params

    def _range_request(self, coll, params: Dict, group_by_field: Optional[str]) -> Optional[Tuple[float, float]]:
        """The (radius, range_filter) of a request's search params, or None; refuses what range search is not built for."""
        bounds = range_bounds(params, coll.metric if coll.kind != "sparse" else "IP")
        if bounds is None:
            return None
        if coll.kind == "sparse":
            raise ValueError(f"range search (radius / range_filter) is not built for the sparse collection {coll.name}: "
                             "the sparse scan has no range clamp")
        if group_by_field is not None:
            raise ValueError("range search (radius / range_filter) cannot be combined with group_by_field")
        if hasattr(coll.handle, "round"):
            raise NotImplementedError("range search (radius / range_filter) is not built for the torchrun form "
                                      "(CollectiveShardSet)")
        return bounds

    def _search_lists_blocking(self, query, collection_name: str, top_k: int, filters: Optional[str], params: Dict,
                               group_by_field: Optional[str] = None, bounds: Optional[Tuple[float, float]] = None,
                               group_size: int = 1):
        """(row ids [k], scores [k]) of ONE query through the host forms (which escalate until the list is proven).  With
        group_by_field: the exact grouped ranking (device_groups.grouped_search), as many entries as there are groups, at
        most k — with group_size > 1 up to group_size entries per group, a group's entries adjacent.
        bounds = (radius, range_filter) of a range search on a dense collection: the range forms of the same paths."""
        coll = self.collections[collection_name]
        path = SearchPath(self, coll, query, float((params.get("params") or params).get("drop_ratio_search", 0.0)))
        if group_by_field is not None:
            from .device_groups import grouped_search
            window = self.group_window(int(top_k), int(group_size))
            return grouped_search(self, path, int(top_k), filters, group_by_field, int(group_size), window)
        k = top_k if bounds is None else int(top_k)    # (a range search has always taken int(top_k), a plain one top_k as given)
        mask = path.base(filters)
        if path.shard is not None and mask is None and not path.sparse and getattr(query, "is_cuda", False):
            ids, sc = self._search_dense_device(path.shard, query, k, bounds)
            return ids[0], sc[0]
        return path.search(mask, k, bounds)

    @staticmethod
    def _search_dense_device(handle, q_dev, top_k: int, bounds: Optional[Tuple[float, float]] = None):
        """Query already in HBM (device-resident embedding cache) and no row mask: device form, no upload, with `bounds`
        the range form; an unproven list (ties at the candidate cut, rows within the scan's error of a bound) is redone
        through the host form."""
        import torch
        q = dense_rows_device([q_dev], q_dev.device, handle.dim)
        ids, sc, flag = list_buffers(1, top_k, q.device)
        stream = torch.cuda.current_stream(q.device)
        out = (ids.data_ptr(), sc.data_ptr(), flag.data_ptr(), 0, stream.cuda_stream)
        if bounds is None:
            handle.search_dense_dev(q.data_ptr(), 1, top_k, *out)
        else:
            rb = torch.tensor(bounds, dtype=torch.float64, device=q.device)
            handle.search_dense_range_dev(q.data_ptr(), 1, top_k, rb.data_ptr(), rb.data_ptr() + 8, *out)
        stream.synchronize()
        if int(flag.item()) != 1:
            if bounds is None:
                return handle.search_dense(q.cpu().numpy(), top_k)
            return handle.search_dense_range(q.cpu().numpy(), top_k, bounds[0], bounds[1])
        return ids.cpu().numpy(), sc.cpu().numpy()

    @staticmethod
    def group_window(top_k: int, group_size: int = 1) -> int:
        """Rows of the ranking a grouping search reads at a time: K' = min(HR_MAX_TOPK, GROUP_WINDOW_FACTOR * top_k *
        group_size)."""
        if not 1 <= top_k <= HR_MAX_TOPK:
            raise ValueError(f"a grouping search takes 1 <= top_k <= HR_MAX_TOPK = {HR_MAX_TOPK}, got {top_k}")
        return min(HR_MAX_TOPK, GROUP_WINDOW_FACTOR * top_k * group_size)

    def _search_blocking(self, query_embedding, collection_name: str, top_k: int, filters: Optional[str],
                         search_params: Optional[Dict], group_by_field: Optional[str] = None,
                         group_size: int = 1) -> List[Dict[str, Any]]:
        return self._format_hits(*self._search_blocking_lists(query_embedding, collection_name, top_k, filters, search_params,
                                                              group_by_field, group_size))

    def _search_blocking_lists(self, query_embedding, collection_name: str, top_k: int, filters: Optional[str],
                               search_params: Optional[Dict], group_by_field: Optional[str] = None, group_size: int = 1):
        coll = self.collections[collection_name]
        params = self._search_params(coll, search_params)
        bounds = self._range_request(coll, params, group_by_field)
        query = self._as_sparse_payload(query_embedding) if coll.kind == "sparse" else query_embedding
        return self._search_lists_blocking(query, collection_name, top_k, filters, params, group_by_field, bounds, group_size)

    def _deep_request(self, coll, top_k, offset, search_params: Optional[Dict], group_by_field: Optional[str],
                      group_size: int) -> int:
        """W of a request that names an offset or a top_k beyond HR_MAX_TOPK; refuses what a deep window (W > HR_MAX_TOPK)
        is not built for.  Nothing is launched for a refused request."""
        window = deep_window(top_k, offset)
        if window <= HR_MAX_TOPK:
            return window
        if group_by_field is not None or group_size != 1:
            raise ValueError(f"a deep window (offset + top_k = {window} > HR_MAX_TOPK = {HR_MAX_TOPK}) cannot be combined "
                             "with group_by_field")
        if range_bounds(self._search_params(coll, search_params), coll.metric if coll.kind != "sparse" else "IP") is not None:
            raise ValueError(f"a deep window (offset + top_k = {window} > HR_MAX_TOPK = {HR_MAX_TOPK}) cannot be combined "
                             "with range search (radius / range_filter)")
        if hasattr(coll.handle, "round"):
            raise NotImplementedError("deep search (offset + top_k > HR_MAX_TOPK) is not built for the torchrun form "
                                      "(CollectiveShardSet)")
        return window

    def _deep_blocking(self, query_embedding, collection_name: str, top_k: int, offset: int, filters: Optional[str],
                       search_params: Optional[Dict]) -> List[Dict[str, Any]]:
        """Entries offset .. offset + top_k - 1 of ONE query's exact ranking through the deep forms (hr_search_*_deep): every
        row of the collection is refined, so the call costs a read of the whole shard.  Only the top_k hits are formatted."""
        coll = self.collections[collection_name]
        params = self._search_params(coll, search_params)
        drop = float((params.get("params") or params).get("drop_ratio_search", 0.0))
        query = self._as_sparse_payload(query_embedding) if coll.kind == "sparse" else query_embedding
        self._count("deep_searches")
        path = SearchPath(self, coll, query, drop)
        return self._format_hits(*path.search(path.base(filters), top_k, offset=offset))

    def _iterator_page_blocking(self, query, collection_name: str, k: int, after: Optional[Tuple[float, int]],
                                filters: Optional[str], bounds: Optional[Tuple[float, float]], drop: float) -> List[Dict[str, Any]]:
        """One page of a SearchIterator: the first k hits of ONE query's ranking strictly after `after` = (score, row) through
        the cursor forms (hr_search_*_deep_after), the row mask taken as _deep_blocking takes it.  Not through the front."""
        self._count("iterator_pages")
        path = SearchPath(self, self.collections[collection_name], query, drop)
        return self._format_hits(*path.after(path.base(filters), k, after, bounds))

    def search_iterator(self, query_embedding, collection_name: str, batch_size=1000, limit=None,
                        filters: Optional[str] = None, search_params: Optional[Dict] = None) -> SearchIterator:
        """pymilvus' search_iterator: the collection's ranking for one query, `batch_size` <= 16 384 hits a page, `limit` hits
        in all (None: to the end of the ranking, however deep).  `await it.next()` / `async for page in it` / it.close();
        search_params as search() takes them, radius / range_filter on the dense collections included ("every row with
        cosine > 0.6").  Every page is one full refine of the shard whatever its depth (SearchIterator).  ValueError at
        creation: batch_size or limit out of range, what search() refuses for the collection; NotImplementedError in the
        torchrun form.  Not built: grouping, ranker=, hybrid_search / retrieve()."""
        return SearchIterator(self, query_embedding, collection_name, batch_size, limit, filters, search_params)

    # ---- coalescing front (batching.py) -------------------------------------------------------------------------
    def _coalescer(self, coll):
        """The batching front, or None when this collection cannot use it (spread over several shard handles: those
        searches fan out per shard and merge on the host)."""
        if not self.coalesce:
            return None
        collective = hasattr(coll.handle, "round")          # torchrun form: rounds of one broadcast + one gather
        if not collective and (getattr(coll.handle, "n_shards", 1) != 1 or not hasattr(coll.handle, "handles")):
            return None
        if self._front is None:
            from .batching import SearchCoalescer
            self._front = SearchCoalescer(self)
        return self._front

    def _device_row_mask(self, expr: Optional[str], kind: str):
        """Packed row mask of a filter expression (+ tombstones) for a single-shard collection, as a uint8 CUDA tensor
        evaluated on the device (device_filters.py) and kept per (expression, rows, tombstone epoch): a batch of filtered
        searches uploads nothing.  None = all rows."""
        g = self._global_device_mask(expr)
        if g is None:
            return None
        n_local = self._main.first.num_sparse_rows if kind == "sparse" else self._main.first.num_rows
        if g.numel() * 8 < n_local:
            raise ValueError(f"row mask covers {g.numel() * 8} rows, the collection holds {n_local}")
        return g

    @staticmethod
    def _params_key(params: Dict) -> tuple:
        """What of a request's search params decides which requests may share a launch.  The two numbers of a range search
        are operands of the launch, not part of the key: one marker says "ranged", so that ranged requests with different
        bounds share a launch and never share one with unranged requests."""
        inner = params.get("params") or {}
        key = tuple(sorted((k, v) for k, v in inner.items() if isinstance(v, (int, float, str, bool)) and k not in RANGE_KEYS))
        if any(inner.get(k) is not None for k in RANGE_KEYS):
            key += (("ranged", True),)
        return key

    async def search(self, query_embedding, collection_name: str, top_k: int = 20, filters: Optional[str] = None,
                     search_params: Optional[Dict] = None, *, group_by_field: Optional[str] = None,
                     group_size: int = 1, strict_group_size: Optional[bool] = None, offset: int = 0,
                     ranker: Optional[Any] = None) -> List[Dict[str, Any]]:
        """Collection.search (reference indexing.py:503-525).  offset=o: hits o .. o + top_k - 1 of the ranking, with
        W = o + top_k <= QUERY_MAX_WINDOW (deep_window).  W <= HR_MAX_TOPK is the plain search at top_k = W with the first o
        hits cut; a deeper window takes the deep search (exact, a full read of the shard per query; not with
        group_by_field, range search or the torchrun form).  group_by_field=F (pymilvus' grouping search): the best row
        of each of the top_k best groups of field F, in ranking order — exact at any depth; fewer groups than top_k give a
        shorter list.  F is an integer or a string field of the schema (chunk_index, token_count, doc_id, id / chunk_id,
        timestamp).  group_size=g > 1 is served by a manager created with group_members=True: up to g rows of each of the
        top_k best groups as one flat list, groups in ranking order, a group's rows adjacent and in ranking order; top_k * g
        <= HR_MAX_TOPK.  The answer is exact (pymilvus' strict_group_size=True), so strict_group_size changes nothing.
        ranker=DecayRanker(...) (pymilvus' decay ranker): the first W = max(top_k, ranker.candidates or top_k) <= HR_MAX_TOPK
        hits of the plain ranking are re-scored as normalised score x decay(|field - origin|) and re-sorted (stable), the best
        top_k returned: "score" is the final score, "raw_score" the hit's own.  Not with group_by_field, offset or a deep
        window (ValueError); NotImplementedError in the torchrun form.
        ranker=MMRRanker(...) (vector MMR, what RAG stacks call max_marginal_relevance_search): the first W hits of the plain
        ranking are diversified on the cosine of their STORED embeddings (include/hbmrag.h, hr_mmr_select_vec_dev) and the
        best top_k returned in pick order: "score" stays the hit's own, "mmr_value" is the value it was picked with.  Dense
        collections only (ValueError on sparse_index); otherwise refused like the decay ranker.
        ranker=BoostRanker(...) | FunctionScore(...) (pymilvus' boost ranker and function score): the first W hits of the
        plain ranking are re-scored by the filter expressions their rows match (include/hbmrag.h, hr_boost_rerank_dev) and
        re-sorted (stable), the best top_k returned: "score" is the final score, "raw_score" the hit's own, "boosted_by" the
        indices of the functions that matched.  On every collection; refused like the decay ranker, and for whatever the
        filter language refuses in a function's filter.
        ranker=MaxSimRanker(query_tokens, candidates=None) (late interaction, ColBERT-style MaxSim; a manager created with
        token_dim): the first W hits of the plain ranking are re-scored by the rows' STORED token vectors (include/hbmrag.h,
        hr_maxsim_rerank_dev: S = sum over query tokens of the best stored token's similarity; a row without vectors scores
        0.0) and re-sorted (stable), the best top_k returned: "score" is S, "raw_score" the hit's own.  On every collection
        (the ranker reads row ids, not the first stage's vectors); refused like the decay ranker."""
        if isinstance(ranker, MMRRanker):
            return await self._search_mmr(query_embedding, collection_name, top_k, filters, search_params, ranker,
                                          group_by_field, group_size, strict_group_size, offset)
        if isinstance(ranker, (BoostRanker, FunctionScore)):
            return await self._search_boosted(query_embedding, collection_name, top_k, filters, search_params, ranker,
                                              group_by_field, group_size, strict_group_size, offset)
        if isinstance(ranker, MaxSimRanker):
            return await self._search_maxsim(query_embedding, collection_name, top_k, filters, search_params, ranker,
                                             group_by_field, group_size, strict_group_size, offset)
        if ranker is not None:
            return await self._search_decayed(query_embedding, collection_name, top_k, filters, search_params, ranker,
                                              group_by_field, group_size, strict_group_size, offset)
        if group_by_field is not None or group_size != 1 or strict_group_size is not None:
            self._check_group_request(group_by_field, group_size, top_k, strict_group_size)
        group_size = int(group_size)
        if collection_name not in self.collections:
            raise ValueError(f"Collection {collection_name} not found")
        coll = self.collections[collection_name]
        paged = isinstance(offset, (bool, np.bool_)) or not isinstance(offset, (int, np.integer)) or offset != 0
        if paged or (isinstance(top_k, (int, np.integer)) and top_k > HR_MAX_TOPK):
            window = self._deep_request(coll, top_k, offset, search_params, group_by_field, group_size)
            if window > HR_MAX_TOPK:
                try:
                    return await asyncio.wait_for(
                        asyncio.to_thread(self._deep_blocking, query_embedding, collection_name, int(top_k), int(offset), filters,
                                          search_params),
                        timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)
                except asyncio.TimeoutError:
                    logging.error("shard search timeout for collection %s", collection_name)
                    raise Exception(f"Search timeout for collection {collection_name}")
            if group_by_field is not None:
                raise ValueError("offset cannot be combined with group_by_field")
            # the plain search at depth W (through the batching front as any other), the first `offset` hits cut
            hits = await self.search(query_embedding, collection_name, window, filters, search_params)
            return hits[int(offset):]
        return self._format_hits(*await self._search_lists_async(query_embedding, collection_name, top_k, filters,
                                                                 search_params, group_by_field, group_size))

    async def _search_lists_async(self, query_embedding, collection_name: str, top_k, filters: Optional[str],
                                  search_params: Optional[Dict], group_by_field: Optional[str] = None, group_size: int = 1):
        """(row ids, scores) of a search at top_k <= HR_MAX_TOPK, before _format_hits: through the batching front as a
        raw-list request (an unproven list is redone through the blocking path there), else the blocking path in a thread."""
        coll = self.collections[collection_name]
        front = self._coalescer(coll)
        try:
            if front is not None:
                params = self._search_params(coll, search_params)
                bounds = self._range_request(coll, params, group_by_field)
                query = self._as_sparse_payload(query_embedding) if coll.kind == "sparse" else query_embedding
                if bounds is not None:
                    from .batching import RangedQuery
                    query = RangedQuery(query, bounds)
                fut = front.submit_async("sparse" if coll.kind == "sparse" else "dense",
                                         (collection_name, int(top_k), filters, self._params_key(params), group_by_field,
                                          group_size), query)
                return await asyncio.wait_for(fut, timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)
            return await asyncio.wait_for(
                asyncio.to_thread(self._search_blocking_lists, query_embedding, collection_name, top_k, filters,
                                  search_params, group_by_field, group_size),
                timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)
        except asyncio.TimeoutError:
            logging.error("shard search timeout for collection %s", collection_name)
            raise Exception(f"Search timeout for collection {collection_name}")

    async def hybrid_search(self, dense_embedding, sparse_embedding, top_k: int, filters: Optional[str],
                            weights: Sequence[float], rrf_k: int = 60, semantic_params: Optional[Dict] = None,
                            sparse_params: Optional[Dict] = None, mmr_lambda: Optional[float] = None,
                            fusion: str = "rrf", norms: Optional[Sequence[int]] = None,
                            decay: Optional[DecayRanker] = None, boost: Optional[Any] = None):
        """The semantic search (2 x top_k), the sparse search (2 x top_k) and their rank fusion for ONE request in ONE
        round of the batching front: what `search` + `search` + `fuse_rank_lists_async` return, cut to the fused top_k.

        -> [(hit dict as `search` formats it, with "score" = the score in the list the payload comes from (the semantic
        list if the row is in it, else the sparse one), float64 fused score, method bit mask)] in fused order, or None
        when this manager cannot answer that way (no front, sharded collection, a list the device form could not prove
        exact, bad parameters ...) — the caller then takes the general path, which also owns the error behaviour.

        With `mmr_lambda` the fused list is diversified before the cut (HybridRetriever._mmr_diversify over all of its up to
        4 x top_k entries, on the device): at most top_k entries in MMR order.  Only a manager created with
        mmr_on_device=True whose collection lies on one shard answers that; every other one declines.

        fusion="weighted": the two lists are fused by weighted score fusion (hr_post_args::fusion = 1) instead of RRF;
        norms = the HR_NORM_* codes of the semantic and the sparse list (None = "activation" by the collections' metrics).
        The torchrun form declines such a request; MMR and the rerank consume the fused scores as they do RRF's.

        decay=DecayRanker(...): the WHOLE fused list (4 x top_k entries, as for MMR) is reranked by hr_decay_rerank_dev behind
        the post kernel on the same stream — fused scores are not renormalised: identity, or min-max — and handed to MMR or
        the cut in decayed order.  The second element of a result is then the final score and the hit carries "fused_score".
        The torchrun form declines.

        boost=FunctionScore | BoostRanker: the same with hr_boost_rerank_dev, BEFORE the decay ranker when both are set;
        "fused_score" stays the fusion's."""
        if fusion not in ("rrf", "weighted"):
            raise ValueError(f"fusion must be 'rrf' or 'weighted', got {fusion!r}")
        if boost is not None:
            boost = FunctionScore.of(boost, "boost")
            self._check_boost_functions(boost)      # a filter the language refuses is refused here, not inside a shared launch
        if decay is not None:
            if not isinstance(decay, DecayRanker):
                raise ValueError(f"decay must be a DecayRanker or None, got {decay!r}")
            from .device_decay import check_decay_field
            check_decay_field(decay.field, bool(self._synthetic_rows))
        if mmr_lambda is not None and not self.mmr_on_device:
            return None
        sem, spa = self.collections.get("semantic_index"), self.collections.get("sparse_index")
        if sem is None or spa is None or sem.handle is not spa.handle or 2 * int(top_k) > HR_MAX_TOPK:
            return None
        front = self._coalescer(sem)
        if front is None or (front.collective and not getattr(self._main, "supports_hybrid_round", False)):
            return None        # (the torchrun form answers in one round when its shards allow it: shards.round_hybrid)
        if mmr_lambda is not None and front.collective:
            return None
        fuse_key = ()       # RRF: the request key is what it was
        if fusion == "weighted":
            if front.collective:
                return None    # shards.round_hybrid fuses by RRF: the general path serves a weighted request
            from .retrieval import norm_code
            codes = tuple(int(c) for c in norms) if norms is not None else (norm_code(sem.metric), norm_code("IP"))
            if len(codes) != 2 or any(not 0 <= c <= 4 for c in codes):
                raise ValueError(f"norms must be two HR_NORM_* codes (0..4), got {norms!r}")
            fuse_key = ("weighted",) + codes
        try:
            if range_bounds(self._search_params(sem, semantic_params), sem.metric) is not None:
                return None        # a range on the semantic list: the one-round path has no range form
            sp = self._search_params(spa, sparse_params)
            if range_bounds(sp, "IP") is not None:
                return None        # the general path refuses a range on sparse_index: it owns the error
            drop = float((sp.get("params") or sp).get("drop_ratio_search", 0.0))
            payload = self._as_sparse_payload(sparse_embedding)
        except Exception:
            return None
        if not len(payload[0]):
            return None
        w = list(weights) + [0.0] * (2 - len(weights))
        mmr = mmr_lambda is not None
        request = (dense_embedding, payload, float(w[0]), float(w[1]), float(mmr_lambda) if mmr else 0.0)
        if decay is not None:       # field and norm code in the key, the curve's operands per query
            if front.collective:
                return None
            decay_key = ("decay", decay.field, decay.norm_code("IP", fused=True))
            request += (decay.operands(),)
        if boost is not None:       # both modes, norm code and direction in the key (before the decay ranker's part), the functions per query
            if front.collective or self._device_shard(self._main) is None:
                return None
            fuse_key += ("boost",) + boost.launch_key("IP", fused=True)
            request += (boost.operands(),)
        if decay is not None:
            fuse_key += decay_key
        fut = front.submit_async("hybrid", (int(top_k), filters, drop, int(rrf_k), mmr) + fuse_key, request)
        try:
            # no timer of its own: the caller (HybridRetriever.retrieve) already bounds the whole request with
            # RetrievalConstants.TIMEOUT_SECONDS, and a wait_for here is a task + a timer handle per request on the event
            # loop that serves every in-flight retrieve()
            res = await fut
        except Exception:
            return None
        if res is None:
            return None
        rows, fused_scores, methods, orig = res[:4]
        hits = self._format_hits(rows, orig)
        if decay is not None or boost is not None:
            for hit, raw in zip(hits, res[4].tolist()):
                hit["fused_score"] = raw
        return list(zip(hits, fused_scores.tolist(), methods.tolist()))

    @staticmethod
    def _fuse_inputs(row_lists, id_lists, weights, rrf_k):
        row_to_id = {}
        for rows, ids in zip(row_lists, id_lists):
            for r, i in zip(rows, ids):
                row_to_id.setdefault(int(r), i)
        lists = tuple([np.asarray(r, dtype=np.int64) for r in row_lists] + [np.zeros(0, np.int64)] * (3 - len(row_lists)))
        w = list(weights) + [0.0] * (3 - len(weights))
        return row_to_id, lists, (float(w[0]), float(w[1]), float(w[2]), int(rrf_k))

    @staticmethod
    def _fuse_output(row_to_id, rows, scores, methods):
        return [(row_to_id[int(r)], float(s), [b for b in range(3) if (int(m) >> b) & 1])
                for r, s, m in zip(rows, scores, methods)]

    def _fuse_rows_blocking(self, lists, key):
        wa, wb, wc, rrf_k = key
        return self._main.first.fuse_rrf(lists[0], lists[1], lists[2], wa, wb, wc, rrf_k)

    def fuse_rank_lists(self, row_lists: Sequence[Sequence[int]], id_lists: Sequence[Sequence[Any]],
                        weights: Sequence[float], rrf_k: int = 60):
        """RRF on the device (csrc/fuse.h) over row numbers; returns
        [(id, float64 score, [list indices])] in fused order."""
        if self._main is None:
            raise RuntimeError("no shard handle")
        row_to_id, lists, key = self._fuse_inputs(row_lists, id_lists, weights, rrf_k)
        return self._fuse_output(row_to_id, *self._fuse_rows_blocking(lists, key))

    async def fuse_rank_lists_async(self, row_lists, id_lists, weights, rrf_k: int = 60):
        """The same fusion for a caller on the event loop: concurrent callers share one hr_fuse_rrf_dev launch."""
        if self._main is None:
            raise RuntimeError("no shard handle")
        row_to_id, lists, key = self._fuse_inputs(row_lists, id_lists, weights, rrf_k)
        front = self._coalescer(self.collections["semantic_index"]) if "semantic_index" in self.collections else None
        if front is None or front.collective or max(len(x) for x in lists) > 256:
            return self._fuse_output(row_to_id, *await asyncio.to_thread(self._fuse_rows_blocking, lists, key))
        rows, scores, methods = await asyncio.wait_for(front.submit_async("fuse", key, lists),
                                                       timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)
        return self._fuse_output(row_to_id, rows, scores, methods)

    # ---- weighted score fusion (Milvus' WeightedRanker; the contract is in include/hbmrag.h) -----------------------------
    @staticmethod
    def _score_fuse_inputs(row_lists, id_lists, score_lists, weights, norms):
        """-> (row -> id, (((rows int64, scores float32) x 3), (wa, wb, wc)), key = the three norm codes: requests with equal
        codes share a launch, the weights are per-query operands of it)."""
        row_to_id = {}
        for rows, ids in zip(row_lists, id_lists):
            for r, i in zip(rows, ids):
                row_to_id.setdefault(int(r), i)
        n = len(row_lists)
        if not (len(score_lists) == n and len(norms) >= n and n <= 3):
            raise ValueError("one score list and one norm code per list, up to three lists")
        lists = tuple([(np.asarray(r, dtype=np.int64), np.asarray(s, dtype=np.float32)) for r, s in zip(row_lists, score_lists)]
                      + [(np.zeros(0, np.int64), np.zeros(0, np.float32))] * (3 - n))
        if any(len(r) != len(s) for r, s in lists):
            raise ValueError("a list's rows and scores differ in length")
        w = list(weights) + [0.0] * (3 - len(weights))
        codes = [int(c) for c in norms] + [0] * (3 - len(norms))
        if any(not 0 <= c <= 4 for c in codes):
            raise ValueError(f"norm codes must be HR_NORM_* (0..4), got {codes}")
        return row_to_id, (lists, (float(w[0]), float(w[1]), float(w[2]))), tuple(codes)

    def _fuse_scores_blocking(self, payload, key):
        return self._main.first.fuse_scores(payload[0], key, payload[1])

    def fuse_score_lists(self, row_lists: Sequence[Sequence[int]], id_lists: Sequence[Sequence[Any]],
                         score_lists: Sequence[Sequence[float]], weights: Sequence[float], norms: Sequence[int]):
        """Weighted score fusion on the device (csrc/fuse.h) over row numbers and the lists' fp32 scores; norms = one
        HR_NORM_* code per list.  Returns [(id, float64 score, [list indices])] in fused order."""
        if self._main is None:
            raise RuntimeError("no shard handle")
        row_to_id, payload, key = self._score_fuse_inputs(row_lists, id_lists, score_lists, weights, norms)
        return self._fuse_output(row_to_id, *self._fuse_scores_blocking(payload, key))

    async def fuse_score_lists_async(self, row_lists, id_lists, score_lists, weights, norms):
        """The same fusion for a caller on the event loop: concurrent callers share one hr_fuse_scores_dev launch (a
        kind of its own in the batching front: never one launch with RRF requests)."""
        if self._main is None:
            raise RuntimeError("no shard handle")
        row_to_id, payload, key = self._score_fuse_inputs(row_lists, id_lists, score_lists, weights, norms)
        front = self._coalescer(self.collections["semantic_index"]) if "semantic_index" in self.collections else None
        if front is None or front.collective or max(len(x[0]) for x in payload[0]) > 256:
            return self._fuse_output(row_to_id, *await asyncio.to_thread(self._fuse_scores_blocking, payload, key))
        rows, scores, methods = await asyncio.wait_for(front.submit_async("fuse_scores", key, payload),
                                                       timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)
        return self._fuse_output(row_to_id, rows, scores, methods)

    # ---- multi-list fusion and multi_search (pymilvus' hybrid_search(reqs, rerank, limit); multi_search.py) -----------------
    def _fuse_lists_blocking(self, payload, key):
        """One fusion request alone (managers without a front, the front's one-by-one fallback): hr_fuse_lists_dev with
        B = 1 on the first shard's device, synchronised.  A CPU stand-in manager uses the two restatements.
        -> (rows int64, fp64 fused scores, list masks int32), at most key's top_k entries."""
        from .multi_search import fuse_lists_host, stage_fuse_lists
        first = getattr(self._main, "first", None)
        if first is None or not hasattr(first, "_h"):
            return fuse_lists_host(payload, key)
        import torch
        from . import _native as nat
        mode, n_lists, k_in, norms, rrf_k, top_k = key
        ids, sc, _ = stage_fuse_lists([payload], key)
        dev = torch.device("cuda", first.device)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            d_ids = torch.from_numpy(ids).to(dev)
            d_sc = torch.from_numpy(sc).to(dev) if sc is not None else None
            oi = torch.empty((1, top_k), dtype=torch.int64, device=dev)
            os_ = torch.empty((1, top_k), dtype=torch.float64, device=dev)
            om = torch.empty((1, top_k), dtype=torch.int32, device=dev)
            on = torch.empty((1,), dtype=torch.int32, device=dev)
            nat.fuse_lists_dev(d_ids.data_ptr(), d_sc.data_ptr() if d_sc is not None else 0, n_lists, k_in, 1, mode, rrf_k,
                               norms, payload[1], 0, top_k, oi.data_ptr(), os_.data_ptr(), om.data_ptr(), on.data_ptr(),
                               stream.cuda_stream)
            stream.synchronize()
            n = int(on.item())
            return oi[0, :n].cpu().numpy(), os_[0, :n].cpu().numpy(), om[0, :n].cpu().numpy()

    async def fuse_lists_async(self, row_lists, score_lists, weights, *, mode: str = "rrf", norms: Optional[Sequence[int]] = None,
                               rrf_k: int = 60, top_k: Optional[int] = None):
        """Fusion of up to 16 ranked lists of row numbers (score_lists: their fp32 scores, read for mode="weighted" with one
        HR_NORM_* code per list in `norms`) -> (rows int64, fp64 fused scores, list masks: bit l = list l) in fused order,
        at most top_k (default: all, up to 3 * HR_MAX_TOPK).  On one GPU shard through the batching front (kind "fuse_n"):
        concurrent callers with equal (mode, lists, padded length, norms, rrf_k, top_k) share one hr_fuse_lists_dev launch,
        their weights travel per query.  Other managers fuse one request at a time (_fuse_lists_blocking)."""
        from . import _native as nat
        from .multi_search import check_fuse_lists
        if mode not in ("rrf", "weighted"):
            raise ValueError(f"mode must be 'rrf' or 'weighted', got {mode!r}")
        payload, key = check_fuse_lists(row_lists, score_lists, weights, nat.HR_FUSE_WEIGHTED if mode == "weighted" else nat.HR_FUSE_RRF,
                                        norms, rrf_k, top_k)
        front = self._coalescer(self.collections["semantic_index"]) if "semantic_index" in self.collections else None
        if front is None or front.collective or self._device_shard(self._main) is None:
            return await asyncio.to_thread(self._fuse_lists_blocking, payload, key)
        return await asyncio.wait_for(front.submit_async("fuse_n", key, payload), timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)

    def _multi_request(self, requests, ranker, limit):
        """The refusals of multi_search, before anything is searched -> (requests, multi_search.FusionPlan)."""
        from .multi_search import check_ranker, check_requests
        reqs = check_requests(requests, self.collections)
        metrics = []
        for r in reqs:
            coll = self.collections[r.collection_name]
            if hasattr(coll.handle, "round"):
                raise NotImplementedError("multi_search is not built for the torchrun form (CollectiveShardSet)")
            self._range_request(coll, self._search_params(coll, r.search_params), None)   # metric mismatch, bad or unsupported range
            metrics.append("IP" if coll.kind == "sparse" else coll.metric)
        return reqs, check_ranker(ranker, len(reqs), metrics, limit)

    async def multi_search(self, requests, ranker, limit: int = 20) -> List[Dict[str, Any]]:
        """pymilvus' Collection.hybrid_search(reqs, rerank, limit): 1 .. 16 SearchRequests, each exactly the plain search() of
        its collection at top_k = request.limit with its own filter and params, fused by an RRFRanker or a WeightedRanker
        into one ranking of at most `limit` <= 3 * HR_MAX_TOPK rows.  The three collections share one row space, so requests
        may name any of them; the fusion key is the global row number.  The sub-searches go to the batching front as raw
        lists (same-key ones share one scan launch), the lists to hr_fuse_lists_dev (kind "fuse_n"), and only the fused rows
        are formatted.  A hit's "score" is the fused fp64 score, "original_score" its score in the first request that holds
        it, "requests" the ascending indices of the requests that hold it.  A failing sub-search fails the call."""
        reqs, plan = self._multi_request(requests, ranker, limit)
        self._count("multi_searches")
        lists = await asyncio.gather(*[self._search_lists_async(r.data, r.collection_name, r.limit, r.filters, r.search_params)
                                       for r in reqs])
        rows, scores, masks = await self.fuse_lists_async(
            [l[0] for l in lists], [l[1] for l in lists], plan.weights, mode="weighted" if plan.norms is not None else "rrf",
            norms=plan.norms, rrf_k=plan.rrf_k, top_k=plan.limit)
        from .multi_search import lists_of_mask
        hits = self._format_hits(rows, scores)
        for hit, m in zip(hits, masks.tolist()):
            held = lists_of_mask(m)
            ids, sc = lists[held[0]]
            hit["requests"] = held
            hit["original_score"] = float(sc[int(np.flatnonzero(np.asarray(ids) == hit["_row"])[0])])
        return hits

    # ---- decay ranker (pymilvus' decay ranker; the contract is in include/hbmrag.h, the restatement in decay.py) ---------
    def _decay_request(self, collection_name: str, top_k, ranker, group_by_field, group_size, strict_group_size, offset):
        """(collection, W, norm code) of a search with a ranker, or the refusal — before anything is searched."""
        if not isinstance(ranker, DecayRanker):
            raise ValueError(f"ranker must be a DecayRanker, an MMRRanker, a BoostRanker, a FunctionScore, a MaxSimRanker or None, got {ranker!r}")
        if collection_name not in self.collections:
            raise ValueError(f"Collection {collection_name} not found")
        coll = self.collections[collection_name]
        if group_by_field is not None or group_size != 1 or strict_group_size is not None:
            raise ValueError("ranker cannot be combined with group_by_field")
        if isinstance(offset, (bool, np.bool_)) or not isinstance(offset, (int, np.integer)) or offset != 0:
            raise ValueError(f"ranker cannot be combined with offset, got offset={offset!r}")
        if isinstance(top_k, (bool, np.bool_)) or not isinstance(top_k, (int, np.integer)) or top_k < 1:
            raise ValueError(f"top_k must be an integer >= 1, got {top_k!r}")
        window = ranker.window(top_k)
        if window > HR_MAX_TOPK:
            raise ValueError(f"ranker reranks the best max(top_k, candidates) = {window} rows: a deep window (> HR_MAX_TOPK = "
                             f"{HR_MAX_TOPK}) is not built")
        from .device_decay import check_decay_field
        check_decay_field(ranker.field, bool(self._synthetic_rows))
        if hasattr(coll.handle, "round"):
            raise NotImplementedError("the decay ranker is not built for the torchrun form (CollectiveShardSet)")
        return coll, window, ranker.norm_code("IP" if coll.kind == "sparse" else coll.metric)

    async def _search_decayed(self, query_embedding, collection_name, top_k, filters, search_params, ranker, group_by_field,
                              group_size, strict_group_size, offset) -> List[Dict[str, Any]]:
        coll, window, norm = self._decay_request(collection_name, top_k, ranker, group_by_field, group_size,
                                                 strict_group_size, offset)
        operands = ranker.operands()       # origin=None reads the clock here, once per request
        hits = await self.search(query_embedding, collection_name, window, filters, search_params)
        if not hits:
            return hits
        rows = np.asarray([h["_row"] for h in hits], dtype=np.int64)
        scores = np.asarray([h["score"] for h in hits], dtype=np.float32)      # fp32 list scores, widened by _format_hits
        pos, _, final = await self._decay_rows_async(rows, scores, ranker.field, operands, norm)
        out = []
        for p, f in zip(pos[:int(top_k)], final[:int(top_k)]):
            hit = hits[int(p)]
            hit["raw_score"], hit["score"] = hit["score"], float(f)
            out.append(hit)
        return out

    # ---- late interaction (MaxSim; the contract is in include/hbmrag.h, the restatement in maxsim.py) ---------------------
    def _check_query_tokens(self, query_tokens) -> np.ndarray:
        """fp16 [Tq, token_dim] of a query's token vectors, or ValueError: a manager without token_dim, tokens that are
        not 2-D, of another dim, with Tq outside 1..HR_MAX_QUERY_TOKENS or not finite as fp16."""
        if self.token_dim is None:
            raise ValueError("late interaction needs a manager created with token_dim=...")
        if self._synthetic_rows:
            raise ValueError("a synthetic-payload collection keeps no token vectors")
        from ._native import HR_MAX_QUERY_TOKENS
        tokens = as_fp16_tokens("query_tokens", query_tokens, self.token_dim)
        if not 1 <= tokens.shape[0] <= HR_MAX_QUERY_TOKENS:
            raise ValueError(f"query_tokens must hold 1..{HR_MAX_QUERY_TOKENS} token vectors, got {tokens.shape[0]}")
        return tokens

    def _maxsim_request(self, collection_name: str, top_k, ranker, group_by_field, group_size, strict_group_size, offset):
        """(collection, W, fp16 query tokens) of a search with a MaxSimRanker, or the refusal — before anything is searched."""
        tokens = self._check_query_tokens(ranker.query_tokens)
        if collection_name not in self.collections:
            raise ValueError(f"Collection {collection_name} not found")
        coll = self.collections[collection_name]
        if group_by_field is not None or group_size != 1 or strict_group_size is not None:
            raise ValueError("ranker cannot be combined with group_by_field")
        if isinstance(offset, (bool, np.bool_)) or not isinstance(offset, (int, np.integer)) or offset != 0:
            raise ValueError(f"ranker cannot be combined with offset, got offset={offset!r}")
        if isinstance(top_k, (bool, np.bool_)) or not isinstance(top_k, (int, np.integer)) or top_k < 1:
            raise ValueError(f"top_k must be an integer >= 1, got {top_k!r}")
        window = ranker.window(top_k)
        if window > HR_MAX_TOPK:
            raise ValueError(f"ranker reranks the best max(top_k, candidates) = {window} rows: a deep window (> HR_MAX_TOPK = "
                             f"{HR_MAX_TOPK}) is not built")
        if hasattr(coll.handle, "round"):
            raise NotImplementedError("the late-interaction rerank is not built for the torchrun form (CollectiveShardSet)")
        return coll, window, tokens

    async def _search_maxsim(self, query_embedding, collection_name, top_k, filters, search_params, ranker, group_by_field,
                             group_size, strict_group_size, offset) -> List[Dict[str, Any]]:
        _, window, tokens = self._maxsim_request(collection_name, top_k, ranker, group_by_field, group_size,
                                                 strict_group_size, offset)
        hits = await self.search(query_embedding, collection_name, window, filters, search_params)
        if not hits:
            return hits
        rows = np.asarray([h["_row"] for h in hits], dtype=np.int64)
        pos, _, final = await self._maxsim_rows_async(rows, tokens)
        out = []
        for p, f in zip(pos[:int(top_k)], final[:int(top_k)]):
            hit = hits[int(p)]
            hit["raw_score"], hit["score"] = hit["score"], float(f)
            out.append(hit)
        return out

    def _maxsim_rows_blocking(self, payload, key=None):
        """The numpy restatement over row numbers and the host column (sharded managers, stand-ins, the front's one-by-one
        fallback): payload = (rows int64, fp16 query tokens) -> (positions, rows, float64 scores), whole."""
        rows, tokens = payload
        self._count("maxsim_host_reranks")
        col = self._token_vector_column()
        pos, ids, final = maxsim_rerank_csr(np.asarray(rows).tolist(), tokens, col.indptr(), col.values(), 0, len(rows))
        return np.asarray(pos, dtype=np.int32), np.asarray(ids, dtype=np.int64), np.asarray(final, dtype=np.float64)

    async def _maxsim_rows_async(self, rows: np.ndarray, tokens: np.ndarray):
        """(positions, rows, scores) of ONE list in late-interaction order, whole.  On one GPU shard through the batching
        front (kind "maxsim": the padded list length and the token dim are the key, the tokens and their count travel per
        query, so concurrent requests with different token counts share one hr_maxsim_rerank_dev launch).  Everything else
        is reranked on the host by the restatement, with the same result, counted in stats["maxsim_host_reranks"]."""
        n, K = len(rows), HR_MAX_TOPK
        width = next(w for w in (K // 4, K, 3 * K, n) if n <= w)      # few distinct launch shapes
        key = ("semantic_index", width, int(self.token_dim))
        payload = (rows, tokens)
        front = self._coalescer(self.collections["semantic_index"]) if "semantic_index" in self.collections else None
        if front is None or front.collective or n > 3 * K or self._device_shard(self._main) is None:
            return await asyncio.to_thread(self._maxsim_rows_blocking, payload, key)
        return await asyncio.wait_for(front.submit_async("maxsim", key, payload),
                                      timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)

    def _maxsim_list_request(self, rows, query_tokens, top_k):
        tokens = self._check_query_tokens(query_tokens)
        rows = [(-1 if r is None else int(r)) for r in rows]          # a hit without a row number has no vectors: S = 0.0
        if isinstance(top_k, (bool, np.bool_)) or not isinstance(top_k, (int, np.integer)) or top_k < 1:
            raise ValueError(f"top_k must be an integer >= 1, got {top_k!r}")
        return np.asarray(rows, dtype=np.int64), tokens, int(top_k)

    def maxsim_rerank_lists(self, rows, query_tokens, top_k: int):
        """The late-interaction rerank over ONE fused list (row numbers, None for a hit without one), blocking, through the
        host restatement: -> (positions into the list, float64 scores S) of the best top_k in late-interaction order."""
        rows, tokens, k = self._maxsim_list_request(rows, query_tokens, top_k)
        if not len(rows):
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
        pos, _, final = self._maxsim_rows_blocking((rows, tokens))
        return pos[:k], final[:k]

    async def maxsim_rerank_lists_async(self, rows, query_tokens, top_k: int):
        """maxsim_rerank_lists for a caller on the event loop: on one GPU shard concurrent callers share one
        hr_maxsim_rerank_dev launch (kind "maxsim" of the batching front); sharded managers use the restatement."""
        rows, tokens, k = self._maxsim_list_request(rows, query_tokens, top_k)
        if not len(rows):
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
        pos, _, final = await self._maxsim_rows_async(rows, tokens)
        return pos[:k], final[:k]

    async def maxsim_search(self, query_tokens, top_k: int = 20, filters: Optional[str] = None, *,
                            offset: int = 0) -> List[Dict[str, Any]]:
        """MaxSim as the FIRST stage (Milvus 2.6: MAX_SIM as the metric of a search over an embedding list): the whole
        collection is ranked by the rows' stored token vectors, so a row the pooled embedding ranks 5 000th is found.
        The hits are the rows that pass `filters` and the tombstones AND hold at least one token vector, by score
        descending, then row ascending; "score" is the fp32 MaxSim score, (float)S of include/hbmrag.h (hr_maxsim_scan_dev);
        the dicts are those search() on semantic_index returns for the rows.  Entries offset .. offset + top_k - 1, with
        offset + top_k <= QUERY_MAX_WINDOW (deep_window); a shorter ranking gives a shorter list.  Two rows whose fp64 S
        differ by less than an fp32 ulp tie and are ordered by row: maxsim_rerank_lists on the hits gives the fp64 order
        of a window.  One GPU shard: hr_maxsim_scan_dev over the HBM mirror under the cached device mask, then
        hr_deep_topk_dev (stats["maxsim_searches"]); every call reads the tokens of every row that passes.  Sharded
        managers and stand-ins: the restatement (maxsim.maxsim_search_csr) over the host column and host mask
        (stats["maxsim_host_searches"]).  ValueError before anything runs: a manager without token_dim, bad tokens (the
        MaxSimRanker rule), the window rule, an expression the filter language refuses; NotImplementedError in the
        torchrun form."""
        tokens = self._check_query_tokens(query_tokens)
        deep_window(top_k, offset)
        if "semantic_index" not in self.collections:
            raise ValueError("Collection semantic_index not found")
        if hasattr(self.collections["semantic_index"].handle, "round"):
            raise NotImplementedError("the MaxSim search is not built for the torchrun form (CollectiveShardSet)")
        if filters:
            _filters.lower(filters)          # whatever the filter language refuses, before a mask is built
        try:
            return await asyncio.wait_for(asyncio.to_thread(self._maxsim_search_blocking, tokens, int(top_k), int(offset), filters),
                                          timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)
        except asyncio.TimeoutError:
            logging.error("shard search timeout for the MaxSim search")
            raise Exception("Search timeout for the MaxSim search")

    def _maxsim_search_blocking(self, tokens: np.ndarray, top_k: int, offset: int, filters: Optional[str]) -> List[Dict[str, Any]]:
        """ONE query's MaxSim ranking, entries offset .. offset + top_k - 1.  The score / row / scratch arrays (8 bytes per
        row + the selection's scratch) belong to the call."""
        shard = self._device_shard(self.collections["semantic_index"].handle)
        if shard is None:
            mask = self._row_mask(filters)
            self._count("maxsim_host_searches")
            col = self._token_vector_column()
            return self._format_hits(*maxsim_search_csr(tokens, col.indptr(), col.values(), mask, top_k, offset))
        import torch
        from . import _native as nat
        mask = self._device_row_mask(filters, "dense")
        self._count("maxsim_searches")
        n_rows = int(shard.num_rows)
        if n_rows == 0:
            return []
        indptr, val, tok_rows = self._token_vectors_on_device().tensors()
        dev = torch.device("cuda", int(shard.device))
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            d_q = torch.from_numpy(np.ascontiguousarray(tokens)).to(dev)
            d_qn = torch.tensor([tokens.shape[0]], dtype=torch.int32, device=dev)
            scores = torch.empty((1, n_rows), dtype=torch.float32, device=dev)
            rows = torch.empty((1, n_rows), dtype=torch.int32, device=dev)
            scratch = torch.empty(max(nat.deep_topk_scratch_bytes(n_rows, 1, top_k + offset) // 8, 1), dtype=torch.int64, device=dev)
            out_ids = torch.empty((1, top_k), dtype=torch.int64, device=dev)
            out_sc = torch.empty((1, top_k), dtype=torch.float32, device=dev)
            nat.maxsim_scan_dev(d_q.data_ptr(), d_qn.data_ptr(), 1, int(tokens.shape[0]), int(self.token_dim),
                                indptr.data_ptr() if tok_rows else 0, val.data_ptr() if tok_rows else 0, tok_rows, n_rows,
                                mask.data_ptr() if mask is not None else 0, scores.data_ptr(), rows.data_ptr(), stream.cuda_stream)
            nat.deep_topk_dev(scores.data_ptr(), rows.data_ptr(), n_rows, 1, top_k, offset, False, int(getattr(shard, "row_offset", 0)),
                              out_ids.data_ptr(), out_sc.data_ptr(), scratch.data_ptr(), stream.cuda_stream)
            ids, sc = out_ids.cpu().numpy()[0], out_sc.cpu().numpy()[0]      # the copies wait for the stream
        return self._format_hits(ids, sc)

    # ---- boost ranker / function score (the contract is in include/hbmrag.h, the restatement in boost.py) ------------------
    def _check_boost_functions(self, spec: FunctionScore) -> None:
        """ValueError for what this collection cannot serve of a function score: a random_score field a payload-free
        collection cannot derive, and whatever the filter language refuses for a function's filter (its caps, TEXT_MATCH on
        a payload-free collection): the masks are evaluated here, into the caches the rerank reads."""
        for f in spec.functions:
            if f.field is not None and self._synthetic_rows:
                from .device_groups import check_synthetic_group_field
                check_synthetic_group_field(f.field)
        device = self._device_shard(self._main) is not None
        for f in spec.functions:
            if f.filter is not None:
                (self._global_device_mask if device else self._row_mask)(f.filter)

    def _boost_request(self, collection_name: str, top_k, ranker, group_by_field, group_size, strict_group_size, offset):
        """(collection, W, FunctionScore, launch key) of a search with a boost ranker, or the refusal — before anything is searched."""
        spec = FunctionScore.of(ranker)
        if collection_name not in self.collections:
            raise ValueError(f"Collection {collection_name} not found")
        coll = self.collections[collection_name]
        if group_by_field is not None or group_size != 1 or strict_group_size is not None:
            raise ValueError("ranker cannot be combined with group_by_field")
        if isinstance(offset, (bool, np.bool_)) or not isinstance(offset, (int, np.integer)) or offset != 0:
            raise ValueError(f"ranker cannot be combined with offset, got offset={offset!r}")
        if isinstance(top_k, (bool, np.bool_)) or not isinstance(top_k, (int, np.integer)) or top_k < 1:
            raise ValueError(f"top_k must be an integer >= 1, got {top_k!r}")
        window = spec.window(top_k)
        if window > HR_MAX_TOPK:
            raise ValueError(f"ranker reranks the best max(top_k, candidates) = {window} rows: a deep window (> HR_MAX_TOPK = "
                             f"{HR_MAX_TOPK}) is not built")
        if hasattr(coll.handle, "round"):
            raise NotImplementedError("the boost ranker is not built for the torchrun form (CollectiveShardSet)")
        self._check_boost_functions(spec)
        return coll, window, spec, spec.launch_key("IP" if coll.kind == "sparse" else coll.metric)

    async def _search_boosted(self, query_embedding, collection_name, top_k, filters, search_params, ranker, group_by_field,
                              group_size, strict_group_size, offset) -> List[Dict[str, Any]]:
        _, window, spec, modes = await asyncio.to_thread(self._boost_request, collection_name, top_k, ranker, group_by_field,
                                                         group_size, strict_group_size, offset)
        hits = await self.search(query_embedding, collection_name, window, filters, search_params)
        if not hits:
            return hits
        rows = np.asarray([h["_row"] for h in hits], dtype=np.int64)
        scores = np.asarray([h["score"] for h in hits], dtype=np.float32)      # fp32 list scores, widened by _format_hits
        pos, _, final, matched = await self._boost_rows_async(rows, scores, spec.operands(), modes)
        out = []
        for p, f, m in zip(pos[:int(top_k)], final[:int(top_k)], matched[:int(top_k)]):
            hit = hits[int(p)]
            hit["raw_score"], hit["score"], hit["boosted_by"] = hit["score"], float(f), matched_functions(int(m))
            out.append(hit)
        return out

    def _boost_rows_blocking(self, payload, key):
        """The host restatement over row numbers (sharded managers, stand-ins, the front's one-by-one fallback):
        payload = (rows int64, scores, functions), key = (function mode, boost mode, norm, direction, ...) -> (positions, rows,
        float64 final scores, matched bits).  A function's rows are _row_mask(filter): the host view of the mask the device
        form reads; its keys the host group keys."""
        rows, scores, functions = payload
        self._count("boost_host_reranks")
        n_rows = self.num_rows
        rows = np.asarray(rows, dtype=np.int64)
        inside = (rows >= 0) & (rows < n_rows)
        at = np.where(inside, rows, 0)
        matches, specs = [], []
        for expr, weight, seed, field in functions:
            keep = self._row_mask(expr) if expr is not None else None
            matches.append([True] * len(rows) if keep is None else (inside & keep[:n_rows][at] if n_rows else inside).tolist())
            if seed is None:
                specs.append(weight)
            else:
                keys = rows if field is None or not n_rows else np.where(inside, self._host_group_keys(field)[:n_rows][at], rows)
                specs.append((weight, seed, keys.tolist()))
        pos, ids, final, hit = boost_rerank(rows.tolist(), [float(x) for x in scores], matches, specs, int(key[0]), int(key[1]),
                                            int(key[2]), bool(key[3]), len(rows))
        return (np.asarray(pos, dtype=np.int32), np.asarray(ids, dtype=np.int64), np.asarray(final, dtype=np.float64),
                np.asarray(hit, dtype=np.int32))

    async def _boost_rows_async(self, rows: np.ndarray, scores: np.ndarray, functions, modes):
        """(positions, rows, final scores, matched bits) of ONE list in boosted order, whole.  On one GPU shard through the
        batching front: both modes, the norm code, the direction, the padded list length and the score type are the request
        key, the functions travel per query, so concurrent requests with different filters, weights and seeds share one
        hr_boost_rerank_dev launch.  Everything else is reranked on the host by the restatement, with the same result, and
        counted in stats["boost_host_reranks"]: a manager without a front (sharded, coalesce=False), a list longer than
        3 * HR_MAX_TOPK entries and, inside the front, the requests of a batch whose launch was refused."""
        n, K = len(rows), HR_MAX_TOPK
        width = next(w for w in (K // 4, K, 3 * K, n) if n <= w)      # few distinct launch shapes
        key = tuple(int(m) for m in modes) + (width, scores.dtype == np.float64)
        payload = (rows, scores, tuple(functions))
        front = self._coalescer(self.collections["semantic_index"]) if "semantic_index" in self.collections else None
        if front is None or front.collective or n > 3 * K or self._device_shard(self._main) is None:
            return await asyncio.to_thread(self._boost_rows_blocking, payload, key)
        return await asyncio.wait_for(front.submit_async("boost", key, payload),
                                      timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)

    def _boost_list_request(self, rows, scores, spec):
        spec = FunctionScore.of(spec, "boost")
        self._check_boost_functions(spec)           # a filter the language refuses is refused here, not inside a shared launch
        rows, scores = np.asarray(rows, dtype=np.int64), np.asarray(scores, dtype=np.float64)
        if rows.shape != scores.shape or rows.ndim != 1:
            raise ValueError("a list's rows and scores differ in length")
        return rows, scores, spec.operands(), spec.launch_key("IP", fused=True)

    def boost_rerank_lists(self, rows, scores, spec):
        """The boost ranker over ONE fused list (row numbers and float64 fused scores), blocking, through the host
        restatement: -> (positions into the list, float64 final scores) in boosted order.  Fused scores are not
        renormalised: identity, or min-max with normalization="minmax"; the order is descending."""
        rows, scores, functions, modes = self._boost_list_request(rows, scores, spec)
        pos, _, final, _ = self._boost_rows_blocking((rows, scores, functions), modes)
        return pos, final

    async def boost_rerank_lists_async(self, rows, scores, spec):
        """boost_rerank_lists for a caller on the event loop: on one GPU shard concurrent callers share one
        hr_boost_rerank_dev launch (a kind of its own in the batching front); sharded managers use the restatement."""
        rows, scores, functions, modes = self._boost_list_request(rows, scores, spec)
        pos, _, final, _ = await self._boost_rows_async(rows, scores, functions, modes)
        return pos, final

    # ---- vector MMR (the contract is in include/hbmrag.h, the restatement in mmr.py) ----------------------------------------
    def _ranker_request(self, collection_name: str, top_k, ranker, group_by_field, group_size, strict_group_size, offset):
        """The refusals of a search with a ranker of either kind, before anything is searched."""
        check = self._maxsim_request if isinstance(ranker, MaxSimRanker) else self._mmr_request if isinstance(ranker, MMRRanker) else \
            self._boost_request if isinstance(ranker, (BoostRanker, FunctionScore)) else self._decay_request
        return check(collection_name, top_k, ranker, group_by_field, group_size, strict_group_size, offset)

    def _mmr_request(self, collection_name: str, top_k, ranker, group_by_field, group_size, strict_group_size, offset):
        """(collection, W, norm code) of a search with an MMRRanker, or the refusal — before anything is searched."""
        if collection_name not in self.collections:
            raise ValueError(f"Collection {collection_name} not found")
        coll = self.collections[collection_name]
        if coll.kind == "sparse":
            raise ValueError(f"vector MMR diversifies on stored dense embeddings: {collection_name} has none")
        if group_by_field is not None or group_size != 1 or strict_group_size is not None:
            raise ValueError("ranker cannot be combined with group_by_field")
        if isinstance(offset, (bool, np.bool_)) or not isinstance(offset, (int, np.integer)) or offset != 0:
            raise ValueError(f"ranker cannot be combined with offset, got offset={offset!r}")
        if isinstance(top_k, (bool, np.bool_)) or not isinstance(top_k, (int, np.integer)) or top_k < 1:
            raise ValueError(f"top_k must be an integer >= 1, got {top_k!r}")
        window = ranker.window(top_k)
        if window > HR_MAX_TOPK:
            raise ValueError(f"ranker diversifies the best max(top_k, candidates) = {window} rows: a deep window (> HR_MAX_TOPK = "
                             f"{HR_MAX_TOPK}) is not built")
        norm = ranker.norm_code(coll.metric)
        if hasattr(coll.handle, "round"):
            raise NotImplementedError("vector MMR is not built for the torchrun form (CollectiveShardSet)")
        return coll, window, norm

    async def _search_mmr(self, query_embedding, collection_name, top_k, filters, search_params, ranker, group_by_field,
                          group_size, strict_group_size, offset) -> List[Dict[str, Any]]:
        _, window, norm = self._mmr_request(collection_name, top_k, ranker, group_by_field, group_size, strict_group_size, offset)
        hits = await self.search(query_embedding, collection_name, window, filters, search_params)
        if not hits:
            return hits
        rows = np.asarray([h["_row"] for h in hits], dtype=np.int64)
        scores = np.asarray([h["score"] for h in hits], dtype=np.float32)      # fp32 list scores, widened by _format_hits
        pos, val = await self._mmr_rows_async(collection_name, rows, scores, float(ranker.lambda_mult), int(top_k), norm)
        out = []
        for p, v in zip(pos, val):
            hit = hits[int(p)]
            hit["mmr_value"] = float(v)
            out.append(hit)
        return out

    def _mmr_rows_blocking(self, payload, key):
        """The host restatement over row numbers (sharded managers, stand-ins, the front's one-by-one fallback):
        payload = (rows int64, scores, lambda, k_out), key = (collection, width, norm, ...) -> (positions, float64 values).
        A row outside the collection (-1: a hit without a row number) has the zero vector."""
        rows, scores, lam, k_out = payload
        coll = self.collections[key[0]]
        self._count("mmr_host_selects")
        rows = np.asarray(rows, dtype=np.int64)
        inside = (rows >= 0) & (rows < coll.handle.num_rows)
        vectors = np.zeros((len(rows), int(coll.dim)), dtype=np.float32)
        if inside.any():
            vectors[inside] = coll.handle.get_dense_rows(rows[inside])
        pos, val = vector_mmr([float(x) for x in scores], vectors, lam, k_out, int(key[2]))
        return np.asarray(pos, dtype=np.int32), np.asarray(val, dtype=np.float64)

    async def _mmr_rows_async(self, collection_name: str, rows: np.ndarray, scores: np.ndarray, lam: float, k_out: int, norm: int):
        """(positions in pick order, the value of every pick) of ONE list.  On one GPU shard through the batching front:
        the collection, the padded list length, the norm code and the score type are the request key, lambda travels per
        query, so concurrent requests with different lambdas share one hr_mmr_select_vec_dev launch.  Everything else is
        selected on the host by the restatement, over the vectors of ShardSet.get_dense_rows, with the same result, and
        counted in stats["mmr_host_selects"]."""
        n, K = len(rows), HR_MAX_TOPK
        width = next(w for w in (K // 4, K, 3 * K, n) if n <= w)      # few distinct launch shapes
        key = (collection_name, width, int(norm), scores.dtype == np.float64)
        payload = (rows, scores, float(lam), max(1, min(int(k_out), n)))
        coll = self.collections[collection_name]
        front = self._coalescer(coll)
        if front is None or front.collective or n > 3 * K or self._device_shard(coll.handle) is None:
            return await asyncio.to_thread(self._mmr_rows_blocking, payload, key)
        return await asyncio.wait_for(front.submit_async("mmr", key, payload),
                                      timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)

    def _mmr_list_request(self, rows, scores, lam, k):
        rows = np.asarray([-1 if r is None else int(r) for r in rows], dtype=np.int64)
        scores = np.asarray(scores, dtype=np.float64)
        if rows.shape != scores.shape or rows.ndim != 1:
            raise ValueError("a list's rows and scores differ in length")
        if "semantic_index" not in self.collections:
            raise ValueError("Collection semantic_index not found")
        return rows, scores, float(lam), int(k)

    def mmr_select_lists(self, rows, scores, lam: float, k: int):
        """Vector MMR over ONE fused list (row numbers, None for a hit without one, and float64 fused scores), blocking,
        through the host restatement: -> list positions in pick order, at most k.  The similarity is the cosine of the
        semantic_index stored vectors; the scores are taken as they are."""
        rows, scores, lam, k = self._mmr_list_request(rows, scores, lam, k)
        if not len(rows):
            return []
        from ._native import HR_NORM_NONE
        pos, _ = self._mmr_rows_blocking((rows, scores, lam, max(1, k)), ("semantic_index", len(rows), HR_NORM_NONE))
        return [int(p) for p in pos[:k]]

    async def mmr_select_lists_async(self, rows, scores, lam: float, k: int):
        """mmr_select_lists for a caller on the event loop: on one GPU shard concurrent callers share one
        hr_mmr_select_vec_dev launch (a kind of its own in the batching front); sharded managers use the restatement."""
        rows, scores, lam, k = self._mmr_list_request(rows, scores, lam, k)
        if not len(rows):
            return []
        from ._native import HR_NORM_NONE
        pos, _ = await self._mmr_rows_async("semantic_index", rows, scores, lam, max(1, k), HR_NORM_NONE)
        return [int(p) for p in pos[:k]]

    def _decay_rows_blocking(self, payload, key):
        """The host restatement over row numbers (sharded managers, stand-ins, the front's one-by-one fallback):
        payload = (rows int64, scores, operands), key = (field, norm, ...) -> (positions, rows, float64 final scores)."""
        from .device_decay import host_values
        rows, scores, operands = payload
        self._count("decay_host_reranks")
        values = host_values(None if self._synthetic_rows else self._cols, key[0], self.num_rows, rows)
        pos, ids, final = decay_rerank(np.asarray(rows).tolist(), [float(x) for x in scores], values.tolist(), operands,
                                       int(key[1]), len(rows))
        return np.asarray(pos, dtype=np.int32), np.asarray(ids, dtype=np.int64), np.asarray(final, dtype=np.float64)

    async def _decay_rows_async(self, rows: np.ndarray, scores: np.ndarray, field: str, operands, norm: int):
        """(positions, rows, final scores) of ONE list in decayed order, whole.  On one GPU shard through the batching front:
        the field, the norm code, the padded list length and the score type are the request key, the operands travel per
        query, so concurrent requests with different curves share one hr_decay_rerank_dev launch.  Everything else is
        reranked on the host by the restatement, with the same result, and counted in stats["decay_host_reranks"]: a manager
        without a front (sharded, coalesce=False), a list longer than 3 * HR_MAX_TOPK entries (three modality lists at a
        large top_k on the general path) and, inside the front, the requests of a batch whose launch was refused."""
        n, K = len(rows), HR_MAX_TOPK
        width = next(w for w in (K // 4, K, 3 * K, n) if n <= w)      # few distinct launch shapes
        key = (field, int(norm), width, scores.dtype == np.float64)
        payload = (rows, scores, tuple(operands))
        front = self._coalescer(self.collections["semantic_index"]) if "semantic_index" in self.collections else None
        if front is None or front.collective or n > 3 * K or self._device_shard(self._main) is None:
            return await asyncio.to_thread(self._decay_rows_blocking, payload, key)
        return await asyncio.wait_for(front.submit_async("decay", key, payload),
                                      timeout=IndexingConstants.MILVUS_TIMEOUT_SECONDS)

    def _decay_list_request(self, rows, scores, ranker: DecayRanker, operands=None):
        if not isinstance(ranker, DecayRanker):
            raise ValueError(f"decay must be a DecayRanker, got {ranker!r}")
        from .device_decay import check_decay_field
        check_decay_field(ranker.field, bool(self._synthetic_rows))
        rows, scores = np.asarray(rows, dtype=np.int64), np.asarray(scores, dtype=np.float64)
        if rows.shape != scores.shape or rows.ndim != 1:
            raise ValueError("a list's rows and scores differ in length")
        return rows, scores, tuple(operands) if operands is not None else ranker.operands(), ranker.norm_code("IP", fused=True)

    def decay_rerank_lists(self, rows, scores, ranker: DecayRanker, operands=None):
        """The decay ranker over ONE fused list (row numbers and float64 fused scores), blocking, through the host
        restatement: -> (positions into the list, float64 final scores) in decayed order.  Fused scores are not
        renormalised: identity, or min-max with normalization="minmax"."""
        rows, scores, operands, norm = self._decay_list_request(rows, scores, ranker, operands)
        pos, _, final = self._decay_rows_blocking((rows, scores, operands), (ranker.field, norm))
        return pos, final

    async def decay_rerank_lists_async(self, rows, scores, ranker: DecayRanker, operands=None):
        """decay_rerank_lists for a caller on the event loop: on one GPU shard concurrent callers share one
        hr_decay_rerank_dev launch (a kind of its own in the batching front); sharded managers use the restatement."""
        rows, scores, operands, norm = self._decay_list_request(rows, scores, ranker, operands)
        pos, _, final = await self._decay_rows_async(rows, scores, ranker.field, operands, norm)
        return pos, final

    # ------------------------------------------------------------------ embeddings
    async def _run_encoder(self, fn, *args):
        if asyncio.iscoroutinefunction(fn):
            return await fn(*args)
        if getattr(self.embedding_generator, "run_inline", False):
            # the generator declares its synchronous hooks cheap (a lookup, a hash): no thread-pool hop per request (the
            # reference offloads every sync hook, indexing.py:610-620 — right for a model forward, 60 us of pure overhead
            # for a table)
            return fn(*args)
        return await asyncio.get_event_loop().run_in_executor(self.embedding_executor, lambda: fn(*args))

    async def _generate_semantic_embeddings_batch(self, texts: List[str]) -> List[np.ndarray]:
        cache = get_semantic_cache()
        out: List[Optional[np.ndarray]] = []
        missing: List[int] = []
        for i, t in enumerate(texts):
            hit = await cache.get(t)
            out.append(hit)
            if hit is None:
                missing.append(i)
        if missing and self.embedding_generator:
            gen = self.embedding_generator
            batch_fn = getattr(gen, "encode_semantic_batch", None)
            miss_texts = [texts[i] for i in missing]
            if batch_fn is not None:   # one batched forward instead of the reference's per-text loop (:584-587)
                vecs = await self._run_encoder(batch_fn, miss_texts)
            elif asyncio.iscoroutinefunction(gen.encode_semantic):
                vecs = [await gen.encode_semantic(t) for t in miss_texts]
            else:
                vecs = await asyncio.get_event_loop().run_in_executor(
                    self.embedding_executor, lambda: [gen.encode_semantic(t) for t in miss_texts])
            for i, v in zip(missing, vecs):
                await cache.put(texts[i], v)
                out[i] = v
        else:
            for i in missing:  # placeholder, uncached in the batch path as in the reference (:593-597)
                out[i] = np.random.randn(self.semantic_dim).astype(np.float32)
        return out  # type: ignore[return-value]

    def _device_table(self):
        """The device-resident table of semantic query embeddings, created on first use together with its counters."""
        if self._dev_cache is None:
            self._dev_cache = DeviceEmbeddingTable(self._dev_cache_slots, self.semantic_dim, f"cuda:{self.device}")
            self.device_cache_stats = {"hits": 0, "misses": 0}
        return self._dev_cache

    def _count_device_lookup(self, vec):
        """Book a lookup in the device table as a hit (a row) or a miss (None); hands `vec` back."""
        self.device_cache_stats["hits" if vec is not None else "misses"] += 1
        return vec

    def _device_query_embedding(self, text: str):
        """float32 [dim] CUDA tensor for `text` from the device-resident table (filled on a miss)."""
        key = EmbeddingCache._materialize_key(text)
        vec = self._count_device_lookup(self._device_table().lookup(key))
        if vec is not None:
            return vec
        gen = self.embedding_generator
        if gen is not None and hasattr(gen, "encode_to_device"):
            fresh = gen.encode_to_device([text])[0]
        elif gen is not None:
            fresh = np.asarray(gen.encode_semantic(text), dtype=np.float32)
        else:
            fresh = np.random.randn(self.semantic_dim).astype(np.float32)
        return self._dev_cache.store(key, fresh)

    async def _generate_semantic_embedding(self, text: str):
        gen = self.embedding_generator
        if self._dev_cache_slots > 0 and self._main is not None and not (
                gen is not None and asyncio.iscoroutinefunction(gen.encode_semantic)):
            key = EmbeddingCache._materialize_key(text)
            hit = self._device_table().lookup(key)
            if hit is not None:          # a hit is a dictionary lookup: no executor hop, no task
                return self._count_device_lookup(hit)
            front = self._encode_front(gen)
            if front is not None:        # the misses of a round share ONE encoder forward (batching.py::_enqueue_encode)
                self._count_device_lookup(None)
                return await front.submit_async("encode", ("encode",), (key, text))
            return await asyncio.get_event_loop().run_in_executor(self.embedding_executor, self._device_query_embedding, text)
        front = self._encode_front(gen)
        if front is not None:
            key = EmbeddingCache._materialize_key(text)

            async def compute_batched() -> np.ndarray:   # the host cache holds host arrays (reference indexing.py:601-627)
                row = await front.submit_async("encode", ("encode",), (key, text))
                return await asyncio.get_event_loop().run_in_executor(self.embedding_executor, lambda: row.cpu().numpy())
            return await get_semantic_cache().get_or_compute(text, compute_batched)

        async def compute() -> np.ndarray:
            if self.embedding_generator:
                return await self._run_encoder(self.embedding_generator.encode_semantic, text)
            return np.random.randn(self.semantic_dim).astype(np.float32)
        return await get_semantic_cache().get_or_compute(text, compute)

    def _encode_front(self, gen):
        """The batching front when it can encode queries for this manager (a generator with `encode_to_device` on a
        single-shard, single-process manager), else None."""
        if gen is None or not hasattr(gen, "encode_to_device") or not self.coalesce or "semantic_index" not in self.collections:
            return None
        front = self._coalescer(self.collections["semantic_index"])
        return None if front is None or front.collective else front

    async def _generate_sparse_embedding(self, text: str, role: str = "query"):
        gen = self.embedding_generator
        if gen:
            fn = gen.encode_sparse
            if role == "query" and hasattr(gen, "encode_sparse_query"):
                fn = gen.encode_sparse_query
            return await self._run_encoder(fn, text)
        nnz = min(100, self.sparse_dim)
        picks = np.random.choice(self.sparse_dim, size=nnz, replace=False)
        vals = np.abs(np.random.randn(nnz).astype(np.float32))
        order = np.argsort(picks)
        return {"indices": picks[order].tolist(), "values": vals[order].astype(float).tolist()}

    async def _generate_domain_embedding(self, text: str, domain: Optional[str] = None) -> np.ndarray:
        gen = self.embedding_generator
        if gen:
            if asyncio.iscoroutinefunction(gen.encode_domain):
                return await gen.encode_domain(text, domain or "")
            return await asyncio.get_event_loop().run_in_executor(self.embedding_executor,
                                                                  lambda: gen.encode_domain(text, domain))
        return np.random.randn(self.domain_dim).astype(np.float32)

    # ------------------------------------------------------------------ query (rows by expression, no query vector)
    COUNT_FIELD = "count(*)"
    QUERY_FIELDS = ("id", "chunk_id", "doc_id", "content", "chunk_index", "token_count", "entropy", "redundancy",
                    "domain_density", "metadata_json", "timestamp", "embedding")
    # what a payload-free (synthetic) collection can derive from the row number: the fields _format_hits shows for it
    SYNTHETIC_QUERY_FIELDS = {"id": lambda r: MilvusIndexManager.synthetic_id(r), "chunk_id": lambda r: MilvusIndexManager.synthetic_id(r),
                              "doc_id": lambda r: f"doc{r // 10}", "content": lambda r: "", "chunk_index": lambda r: r % 10,
                              "entropy": lambda r: 0.0, "redundancy": lambda r: 0.0, "domain_density": lambda r: 0.0,
                              "timestamp": lambda r: ""}

    def _query_request(self, collection_name: str, output_fields, limit, offset):
        """Check a query's arguments before anything is evaluated -> (collection, fields without duplicates, count?, limit, offset)."""
        if collection_name not in self.collections:
            raise ValueError(f"Collection {collection_name} not found")
        coll = self.collections[collection_name]
        if output_fields is None:
            output_fields = []
        if isinstance(output_fields, str) or not all(isinstance(f, str) for f in output_fields):
            raise ValueError(f"output_fields must be a list of field names, got {output_fields!r}")
        fields = list(dict.fromkeys(output_fields))
        count = self.COUNT_FIELD in fields
        if count and len(fields) != 1:
            raise ValueError(f"{self.COUNT_FIELD} cannot be combined with other output fields: {fields}")
        for f in fields:
            if not count and f not in self.QUERY_FIELDS:
                raise ValueError(f"unknown output field: {f!r} (known: {', '.join(self.QUERY_FIELDS)}, {self.COUNT_FIELD})")
            if not count and self._synthetic_rows and f != "embedding" and f not in self.SYNTHETIC_QUERY_FIELDS:
                raise ValueError(f"this shard was bulk-ingested without payload columns: it has no {f}")
        for name, v in (("offset", offset), ("limit", limit)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError(f"{name} must be an integer, got {v!r}")
        if offset is None or offset < 0:
            raise ValueError(f"offset must be >= 0, got {offset!r}")
        if limit is not None and (limit < 0 or not 1 <= offset + limit <= QUERY_MAX_WINDOW):
            raise ValueError(f"a query takes 1 <= offset + limit <= {QUERY_MAX_WINDOW} and limit >= 0, got offset={offset}, limit={limit}")
        if "embedding" in fields and not hasattr(coll.handle, "handles"):
            raise NotImplementedError("reading stored vectors back (embedding) is not built for the torchrun form "
                                      "(CollectiveShardSet)")
        return coll, fields, count, (None if limit is None else int(limit)), int(offset)

    def _query_rows(self, expr: Optional[str], limit: Optional[int], offset: int) -> Tuple[int, np.ndarray, bool]:
        """(rows that pass, the page's global rows, whether the page came from the device mask)."""
        on_device = self._device_shard(self._main) is not None
        total, rows = (self._query_rows_device if on_device else self._query_rows_host)(expr, limit, offset)
        return total, rows, on_device

    def _query_rows_device(self, expr: Optional[str], limit: Optional[int], offset: int) -> Tuple[int, np.ndarray]:
        """(rows that pass, the page's global rows) of one GPU shard: the cached packed mask of `expr` + tombstones stays in
        HBM and hr_mask_rows_dev turns it into the page; two counts and the page's ids come back, nothing row-sized moves.
        limit None: count first, then fetch everything after `offset`."""
        import torch
        nat = self._native
        n = self.num_rows
        dev = torch.device("cuda", self._main.first.device)
        with torch.cuda.device(dev):
            mask = self._global_device_mask(expr)          # None: every row passes (no expression, no tombstone)
            ptr = mask.data_ptr() if mask is not None else 0
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            scratch = torch.empty(max(nat.mask_rows_scratch_bytes(n), 8), dtype=torch.uint8, device=dev) if ptr else None
            stream = torch.cuda.current_stream(dev)

            def page(lim: int):
                rows = torch.empty(max(lim, 1), dtype=torch.int64, device=dev)
                nat.mask_rows_dev(ptr, n, 0, offset, lim, rows.data_ptr(), counts.data_ptr(),
                                  scratch.data_ptr() if scratch is not None else 0, stream.cuda_stream)
                total, written = (int(x) for x in counts.cpu().tolist())     # synchronises the stream
                return total, rows[:written].cpu().numpy()

            if limit is None:
                total, _ = page(0)
                if total <= offset:
                    return total, np.zeros(0, np.int64)
                limit = total - offset
            return page(limit)

    def _query_rows_host(self, expr: Optional[str], limit: Optional[int], offset: int) -> Tuple[int, np.ndarray]:
        """The same contract over the host view of the mask (several shards, the torchrun form on rank 0, CPU stand-ins)."""
        keep = self._row_mask(expr)
        rows = np.arange(self.num_rows, dtype=np.int64) if keep is None else np.flatnonzero(keep).astype(np.int64)
        return int(rows.shape[0]), rows[offset:] if limit is None else rows[offset:offset + limit]

    def _query_blocking(self, collection_name: str, expr: Optional[str], output_fields, limit: Optional[int],
                        offset: int) -> List[Dict[str, Any]]:
        coll, fields, count, limit, offset = self._query_request(collection_name, output_fields, limit, offset)
        expr = expr if (expr is not None and str(expr).strip()) else None
        if expr is None and limit is None and not count:
            raise ValueError("a query without an expression needs a limit")
        if count:
            limit, offset = 0, 0
        total, rows, on_device = self._query_rows(expr, limit, offset)
        self._count("queries")
        if on_device:
            self._count("query_device")
        if count:
            return [{self.COUNT_FIELD: total}]
        vectors = None
        if "embedding" in fields and len(rows):
            vectors = self._sparse_payloads(coll, rows) if coll.kind == "sparse" else coll.handle.get_dense_rows(rows)
        if self._synthetic_rows:
            getters = {f: self.SYNTHETIC_QUERY_FIELDS[f] for f in ["id"] + fields if f != "embedding"}
        else:
            c = self._cols
            getters = {f: c["id" if f == "chunk_id" else f].__getitem__ for f in ["id"] + fields if f != "embedding"}
        out = []
        for i, row in enumerate(rows.tolist()):
            ent = {f: get(row) for f, get in getters.items()}
            if "embedding" in fields:
                ent["embedding"] = vectors[i]
            out.append(ent)
        return out

    async def query(self, collection_name: str, expr: Optional[str] = None, output_fields: Optional[Sequence[str]] = None,
                    limit: Optional[int] = None, offset: int = 0) -> List[Dict[str, Any]]:
        """pymilvus' Collection.query: the rows that pass `expr` (the filter language of filters.py; "" or None = every
        row, then `limit` is required) and are not deleted, in ASCENDING GLOBAL ROW order — Milvus promises none; this one
        is promised, so pages concatenate — without the first `offset`, at most `limit` of them (limit=None with an
        expression: all of them).  1 <= offset + limit <= QUERY_MAX_WINDOW.  -> flat dicts: the primary key "id" always,
        the requested fields besides (QUERY_FIELDS); "embedding" is the stored vector of the named collection as float32
        [dim] (fp16 shards widened exactly); on sparse_index it is the stored payload {"indices": int32 [nnz], "values":
        float32 [nnz]} — the shape of an ingested payload, which search() takes as it is (_sparse_payloads has the rule for
        rows without entries).  output_fields=["count(*)"] -> [{"count(*)": n}].  Refusals are ValueError."""
        return await asyncio.to_thread(self._query_blocking, collection_name, expr, output_fields, limit, offset)

    # ------------------------------------------------------------------ stored vectors as queries
    def _sparse_rows_device(self, h, rows: np.ndarray):
        """The CSR of the stored sparse rows `rows` of one GPU shard whose local rows are the global rows, through
        hr_get_sparse_rows_dev: the count pass sizes the entry buffers, the second call fills them.  A row the shard has no
        sparse row for is empty (the device form's rule for an id outside the shard)."""
        import torch
        nat = self._native
        n = int(rows.shape[0])
        dev = torch.device("cuda", h.device)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            d_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64) + int(getattr(h, "row_offset", 0))).to(dev)
            indptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            scratch = torch.empty(nat.get_sparse_rows_scratch_bytes(n), dtype=torch.uint8, device=dev)

            def call(idx, val, cap):
                h.get_sparse_rows_dev(d_rows.data_ptr(), n, indptr.data_ptr(), idx.data_ptr() if cap else 0,
                                      val.data_ptr() if cap else 0, cap, counts.data_ptr(), scratch.data_ptr(), stream.cuda_stream)
                return int(counts.cpu()[0])      # synchronises the stream

            total = call(None, None, 0)
            idx = torch.empty(total, dtype=torch.int32, device=dev)
            val = torch.empty(total, dtype=torch.float32, device=dev)
            if total and call(idx, val, total) != total:
                raise RuntimeError("the sparse rows changed while they were read")
            return indptr.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()

    def _sparse_payloads(self, coll, rows: np.ndarray) -> List[Dict[str, np.ndarray]]:
        """The stored sparse payloads of the global rows `rows`, in that order, each {"indices": int32 [nnz], "values":
        float32 [nnz]} — indices ascending, the stored bits.  index_chunks and the bulk ingests give every row of a batch
        that carries sparse payloads a sparse row (an EMPTY one where a chunk's encoding failed or a shard refused the
        batch), so sparse row r belongs to entity r and a failed encoding reads back as two empty arrays.  Only rows
        appended without any sparse payload after the last batch with one (sparse encoding switched off, add_rows without
        a CSR) have no sparse row at all; they lie beyond num_sparse_rows and read back as two empty arrays too — on one
        GPU shard by the device form's rule for an id outside the shard, elsewhere by ShardSet.get_sparse_rows."""
        s = coll.handle
        # rows_of ascends without repeats: it is the identity exactly when its last entry is its length - 1
        one_gpu = s.n_shards == 1 and is_native_handle(s.first) and len(s.rows_of[0]) and \
            int(s.rows_of[0][-1]) == len(s.rows_of[0]) - 1
        ptr, idx, val = self._sparse_rows_device(s.first, rows) if one_gpu else s.get_sparse_rows(rows)
        return [{"indices": idx[ptr[i]:ptr[i + 1]].copy(), "values": val[ptr[i]:ptr[i + 1]].copy()} for i in range(len(rows))]

    def _rows_of_ids(self, ids) -> np.ndarray:
        """The global row of every primary key of `ids`, in request order: `id in [...]` through the filter language (on
        one GPU shard the device mask; keys that share their first 16 bytes through its undecided-rows host path), the mask
        as a page of ascending rows, the rows matched to the request by the host id column.  Of several live rows with one
        id the lowest is taken.  ValueError for an id no live row carries."""
        if not isinstance(ids, (list, tuple)) or not len(ids):
            raise ValueError(f"ids must be a non-empty list of primary keys, got {ids!r}")
        for i in ids:
            if not isinstance(i, str):
                raise ValueError(f"a primary key is a string, got {i!r}")
        wanted = list(dict.fromkeys(ids))
        _, rows, _ = self._query_rows("id in " + _filters._show_list(wanted), None, 0)
        id_of = self.synthetic_id if self._synthetic_rows else self._cols["id"].__getitem__
        row_of: Dict[str, int] = {}
        for r in rows.tolist():
            row_of.setdefault(id_of(r), r)         # ascending rows: the lowest row of an id stays
        for i in wanted:
            if i not in row_of:
                raise ValueError(f"no entity with id {i!r} in this collection (deleted entities are not found)")
        return np.asarray([row_of[i] for i in ids], dtype=np.int64)

    def _stored_queries_blocking(self, ids, collection_name: str) -> list:
        """What search() takes as the query for each entity of `ids`: its stored vector of the named collection."""
        if collection_name not in self.collections:
            raise ValueError(f"Collection {collection_name} not found")
        coll = self.collections[collection_name]
        if not hasattr(coll.handle, "handles"):
            raise NotImplementedError("search by primary key is not built for the torchrun form (CollectiveShardSet)")
        rows = self._rows_of_ids(ids)
        self._count("search_by_ids")
        if coll.kind == "sparse":
            return self._sparse_payloads(coll, rows)
        return list(coll.handle.get_dense_rows(rows))

    async def search_by_ids(self, ids, collection_name: str, top_k: int = 20, filters: Optional[str] = None,
                            search_params: Optional[Dict] = None, *, group_by_field: Optional[str] = None,
                            group_size: int = 1, strict_group_size: Optional[bool] = None,
                            ranker: Optional[Any] = None) -> List[List[Dict[str, Any]]]:
        """pymilvus' search by primary key ("more like this entity"): one hit list per id of `ids`, in request order, each
        exactly what search() returns for that entity's STORED vector of the named collection with the same arguments —
        the fp32-widened stored row of a dense collection, the stored payload of sparse_index; filters, range params and
        grouping and `ranker` pass through untouched.  The entity itself is NOT excluded (it is its own best hit wherever the metric
        makes it so): a `range_filter` or the filter `id not in [...]` drops it.  A duplicate id gives two equal lists; of
        several live rows with one id (a re-ingest without a delete) the lowest row is used.  The vectors are fetched once
        for all ids and make one hop through the host; the searches are search() calls, so concurrent ones share the
        batching front's launches.  ValueError: `ids` empty or not a list, an id that is not a string, an id no live row
        carries (a deleted entity is not found), and whatever the filter language (its list cap) and search() (a sparse
        row of more than HR_MAX_QUERY_NNZ entries) refuse.  NotImplementedError in the torchrun form."""
        if ranker is not None:      # refused before the vectors are fetched
            self._ranker_request(collection_name, top_k, ranker, group_by_field, group_size, strict_group_size, 0)
        queries = await asyncio.to_thread(self._stored_queries_blocking, ids, collection_name)
        extra = {"ranker": ranker} if ranker is not None else {}
        return list(await asyncio.gather(*(self.search(q, collection_name, top_k, filters, search_params,
                                                       group_by_field=group_by_field, group_size=group_size,
                                                       strict_group_size=strict_group_size, **extra) for q in queries)))

    def _search_by_ids_blocking(self, ids, collection_name: str, top_k: int, filters: Optional[str],
                                search_params: Optional[Dict], group_by_field: Optional[str], group_size: int,
                                strict_group_size: Optional[bool]) -> List[List[Dict[str, Any]]]:
        """search_by_ids for a synchronous caller: the same lists, every search through the blocking path."""
        if group_by_field is not None or group_size != 1 or strict_group_size is not None:
            self._check_group_request(group_by_field, group_size, top_k, strict_group_size)
        return [self._search_blocking(q, collection_name, top_k, filters, search_params, group_by_field, int(group_size))
                for q in self._stored_queries_blocking(ids, collection_name)]

    # ------------------------------------------------------------------ misc
    def get_collection_stats(self, collection_name: str) -> Dict[str, Any]:
        coll = self.collections.get(collection_name)
        if coll is None:
            return {}
        return {"name": collection_name, "num_entities": coll.num_entities, "schema": coll.schema,
                "indexes": coll.indexes}

    async def delete_by_filter(self, collection_name: str, expr: str):
        if collection_name in self.collections:
            self.collections[collection_name].delete(expr)

    async def close(self):
        if self._front is not None:
            await asyncio.to_thread(self._front.close)
            self._front = None
        self._dev_masks.clear()
        for h in (self._main, self._domain):
            if h is not None:
                try:
                    h.close()
                except Exception:
                    pass
        self._main = self._domain = None
        self.collections.clear()
        if hasattr(self, "embedding_executor"):
            self.embedding_executor.shutdown(wait=True)


HbmIndexManager = MilvusIndexManager
