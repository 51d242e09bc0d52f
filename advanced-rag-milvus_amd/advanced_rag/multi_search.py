"""Multi-request search: pymilvus' `Collection.hybrid_search(reqs, rerank, limit)` for this manager.

`await manager.multi_search([SearchRequest(...), ...], RRFRanker() | WeightedRanker(...), limit)` runs up to 16 plain
searches — each on any of the three collections, with its own limit, filter and params — and fuses their ranked lists
into ONE ranking on the device (hr_fuse_lists_dev, csrc/fuse_lists.h).  The contract of the fusion is the three-list
fusion's with "three lists" replaced by "L lists"; `retrieval.rrf_rank_lists` and `retrieval.score_fuse_lists` restate it.
The fusion key is the global row number: the three collections share one row space.

This module holds the three spec classes, the refusals and the host restatement over row numbers; the searches, the
batching front and hit formatting are the manager's (indexing.py, batching.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._native import HR_FUSE_RRF, HR_FUSE_WEIGHTED, HR_MAX_FUSE_LISTS, HR_MAX_TOPK

MAX_FUSED = 3 * HR_MAX_TOPK          # a fused list still fits the decay ranker, MMR and the group pass
NORMALIZATIONS = ("activation", "minmax")


def _integer(name: str, v, lo: int, hi: int) -> int:
    """An integer in lo .. hi; bool and floats are refused, as deep_window refuses them."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    if not lo <= v <= hi:
        raise ValueError(f"{name} must be in {lo} .. {hi}, got {v}")
    return int(v)


def _weights(weights, what: str) -> Tuple[float, ...]:
    out = []
    for w in weights:
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what}: a weight must be a number, got {w!r}")
        if not math.isfinite(float(w)):
            raise ValueError(f"{what}: a weight must be finite, got {w!r}")
        out.append(float(w))
    return tuple(out)


@dataclass
class SearchRequest:
    """One sub-search (pymilvus' AnnSearchRequest): exactly `manager.search(data, collection_name, top_k=limit, filters,
    search_params)`.  data: a dense vector, or a sparse embedding for sparse_index."""
    data: Any
    collection_name: str
    limit: int = 20
    filters: Optional[str] = None
    search_params: Optional[Dict] = None

    def __post_init__(self):
        self.check()

    def check(self) -> "SearchRequest":
        if not isinstance(self.collection_name, str):
            raise ValueError(f"collection_name must be a string, got {self.collection_name!r}")
        self.limit = _integer("SearchRequest.limit", self.limit, 1, HR_MAX_TOPK)
        if self.filters is not None and not isinstance(self.filters, str):
            raise ValueError(f"filters must be an expression string or None, got {self.filters!r}")
        if self.search_params is not None and not isinstance(self.search_params, dict):
            raise ValueError(f"search_params must be a dict or None, got {self.search_params!r}")
        return self


class RRFRanker:
    """Reciprocal-rank fusion: score = sum over the requests that hold the row of weight / (k + rank), rank from 1.
    weights: one finite number per request; None = all 1.0."""

    def __init__(self, k: int = 60, weights: Optional[Sequence[float]] = None):
        self.k = _integer("RRFRanker.k", k, 1, 1 << 30)
        self.weights = None if weights is None else _weights(weights, "RRFRanker")

    def __repr__(self):
        return f"RRFRanker(k={self.k}, weights={self.weights})"


class WeightedRanker:
    """Weighted score fusion: score = sum over the requests that hold the row of weight * n(score); n normalises a request's
    scores into [0, 1] — "activation" by the collection's metric, or "minmax" over the request's list (HR_NORM_*,
    include/hbmrag.h), mapped per request through retrieval.norm_code as DecayRanker does."""

    def __init__(self, *weights: float, normalization: str = "activation"):
        if normalization not in NORMALIZATIONS:
            raise ValueError(f"normalization must be one of {', '.join(NORMALIZATIONS)}, got {normalization!r}")
        if not weights:
            raise ValueError("WeightedRanker takes one weight per request")
        self.weights = _weights(weights, "WeightedRanker")
        self.normalization = normalization

    def __repr__(self):
        return f"WeightedRanker{self.weights + (self.normalization,)}"


@dataclass
class FusionPlan:
    """What a checked multi_search call fuses with: the mode, one weight (and, weighted, one HR_NORM_* code) per request."""
    mode: int
    weights: Tuple[float, ...]
    norms: Optional[Tuple[int, ...]]
    rrf_k: int
    limit: int


def check_ranker(ranker, n_requests: int, metrics: Sequence[str], limit) -> FusionPlan:
    """The refusals that concern the ranker and the limit; metrics = the metric each request's collection ranks by."""
    limit = _integer("limit", limit, 1, MAX_FUSED)
    if isinstance(ranker, RRFRanker):
        k = _integer("RRFRanker.k", ranker.k, 1, 1 << 30)
        weights = (1.0,) * n_requests if ranker.weights is None else _weights(ranker.weights, "RRFRanker")
        mode, norms = HR_FUSE_RRF, None
    elif isinstance(ranker, WeightedRanker):
        from .retrieval import norm_code
        if ranker.normalization not in NORMALIZATIONS:
            raise ValueError(f"normalization must be one of {', '.join(NORMALIZATIONS)}, got {ranker.normalization!r}")
        weights = _weights(ranker.weights, "WeightedRanker")
        mode, k = HR_FUSE_WEIGHTED, 60
        norms = tuple(norm_code(m, ranker.normalization) for m in metrics)
    else:
        raise ValueError(f"ranker must be an RRFRanker or a WeightedRanker, got {ranker!r}")
    if len(weights) != n_requests:
        raise ValueError(f"{type(ranker).__name__} holds {len(weights)} weights for {n_requests} requests")
    return FusionPlan(mode, weights, norms, k, limit)


def check_requests(requests, collections) -> List[SearchRequest]:
    """1 .. 16 SearchRequests that name known collections, each checked again (the fields are mutable)."""
    if isinstance(requests, SearchRequest) or not isinstance(requests, (list, tuple)):
        raise ValueError(f"requests must be a list of SearchRequest, got {requests!r}")
    if not 1 <= len(requests) <= HR_MAX_FUSE_LISTS:
        raise ValueError(f"multi_search takes 1 .. {HR_MAX_FUSE_LISTS} requests, got {len(requests)}")
    for i, r in enumerate(requests):
        if not isinstance(r, SearchRequest):
            raise ValueError(f"request {i} is not a SearchRequest: {r!r}")
        r.check()
        if r.collection_name not in collections:
            raise ValueError(f"Collection {r.collection_name} not found")
    return list(requests)


def padded_length(n: int) -> int:
    """The list length a fusion request is padded to (with -1): few distinct launch shapes, so that requests share a launch."""
    return next(w for w in (8, 16, 32, 64, 128, HR_MAX_TOPK) if n <= w)


def check_fuse_lists(row_lists, score_lists, weights, mode, norms, rrf_k, top_k):
    """The operands of one fusion request -> (payload = (((rows int64, scores float32) per list), weights), key = (mode,
    n_lists, padded k_in, norms, rrf_k, top_k)): requests with equal keys share a launch, the weights travel per query."""
    n = len(row_lists)
    if not 1 <= n <= HR_MAX_FUSE_LISTS:
        raise ValueError(f"a fusion takes 1 .. {HR_MAX_FUSE_LISTS} lists, got {n}")
    if mode not in (HR_FUSE_RRF, HR_FUSE_WEIGHTED):
        raise ValueError(f"mode must be HR_FUSE_RRF or HR_FUSE_WEIGHTED, got {mode!r}")
    weights = _weights(weights, "fusion")
    if len(weights) != n:
        raise ValueError(f"{len(weights)} weights for {n} lists")
    weighted = mode == HR_FUSE_WEIGHTED
    if weighted:
        if score_lists is None or len(score_lists) != n or norms is None or len(norms) != n:
            raise ValueError("weighted fusion takes one score list and one norm code per list")
        norms = tuple(int(c) for c in norms)
        if any(not 0 <= c <= 4 for c in norms):
            raise ValueError(f"norm codes must be HR_NORM_* (0..4), got {norms}")
    lists = []
    for l in range(n):
        rows = np.asarray(row_lists[l], dtype=np.int64).reshape(-1)
        neg = np.flatnonzero(rows < 0)
        if len(neg):
            rows = rows[:int(neg[0])]            # a list ends at its first id < 0
        sc = np.asarray(score_lists[l], dtype=np.float32).reshape(-1)[:len(rows)] if weighted else np.zeros(len(rows), np.float32)
        if len(sc) != len(rows):
            raise ValueError("a list's rows and scores differ in length")
        if len(rows) > HR_MAX_TOPK:
            raise ValueError(f"a list holds at most HR_MAX_TOPK = {HR_MAX_TOPK} entries, got {len(rows)}")
        lists.append((rows, sc))
    k_in = padded_length(max(1, max(len(r) for r, _ in lists)))
    total = max(1, sum(len(r) for r, _ in lists))
    top_k = min(total, MAX_FUSED) if top_k is None else _integer("top_k", top_k, 1, MAX_FUSED)
    key = (int(mode), n, k_in, norms if weighted else None, _integer("rrf_k", rrf_k, 1, 1 << 30), top_k)
    return (tuple(lists), weights), key


def stage_fuse_lists(payloads, key):
    """Host staging of the requests of one launch: ids [B, L, k] (-1 padded), scores [B, L, k] fp32 (None for RRF) and
    the per-query weights [B, L]."""
    mode, n, k_in = key[0], key[1], key[2]
    B = len(payloads)
    ids = np.full((B, n, k_in), -1, dtype=np.int64)
    sc = np.zeros((B, n, k_in), dtype=np.float32) if mode == HR_FUSE_WEIGHTED else None
    wq = np.empty((B, n), dtype=np.float64)
    for i, (lists, weights) in enumerate(payloads):
        wq[i] = weights
        for l, (rows, scores) in enumerate(lists):
            ids[i, l, :len(rows)] = rows
            if sc is not None:
                sc[i, l, :len(rows)] = scores
    return ids, sc, wq


def fuse_lists_host(payload, key):
    """One fusion request through the two restatements (CPU stand-in managers): -> (rows int64, fp64 scores, list masks)."""
    from .retrieval import rrf_rank_lists, score_fuse_lists
    lists, weights = payload
    mode, _, _, norms, rrf_k, top_k = key
    if mode == HR_FUSE_RRF:
        fused = rrf_rank_lists([r.tolist() for r, _ in lists], weights, rrf_k)
    else:
        fused = score_fuse_lists([(r.tolist(), s) for r, s in lists], weights, norms)
    fused = fused[:top_k]
    return (np.asarray([f[0] for f in fused], dtype=np.int64), np.asarray([f[1] for f in fused], dtype=np.float64),
            np.asarray([sum(1 << l for l in f[2]) for f in fused], dtype=np.int32))


def lists_of_mask(mask: int) -> List[int]:
    return [l for l in range(HR_MAX_FUSE_LISTS) if (int(mask) >> l) & 1]
