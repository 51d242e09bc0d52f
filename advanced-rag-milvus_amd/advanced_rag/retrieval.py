"""Hybrid retrieval engine: dense + sparse (+ optional domain) search, RRF
fusion, MMR, rerank — the reference's HybridRetriever surface on top of the
HBM shard store.

Behavioural source: reference src/advanced_rag/retrieval.py
  QueryClassifier            :22-67      RetrievalConfig          :70-101
  profiles                   :142-213    retrieve (timeout)       :215-247
  _retrieve_inner            :249-339    _search_*                :341-419
  _fuse_results (RRF k=60)   :421-491    _mmr_diversify           :493-516
  rerank                     :518-563    _build_filter_expression :565-632
  CrossEncoderReranker       :651-681
Where the index manager is the HBM one, the rank fusion runs in the HIP kernel
(csrc/fuse.h) through `index_manager.fuse_rank_lists`; for any other duck-typed
manager (the reference's test fakes) the same arithmetic runs on the host.
"""
from __future__ import annotations

import asyncio
import logging
import math
import re
from dataclasses import dataclass
from datetime import datetime
from typing import Any, Callable, Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from .decay import decay_rerank
from ._native import (HR_MAX_TOPK, HR_NORM_ATAN, HR_NORM_ATAN_DIST, HR_NORM_COSINE, HR_NORM_MINMAX,   # importing the
                      HR_NORM_MINMAX_DIST)                        # binding module does not load the library
from .constants import RetrievalConstants
from .ranker import LearnedRanker

logger = logging.getLogger(__name__)

_TROUBLE_WORDS = ("error", "exception", "stack trace", "failed", "failure", "bug")
_SUMMARY_WORDS = ("summarize", "summary", "tl;dr", "overview")
_METHOD_ORDER = ("semantic", "sparse", "domain")
FUSED_GROUP_FIELDS = ("doc_id", "chunk_index", "timestamp", "id", "chunk_id")   # what a hit dict shows of the groupable fields
FUSION_MODES = ("rrf", "weighted")
SCORE_NORMALIZATIONS = ("activation", "minmax")
_METHODS_OF_MASK = tuple(tuple(m for b, m in enumerate(_METHOD_ORDER) if (mask >> b) & 1) for mask in range(8))


class QueryClassifier:
    """Substring rules -> retrieval profile name (checked in this order:
    troubleshooting, summary, faq, analysis, default)."""

    def __init__(self, max_faq_len: int = 80, long_query_len: int = 200):
        self.max_faq_len = max_faq_len
        self.long_query_len = long_query_len

    def classify(self, query: str) -> str:
        text = (query or "").strip()
        if not text:
            return "default"
        low = text.lower()
        if any(w in low for w in _TROUBLE_WORDS):
            return "troubleshooting"
        if any(w in low for w in _SUMMARY_WORDS):
            return "summary"
        if text.endswith("?") and len(text) <= self.max_faq_len:
            return "faq"
        if len(text) >= self.long_query_len:
            return "analysis"
        return "default"


@dataclass
class RetrievalConfig:
    # carried around but unused by the fusion math (as in the reference) — also by fusion="weighted", whose weights are
    # dense_weight / sparse_weight as for RRF
    hybrid_alpha: float = 0.7
    top_k: int = 20
    rerank_top_k: int = 5
    enable_reranking: bool = True
    dense_weight: float = 0.7
    sparse_weight: float = 0.3
    enable_mmr: bool = False
    mmr_lambda: float = 0.7
    enable_learned_ranker: bool = False
    semantic_search_params: Optional[Dict] = None
    sparse_search_params: Optional[Dict] = None
    # grouping search (pymilvus' group_by_field): every modality ranks the best chunk of each group (2 x top_k documents
    # instead of 2 x top_k chunks) and the fused list keeps the first hit of every group.  None = chunks, as the reference.
    group_by_field: Optional[str] = None
    # with group_by_field: up to group_size chunks of every group in every modality list and in the fused list (pymilvus'
    # group_size; needs an index manager created with group_members=True, and 2 * top_k * group_size <= 256)
    group_size: int = 1
    # the dict form of a filter also takes {"field": {"$in": [...]}} and {"$nin": [...]} (-> `field in [..]` / `field not in
    # [..]`).  False = they are refused, as the reference refuses them.
    extended_filter_operators: bool = False
    # how the modality lists are fused: "rrf" (reciprocal-rank fusion, the reference's) or "weighted" (Milvus'
    # WeightedRanker: every list's scores normalised into [0, 1], then their weighted sum — score_fuse_lists below)
    fusion: str = "rrf"
    # with fusion="weighted": "activation" normalises by the list's metric (COSINE (1 + s) / 2, IP 0.5 + atan(s) / pi, L2
    # 1 - 2 atan(s) / pi), "minmax" by the smallest and largest score of each list
    score_normalization: str = "activation"
    # decay ranker (decay.DecayRanker) over the WHOLE fused list, right after the fusion and before the group pass, MMR and
    # the cut: score = fused score x decay(|field - origin|), "fused_score" keeps the fusion's.  RRF and weighted fused
    # scores are not renormalised: normalization="activation" means identity on a fused list, "minmax" rescales by the
    # list's smallest and largest fused score.  `candidates` is not used here (the whole fused list is the window).
    decay: Optional[Any] = None
    # what enable_mmr diversifies on: "tokens" (the reference's token-Jaccard of the contents) or "embedding" (vector MMR: the
    # cosine of the hits' stored semantic_index vectors, mmr.py; such a request takes the general path)
    mmr_similarity: str = "tokens"
    # boost ranker (boost.FunctionScore, or a bare boost.BoostRanker) over the WHOLE fused list, right after the fusion and
    # BEFORE the decay ranker (both may be set), the group pass, MMR and the cut: score = fused score (x or +) the combined
    # weight of the functions whose filter the hit's row matches, "fused_score" keeps the fusion's.  On a fused list
    # "none" and "activation" mean identity, "minmax" rescales by the list's extremes; the order is descending.
    # `candidates` is not used here (the whole fused list is the window).
    boost: Optional[Any] = None
    # late interaction (ColBERT-style MaxSim, maxsim.py): the WHOLE fused list is re-scored by the rows' stored token vectors
    # against the query's token vectors (embedding_generator.encode_token_vectors([query])) — after the boost and the decay
    # ranker, before the group pass, MMR and the cut; "fused_score" keeps the fusion's.  Takes the general path; needs an index
    # manager created with token_dim and a generator with that hook (ValueError otherwise).
    late_interaction: bool = False

    def __post_init__(self):
        if self.boost is not None:
            from .boost import BoostRanker, FunctionScore
            if not isinstance(self.boost, (BoostRanker, FunctionScore)):
                raise ValueError(f"boost must be a FunctionScore, a BoostRanker or None, got {self.boost!r}")
        if self.mmr_similarity not in ("tokens", "embedding"):
            raise ValueError(f"mmr_similarity must be 'tokens' or 'embedding', got {self.mmr_similarity!r}")
        if self.decay is not None:
            from .decay import DecayRanker
            if not isinstance(self.decay, DecayRanker):
                raise ValueError(f"decay must be a DecayRanker or None, got {self.decay!r}")
        if self.fusion not in FUSION_MODES:
            raise ValueError(f"fusion must be one of {', '.join(FUSION_MODES)}, got {self.fusion!r}")
        if self.score_normalization not in SCORE_NORMALIZATIONS:
            raise ValueError(f"score_normalization must be one of {', '.join(SCORE_NORMALIZATIONS)}, "
                             f"got {self.score_normalization!r}")
        if self.group_by_field is not None:
            # refused here, once: inside retrieve() a modality whose search raises degrades to "no hits".  token_count can be
            # grouped on by search(), but a hit does not show it, so the fused list could not be deduplicated on it
            from .columns import check_group_field
            if not isinstance(self.group_by_field, str):
                raise ValueError(f"unknown group_by_field: {self.group_by_field!r}")
            if check_group_field(self.group_by_field) not in FUSED_GROUP_FIELDS:
                raise ValueError(f"group_by_field {self.group_by_field!r} is not shown by a hit: retrieve() groups on one of "
                                 f"{', '.join(FUSED_GROUP_FIELDS)}")
        if isinstance(self.group_size, bool) or not isinstance(self.group_size, int) or self.group_size < 1:
            raise ValueError(f"group_size must be an integer >= 1, got {self.group_size!r}")
        if self.group_size > 1 and self.group_by_field is None:
            raise ValueError(f"group_size={self.group_size} needs group_by_field")
        if self.semantic_search_params is None:
            self.semantic_search_params = {"metric_type": "COSINE", "params": {"ef": 64}}
        if self.sparse_search_params is None:
            self.sparse_search_params = {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}


def rrf_rank_lists(lists: Sequence[Sequence[Any]], weights: Sequence[float], rrf_k: int = 60):
    """Host RRF over ranked id lists: returns [(id, float64 score, [list indices])] in
    fused order.  Same arithmetic and ordering as the HIP kernel."""
    table: Dict[Any, List] = {}
    for li, (ids, w) in enumerate(zip(lists, weights)):
        for rank, doc_id in enumerate(ids, start=1):
            ent = table.get(doc_id)
            if ent is None:
                ent = table[doc_id] = [0.0, []]
            ent[0] += (1.0 / (rrf_k + rank)) * w
            ent[1].append(li)
    fused = [(doc_id, ent[0], ent[1]) for doc_id, ent in table.items()]
    fused.sort(key=lambda t: t[1], reverse=True)  # stable: ties keep first-seen order
    return fused


_PI = float.fromhex("0x1.921fb54442d18p+1")         # 0x400921FB54442D18
_HALF_PI = float.fromhex("0x1.921fb54442d18p+0")    # 0x3FF921FB54442D18
_ATAN_SERIES = tuple((-1.0 if i & 1 else 1.0) * (1.0 / (2 * i + 1)) for i in range(12))


def canonical_atan(x: float) -> float:
    """The arctangent of the weighted score fusion: no table, no library call, every step one IEEE fp64 operation
    (Python floats; math.sqrt is correctly rounded), so that this function and the HIP kernel (csrc/fuse.h) give the same
    bits.  |x| > 1 is inverted, three half-angle steps, a 12-term series.  Within a few ulp of math.atan."""
    x = float(x)
    a = abs(x)
    inv = a > 1.0
    if inv:
        a = 1.0 / a
    for _ in range(3):
        a = a / (1.0 + math.sqrt(1.0 + a * a))
    t = a * a
    p = _ATAN_SERIES[11]
    for i in range(10, -1, -1):
        p = _ATAN_SERIES[i] + t * p
    r = 8.0 * (a * p)
    if inv:
        r = _HALF_PI - r
    return math.copysign(r, x)


def norm_code(metric: str, normalization: str = "activation") -> int:
    """HR_NORM_* of a list ranked by `metric` ("COSINE", "IP" — also what sparse_index ranks by — or "L2")."""
    dist = str(metric).upper() == "L2"
    if normalization == "minmax":
        return HR_NORM_MINMAX_DIST if dist else HR_NORM_MINMAX
    if normalization != "activation":
        raise ValueError(f"score_normalization must be one of {', '.join(SCORE_NORMALIZATIONS)}, got {normalization!r}")
    return HR_NORM_ATAN_DIST if dist else HR_NORM_COSINE if str(metric).upper() == "COSINE" else HR_NORM_ATAN


def normalise_scores(scores: Sequence[float], code: int, atan: Callable[[float], float] = canonical_atan,
                     widened: bool = False) -> List[float]:
    """One list's scores -> [0, 1] values by the table of include/hbmrag.h (every operation rounded on its own).
    widened: the scores are doubles already (fp32 scores widened by the caller, or the fp64 scores of a fused list: the
    decay ranker's) and are taken as they are."""
    # the lists hold fp32 scores: widened, never rounded again
    s = [float(x) for x in scores] if widened else [float(np.float32(x)) for x in scores]
    if code == HR_NORM_COSINE:
        return [(1.0 + v) * 0.5 for v in s]
    if code == HR_NORM_ATAN:
        return [0.5 + atan(v) / _PI for v in s]
    if code == HR_NORM_ATAN_DIST:
        return [1.0 - (2.0 * atan(v)) / _PI for v in s]
    if code not in (HR_NORM_MINMAX, HR_NORM_MINMAX_DIST):
        raise ValueError(f"norm code {code!r} is not one of HR_NORM_*")
    if not s:
        return []
    lo, hi = min(s), max(s)
    if hi == lo:
        return [1.0] * len(s)
    return [(v - lo) / (hi - lo) for v in s] if code == HR_NORM_MINMAX else [(hi - v) / (hi - lo) for v in s]


def score_fuse_lists(lists: Sequence[Tuple[Sequence[Any], Sequence[float]]], weights: Sequence[float],
                     norms: Sequence[int], atan: Callable[[float], float] = canonical_atan):
    """Host weighted score fusion over ranked (ids, fp32 scores) lists: returns [(id, float64 score, [list indices])]
    in fused order.  Same arithmetic and ordering as the HIP kernel: score[id] = 0.0, then += n * w (multiply, then add)
    for every list that holds the id, lists in the order given; the stable descending sort keeps first-seen order."""
    table: Dict[Any, List] = {}
    for li, ((ids, scores), w, code) in enumerate(zip(lists, weights, norms)):
        for doc_id, n in zip(ids, normalise_scores(scores, code, atan)):
            ent = table.get(doc_id)
            if ent is None:
                ent = table[doc_id] = [0.0, []]
            ent[0] += n * w
            ent[1].append(li)
    fused = [(doc_id, ent[0], ent[1]) for doc_id, ent in table.items()]
    fused.sort(key=lambda t: t[1], reverse=True)  # stable: ties keep first-seen order
    return fused


class HybridRetriever:
    ALLOWED_FILTER_FIELDS: Set[str] = {"doc_id", "chunk_id", "domain_density", "timestamp", "entropy", "redundancy",
                                       "chunk_index", "token_count"}
    ALLOWED_OPERATORS: Set[str] = {"$gte", "$lte", "$gt", "$lt", "$eq", "$ne"}
    _OP_TEXT = {"$gte": ">=", "$lte": "<=", "$gt": ">", "$lt": "<", "$eq": "==", "$ne": "!="}
    _LIST_OP_TEXT = {"$in": "in", "$nin": "not in"}      # only with RetrievalConfig(extended_filter_operators=True)
    DOMAIN_WEIGHT = 0.2
    RRF_K = 60

    def __init__(self, index_manager, config: Optional[RetrievalConfig] = None,
                 weight_adapter: Optional[Callable[[str], Tuple[float, float]]] = None,
                 classifier: Optional[QueryClassifier] = None,
                 profiles: Optional[Dict[str, RetrievalConfig]] = None,
                 learned_ranker: Optional[LearnedRanker] = None):
        self.index_manager = index_manager
        self.config = config or RetrievalConfig()
        self.weight_adapter = weight_adapter
        self.classifier = classifier or QueryClassifier()
        self.profiles: Dict[str, RetrievalConfig] = profiles or self._build_default_profiles(self.config)
        self.reranker = None
        self.learned_ranker: Optional[LearnedRanker] = learned_ranker

    # ------------------------------------------------------------------ profiles
    @staticmethod
    def _build_default_profiles(base: RetrievalConfig) -> Dict[str, RetrievalConfig]:
        cap = getattr(RetrievalConstants, "MAX_TOP_K", None)

        def clamp_k(v: int) -> int:
            v = int(v)
            return max(1, min(v, cap if cap is not None else v))

        def clamp_rerank(v: int) -> int:
            return max(1, min(int(v), clamp_k(v)))

        def derive(top_k: int, rerank_k: int, rerank: bool, mmr: bool, lam: float) -> RetrievalConfig:
            return RetrievalConfig(hybrid_alpha=base.hybrid_alpha, top_k=clamp_k(top_k),
                                   rerank_top_k=clamp_rerank(rerank_k), enable_reranking=rerank,
                                   dense_weight=base.dense_weight, sparse_weight=base.sparse_weight,
                                   enable_mmr=mmr, mmr_lambda=lam, group_by_field=base.group_by_field,
                                   group_size=base.group_size,
                                   extended_filter_operators=base.extended_filter_operators,
                                   fusion=base.fusion, score_normalization=base.score_normalization, decay=base.decay, boost=base.boost,
                                   mmr_similarity=base.mmr_similarity, late_interaction=base.late_interaction)

        return {
            "default": base,
            "faq": derive(min(base.top_k, 10), base.rerank_top_k, True, False, 0.7),
            "troubleshooting": derive(max(base.top_k, 30), 10, True, True, 0.5),
            "summary": derive(max(base.top_k, 40), 10, False, False, 0.7),
            "analysis": derive(max(base.top_k, 30), 10, True, True, 0.8),
        }

    def _pick_profile(self, query: str, hint: Optional[str]) -> str:
        try:
            if hint and hint in self.profiles:
                return hint
            if self.classifier:
                return self.classifier.classify(query) or "default"
        except Exception:
            pass
        return "default"

    # ------------------------------------------------------------------ retrieve
    async def retrieve(self, query: str, filters: Optional[Dict[str, Any]] = None, use_domain_index: bool = False,
                       domain: Optional[str] = None, profile_hint: Optional[str] = None) -> List[Dict[str, Any]]:
        budget = float(getattr(RetrievalConstants, "TIMEOUT_SECONDS", 0.3))
        try:
            return await asyncio.wait_for(
                self._retrieve_inner(query=query, filters=filters, use_domain_index=use_domain_index, domain=domain,
                                     profile_hint=profile_hint), timeout=budget)
        except asyncio.TimeoutError:
            logger.warning("HybridRetriever.retrieve timed out after %.3f seconds", budget)
            return []

    async def _retrieve_inner(self, query: str, filters: Optional[Dict[str, Any]] = None,
                              use_domain_index: bool = False, domain: Optional[str] = None,
                              profile_hint: Optional[str] = None) -> List[Dict[str, Any]]:
        profile = self._pick_profile(query, profile_hint)
        # The active profile becomes self.config for this request (and stays so
        # afterwards) exactly as reference retrieval.py:281-284 does.
        self.config = self.profiles.get(profile, self.config)
        if self.config.group_size > 1 and 2 * self.config.top_k * self.config.group_size > HR_MAX_TOPK:
            # refused here: inside the searches a modality that raises degrades to "no hits"
            raise ValueError(f"retrieve() with group_size={self.config.group_size} searches 2 * top_k groups per modality: "
                             f"2 * top_k * group_size <= {HR_MAX_TOPK}, got 2 * {self.config.top_k} * {self.config.group_size}")

        dense_q = await self._get_semantic_embedding(query)
        sparse_q = await self._get_sparse_embedding(query)
        expr = self._build_filter_expression(filters) if filters else None
        query_tokens = await self._get_query_tokens(query) if self.config.late_interaction else None

        fused = await self._retrieve_one_round(query, dense_q, sparse_q, expr) if not (use_domain_index and domain) else None
        if fused is not None:
            return self._tag_profile(fused, profile)[:self.config.top_k]

        searches = [self._search_semantic(dense_q, expr), self._search_sparse(sparse_q, expr)]
        if use_domain_index and domain:
            domain_q = await self._get_domain_embedding(query, domain)
            searches.append(self._search_domain(domain_q, expr))
        hit_lists = await asyncio.gather(*searches)

        self._adapt_weights(query)
        fused = await self._fuse_results_async(hit_lists[0], hit_lists[1], hit_lists[2] if len(hit_lists) > 2 else [],
                                               **({"query_tokens": query_tokens} if query_tokens is not None else {}))
        return self._tag_profile(fused, profile)[:self.config.top_k]

    async def _get_query_tokens(self, query: str):
        """The query's token vectors for the late-interaction rerank: embedding_generator.encode_token_vectors([query])
        -> (indptr, values), one row.  ValueError when the manager or the generator cannot serve it."""
        mgr = self.index_manager
        gen = getattr(mgr, "embedding_generator", None)
        if getattr(mgr, "maxsim_rerank_lists_async", None) is None or getattr(mgr, "token_dim", None) is None:
            raise ValueError("RetrievalConfig(late_interaction=True) needs an index manager created with token_dim=...")
        if gen is None or not hasattr(gen, "encode_token_vectors"):
            raise ValueError("RetrievalConfig(late_interaction=True) needs an embedding generator with encode_token_vectors")
        indptr, values = await mgr._run_encoder(gen.encode_token_vectors, [query])
        indptr = np.asarray(indptr, dtype=np.int64)
        return mgr._check_query_tokens(np.asarray(values)[int(indptr[0]): int(indptr[1])])

    # ------------------------------------------------------------------ several wordings, one ranking
    MAX_WORDINGS = 8

    async def retrieve_multi(self, queries: Sequence[str], filters: Optional[Dict[str, Any]] = None,
                             profile_hint: Optional[str] = None,
                             query_weights: Optional[Sequence[float]] = None) -> List[Dict[str, Any]]:
        """RAG-fusion: 1 .. 8 wordings of one question, fused into ONE ranking.  The profile is picked from queries[0]; every
        wording is embedded once and searched on semantic_index and sparse_index at 2 * top_k (<= HR_MAX_TOPK); the lists
        are fused in the order sem_0, spa_0, sem_1, spa_1, ... with weights dense_weight * qw_i and sparse_weight * qw_i
        (query_weights, default 1.0) by config.fusion — through the manager's `fuse_lists_async` (hr_fuse_lists_dev) where it
        has one, else by the restatements — and cut to 3 * HR_MAX_TOPK entries.  Then retrieve()'s tail: the decay ranker,
        the group pass, MMR and the cut.  A hit's `retrieval_methods` is the ordered set of modalities of the lists that
        hold it, `queries` the wordings that found it.  One wording gives what retrieve() of it gives.  The timeout and the
        "a failing modality degrades to no hits" rule are retrieve()'s."""
        if isinstance(queries, str) or not isinstance(queries, (list, tuple)) or not 1 <= len(queries) <= self.MAX_WORDINGS:
            raise ValueError(f"retrieve_multi takes a list of 1 .. {self.MAX_WORDINGS} queries, got {queries!r}")
        if not all(isinstance(q, str) for q in queries):
            raise ValueError("every query must be a string")
        qw = [1.0] * len(queries) if query_weights is None else list(query_weights)
        if len(qw) != len(queries):
            raise ValueError(f"{len(qw)} query_weights for {len(queries)} queries")
        for w in qw:
            if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w):
                raise ValueError(f"a query weight must be a finite number, got {w!r}")
        budget = float(getattr(RetrievalConstants, "TIMEOUT_SECONDS", 0.3))
        try:
            return await asyncio.wait_for(self._retrieve_multi_inner(list(queries), filters, profile_hint, [float(w) for w in qw]),
                                          timeout=budget)
        except asyncio.TimeoutError:
            logger.warning("HybridRetriever.retrieve_multi timed out after %.3f seconds", budget)
            return []

    async def _retrieve_multi_inner(self, queries, filters, profile_hint, qw) -> List[Dict[str, Any]]:
        profile = self._pick_profile(queries[0], profile_hint)
        self.config = self.profiles.get(profile, self.config)
        cfg = self.config
        if 2 * cfg.top_k * cfg.group_size > HR_MAX_TOPK:
            raise ValueError(f"retrieve_multi searches 2 * top_k rows per list: 2 * top_k * group_size <= {HR_MAX_TOPK}, "
                             f"got 2 * {cfg.top_k} * {cfg.group_size}")
        embedded = [(await self._get_semantic_embedding(q), await self._get_sparse_embedding(q)) for q in queries]
        expr = self._build_filter_expression(filters) if filters else None
        lists = await asyncio.gather(*[s for d, p in embedded for s in (self._search_semantic(d, expr), self._search_sparse(p, expr))])
        self._adapt_weights(queries[0])
        weights = [w * q for q in qw for w in (cfg.dense_weight, cfg.sparse_weight)]
        ranked = await self._rank_fusion_multi(lists, weights)
        # payload of an id: its first semantic hit, else its first sparse hit (one wording: exactly retrieve()'s choice)
        by_modality = [[], [], []]
        found: Dict[Any, List[str]] = {}
        seen = (set(), set())
        for l, hits in enumerate(lists):
            for hit in hits:
                if hit["id"] not in seen[l % 2]:
                    seen[l % 2].add(hit["id"])
                    by_modality[l % 2].append(hit)
        for doc_id, _, seen_in in ranked:
            found[doc_id] = [queries[i] for i in sorted({l // 2 for l in seen_in})]
        ranked = [(doc_id, score, sorted({l % 2 for l in seen_in})) for doc_id, score, seen_in in ranked]
        fused = await self._finish_ranked_async(by_modality, ranked)
        for hit in fused:
            hit["queries"] = found[hit["id"]]
        return self._tag_profile(fused, profile)[:cfg.top_k]

    async def _rank_fusion_multi(self, hit_lists, weights):
        """-> [(id, float64 score, [list indices])] in fused order, at most 3 * HR_MAX_TOPK entries."""
        cut = 3 * HR_MAX_TOPK
        weighted = self.config.fusion == "weighted"
        norms = [self._list_norms()[l % 2] for l in range(len(hit_lists))] if weighted else None
        id_lists = [[h["id"] for h in hits] for hits in hit_lists]
        score_lists = [[h["score"] for h in hits] for hits in hit_lists]
        device_fuse = getattr(self.index_manager, "fuse_lists_async", None)
        rows = [[h.get("_row") for h in hits] for hits in hit_lists]
        if device_fuse is not None and all(r is not None for lst in rows for r in lst) and any(rows):
            try:
                row_to_id = {r: i for rs, ids in zip(rows, id_lists) for r, i in zip(rs, ids)}
                f_rows, f_scores, f_masks = await device_fuse(rows, score_lists, weights, mode="weighted" if weighted else "rrf",
                                                              norms=norms, rrf_k=self.RRF_K)
                return [(row_to_id[int(r)], float(s), [l for l in range(len(hit_lists)) if (int(m) >> l) & 1])
                        for r, s, m in zip(f_rows, f_scores, f_masks)]
            except Exception:  # pragma: no cover - fall through to the host arithmetic
                logger.exception("device multi-list fusion failed; using host arithmetic")
        if weighted:
            return score_fuse_lists(list(zip(id_lists, score_lists)), weights, norms)[:cut]
        return rrf_rank_lists(id_lists, weights, self.RRF_K)[:cut]

    def _adapt_weights(self, query: str) -> None:
        if self.weight_adapter:
            try:
                dw, sw = self.weight_adapter(query)
                dw = min(1.0, max(0.0, float(dw)))
                sw = min(1.0, max(0.0, float(sw)))
                if dw + sw > 0:
                    self.config.dense_weight, self.config.sparse_weight = dw, sw
            except Exception:
                pass

    @staticmethod
    def _tag_profile(fused: List[Dict[str, Any]], profile: str) -> List[Dict[str, Any]]:
        for hit in fused:
            meta = hit.get("metadata")
            if isinstance(meta, dict):
                meta.setdefault("retrieval_profile", profile)
            else:
                hit["retrieval_profile"] = profile
        return fused

    async def _retrieve_one_round(self, query: str, dense_q, sparse_q, expr: Optional[str]) -> Optional[List[Dict[str, Any]]]:
        """Both searches and their rank fusion as ONE request to an index manager that offers `hybrid_search` (the HBM
        manager's batching front: one device round per retrieve() instead of two, and only the fused top_k hits are
        ever formatted).  Same lists, same arithmetic, same hit dicts as the general path below; None = take that path
        (a manager without the entry point; a request it declined; MMR, which needs the whole fused list, unless the
        manager diversifies on the device: `mmr_on_device`)."""
        one_round = getattr(self.index_manager, "hybrid_search", None)
        if self.config.group_by_field is not None:
            return None        # the one-round path does not group: the general path serves the request
        if self.config.late_interaction:
            return None        # the whole fused list is reranked behind the fusion: the general path
        if one_round is None or (self.config.enable_mmr and (not getattr(self.index_manager, "mmr_on_device", False)
                                                             or self.config.mmr_similarity == "embedding")):
            return None
        known = getattr(self.index_manager, "collections", None)
        if known is None or "sparse_index" not in known or "semantic_index" not in known:
            return None
        cfg = self.config
        extra = {"mmr_lambda": cfg.mmr_lambda} if cfg.enable_mmr else {}
        if cfg.fusion == "weighted":     # (a default config makes the call it always made)
            extra.update(fusion="weighted", norms=tuple(self._list_norms()[:2]))
        if cfg.decay is not None:
            extra.update(decay=cfg.decay)
        if cfg.boost is not None:
            extra.update(boost=cfg.boost)
        saved = (cfg.dense_weight, cfg.sparse_weight)
        self._adapt_weights(query)   # the adapter sees only the query: applying it before the searches changes nothing
        try:
            ranked = await one_round(dense_q, sparse_q, top_k=cfg.top_k, filters=expr,
                                     weights=(cfg.dense_weight, cfg.sparse_weight), rrf_k=self.RRF_K,
                                     semantic_params=cfg.semantic_search_params, sparse_params=cfg.sparse_search_params,
                                     **extra)
        except Exception:  # pragma: no cover - the general path owns the error behaviour
            logger.exception("one-round hybrid search failed; taking the general path")
            ranked = None
        if ranked is None:
            cfg.dense_weight, cfg.sparse_weight = saved   # the general path applies the adapter itself
            return None
        now = None
        fused = []
        for hit, score, mask in ranked:     # _finish_fused_hit, inlined for the 20 hits of every request
            hit["method"] = _METHOD_ORDER[0] if mask & 1 else _METHOD_ORDER[1]
            hit["original_score"] = hit["score"]
            hit.pop("_row", None)
            hit["score"] = score
            hit["retrieval_methods"] = list(_METHODS_OF_MASK[mask & 7])
            meta = hit.get("metadata")
            if isinstance(meta, dict) and meta.get("timestamp") and "recency" not in meta:
                now = now or datetime.utcnow()
                try:
                    age_days = max(0.0, (now - datetime.fromisoformat(str(meta["timestamp"]))).total_seconds() / 86400.0)
                    meta["recency"] = float(1.0 / (1.0 + age_days))
                except Exception:
                    pass
            fused.append(hit)
        return fused

    async def _tagged_search(self, method: str, embedding, collection: str, top_k: int, filters, params):
        group = {"group_by_field": self.config.group_by_field} if self.config.group_by_field is not None else {}
        if self.config.group_size > 1:
            group["group_size"] = self.config.group_size
        try:
            hits = await self.index_manager.search(query_embedding=embedding, collection_name=collection,
                                                   top_k=top_k, filters=filters, search_params=params, **group)
        except ValueError:
            if self.config.group_size > 1:
                raise      # a manager without group_members=True refuses the request: that is the caller's to see
            return []
        except Exception:
            return []  # a failing modality degrades to "no hits" (reference :355-358, :387-389, :411-413)
        for h in hits:
            h["method"] = method
            h["original_score"] = h["score"]
        return hits

    async def _search_semantic(self, embedding, filters: Optional[str]) -> List[Dict[str, Any]]:
        return await self._tagged_search("semantic", embedding, "semantic_index", self.config.top_k * 2, filters,
                                         self.config.semantic_search_params)

    async def _search_sparse(self, embedding, filters: Optional[str]) -> List[Dict[str, Any]]:
        known = getattr(self.index_manager, "collections", None)
        if known is not None and "sparse_index" not in known:
            return []
        return await self._tagged_search("sparse", embedding, "sparse_index", self.config.top_k * 2, filters,
                                         self.config.sparse_search_params)

    async def _search_domain(self, embedding, filters: Optional[str]) -> List[Dict[str, Any]]:
        return await self._tagged_search("domain", embedding, "domain_index", self.config.top_k, filters,
                                         self.config.semantic_search_params)

    # ------------------------------------------------------------------ fusion
    def _list_norms(self) -> List[int]:
        """HR_NORM_* of the semantic, sparse and domain lists for fusion="weighted": from the collections' metrics where the
        manager shows them, else from the request's search params (sparse_index ranks by IP)."""
        cfg = self.config
        known = getattr(self.index_manager, "collections", None)

        def metric(name: str) -> str:
            coll = known.get(name) if isinstance(known, dict) else None
            return getattr(coll, "metric", None) or (cfg.semantic_search_params or {}).get("metric_type", "COSINE")

        n = cfg.score_normalization
        return [norm_code(metric("semantic_index"), n), norm_code("IP", n), norm_code(metric("domain_index"), n)]

    def _rank_fusion(self, hit_lists: Sequence[List[Dict]], weights: Sequence[float]):
        """-> [(position_of_payload (list idx, rank idx), float64 score, [list indices])] in fused order."""
        id_lists = [[h["id"] for h in hits] for hits in hit_lists]
        if self.config.fusion == "weighted":
            norms, score_lists = self._list_norms(), [[h["score"] for h in hits] for hits in hit_lists]
            device_fuse = getattr(self.index_manager, "fuse_score_lists", None)
            rows = [[h.get("_row") for h in hits] for hits in hit_lists]
            if device_fuse is not None and all(r is not None for lst in rows for r in lst) and any(rows):
                try:
                    return device_fuse(rows, id_lists, score_lists, list(weights), norms)
                except Exception:  # pragma: no cover - fall through to the host arithmetic
                    logger.exception("device score fusion failed; using host arithmetic")
            return score_fuse_lists(list(zip(id_lists, score_lists)), weights, norms)
        device_fuse = getattr(self.index_manager, "fuse_rank_lists", None)
        if device_fuse is not None:
            rows = [[h.get("_row") for h in hits] for hits in hit_lists]
            if all(r is not None for lst in rows for r in lst) and any(rows):
                try:
                    return device_fuse(rows, id_lists, list(weights), self.RRF_K)
                except Exception:  # pragma: no cover - fall through to the host arithmetic
                    logger.exception("device rank fusion failed; using host arithmetic")
        return rrf_rank_lists(id_lists, weights, self.RRF_K)

    def _fuse_results(self, semantic_results: List[Dict], sparse_results: List[Dict],
                      domain_results: Optional[List[Dict]] = None) -> List[Dict[str, Any]]:
        hit_lists = [semantic_results or [], sparse_results or [], domain_results or []]
        weights = [self.config.dense_weight, self.config.sparse_weight, self.DOMAIN_WEIGHT]
        ranked = self._rank_fusion(hit_lists, weights)
        fused_of = None
        if self.config.boost is not None and ranked:
            device = self._boost_device("boost_rerank_lists")
            ranked, fused_of = self._decay_ranked(ranked, *device(*self._boost_inputs(hit_lists, ranked), self.config.boost))
        if self.config.decay is not None and ranked:
            rows, scores, values, operands, norm = self._decay_inputs(hit_lists, ranked)
            device = getattr(self.index_manager, "decay_rerank_lists", None)
            order = device(rows, scores, self.config.decay, operands) if device is not None and rows is not None else \
                decay_rerank(list(range(len(ranked))), scores, values, operands, norm, len(ranked))[::2]
            ranked, before = self._decay_ranked(ranked, *order)
            fused_of = before if fused_of is None else fused_of      # (the fusion's scores, not the boosted ones)
        return self._assemble_fused(hit_lists, ranked, fused_of)

    # ---- vector MMR (RetrievalConfig.mmr_similarity="embedding") ----
    def _mmr_embedding_host(self, fused):
        """Without a manager that holds the vectors every hit has the zero vector: all similarities are 0."""
        from .mmr import vector_mmr
        pos, _ = vector_mmr([float(h["score"]) for h in fused], np.zeros((len(fused), 1), dtype=np.float32),
                            self.config.mmr_lambda, self.config.top_k)
        return pos

    def _mmr_embedding(self, fused: List[Dict[str, Any]], rows) -> List[Dict[str, Any]]:
        select = getattr(self.index_manager, "mmr_select_lists", None)
        pos = select(rows, [float(h["score"]) for h in fused], self.config.mmr_lambda, self.config.top_k) \
            if select is not None else self._mmr_embedding_host(fused)
        return [fused[int(p)] for p in pos]

    async def _mmr_embedding_async(self, fused: List[Dict[str, Any]], rows) -> List[Dict[str, Any]]:
        select = getattr(self.index_manager, "mmr_select_lists_async", None)
        if select is None:
            return self._mmr_embedding(fused, rows)
        pos = await select(rows, [float(h["score"]) for h in fused], self.config.mmr_lambda, self.config.top_k)
        return [fused[int(p)] for p in pos]

    def _decay_inputs(self, hit_lists, ranked):
        """What the decay ranker takes for a fused list: (rows or None when a hit carries no row number, float64 fused scores,
        the field values as a hit's metadata shows them — for a manager that cannot look rows up —, operands, norm code)."""
        from .decay import DECAY_FIELDS, epoch_seconds
        spec = self.config.decay
        payload: Dict[Any, Dict] = {}
        for hits in hit_lists:
            for hit in hits:
                payload.setdefault(hit["id"], hit)
        rows = [payload[doc_id].get("_row") for doc_id, _, _ in ranked]
        values = []
        for doc_id, _, _ in ranked:
            v = (payload[doc_id].get("metadata") or {}).get(spec.field)
            if DECAY_FIELDS[spec.field] == "epoch":
                values.append(epoch_seconds(v))
            else:
                values.append(float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else float("nan"))
        return (rows if all(r is not None for r in rows) else None, [float(s) for _, s, _ in ranked], values, spec.operands(),
                spec.norm_code("IP", fused=True))

    def _boost_device(self, name: str):
        """The manager's boost rerank of a fused list.  The functions are filter expressions over the collection's rows: only
        a manager that holds the rows can say which hits match, so there is no stand-alone host form."""
        device = getattr(self.index_manager, name, None)
        if device is None:
            raise ValueError(f"RetrievalConfig(boost=...) needs an index manager with {name}")
        return device

    @staticmethod
    def _boost_inputs(hit_lists, ranked):
        """(rows, float64 fused scores) of a fused list for the manager's boost rerank."""
        payload: Dict[Any, Dict] = {}
        for hits in hit_lists:
            for hit in hits:
                payload.setdefault(hit["id"], hit)
        rows = [payload[doc_id].get("_row") for doc_id, _, _ in ranked]
        if any(r is None for r in rows):
            raise ValueError("RetrievalConfig(boost=...) needs hits that carry their row number")
        return rows, [float(s) for _, s, _ in ranked]

    @staticmethod
    def _decay_ranked(ranked, pos, final):
        """The fused ranking reordered by the decay ranker -> (ranked with the final scores, id -> fused score)."""
        fused_of = {doc_id: score for doc_id, score, _ in ranked}
        return [(ranked[int(p)][0], float(f), ranked[int(p)][2]) for p, f in zip(pos, final)], fused_of

    async def _fuse_results_async(self, semantic_results, sparse_results, domain_results=None, query_tokens=None) -> List[Dict[str, Any]]:
        """_fuse_results for a caller on the event loop: with the HBM index manager the rank fusion of concurrent
        retrieve() calls shares one device launch (index_manager.fuse_rank_lists_async); same arithmetic, same result."""
        hit_lists = [semantic_results or [], sparse_results or [], domain_results or []]
        weights = [self.config.dense_weight, self.config.sparse_weight, self.DOMAIN_WEIGHT]
        weighted = self.config.fusion == "weighted"
        device_fuse = getattr(self.index_manager, "fuse_score_lists_async" if weighted else "fuse_rank_lists_async", None)
        ranked = None
        if device_fuse is not None:
            rows = [[h.get("_row") for h in hits] for hits in hit_lists]
            if all(r is not None for lst in rows for r in lst) and any(rows):
                try:
                    id_lists = [[h["id"] for h in hits] for hits in hit_lists]
                    if weighted:
                        ranked = await device_fuse(rows, id_lists, [[h["score"] for h in hits] for hits in hit_lists],
                                                   list(weights), self._list_norms())
                    else:
                        ranked = await device_fuse(rows, id_lists, list(weights), self.RRF_K)
                except Exception:  # pragma: no cover - fall through to the host arithmetic
                    logger.exception("device rank fusion failed; using host arithmetic")
        if ranked is None:
            ranked = self._rank_fusion(hit_lists, weights)
        return await self._finish_ranked_async(hit_lists, ranked, **({"query_tokens": query_tokens} if query_tokens is not None else {}))

    async def _finish_ranked_async(self, hit_lists, ranked, query_tokens=None) -> List[Dict[str, Any]]:
        """What follows a rank fusion: the boost ranker, the decay ranker, the hit dicts, the group pass and MMR (the cut is
        the caller's)."""
        boosted_of = None
        if self.config.boost is not None and ranked:
            device = self._boost_device("boost_rerank_lists_async")
            ranked, boosted_of = self._decay_ranked(ranked, *await device(*self._boost_inputs(hit_lists, ranked), self.config.boost))
        if self.config.decay is not None and ranked:
            rows, scores, values, operands, norm = self._decay_inputs(hit_lists, ranked)
            device = getattr(self.index_manager, "decay_rerank_lists_async", None)
            if device is not None and rows is not None:
                order = await device(rows, scores, self.config.decay, operands)
            else:
                order = decay_rerank(list(range(len(ranked))), scores, values, operands, norm, len(ranked))[::2]
            ranked, fused_of = self._decay_ranked(ranked, *order)
            fused_of = fused_of if boosted_of is None else boosted_of      # (the fusion's scores, not the boosted ones)
        else:
            fused_of = boosted_of
        if query_tokens is not None and ranked:      # late interaction: S over the stored token vectors, whole list
            row_of: Dict[Any, Any] = {}
            for hits in hit_lists:
                for hit in hits:
                    row_of.setdefault(hit["id"], hit.get("_row"))      # (None: another manager's hit, no vectors, S = 0.0)
            rows = [row_of[doc_id] for doc_id, _, _ in ranked]
            pos, final = await self.index_manager.maxsim_rerank_lists_async(rows, query_tokens, len(ranked))
            ranked, before = self._decay_ranked(ranked, pos, final)
            fused_of = before if fused_of is None else fused_of      # (the fusion's scores)
        pending: List[Any] = []      # vector MMR: the rows of the fused hits, the selection goes through the manager's front
        fused = self._assemble_fused(hit_lists, ranked, fused_of, mmr_rows=pending)
        return await self._mmr_embedding_async(fused, pending) if pending else fused

    def _assemble_fused(self, hit_lists, ranked, fused_of: Optional[Dict[Any, float]] = None,
                        mmr_rows: Optional[List[Any]] = None) -> List[Dict[str, Any]]:
        # payload of an id = the hit from the semantic list if present (overwritten
        # by a later semantic duplicate), else the first sparse/domain hit
        payload: Dict[Any, Dict] = {}
        for hit in hit_lists[0]:
            payload[hit["id"]] = hit
        for hits in hit_lists[1:]:
            for hit in hits:
                payload.setdefault(hit["id"], hit)

        embedding = self.config.enable_mmr and self.config.mmr_similarity == "embedding"
        # the row numbers, before _finish_fused_hit pops them (None: another manager's hit, the zero vector)
        rows = [payload[doc_id].get("_row") for doc_id, _, _ in ranked] if embedding else None
        now = datetime.utcnow()
        fused = [self._finish_fused_hit(payload[doc_id], score, seen_in, now) for doc_id, score, seen_in in ranked]
        row_of = {id(hit): row for hit, row in zip(fused, rows)} if embedding else None
        if fused_of is not None:      # a decay ranker reordered the list: "score" is the final one, the fusion's is kept
            for hit, (doc_id, _, _) in zip(fused, ranked):
                hit["fused_score"] = fused_of[doc_id]
        if self.config.group_by_field is not None:
            fused = self._first_per_group(fused, self.config.group_by_field, self.config.group_size)
        if embedding and fused:
            rows = [row_of[id(hit)] for hit in fused]      # the group pass may have dropped hits
            if mmr_rows is not None:
                mmr_rows.extend(rows)
                return fused
            return self._mmr_embedding(fused, rows)
        if self.config.enable_mmr and fused:
            return self._mmr_diversify(fused, self.config.top_k, self.config.mmr_lambda)
        return fused

    @staticmethod
    def _first_per_group(fused: List[Dict[str, Any]], field: str, group_size: int = 1) -> List[Dict[str, Any]]:
        """The first group_size hits of every group, in fused order.  The modality lists are grouped already, but the fusion
        goes by chunk id: more chunks of one document can arrive from different modalities.  Before MMR and before the cut."""
        seen: Dict[Any, int] = {}
        out = []
        for hit in fused:
            key = hit["id"] if field in ("id", "chunk_id") else (hit.get("metadata") or {}).get(field)
            if key is None:            # another manager's hit without the field: a group of its own
                out.append(hit)
            elif seen.get(key, 0) < group_size:
                seen[key] = seen.get(key, 0) + 1
                out.append(hit)
        return out

    @staticmethod
    def _finish_fused_hit(hit: Dict[str, Any], score: float, seen_in, now) -> Dict[str, Any]:
        hit.pop("_row", None)  # manager-internal row number (device rank fusion); not part of the reference's hit dict
        hit["score"] = score
        hit["retrieval_methods"] = [m for i, m in enumerate(_METHOD_ORDER) if i in seen_in]
        meta = hit.get("metadata")
        if isinstance(meta, dict) and meta.get("timestamp") and "recency" not in meta:   # "" never parses: no recency
            try:
                age_days = max(0.0, (now - datetime.fromisoformat(str(meta["timestamp"]))).total_seconds() / 86400.0)
                meta["recency"] = float(1.0 / (1.0 + age_days))
            except Exception:
                pass
        return hit

    @staticmethod
    def _mmr_diversify(ranked: List[Dict[str, Any]], k: int, mmr_lambda: float) -> List[Dict[str, Any]]:
        """Greedy MMR on token-Jaccard similarity; the first strictly better candidate wins."""
        pool = [(r, set((r.get("content") or "").lower().split())) for r in ranked]
        chosen: List[Tuple[Dict[str, Any], set]] = []
        while pool and len(chosen) < k:
            best_i, best_val = None, -1e9
            for i, (r, toks) in enumerate(pool):
                if not chosen:
                    val = r["score"]
                else:
                    sim = max((len(toks & t2) / (len(toks | t2) or 1)) for _, t2 in chosen)
                    val = mmr_lambda * r["score"] - (1 - mmr_lambda) * sim
                if val > best_val:
                    best_i, best_val = i, val
            if best_i is None:  # every candidate scored <= -1e9; the reference would append None here
                break
            chosen.append(pool.pop(best_i))
        return [r for r, _ in chosen]

    # ------------------------------------------------------------------ rerank
    async def rerank(self, query: str, results: List[Dict[str, Any]], top_k: Optional[int] = None) -> List[Dict[str, Any]]:
        if not self.config.enable_reranking or not results:
            return results[:top_k] if top_k else results
        top_k = top_k or self.config.rerank_top_k
        if self.learned_ranker and self.config.enable_learned_ranker:
            new_scores = await self.learned_ranker.score(query, results)
        elif self.reranker:
            new_scores = await self.reranker.score([(query, r["content"]) for r in results])
        else:
            # the reference's placeholder: retrieval score + N(0, 0.01) (retrieval.py:549-553)
            # (one vector draw: the same values, in the same order, as a scalar draw per result from numpy's global stream)
            new_scores = [r["score"] + e for r, e in zip(results, np.random.normal(0, 0.01, len(results)).tolist())]
        for r, s in zip(results, new_scores):
            r["rerank_score"] = s
            r["original_retrieval_score"] = r["score"]
            r["score"] = s
        results.sort(key=lambda r: r["rerank_score"], reverse=True)
        return results[:top_k]

    # ------------------------------------------------------------------ filters
    @staticmethod
    def _quote(value: str) -> str:
        return '"' + value.replace("\\", "\\\\").replace('"', '\\"') + '"'

    @classmethod
    def _quote_list(cls, field: str, operand: Any) -> str:
        """["a", "b"] -> '["a", "b"]': a list of str, or of int / float / bool."""
        if not isinstance(operand, (list, tuple)):
            raise ValueError(f"Invalid value type for {field}: {type(operand)} (a list is expected)")
        if not (all(isinstance(v, str) for v in operand) or
                all(isinstance(v, (int, float, bool)) and not isinstance(v, str) for v in operand)):
            raise ValueError(f"Invalid list for {field}: its members must be all strings or all numbers")
        return "[" + ", ".join(cls._quote(v) if isinstance(v, str) else f"{v}" for v in operand) + "]"

    @classmethod
    def _text_match_term(cls, operand: Any) -> str:
        """{"content": {"$text_match": "disk failure"}} or {"$text_match": {"query": "...", "minimum_should_match": 2}}
        -> 'TEXT_MATCH(content, "disk failure"[, minimum_should_match=2])' (filters.py has the semantics)."""
        m = None
        if isinstance(operand, dict):
            if not set(operand) <= {"query", "minimum_should_match"} or "query" not in operand:
                raise ValueError(f"$text_match takes a string, or query and minimum_should_match, got {sorted(operand)}")
            operand, m = operand["query"], operand.get("minimum_should_match")
        if not isinstance(operand, str):
            raise ValueError(f"Invalid value type for content: {type(operand)}")
        if m is None:
            return f"TEXT_MATCH(content, {cls._quote(operand)})"
        if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= 16384:
            raise ValueError(f"minimum_should_match must be an integer from 1 to 16384, got {m!r}")
        return f"TEXT_MATCH(content, {cls._quote(operand)}, minimum_should_match={m})"

    def _build_filter_expression(self, filters: Dict[str, Any]) -> Optional[str]:
        """{"doc_id": "d1", "entropy": {"$gte": 0.2}} -> 'doc_id == "d1" and entropy >= 0.2'."""
        terms: List[str] = []
        for field, cond in filters.items():
            if (field == "content" and self.config.extended_filter_operators and isinstance(cond, dict)
                    and set(cond) == {"$text_match"}):
                terms.append(self._text_match_term(cond["$text_match"]))
                continue
            if field not in self.ALLOWED_FILTER_FIELDS:
                logger.warning("Invalid filter field attempted: %s", field)
                raise ValueError(f"Invalid filter field: {field}")
            if not re.match(r"^[a-zA-Z_][a-zA-Z0-9_]*$", field):
                raise ValueError(f"Invalid field name format: {field}")
            if isinstance(cond, dict):
                for op, operand in cond.items():
                    if op in self._LIST_OP_TEXT and self.config.extended_filter_operators:
                        terms.append(f"{field} {self._LIST_OP_TEXT[op]} {self._quote_list(field, operand)}")
                        continue
                    if op not in self.ALLOWED_OPERATORS:
                        logger.warning("Invalid operator attempted: %s", op)
                        raise ValueError(f"Invalid operator: {op}")
                    if not isinstance(operand, (int, float, str, bool)):
                        raise ValueError(f"Invalid value type for {field}: {type(operand)}")
                    rhs = self._quote(operand) if isinstance(operand, str) else f"{operand}"
                    terms.append(f"{field} {self._OP_TEXT[op]} {rhs}")
            elif isinstance(cond, str):
                terms.append(f"{field} == {self._quote(cond)}")
            elif isinstance(cond, (int, float, bool)):
                terms.append(f"{field} == {cond}")
            else:
                raise ValueError(f"Unsupported value type for {field}: {type(cond)}")
        return " and ".join(terms) if terms else None

    # ------------------------------------------------------------------ embeddings
    async def _get_semantic_embedding(self, text: str):
        return await self.index_manager._generate_semantic_embedding(text)

    async def _get_sparse_embedding(self, text: str):
        return await self.index_manager._generate_sparse_embedding(text)

    async def _get_domain_embedding(self, text: str, domain: str):
        return await self.index_manager._generate_domain_embedding(text, domain)


class CrossEncoderReranker:
    """Pair scorer plugged into HybridRetriever.reranker.  With `model` set
    (anything exposing predict(pairs) -> array, e.g. encoders.CrossEncoderModel)
    it scores with the model; without one it returns the reference's dummy
    0.5 + 0.1*N(0,1) scores (retrieval.py:680-681)."""

    def __init__(self, model_name: str = "cross-encoder/ms-marco-MiniLM-L-6-v2", model=None):
        self.model_name = model_name
        self.model = model

    async def score(self, pairs: List[tuple]) -> List[float]:
        if self.model:
            return np.asarray(self.model.predict(pairs)).tolist()
        return [0.5 + np.random.randn() * 0.1 for _ in pairs]
