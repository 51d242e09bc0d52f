"""Vector MMR: greedy maximal-marginal-relevance selection on the cosine of the STORED embeddings.

The contract is the table in include/hbmrag.h (hr_mmr_select_vec_dev).  This module holds the spec object a caller passes
(`MMRRanker`: what RAG stacks call max_marginal_relevance_search(k, fetch_k, lambda_mult)) and the pure-Python restatement
of the device kernel (csrc/mmr.h, mmr_select_vec_kernel): every operation one IEEE fp64 operation on Python floats or
numpy float64 arrays, so that host and device agree bit for bit."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._native import (HR_NORM_MINMAX, HR_NORM_MINMAX_DIST,
                      HR_NORM_NONE)   # importing the binding module does not load the library

MMR_NORMALIZATIONS = ("none", "activation", "minmax")
MMR_SIMILARITIES = ("tokens", "embedding")      # RetrievalConfig.mmr_similarity


@dataclass(frozen=True)
class MMRRanker:
    """search(..., ranker=MMRRanker(...)).

    lambda_mult    1.0 = relevance only (the plain ranking), 0.0 = diversity only; a finite number in [0, 1]
    candidates     diversify the best max(top_k, candidates) rows of the plain ranking (fetch_k) instead of the best top_k
    normalization  what the relevance term is: "none" (the raw score; refused on L2, where a smaller score is the better
                   one), "activation" (by the collection's metric) or "minmax"
    """
    lambda_mult: float = 0.5
    candidates: Optional[int] = None
    normalization: str = "none"

    def __post_init__(self):
        lam = self.lambda_mult
        if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not math.isfinite(float(lam)) or not 0.0 <= float(lam) <= 1.0:
            raise ValueError(f"lambda_mult must be a finite number in [0, 1], got {lam!r}")
        if self.candidates is not None and (isinstance(self.candidates, bool) or not isinstance(self.candidates, int)
                                            or self.candidates < 1):
            raise ValueError(f"candidates must be an integer >= 1 or None, got {self.candidates!r}")
        if not isinstance(self.normalization, str) or self.normalization not in MMR_NORMALIZATIONS:
            raise ValueError(f"normalization must be one of {', '.join(MMR_NORMALIZATIONS)}, got {self.normalization!r}")

    def window(self, top_k: int) -> int:
        """W: how deep the plain ranking is read before the selection."""
        return max(int(top_k), int(self.candidates or top_k))

    def norm_code(self, metric: str) -> int:
        """HR_NORM_* (or HR_NORM_NONE) for a list ranked by `metric`, as DecayRanker.norm_code maps it."""
        dist = str(metric).upper() == "L2"
        if self.normalization == "minmax":
            return HR_NORM_MINMAX_DIST if dist else HR_NORM_MINMAX
        if self.normalization == "none":
            if dist:
                raise ValueError("normalization='none' is refused on an L2 collection, where a smaller score is the better one")
            return HR_NORM_NONE
        from .retrieval import norm_code
        return norm_code(metric, "activation")


def _norm2(X: np.ndarray) -> np.ndarray:
    """The canonical fp64 sum of squares of every row (k-ordered): the store's norm2."""
    s = np.zeros(X.shape[0], dtype=np.float64)
    for k in range(X.shape[1]):
        s = s + X[:, k] * X[:, k]
    return s


def _cosine(A64: np.ndarray, NA: np.ndarray, B64: np.ndarray, NB: np.ndarray) -> np.ndarray:
    S = np.zeros((A64.shape[0], B64.shape[0]), dtype=np.float64)
    for k in range(A64.shape[1]):
        S = S + A64[:, k, None] * B64[None, :, k]       # fp32 x fp32 products are exact in fp64; one rounded add per k
    d = NA[:, None] * NB[None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = np.where(d > 0.0, S / np.sqrt(d), 0.0)
        return c.astype(np.float32).astype(np.float64)


def canonical_cosine(A, B) -> np.ndarray:
    """sim of include/hbmrag.h for every pair: float64 [n, m] (or [n] for a 1-D B) of (double)(float) c,
    c = d > 0 ? S / sqrt(d) : 0, S the k-ordered fp64 sum of the exact products A[i, k] * B[j, k], d = N_i * N_j with N the
    k-ordered fp64 sum of squares.  A / B: fp16 or fp32 rows (widened exactly)."""
    A = np.asarray(A)
    B = np.asarray(B)
    single = B.ndim == 1
    A64 = np.atleast_2d(A).astype(np.float64)
    B64 = np.atleast_2d(B).astype(np.float64)
    if A64.shape[1] != B64.shape[1]:
        raise ValueError(f"rows of {A64.shape[1]} and of {B64.shape[1]} elements")
    out = _cosine(A64, _norm2(A64), B64, _norm2(B64))
    return out[:, 0] if single else out


def relevance(scores: Sequence[float], norm: int) -> List[float]:
    """rel_i = n(s_i) as the kernel computes it: scores are doubles already (fp32 widened by the caller, or fp64); lo / hi
    by comparisons that a NaN never wins."""
    s = [float(x) for x in scores]
    if norm == HR_NORM_NONE:
        return s
    if norm not in (HR_NORM_MINMAX, HR_NORM_MINMAX_DIST):
        from .retrieval import normalise_scores
        return normalise_scores(s, norm, widened=True)
    lo, hi = math.inf, -math.inf
    for v in s:
        lo = v if v < lo else lo
        hi = v if v > hi else hi
    if hi == lo:
        return [1.0] * len(s)
    with np.errstate(invalid="ignore"):
        s64 = np.asarray(s, dtype=np.float64)      # numpy: inf - inf is NaN, not an exception
        out = (s64 - lo) / (hi - lo) if norm == HR_NORM_MINMAX else (hi - s64) / (hi - lo)
    return [float(x) for x in out]


def vector_mmr(scores: Sequence[float], vectors, lam: float, k_out: int, norm: int = HR_NORM_NONE,
               m_starts_at_zero: bool = False) -> Tuple[List[int], List[float]]:
    """Host restatement of hr_mmr_select_vec_dev for ONE list: scores = the list's valid prefix, vectors [n, dim] = the
    stored rows of its entries (a row of zeros for an id outside the collection).
    -> (list positions in pick order, val at the time of each pick); shorter than k_out when the list is, or when nobody
    qualifies (the device pads with -1 / 0.0).  m_starts_at_zero=True is the Jaccard kernel's rule (the running maximum
    starts at 0), kept only so that a test can show where the two differ."""
    rel = relevance(scores, norm)
    n = len(rel)
    V = np.asarray(vectors)
    if V.ndim != 2 or V.shape[0] != n:
        raise ValueError(f"vectors must be [{n}, dim], got {V.shape}")
    V = V.astype(np.float64)
    N = _norm2(V)
    lam = float(lam)
    one_minus = 1.0 - lam
    alive = [True] * n
    m = [0.0] * n
    pos: List[int] = []
    val: List[float] = []
    limit = min(int(k_out), n)
    while len(pos) < limit:
        best, bv = -1, 0.0
        for i in range(n):
            if not alive[i]:
                continue
            v = lam * rel[i] - one_minus * m[i] if pos else rel[i]
            if v > -1e9 and (best < 0 or v > bv):
                best, bv = i, v
        if best < 0:
            break
        alive[best] = False
        first = not pos
        pos.append(best)
        val.append(bv)
        if len(pos) >= limit:
            break
        sim = _cosine(V, N, V[best:best + 1], N[best:best + 1])[:, 0]
        for i in range(n):
            if alive[i]:
                c = float(sim[i])
                m[i] = c if ((first and not m_starts_at_zero) or c > m[i]) else m[i]
    return pos, val
