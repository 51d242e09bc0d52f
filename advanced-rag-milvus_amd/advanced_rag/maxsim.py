"""Late-interaction rerank (ColBERT-style MaxSim): S = sum over query tokens of the best stored token's similarity, then
a stable descending sort.

The contract is the table in include/hbmrag.h (hr_maxsim_rerank_dev).  This module holds the spec object a caller passes
(`MaxSimRanker`) and the numpy restatement of the device kernel (csrc/maxsim.h): a float32 loop over k (an fp16 x fp16
product is exact in float32, so "float32 product, then one rounded float32 add" IS the fma chain of the contract), a
float64 sum over the query tokens, a stable sort.  Host and device agree bit for bit.

MaxSim as a first-stage search (hr_maxsim_scan_dev + hr_deep_topk_dev; manager.maxsim_search) is restated by
`maxsim_search_csr`: the same S, rounded once to float32, ranked by (score descending, row ascending)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from ._native import HR_MAX_QUERY_TOKENS, HR_MAX_TOKEN_DIM   # importing the binding module does not load the library


def check_token_dim(token_dim: Any) -> int:
    if isinstance(token_dim, bool) or not isinstance(token_dim, (int, np.integer)) or token_dim < 8 or token_dim % 8 \
            or token_dim > HR_MAX_TOKEN_DIM:
        raise ValueError(f"token_dim must be a multiple of 8 in 8..{HR_MAX_TOKEN_DIM}, got {token_dim!r}")
    return int(token_dim)


def as_fp16_tokens(what: str, values: Any, token_dim: Optional[int] = None) -> np.ndarray:
    """`values` -> C-contiguous float16 [n, dim]: numpy's astype(float16), round to nearest even (pinned: these are the
    stored bits).  ValueError for anything not 2-D, a wrong dim, or an element that is NaN / inf AS STORED in fp16 (a
    float32 beyond 65504 rounds to inf and is refused)."""
    a = np.asarray(values)
    if a.ndim != 2:
        raise ValueError(f"{what} must be a 2-D array [tokens, dim], got shape {a.shape}")
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{what} must be numeric, got dtype {a.dtype}")
    if token_dim is not None and a.shape[1] != token_dim:
        raise ValueError(f"{what} must have dim {token_dim}, got {a.shape[1]}")
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(a.astype(np.float16))
    if not np.isfinite(h).all():
        raise ValueError(f"{what} must be finite as stored in fp16 (NaN / inf, or a magnitude beyond 65504)")
    return h


@dataclass(frozen=True, eq=False)
class MaxSimRanker:
    """search(..., ranker=MaxSimRanker(query_tokens, candidates=None)).

    query_tokens   the query's token vectors [Tq, token_dim], 1 <= Tq <= 64; rounded to fp16 once, here
    candidates     rerank the best max(top_k, candidates) rows of the plain ranking instead of the best top_k
    """
    query_tokens: Any
    candidates: Optional[int] = None

    def __post_init__(self):
        h = as_fp16_tokens("query_tokens", self.query_tokens)
        if not 1 <= h.shape[0] <= HR_MAX_QUERY_TOKENS:
            raise ValueError(f"query_tokens must hold 1..{HR_MAX_QUERY_TOKENS} token vectors, got {h.shape[0]}")
        check_token_dim(h.shape[1])
        if self.candidates is not None and (isinstance(self.candidates, bool) or not isinstance(self.candidates, (int, np.integer))
                                            or self.candidates < 1):
            raise ValueError(f"candidates must be an integer >= 1 or None, got {self.candidates!r}")
        h.setflags(write=False)
        object.__setattr__(self, "query_tokens", h)

    def window(self, top_k: int) -> int:
        """W: how deep the plain ranking is read before the rerank."""
        return max(int(top_k), int(self.candidates or top_k))


def token_similarities(query_tokens: np.ndarray, doc_tokens: np.ndarray) -> np.ndarray:
    """s(t, u) for fp16 [Tq, dim] x fp16 [T, dim] -> float32 [Tq, T]: the k-ascending chain, one float32 product (exact)
    and one rounded float32 add per k."""
    q = np.asarray(query_tokens, dtype=np.float16).astype(np.float32)
    d = np.asarray(doc_tokens, dtype=np.float16).astype(np.float32)
    acc = np.zeros((q.shape[0], d.shape[0]), dtype=np.float32)
    for k in range(q.shape[1]):
        acc = acc + q[:, k, None] * d[None, :, k]   # float32 throughout
    return acc


def maxsim_score(query_tokens: np.ndarray, doc_tokens: Optional[np.ndarray]) -> float:
    """S of one row: float64 sum, in ascending t, of the per-token maxima; 0.0 for a row without tokens."""
    Tq = len(query_tokens)
    if doc_tokens is None or len(doc_tokens) == 0:
        m = np.zeros(Tq, dtype=np.float32)
    else:
        m = token_similarities(query_tokens, doc_tokens).max(axis=1)
    S = np.float64(0.0)
    for t in range(Tq):
        S = S + np.float64(m[t])
    return float(S)


def maxsim_scores(query_tokens: Any, doc_token_lists: Sequence[Optional[np.ndarray]]) -> List[float]:
    """S for every entry of doc_token_lists (fp16 [T_r, dim] each; None or an empty array = a row without tokens)."""
    q = np.asarray(query_tokens, dtype=np.float16)
    return [maxsim_score(q, d) for d in doc_token_lists]


def maxsim_rerank(ids: Sequence[int], query_tokens: Any, doc_token_lists: Sequence[Optional[np.ndarray]],
                  k_out: int) -> Tuple[List[int], List[int], List[float]]:
    """Host restatement of hr_maxsim_rerank_dev for ONE list: ids = the list's valid prefix, doc_token_lists[i] = the
    stored token vectors of ids[i] (None / empty where the row has none or lies outside the store).
    -> (positions, ids, scores) of the first k_out entries in the stable descending order of S."""
    S = maxsim_scores(query_tokens, doc_token_lists)
    order = sorted(range(len(ids)), key=lambda i: S[i], reverse=True)[:k_out]   # stable: ties keep input order
    return order, [int(ids[i]) for i in order], [S[i] for i in order]


def maxsim_scores_csr(query_tokens: Any, indptr: np.ndarray, values: np.ndarray, rows: Sequence[int]) -> np.ndarray:
    """S (float64 [len(rows)]) for rows of a CSR token store (indptr int64 [n_rows + 1], values fp16 [n_tok, dim]); a row
    outside [0, n_rows) has no tokens.  The same arithmetic as maxsim_scores, with the similarities of every needed
    token taken in one pass over k."""
    q = np.asarray(query_tokens, dtype=np.float16)
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n_rows = len(indptr) - 1
    ok = (rows >= 0) & (rows < n_rows)
    safe = np.where(ok, rows, 0)
    beg = np.where(ok, indptr[safe], 0) if n_rows > 0 else np.zeros(len(rows), dtype=np.int64)
    cnt = np.where(ok, indptr[safe + 1] - indptr[safe], 0) if n_rows > 0 else np.zeros(len(rows), dtype=np.int64)
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(cnt, out=off[1:])
    take = np.repeat(beg - off[:-1], cnt) + np.arange(off[-1], dtype=np.int64)
    m = np.zeros((len(rows), len(q)), dtype=np.float32)
    if off[-1] > 0:
        sims = token_similarities(q, np.asarray(values)[take])
        has = np.flatnonzero(cnt > 0)
        m[has] = np.maximum.reduceat(sims, off[:-1][has], axis=1).T
    S = np.zeros(len(rows), dtype=np.float64)
    for t in range(len(q)):
        S = S + m[:, t].astype(np.float64)
    return S


def maxsim_search_csr(query_tokens: Any, indptr: np.ndarray, values: np.ndarray, mask: Optional[np.ndarray], top_k: int,
                      offset: int = 0, first_row: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Host restatement of the first-stage MaxSim search (hr_maxsim_scan_dev, then hr_deep_topk_dev) over a CSR token store
    whose row 0 is global row first_row.  The hits are the rows that hold at least one token vector and pass the bool
    `mask` over local rows (None = all; rows beyond the mask do not pass); the score of a hit is np.float32(S), S rounded
    once; the ranking R is score descending, then row ascending.  -> (ids int64, scores float32) of R[offset : offset +
    top_k], shorter when R is."""
    indptr = np.asarray(indptr, dtype=np.int64)
    has = np.diff(indptr) > 0
    if mask is not None:
        m = np.asarray(mask, dtype=bool).reshape(-1)[:len(has)]
        has[:len(m)] &= m
        has[len(m):] = False
    rows = np.flatnonzero(has).astype(np.int64)
    scores = maxsim_scores_csr(query_tokens, indptr, values, rows).astype(np.float32)
    order = np.lexsort((rows, -scores))[int(offset): int(offset) + int(top_k)]   # S is finite and never -0.0: negation keeps the order
    return rows[order] + int(first_row), scores[order]


def maxsim_rerank_csr(ids: Sequence[int], query_tokens: Any, indptr: np.ndarray, values: np.ndarray, first_row: int,
                      k_out: int) -> Tuple[List[int], List[int], List[float]]:
    """maxsim_rerank over a CSR token store whose row 0 is global row first_row."""
    ids = [int(i) for i in ids]
    S = maxsim_scores_csr(query_tokens, indptr, values, [i - first_row for i in ids]).tolist()
    order = sorted(range(len(ids)), key=lambda i: S[i], reverse=True)[:k_out]
    return order, [ids[i] for i in order], [S[i] for i in order]
