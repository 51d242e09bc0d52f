"""The range-search yardstick of the tests (no GPU): the result semantics of include/hbmrag.h restated in numpy, the
library's scan error bound and range bounds (prep_queries_kernel: hi_a, lo_a) restated in numpy, and the planted
"annulus" corpus the GPU tests search.

Semantics: a range search returns oracle.topk over the rows whose canonical fp32 score, widened to double, lies in the
range — COSINE / IP: radius < s <= range_filter; L2: range_filter <= D < radius.  Nothing new is asked of the oracle."""
import functools
import math

import numpy as np

import oracle
from l2_yardstick import l2_dist_np

IP, COSINE, L2 = 0, 1, 2          # HR_METRIC_*
INF = float("inf")


# ---- semantics ------------------------------------------------------------------------------------------------------
def fill(metric, radius, range_filter):
    """An absent side is unbounded: radius = -inf, range_filter = +inf for COSINE and IP, the opposite for L2."""
    if radius is None:
        radius = INF if metric == L2 else -INF
    if range_filter is None:
        range_filter = -INF if metric == L2 else INF
    return float(radius), float(range_filter)


def in_range(score32, metric, radius, range_filter):
    v = np.asarray(score32, np.float32).astype(np.float64)
    radius, range_filter = fill(metric, radius, range_filter)
    if metric == L2:
        return (range_filter <= v) & (v < radius)
    return (radius < v) & (v <= range_filter)


def scores(X, q, metric):
    """Canonical fp32 scores (distances for L2) of every row."""
    if metric == L2:
        return l2_dist_np(X, np.asarray(q, np.float32))
    return oracle.dense_scores(X, np.asarray(q, np.float32), metric)


def l2_dist_batch(X, Q):
    """l2_dist_np for a batch: the same k-ordered fp64 chain, vectorised over (query, row)."""
    XT = np.ascontiguousarray(X.astype(np.float64).T)              # [d, n]: one contiguous row per k
    QT = np.ascontiguousarray(np.atleast_2d(Q).astype(np.float64).T)
    s = np.zeros((QT.shape[1], XT.shape[1]))
    d = np.empty_like(s)
    for k in range(XT.shape[0]):
        np.subtract(XT[k][None, :], QT[k][:, None], out=d)
        np.multiply(d, d, out=d)
        s += d
    return s.astype(np.float32)


def topk_in_range(s, metric, k, radius, range_filter, mask=None, row_offset=0):
    """One query: (ids [k], scores [k]) of the best k rows among those in range (and in the mask)."""
    ok = in_range(s, metric, radius, range_filter)
    if mask is not None:
        ok &= np.asarray(mask, bool)
    ok = np.packbits(ok, bitorder="little")            # the oracle's row mask: bit r % 8 of byte r / 8
    if metric == L2:
        i, v = oracle.topk(-s, k, ok, False, row_offset)
        v = -v
        v[i < 0] = 0.0
        return i, v
    return oracle.topk(s, k, ok, False, row_offset)


def range_search(X, Q, k, metric, radius, range_filter, mask=None, score_rows=None):
    """ids [B, k], scores [B, k].  radius / range_filter: None, a number, or one entry per query (None entries allowed).
    score_rows: precomputed scores [B, n] (shared between tests)."""
    Q = np.atleast_2d(Q)
    B = Q.shape[0]
    per = lambda b, i: b[i] if isinstance(b, (list, tuple, np.ndarray)) else b  # noqa: E731
    ids = np.empty((B, k), np.int64)
    sc = np.empty((B, k), np.float32)
    for b in range(B):
        s = score_rows[b] if score_rows is not None else scores(X, Q[b], metric)
        ids[b], sc[b] = topk_in_range(s, metric, k, per(radius, b), per(range_filter, b), mask)
    return ids, sc


def bounds_arrays(metric, radius, range_filter, B):
    """Per-query bound lists -> the two float64 arrays the C ABI takes (None entries filled with the unbounded value)."""
    r = np.array([fill(metric, radius[b], range_filter[b])[0] for b in range(B)], np.float64)
    f = np.array([fill(metric, radius[b], range_filter[b])[1] for b in range(B)], np.float64)
    return r, f


# ---- the library's arithmetic, restated -----------------------------------------------------------------------------
def padded_dim(dim, f16):
    tile = 4 * (8 if f16 else 4)                       # elements of one 1 KiB tile along k
    kt = -(-dim // tile)
    return 4 * -(-kt // 4) * tile                      # KT rounded up to the scans' prefetch depth


def canonical_qn2(q):
    s = 0.0
    for x in np.asarray(q, np.float32).astype(np.float64):
        s = s + x * x
    return s


def max_row_norm(X):
    """The shard's largest row norm as the library keeps it: (float) sqrt of the k-ordered fp64 sum of squares."""
    X64 = X.astype(np.float64)
    s = np.zeros(X64.shape[0])
    for k in range(X64.shape[1]):
        s += X64[:, k] * X64[:, k]
    return np.float32(np.sqrt(s).astype(np.float32).max(initial=0))


def scan_eps(metric, f16, dim, M, qn2):
    """eps(q): the scans' bound on |a - t| (dense_eps, dense_l2_rt_eps, prep_queries_kernel), as a double."""
    unit = 2.0 * padded_dim(dim, f16) * 2.0 ** -24 + 1e-6
    unit += 2.0 ** -11 * 1.01 if f16 else 2.0 ** -22
    M = float(np.float32(M))
    if metric == COSINE:
        return float(np.float32(unit))
    if metric == IP:
        return float(np.float32(unit * M * 1.0001))
    eps_abs = np.float32((unit + 2.0 ** -24 * 1.01) * M * 1.0001)
    Mm = M * 1.0001
    rt = np.float32(min(2.0 ** -22 * 1.01 * 0.5 * Mm * Mm, 3.0e38))
    with np.errstate(over="ignore"):
        c = np.float32(1.0 / math.sqrt(qn2)) if qn2 > 0 else np.float32(1.0)
        e = np.float32(np.float32(rt * c) * np.float32(1.000001))
    if not e < np.float32(3.0e38):
        e = np.float32(np.inf)
    return float(eps_abs) + float(e)


def f32_up(x):
    """The smallest float32 >= x."""
    with np.errstate(over="ignore"):
        f = np.float32(x)
    if float(f) < x:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def f32_down(x):
    return -f32_up(-x)


def range_scan_bounds(metric, qn2, radius, range_filter, eps, M):
    """(hi_a, lo_a) of one query as prep_queries_kernel writes them (range_scan_bounds in csrc/dense.h).  In the scan's
    domain t (COSINE: the cosine; IP: S / |q|; L2: (|q|^2 - D) / (2 |q|)):
      hi_a >= t + eps for every row whose canonical score passes range_filter, lo_a < t - eps for every row whose
      canonical score passes radius.
    The slack between the canonical fp32 score and the exact value: the cast is one rounding to
    nearest, 2^-24 relative (2^-149 absolute below the normal range); the fp64 chain of at most 4096 terms is within 2^-40
    of the exact value relative to |x| |q| (COSINE: to 1; L2: to D, a sum of non-negative terms)."""
    hi, lo = np.float32(np.inf), np.float32(-np.inf)
    M = float(np.float32(M))
    if not qn2 > 0.0:
        return hi, lo
    nq = math.sqrt(qn2)
    c = 1.0 / nq
    with np.errstate(over="ignore", under="ignore"):
        cf = np.float32(c)
    if not (cf >= np.float32(2.0 ** -126) and cf < np.float32(np.inf)) or not eps < 3.0e38:
        return hi, lo
    with np.errstate(over="ignore", invalid="ignore"):
        if metric == COSINE:
            t_hi, t_lo = range_filter + 2.0 ** -23, radius - 2.0 ** -23
        elif metric == IP:
            sl = 2.0 ** -23 * M * nq * 1.0001 + 2.0 ** -149
            t_hi, t_lo = (range_filter + sl) * c, (radius - sl) * c
        else:
            d_lo = range_filter * (1.0 - 2.0 ** -23) - 2.0 ** -149
            d_hi = radius * (1.0 + 2.0 ** -23) + 2.0 ** -149 if radius > 0.0 else 0.0
            if not range_filter > 0.0:
                t_hi = INF
            else:
                d_lo = max(d_lo, 0.0)
                t_hi = (qn2 - d_lo) * 0.5 * c
                t_hi += 2.0 ** -39 * (qn2 + d_lo) * 0.5 * c
            t_lo = (qn2 - d_hi) * 0.5 * c
            t_lo -= 2.0 ** -39 * (qn2 + d_hi) * 0.5 * c
        t_hi += abs(t_hi) * 2.0 ** -40
        t_lo -= abs(t_lo) * 2.0 ** -40
        e = eps * (1.0 + 2.0 ** -20)
        return f32_up(t_hi + e), f32_down(t_lo - e)


def exact_t(X, q, metric):
    """The exact scan-domain value t of every row, in extended precision (np.longdouble: the fp64 inputs are exact)."""
    LD = np.longdouble
    Xl, ql = X.astype(LD), np.asarray(q, np.float32).astype(LD)
    qn2 = (ql * ql).sum()
    if not qn2 > 0:
        return None
    nq = np.sqrt(qn2)
    if metric == L2:
        d = Xl - ql[None, :]
        return (qn2 - (d * d).sum(axis=1)) / (2 * nq)
    s = Xl @ ql
    if metric == IP:
        return s / nq
    xn = np.sqrt((Xl * Xl).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(xn > 0, s / (xn * nq), LD(0))


# ---- the planted corpus ---------------------------------------------------------------------------------------------
ANNULUS = dict(n=20011, d=128, B=8, n_in=40, n_above=1500, cos_in=(0.60, 0.80), cos_above=(0.95, 0.999),
               radius=0.5, range_filter=0.9, l2_range_filter=0.2, l2_radius=1.0)


@functools.lru_cache(maxsize=None)
def annulus():
    """-> (X float32 [n, d] unit rows, Q float32 [B, d] unit queries, in_rows [B, n_in]).  Per query n_in rows at cosines
    cos_in (evenly spaced) and n_above rows at cosines cos_above, their noise orthogonalised against the query so that
    the cosine is the planted one; the rows sit at a random permutation of row numbers; the rest is random."""
    a = ANNULUS
    rng = np.random.default_rng(20011)
    n, d, B = a["n"], a["d"], a["B"]
    Qh, _ = np.linalg.qr(rng.standard_normal((d, B)))
    Qh = Qh.T                                             # orthonormal queries: a row planted for one is noise to the others
    X = rng.standard_normal((n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    perm = rng.permutation(n)
    per_q = a["n_in"] + a["n_above"]
    in_rows = np.empty((B, a["n_in"]), np.int64)
    for b in range(B):
        rows = perm[b * per_q:(b + 1) * per_q]
        cos = np.concatenate([np.linspace(*a["cos_in"], a["n_in"]), rng.uniform(*a["cos_above"], a["n_above"])])
        noise = rng.standard_normal((per_q, d))
        noise -= (noise @ Qh[b])[:, None] * Qh[b][None, :]
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        X[rows] = cos[:, None] * Qh[b][None, :] + np.sqrt(1.0 - cos * cos)[:, None] * noise
        in_rows[b] = rows[:a["n_in"]]
    return X.astype(np.float32), Qh.astype(np.float32), in_rows
