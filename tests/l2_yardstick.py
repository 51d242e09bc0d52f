"""The L2 yardstick of the tests: a numpy restatement of HR_METRIC_L2's result semantics (include/hbmrag.h), in the
style of oracle.dense_scores_np — D = k-ordered sequential fp64 sum of d_k * d_k, d_k = (double)x[k] - (double)q[k],
rounded once to fp32 — ranked by (distance asc, row asc) with the oracle's own top-k on the negated distances."""
import numpy as np

import oracle


def l2_dist_np(X: np.ndarray, q: np.ndarray) -> np.ndarray:
    n, d = X.shape
    q64 = q.astype(np.float64)
    s = np.zeros(n, dtype=np.float64)
    for k in range(d):
        dk = X[:, k].astype(np.float64) - np.float64(q64[k])
        s += dk * dk
    return s.astype(np.float32)


def l2_dist_py(x, q) -> np.float32:
    """One row, scalar Python floats (IEEE doubles, one rounding per operation)."""
    s = 0.0
    for k in range(len(q)):
        dk = float(x[k]) - float(q[k])
        s = s + dk * dk
    return np.float32(s)


def l2_search(X: np.ndarray, Q: np.ndarray, k: int, mask=None, row_offset: int = 0):
    """ids [B, k], distances [B, k]: (distance asc, row asc), padded with -1 / +0."""
    Q = np.atleast_2d(Q)
    ids = np.empty((Q.shape[0], k), dtype=np.int64)
    sc = np.empty((Q.shape[0], k), dtype=np.float32)
    for b in range(Q.shape[0]):
        i, s = oracle.topk(-l2_dist_np(X, Q[b]), k, mask, False, row_offset)
        s = -s                      # exact; (-D desc, id asc) is (D asc, id asc)
        s[i < 0] = 0.0              # the padding is +0, not -0
        ids[b], sc[b] = i, s
    return ids, sc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
