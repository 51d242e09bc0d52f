"""Independent numpy restatement of the weighted score fusion (include/hbmrag.h has the contract), shared by the
score-fusion tests.  Written from the formulas, vectorised: numpy's float64 +, -, *, / and sqrt are single, correctly
rounded IEEE operations and numpy never contracts them into an FMA, so the bits are what the contract asks for."""
import numpy as np

PI = np.float64(float.fromhex("0x1.921fb54442d18p+1"))
HALF_PI = np.float64(float.fromhex("0x1.921fb54442d18p+0"))
assert PI.view(np.uint64) == 0x400921FB54442D18 and HALF_PI.view(np.uint64) == 0x3FF921FB54442D18
COSINE, ATAN, ATAN_DIST, MINMAX, MINMAX_DIST = 0, 1, 2, 3, 4
SEMANTIC, SPARSE, DOMAIN = 1, 2, 4


def catan(x):
    """Canonical arctangent of a float64 array."""
    x = np.asarray(x, dtype=np.float64)
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        inv = a > one
        a = np.where(inv, one / np.where(inv, a, one), a)
        for _ in range(3):
            a = a / (one + np.sqrt(one + a * a))
        t = a * a
        c = [np.float64(-1.0 if i % 2 else 1.0) * (one / np.float64(2 * i + 1)) for i in range(12)]
        p = np.full_like(a, c[11])
        for i in range(10, -1, -1):
            p = c[i] + t * p
        r = np.float64(8.0) * (a * p)
        r = np.where(inv, HALF_PI - r, r)
    return np.copysign(r, x)


def normalise(scores, code, atan=catan):
    """fp32 scores of one list's valid prefix -> float64 normalised values."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    one = np.float64(1.0)
    if code == COSINE:
        return (one + s) * np.float64(0.5)
    if code == ATAN:
        return np.float64(0.5) + atan(s) / PI
    if code == ATAN_DIST:
        return one - (np.float64(2.0) * atan(s)) / PI
    assert code in (MINMAX, MINMAX_DIST)
    if not len(s):
        return s
    lo, hi = s.min(), s.max()
    if hi == lo:
        return np.ones_like(s)
    return (s - lo) / (hi - lo) if code == MINMAX else (hi - s) / (hi - lo)


def fuse(lists, weights, norms, atan=catan):
    """lists: up to three (ids, fp32 scores), the valid prefix ending at the first id < 0.
    -> (ids int64, fused float64, method masks int32) in fused order."""
    slot, score, meth = {}, [], []
    ids_out = []
    for li, ((ids, sc), w, code) in enumerate(zip(lists, weights, norms)):
        ids = np.asarray(ids, dtype=np.int64)
        neg = np.nonzero(ids < 0)[0]
        n = int(neg[0]) if len(neg) else len(ids)
        nv = normalise(np.asarray(sc)[:n], code, atan)
        for i in range(n):
            d = int(ids[i])
            if d not in slot:
                slot[d] = len(ids_out)
                ids_out.append(d)
                score.append(np.float64(0.0))
                meth.append(0)
            score[slot[d]] = score[slot[d]] + nv[i] * np.float64(w)
            meth[slot[d]] |= 1 << li
    # stable descending sort: ties keep first-seen order (no negation: -0.0 and NaN must not be touched)
    order = list(range(len(ids_out)))
    order.sort(key=lambda j: score[j], reverse=True)
    return (np.array([ids_out[j] for j in order], dtype=np.int64), np.array([score[j] for j in order], dtype=np.float64),
            np.array([meth[j] for j in order], dtype=np.int32))


def fuse_batch(id_lists, score_lists, weights, norms, top_k, w_query=None):
    """Batched form with the kernel's padding: id_lists / score_lists = up to three [B, k] arrays (None for none).
    -> (ids [B, top_k] -1 padded, scores [B, top_k] 0.0 padded, methods [B, top_k] 0 padded, n [B])."""
    B = len(id_lists[0])
    oi = np.full((B, top_k), -1, dtype=np.int64)
    os_ = np.zeros((B, top_k), dtype=np.float64)
    om = np.zeros((B, top_k), dtype=np.int32)
    on = np.zeros(B, dtype=np.int32)
    for q in range(B):
        lists = [(i[q], s[q]) if i is not None else ((), ()) for i, s in zip(id_lists, score_lists)]
        w = w_query[q] if w_query is not None else weights
        fi, fs, fm = fuse(lists, w, norms)
        n = min(len(fi), top_k)
        oi[q, :n], os_[q, :n], om[q, :n], on[q] = fi[:n], fs[:n], fm[:n], n
    return oi, os_, om, on
