"""The sparse scan's error bound, restated in numpy (no GPU).

The select kernel flags a sparse list proven exact when the k-th refined score beats the largest approximate score
outside the candidates (`cut`) by more than the scan's error bound, or when `cut` lies at or below the query's floor
(nothing outside can score above 0).  This module restates the arithmetic that bound has to cover, as the kernels do it:

  * postings hold the doc weight rounded to fp16 (round to nearest even; a nonzero weight never rounds to zero, it
    becomes the smallest subnormal with its sign: sparse.h posting_weight_bits);
  * the query weights are scaled by scale = 2^30 / (sum|w_q| * max|posting weight|) and each posting adds
    trunc(fma(w16, w_q * scale, 1)) to an int32 accumulator (sparse_scan_kernel);
  * a group's maximum is max(0, acc) * (1 / scale);
  * q_eps, the per-query floor and eps_rel as sparse_query_prep_kernel and sparse_side compute them.

For random unsigned, signed and extreme families it asserts the two facts the proof and the candidate trim rest on:
|approx - exact| stays within q_eps + eps_rel * |approx| for every row, and a row whose clamped maximum lies at or below
the floor cannot score above 0.  A control shows that the unsigned-only bound misses the signed cancellation case, so
the model is sharp enough to notice an edit that makes the bound unsound."""
import numpy as np
import pytest

EPS_REL = 2.0 ** -11 * 1.01 + 2.0 ** -22          # sparse_side: fp16 postings + fp32 rounding
SUBNORMAL_MIN = 2.0 ** -24
INF = np.float32(np.inf)


def posting_weight(w):
    """fp32 doc weights -> the fp16 value a posting holds, as fp32."""
    w = np.asarray(w, np.float32)
    h = w.astype(np.float16).astype(np.float32)
    return np.where((h == 0) & (w != 0), np.copysign(np.float32(SUBNORMAL_MIN), w), h).astype(np.float32)


def query_prep(q_val, max_doc_w, doc_signed, signed_bound=True, floor_max=True):
    """(scale, q_eps, floor) of one query, in fp32 as sparse_query_prep_kernel computes them.  signed_bound=False /
    floor_max=False restate the earlier bound (no signed term, floor 0, max |doc w| not raised to the subnormal)."""
    q_val = np.asarray(q_val, np.float32)
    nnz = q_val.size
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        s = np.float32(np.abs(q_val).sum(dtype=np.float32))
        m = np.float32(max(max_doc_w, SUBNORMAL_MIN) if (floor_max and max_doc_w > 0) else max_doc_w)
        bound = np.float32(s * m)
        scale = np.float32(np.float32(2.0 ** 30) / bound) if bound > 0 else np.float32(0)
    blind = s > 0 and not (0 < scale < INF)
    if blind and signed_bound:
        eps = INF
    elif scale > 0 and np.isfinite(scale):
        eps = np.float32(np.float32(2.0 * (nnz + 1)) / scale + s * np.float32(6.0e-8))
    else:
        eps = np.float32(0)
    is_signed = bool(doc_signed or (q_val < 0).any())
    if signed_bound and is_signed:
        eps = np.float32(eps + np.float32(1.01 * 2.0 ** -11) * bound)
    if signed_bound and (is_signed or not np.isfinite(eps)):
        floor = -eps
    else:
        floor = np.float32(0)
    return scale, eps, floor


def scan(D, present, q_idx, q_val, scale):
    """Approximate scores of every row (D: [n, V] fp32 weights, present: [n, V] stored entries) and the largest
    |partial sum| any order of the integer atomics can reach."""
    ws = (np.asarray(q_val, np.float32) * scale).astype(np.float32)
    w16 = posting_weight(D[:, q_idx]).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        x = (w16 * ws.astype(np.float64) + 1.0).astype(np.float32)     # fma: exact product + 1, one rounding
    assert np.all(np.abs(x[present[:, q_idx]]) < 2.0 ** 31), "a posting leaves the int32 range"
    c = np.where(present[:, q_idx], np.trunc(x), 0).astype(np.int64)
    acc = c.sum(axis=1)
    headroom = np.abs(c).sum(axis=1).max(initial=0)
    inv = np.float32(1) / scale
    return (acc.astype(np.float32) * inv).astype(np.float32), headroom


def exact(D, present, q_idx, q_val):
    """score32: fp64 sum of fp32 products, rounded to fp32 (oracle_sparse_scores)."""
    P = np.where(present[:, q_idx], D[:, q_idx].astype(np.float64) * np.asarray(q_val, np.float64), 0.0)
    return P.sum(axis=1).astype(np.float32)


def check(D, present, q_idx, q_val, **kw):
    """Assert the bound holds for every row; return (approx, exact, eps, floor)."""
    w = D[present]
    max_doc_w = float(np.abs(w).max(initial=0))
    doc_signed = bool((w < 0).any())
    scale, eps, floor = query_prep(q_val, max_doc_w, doc_signed, **kw)
    if not np.isfinite(eps):
        assert floor == -INF                     # the list can never be proven: nothing to check
        return None, None, eps, floor
    approx, headroom = scan(D, present, q_idx, q_val, scale)
    assert headroom < 2 ** 31, "the fixed-point sums overflow int32"
    ex = exact(D, present, q_idx, q_val).astype(np.float64)
    g = np.maximum(approx, 0).astype(np.float64)  # the group maxima start at 0
    tol = float(eps) + EPS_REL * g
    assert np.all(ex <= g + tol), f"a row scores {np.max(ex - g - tol):.3g} above the bound"
    assert np.all(approx.astype(np.float64) <= ex + float(eps) + EPS_REL * np.abs(approx)), "approx too high"
    below = g <= float(floor)
    assert not np.any(ex[below] > 0), "a row at or below the floor qualifies"
    return approx, ex, eps, floor


def family(rng, n, V, density, doc_sign, mag=lambda rng, m: np.abs(rng.standard_normal(m)) + 0.01):
    present = rng.random((n, V)) < density
    D = np.zeros((n, V), np.float32)
    m = int(present.sum())
    D[present] = (mag(rng, m) * doc_sign(rng, m)).astype(np.float32)
    return D, present


POS = lambda rng, m: np.ones(m)  # noqa: E731
NEG = lambda rng, m: -np.ones(m)  # noqa: E731
MIX = lambda rng, m: np.where(rng.random(m) < 0.5, -1.0, 1.0)  # noqa: E731


def queries(rng, V, B, nnz, sign, mag=lambda rng, m: np.abs(rng.standard_normal(m)) + 0.05):
    for _ in range(B):
        qi = np.sort(rng.choice(V, nnz, replace=False))
        yield qi, (mag(rng, nnz) * sign(rng, nnz)).astype(np.float32)


@pytest.mark.parametrize("doc_sign,q_sign", [(POS, POS), (MIX, MIX), (POS, MIX), (NEG, POS), (POS, NEG), (NEG, NEG)],
                         ids=["unsigned", "signed", "signed_query", "negative_docs", "negative_query", "both_negative"])
def test_bound_holds_on_random_families(doc_sign, q_sign):
    rng = np.random.default_rng(1)
    D, present = family(rng, 4000, 96, 0.15, doc_sign)
    for qi, qv in queries(rng, 96, 12, 20, q_sign):
        check(D, present, qi, qv)


@pytest.mark.parametrize("case", ["docs_60000", "docs_1e-9", "docs_signed_1e-9", "query_1e-6_to_1e6", "subnormal_docs",
                                  "zero_weights"])
def test_bound_holds_at_magnitude_extremes(case):
    rng = np.random.default_rng(2)
    sign = MIX if "signed" in case or case == "docs_60000" else POS
    mag = {"docs_60000": lambda rng, m: np.where(rng.random(m) < 0.5, 60000.0, rng.uniform(0.1, 1, m)),
           "docs_1e-9": lambda rng, m: rng.uniform(1e-9, 3e-9, m),
           "docs_signed_1e-9": lambda rng, m: rng.uniform(1e-9, 3e-9, m),
           "subnormal_docs": lambda rng, m: rng.uniform(1e-7, 6e-5, m),
           "zero_weights": lambda rng, m: np.where(rng.random(m) < 0.3, 0.0, rng.uniform(0.1, 1, m))}.get(case)
    D, present = family(rng, 3000, 64, 0.2, sign, mag) if mag else family(rng, 3000, 64, 0.2, POS)
    qmag = (lambda rng, m: 10.0 ** rng.uniform(-6, 6, m)) if case == "query_1e-6_to_1e6" else None
    for qi, qv in queries(rng, 64, 10, 16, MIX if case == "docs_60000" else POS, *([qmag] if qmag else [])):
        check(D, present, qi, qv)


def test_bound_holds_at_the_int32_headroom():
    """HR_MAX_QUERY_NNZ terms at the largest weight the shard accepts, against rows that hold all of them."""
    V = 4096
    D = np.full((4, V), 60000.0, np.float32)
    D[1] *= np.where(np.arange(V) % 2, -1, 1).astype(np.float32)
    present = np.ones_like(D, bool)
    qi = np.arange(V)
    for qv in (np.full(V, 60000.0, np.float32), np.full(V, 1e-3, np.float32)):
        check(D, present, qi, qv)


def test_signed_cancellation_needs_the_signed_term():
    """The construction of the proof-edge GPU test S1: {1: 1000.24, 2: 1000.0} against {1: +1, 2: -1} scores 0.24, the
    fp16 postings say 0.  The earlier bound (relative to the score only, floor 0) does not cover it; the signed term
    does."""
    D = np.zeros((3, 4), np.float32)
    present = np.zeros_like(D, bool)
    D[0, 1], D[0, 2] = 1000.24, 1000.0
    D[1, 3], D[2, 3] = 0.1, 0.2
    present[0, [1, 2]] = present[1, 3] = present[2, 3] = True
    qi, qv = np.array([1, 2, 3]), np.array([1.0, -1.0, 1.0], np.float32)
    with pytest.raises(AssertionError):
        check(D, present, qi, qv, signed_bound=False)
    approx, ex, eps, floor = check(D, present, qi, qv)
    assert ex[0] > 0.2 and approx[0] < 0.01 and eps > 1.0 and floor == -eps


def test_fp16_collisions_are_covered_by_the_relative_term():
    """1000.1 and 1000.2 are one fp16 value: the scan cannot order them, the relative term covers the difference."""
    D = np.array([[1000.1], [1000.2], [999.9]], np.float32)
    present = np.ones_like(D, bool)
    approx, ex, eps, floor = check(D, present, np.array([0]), np.array([1.0], np.float32))
    assert approx[0] == approx[1] and ex[0] != ex[1] and floor == 0


def test_tiny_doc_weights_need_the_raised_maximum():
    """Weights of 1e-9 are stored as 2^-24 (60x more): sized by the fp32 maximum the scale overflows int32."""
    rng = np.random.default_rng(3)
    D, present = family(rng, 500, 16, 0.5, POS, lambda rng, m: rng.uniform(1e-9, 3e-9, m))
    qi, qv = np.arange(16), np.ones(16, np.float32)
    with pytest.raises(AssertionError):
        check(D, present, qi, qv, floor_max=False)
    check(D, present, qi, qv)


@pytest.mark.parametrize("qw,doc_max", [(1e34, 60000.0), (1e-35, 1.0), (1e38, 1.0)])
def test_scale_out_of_range_is_never_proven(qw, doc_max):
    scale, eps, floor = query_prep(np.array([qw, 2 * qw, 0.5 * qw], np.float32), doc_max, False)
    assert not (0 < scale < INF)
    assert eps == INF and floor == -INF
