"""Range search, the parts that need no GPU:

  * indexing.range_bounds: defaults per metric, NaN, non-numbers, empty intervals;
  * the scan-domain bounds hi_a / lo_a of prep_queries_kernel, restated in numpy (tests/range_yardstick.py), against the
    exact value t of every in-range row in extended precision: t never exceeds hi_a - eps and never falls to lo_a + eps,
    for random and adversarial rows (canonical score exactly on a bound, one ulp either side, zero query, tiny / huge |q|);
  * scan_plan() with the range flag: a small program of its own over the recorded table's axes."""
import math
import os
import runpy
import shutil
import subprocess

import numpy as np
import pytest

import range_yardstick as ry
from advanced_rag.indexing import MilvusIndexManager, range_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ---- range_bounds ---------------------------------------------------------------------------------------------------
def P(**kw):
    return {"metric_type": "COSINE", "params": kw}


def test_no_range_params_is_none():
    for metric in ("COSINE", "IP", "L2"):
        assert range_bounds(None, metric) is None
        assert range_bounds({}, metric) is None
        assert range_bounds(P(ef=64), metric) is None
        assert range_bounds(P(radius=None, range_filter=None), metric) is None
        assert range_bounds({"radius": 0.5}, metric) is None          # only search_params["params"] is read


def test_defaults_per_metric():
    assert range_bounds(P(radius=0.5), "COSINE") == (0.5, INF)
    assert range_bounds(P(range_filter=0.9), "IP") == (-INF, 0.9)
    assert range_bounds(P(radius=0.5, range_filter=0.9), "COSINE") == (0.5, 0.9)
    assert range_bounds(P(radius=1.0), "L2") == (1.0, -INF)
    assert range_bounds(P(range_filter=0.2), "L2") == (INF, 0.2)
    assert range_bounds(P(radius=1, range_filter=0), "L2") == (1.0, 0.0)
    assert range_bounds(P(radius=np.float32(0.25), range_filter=np.int64(3)), "IP") == (0.25, 3.0)
    assert all(isinstance(v, float) for v in range_bounds(P(radius=1, range_filter=2), "IP"))


@pytest.mark.parametrize("bad", [float("nan"), "0.5", [0.5], True, complex(1, 0)])
@pytest.mark.parametrize("key", ["radius", "range_filter"])
def test_nan_and_non_numbers_are_refused(key, bad):
    for metric in ("COSINE", "IP", "L2"):
        with pytest.raises(ValueError, match=key):
            range_bounds(P(**{key: bad}), metric)


def test_empty_intervals_are_refused():
    for metric in ("COSINE", "IP"):
        for r, f in ((0.9, 0.5), (0.5, 0.5), (INF, 1.0), (0.0, -INF)):
            with pytest.raises(ValueError, match="empty range"):
                range_bounds(P(radius=r, range_filter=f), metric)
        assert range_bounds(P(radius=0.5, range_filter=math.nextafter(0.5, 1.0)), metric) is not None
    for r, f in ((0.2, 1.0), (0.5, 0.5), (-INF, 0.0), (1.0, INF)):
        with pytest.raises(ValueError, match="empty range"):
            range_bounds(P(radius=r, range_filter=f), "L2")
    assert range_bounds(P(radius=math.nextafter(0.5, 1.0), range_filter=0.5), "L2") is not None
    with pytest.raises(ValueError):
        range_bounds(P(radius=0.5), "HAMMING")


def test_params_key_leaves_the_numbers_out():
    key = MilvusIndexManager._params_key
    plain = key({"metric_type": "COSINE", "params": {"ef": 64}})
    assert plain == (("ef", 64),)                                         # what it was
    a = key(P(ef=64, radius=0.5))
    b = key(P(ef=64, radius=0.7, range_filter=0.9))
    assert a == b != plain and ("ranged", True) in a
    assert not any(k in ("radius", "range_filter") for k, _ in a)
    assert key(P(ef=64, radius=None)) == plain


# ---- hi_a / lo_a ----------------------------------------------------------------------------------------------------
def _check_bounds(X, q, metric, f16, radius, range_filter, M=None):
    """Every row in range by the canonical rule has t <= hi_a - eps and t > lo_a + eps.  -> (hi_a, lo_a, rows in range)."""
    q = np.asarray(q, np.float32)
    qn2 = ry.canonical_qn2(q)
    M = ry.max_row_norm(X) if M is None else M
    eps = ry.scan_eps(metric, f16, X.shape[1], M, qn2)
    radius, range_filter = ry.fill(metric, radius, range_filter)
    hi, lo = ry.range_scan_bounds(metric, qn2, radius, range_filter, eps, M)
    t = ry.exact_t(X, q, metric)
    if t is None or not np.isfinite(eps):
        assert hi == np.inf and lo == -np.inf
        return hi, lo, 0
    s = ry.scores(X, q, metric)
    LD = np.longdouble
    better = s.astype(np.float64) >= range_filter if metric == ry.L2 else s.astype(np.float64) <= range_filter
    worse = s.astype(np.float64) < radius if metric == ry.L2 else s.astype(np.float64) > radius
    assert np.all(t[better] <= LD(float(hi)) - LD(eps)), "a row that passes range_filter lies above the ceiling"
    assert np.all(t[worse] > LD(float(lo)) + LD(eps)), "a row that passes radius lies at or below the floor"
    # and the bounds are not vacuous: within a few eps of the bound itself (finite sides, |q| in range)
    return hi, lo, int((better & worse).sum())


def _rows(rng, n, d, np_dtype, scale=1.0):
    return (rng.standard_normal((n, d)) * scale).astype(np.float32).astype(np_dtype)


@pytest.mark.parametrize("metric", [ry.COSINE, ry.IP, ry.L2], ids=["COSINE", "IP", "L2"])
@pytest.mark.parametrize("np_dtype", [np.float16, np.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("d", [8, 128, 1024])
def test_bounds_cover_random_rows(metric, np_dtype, d):
    rng = np.random.default_rng(d + metric)
    X = _rows(rng, 600, d, np_dtype)
    total = 0
    for _ in range(4):
        q = rng.standard_normal(d).astype(np.float32)
        s = np.sort(ry.scores(X, q, metric).astype(np.float64))
        for lo_q, hi_q in ((0.2, 0.8), (0.5, 0.51), (0.0, 1.0)):
            a, b = s[int(lo_q * 599)], s[int(hi_q * 599)]
            r, f = (b, a) if metric == ry.L2 else (a, b)
            if a == b:
                continue
            total += _check_bounds(X, q, metric, np_dtype == np.float16, r, f)[2]
        for r, f in ((None, None), (s[300], None), (None, s[300])):
            _check_bounds(X, q, metric, np_dtype == np.float16, r, f)
    assert total > 0


@pytest.mark.parametrize("metric", [ry.COSINE, ry.IP, ry.L2], ids=["COSINE", "IP", "L2"])
@pytest.mark.parametrize("np_dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_bounds_cover_rows_on_and_beside_a_bound(metric, np_dtype):
    """Bounds taken from canonical scores themselves, and one float32 ulp either side: the row on the closed side must
    stay under the ceiling / over the floor whichever way its fp64 value was rounded."""
    rng = np.random.default_rng(7 + metric)
    for d in (8, 128, 1024):
        X = _rows(rng, 300, d, np_dtype)
        q = rng.standard_normal(d).astype(np.float32)
        s = ry.scores(X, q, metric)
        for v in np.sort(s)[[3, 100, 150, 296]]:
            # one float32 ulp either side, and the doubles next to the score: a bound between two floats keeps a row whose
            # fp64 value lies beyond it (rounded to the float on the bound's inner side)
            for w in (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf)),
                      np.nextafter(np.float64(v), -np.inf), np.nextafter(np.float64(v), np.inf)):
                w = float(w)
                if metric == ry.L2:
                    _check_bounds(X, q, metric, np_dtype == np.float16, None, w)       # D >= w: closed side
                    _check_bounds(X, q, metric, np_dtype == np.float16, w, None)       # D < w: strict side
                else:
                    _check_bounds(X, q, metric, np_dtype == np.float16, None, w)
                    _check_bounds(X, q, metric, np_dtype == np.float16, w, None)


@pytest.mark.parametrize("metric", [ry.COSINE, ry.IP, ry.L2], ids=["COSINE", "IP", "L2"])
def test_zero_tiny_and_huge_queries(metric):
    rng = np.random.default_rng(11)
    d = 128
    X = _rows(rng, 300, d, np.float16)
    q0 = rng.standard_normal(d).astype(np.float32)
    # zero query, and 1 / |q| outside the normal fp32 range: no ceiling, no floor
    for q in (np.zeros(d, np.float32), q0 * np.float32(1e-37) * np.float32(1e-3), q0 * np.float32(3e36)):
        qn2 = ry.canonical_qn2(q)
        eps = ry.scan_eps(metric, True, d, ry.max_row_norm(X), qn2)
        with np.errstate(over="ignore"):
            in_fp32 = qn2 > 0 and 2.0 ** -126 <= np.float32(1.0 / math.sqrt(qn2)) < np.inf
        if in_fp32 and np.isfinite(eps):
            continue
        hi, lo = ry.range_scan_bounds(metric, qn2, *ry.fill(metric, 0.3, 0.6) if metric != ry.L2 else (0.6, 0.3), eps,
                                      ry.max_row_norm(X))
        assert hi == np.inf and lo == -np.inf
    # tiny and huge |q| that stay in range: the bounds still cover
    for scale in (1e-30, 1e-12, 1e12, 1e30):
        q = (q0.astype(np.float64) * scale).astype(np.float32)
        with np.errstate(over="ignore"):
            s = np.sort(ry.scores(X, q, metric).astype(np.float64))
        if not np.all(np.isfinite(s)):
            continue
        a, b = s[60], s[240]
        if a == b:
            continue
        r, f = (b, a) if metric == ry.L2 else (a, b)
        _check_bounds(X, q, metric, True, r, f)


def test_bounds_are_tight_to_a_few_eps():
    """Not vacuous: for a unit query the ceiling and the floor lie within 3 eps of the bounds themselves."""
    rng = np.random.default_rng(5)
    X = _rows(rng, 64, 128, np.float16)
    q = rng.standard_normal(128)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    qn2 = ry.canonical_qn2(q)
    M = ry.max_row_norm(X)
    for metric, r, f, t_r, t_f in ((ry.COSINE, 0.5, 0.9, 0.5, 0.9), (ry.IP, 0.5, 0.9, 0.5, 0.9),
                                   (ry.L2, 1.0, 0.2, 0.0, 0.4)):
        eps = ry.scan_eps(metric, True, 128, M, qn2)
        hi, lo = ry.range_scan_bounds(metric, qn2, r, f, eps, M)
        assert t_f + eps <= hi <= t_f + 3 * eps + 1e-6 * M
        assert t_r - 3 * eps - 1e-6 * M <= lo < t_r - eps


# ---- scan_plan with the range flag ----------------------------------------------------------------------------------
PLAN_PROGRAM = r"""
#include <cstdio>
#include "scan_plan.h"
using namespace hbmrag;
int main() {
    int KT, dtype, metric, override_, mask, B;
    long long n_rows;
    while (std::scanf("%d %d %d %lld %d %d %d", &KT, &dtype, &metric, &n_rows, &override_, &mask, &B) == 7) {
        const ScanPlan first = scan_plan(KT, dtype, metric, n_rows, override_, mask, B, B, true);
        const ScanPlan plain = scan_plan(KT, dtype, metric, n_rows, override_, mask, B, B);
        std::printf("%d %d %d %d %d %d |", first.kind, first.G, first.chunk_q, (int)first.range, plain.kind, (int)plain.range);
        for (int c0 = 0; first.kind != SCAN_NONE && c0 < B; c0 += first.chunk_q) {
            const int nq = B - c0 < first.chunk_q ? B - c0 : first.chunk_q;
            const ScanPlan p = scan_plan(KT, dtype, metric, n_rows, override_, mask, B, nq, true);
            std::printf(" %d:%d:%d:%d", nq, p.kind, p.G, (int)p.range);
        }
        std::printf("\n");
    }
    return 0;
}
"""


def test_a_range_pass_takes_the_generic_kernels_only(tmp_path):
    gen = runpy.run_path(os.path.join(ROOT, "tests", "golden", "gen_scan_plan_table.py"))
    KTS, BS, MASKS = gen["KTS"], gen["BS"], gen["MASKS"]
    cxx = next((p for p in map(shutil.which, ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++")) if p), None)
    assert cxx, "no host C++ compiler"
    src = tmp_path / "range_plan.cpp"
    src.write_text(PLAN_PROGRAM)
    exe = str(tmp_path / "range_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "advanced-rag-milvus_amd", "csrc"), "-o", exe, str(src)], check=True)
    inputs = ["%d %d %d %d %d %d %d" % (KT, dtype, metric, n_rows, override, mask, B)
              for n_rows, override in ((1000000, 0), (10000000, 0), (1000, 64), (10000000, 16))
              for KT in KTS for dtype in (1, 0) for metric in (0, 1, 2) for B in BS for mask in MASKS]
    out = subprocess.run([exe], input="\n".join(inputs) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(inputs)
    SCAN_NONE, SCAN_LDS, SCAN_BIGQ = 0, 1, 2
    n_two_pass = 0
    for line, got in zip(inputs, out):
        KT, dtype, metric, _, _, mask, B = (int(x) for x in line.split())
        head, passes = got.split("|")
        kind, G, chunk_q, is_range, plain_kind, plain_range = (int(x) for x in head.split())
        assert plain_range == 0                                   # the default argument: the plain plan is untouched
        assert (kind == SCAN_NONE) == (plain_kind == SCAN_NONE), line
        if kind == SCAN_NONE:
            continue
        assert is_range == 1 and kind in (SCAN_LDS, SCAN_BIGQ), (line, got)
        lds_tile_q = 16 * max(1, min(4, 156 // KT))
        if B > lds_tile_q or kind == SCAN_BIGQ:
            assert chunk_q <= 128, (line, got)
        served = 0
        for p in passes.split():
            nq, pk, pg, pr = (int(x) for x in p.split(":"))
            assert pk in (SCAN_LDS, SCAN_BIGQ) and pr == 1 and nq <= 16 * pg <= 128, (line, got)
            served += nq
        assert served == B
        n_two_pass += B == 256 and len(passes.split()) == 2 and kind == SCAN_BIGQ
    assert n_two_pass > 0                                         # 256 ranged queries are two 128-query passes


# ---- the kernel's own bound functions against the restatement -------------------------------------------------------
BOUNDS_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "range_bounds.h"
int main() {
    int metric;
    unsigned long long w[5];
    while (std::scanf("%d %llx %llx %llx %llx %llx", &metric, &w[0], &w[1], &w[2], &w[3], &w[4]) == 6) {
        double v[5];
        std::memcpy(v, w, sizeof v);
        float hi, lo;
        hbmrag::range_scan_bounds(metric, v[0], v[1], v[2], v[3], v[4], &hi, &lo);
        unsigned a, b;
        std::memcpy(&a, &hi, 4);
        std::memcpy(&b, &lo, 4);
        const float u = hbmrag::f32_up(v[1]), d = hbmrag::f32_down(v[1]);
        unsigned c, e;
        std::memcpy(&c, &u, 4);
        std::memcpy(&e, &d, 4);
        std::printf("%08x %08x %08x %08x\n", a, b, c, e);
    }
    return 0;
}
"""


def test_the_kernels_bound_functions_equal_the_restatement(tmp_path):
    """csrc/range_bounds.h is what prep_queries_kernel calls and is plain C++: compiled for the host, range_scan_bounds,
    f32_up and f32_down give the floats of the numpy restatement bit for bit, on random and on edge inputs."""
    cxx = next((p for p in map(shutil.which, ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++")) if p), None)
    assert cxx, "no host C++ compiler"
    src = tmp_path / "bounds.cpp"
    src.write_text(BOUNDS_PROGRAM)
    exe = str(tmp_path / "bounds")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "advanced-rag-milvus_amd", "csrc"), "-o", exe, str(src)], check=True)
    rng = np.random.default_rng(77)
    cases = []
    specials = [0.0, -0.0, 1.0, -1.0, INF, -INF, 0.5, 0.9, 2.0 ** -149, 2.0 ** -130, 3.0e38, -3.0e38, 1e-300, 1e300,
                float(np.nextafter(np.float32(0.9), np.float32(1))), float(np.nextafter(np.float64(np.float32(0.9)), 1.0))]
    for metric in (ry.IP, ry.COSINE, ry.L2):
        for _ in range(1500):
            qn2 = float(10.0 ** rng.uniform(-80, 80)) if rng.random() < 0.3 else float(rng.uniform(0.01, 50.0))
            a, b = np.sort(rng.standard_normal(2) * (10.0 ** rng.uniform(-3, 3)))
            r, f = (b, a) if metric == ry.L2 else (a, b)
            if rng.random() < 0.3:
                r = float(rng.choice(specials))
            if rng.random() < 0.3:
                f = float(rng.choice(specials))
            eps = float(np.float32(10.0 ** rng.uniform(-7, -2))) if rng.random() < 0.9 else float(rng.choice([0.0, INF, 3.1e38]))
            M = float(np.float32(10.0 ** rng.uniform(-3, 3)))
            cases.append((metric, qn2, float(r), float(f), eps, M))
        cases += [(metric, 0.0, 0.1, 0.9, 1e-4, 1.0), (metric, 1e-80, 0.1, 0.9, 1e-4, 1.0), (metric, 1e80, 0.1, 0.9, 1e-4, 1.0)]
    bits64 = lambda x: "%x" % np.float64(x).view(np.uint64)   # noqa: E731
    text = "\n".join("%d %s" % (c[0], " ".join(bits64(x) for x in c[1:])) for c in cases) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    bits32 = lambda x: "%08x" % np.float32(x).view(np.uint32)   # noqa: E731
    finite = 0
    for c, line in zip(cases, out):
        hi, lo = ry.range_scan_bounds(*c)
        want = [bits32(hi), bits32(lo), bits32(ry.f32_up(c[2])), bits32(ry.f32_down(c[2]))]
        got = ["nan" if (int(w, 16) & 0x7FFFFFFF) > 0x7F800000 else w for w in line.split()]      # (a NaN's sign is no one's
        want = ["nan" if (int(w, 16) & 0x7FFFFFFF) > 0x7F800000 else w for w in want]             # to define: inf - inf inputs)
        assert got == want, (c, line, want)
        finite += bool(np.isfinite(hi) and np.isfinite(lo))
    assert finite > 1000
