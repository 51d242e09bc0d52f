"""Weighted score fusion, host side (no GPU): canonical_atan and score_fuse_lists against the independent numpy
restatement of tests/score_fusion_ref.py bit for bit, canonical_atan against math.atan, the configuration fields, and that
a default configuration makes exactly the fusion calls it made before the fusion mode existed."""
import asyncio
import math

import numpy as np
import pytest

import score_fusion_ref as R
from advanced_rag import _native as nat
from advanced_rag.pipeline import PipelineConfig
from advanced_rag.retrieval import (HybridRetriever, RetrievalConfig, canonical_atan, norm_code, normalise_scores,
                                    score_fuse_lists)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def atan_sweep():
    """Fixed sweep: uniform +-1, uniform +-60, 10^+-30, fp32-valued inputs, and the special points."""
    rng = np.random.default_rng(20260115)
    n = 20000
    parts = [rng.uniform(-1, 1, n), rng.uniform(-60, 60, n),
             np.sign(rng.uniform(-1, 1, n)) * 10.0 ** rng.uniform(-30, 30, n),
             rng.uniform(-60, 60, n).astype(np.float32).astype(np.float64),
             rng.standard_normal(n).astype(np.float32).astype(np.float64),
             np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310,
                       np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 0.5, 2.0, 1e300, -1e300])]
    return np.concatenate(parts)


def test_codes_match_the_header():
    assert (nat.HR_NORM_COSINE, nat.HR_NORM_ATAN, nat.HR_NORM_ATAN_DIST, nat.HR_NORM_MINMAX, nat.HR_NORM_MINMAX_DIST) == \
        (R.COSINE, R.ATAN, R.ATAN_DIST, R.MINMAX, R.MINMAX_DIST) == (0, 1, 2, 3, 4)
    fields = dict(nat.PostArgs._fields_)
    assert list(dict(nat.PostArgs._fields_))[-2:] == ["fusion", "norm"] and fields["norm"]._length_ == 3


def test_canonical_atan_equals_the_restatement_bit_for_bit():
    x = atan_sweep()
    got = np.array([canonical_atan(v) for v in x.tolist()])
    assert np.array_equal(bits(got), bits(R.catan(x)))


def test_canonical_atan_special_points():
    assert canonical_atan(0.0) == 0.0 and math.copysign(1.0, canonical_atan(0.0)) == 1.0
    assert canonical_atan(-0.0) == 0.0 and math.copysign(1.0, canonical_atan(-0.0)) == -1.0
    assert canonical_atan(math.inf) == float(R.HALF_PI) and canonical_atan(-math.inf) == -float(R.HALF_PI)
    assert canonical_atan(1.0) == math.atan(1.0)
    assert math.isnan(canonical_atan(math.nan))
    # the half-angle steps halve the smallest denormal to zero: one ulp off, inside the bound below
    assert canonical_atan(5e-324) == 0.0 and canonical_atan(1e-310) == pytest.approx(1e-310, rel=1e-6)


def test_canonical_atan_within_16_ulp_of_math_atan():
    """The bound is a guard (a wrong series term or a lost halving shows as > 10^5 ulp); measured on this sweep: 5.0 ulp
    (6.0 over 8M points of the same ranges)."""
    x = atan_sweep()
    got = np.array([canonical_atan(v) for v in x.tolist()])
    ref = np.array([math.atan(v) for v in x.tolist()])
    ulp = np.abs(got - ref) / np.spacing(np.abs(ref))
    ulp = np.where(got == ref, 0.0, ulp)
    print("canonical_atan: max distance from math.atan = %.1f ulp at x = %r" % (ulp.max(), x[int(ulp.argmax())]))
    assert ulp.max() <= 16.0


def fusion_cases():
    """(name, lists of (ids, fp32 scores), weights, norms): the cases of the GPU test in miniature, string ids included."""
    rng = np.random.default_rng(7)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    cases = []
    for code_a, code_b in ((0, 1), (2, 1), (3, 3), (4, 3), (1, 0)):
        a = np.sort(rng.uniform(-1, 1, 40).astype(np.float32))[::-1]
        if code_a in (2, 4):
            a = np.sort(rng.uniform(0, 4, 40).astype(np.float32))
        b = np.sort(rng.uniform(-3, 25, 40).astype(np.float32))[::-1]
        ia, ib = rng.permutation(100)[:40], rng.permutation(100)[:40]
        cases.append((f"codes{code_a}{code_b}", [(ia.tolist(), a), (ib.tolist(), b)], (0.7, 0.3), (code_a, code_b)))
    cases.append(("three_lists", [(["a", "b", "c"], f32([0.9, 0.5, 0.1])), (["c", "d"], f32([12.5, 3.0])),
                                  (["d", "a", "e"], f32([0.4, 0.3, -0.2]))], (0.7, 0.3, 0.2), (0, 1, 0)))
    cases.append(("disjoint", [([1, 2], f32([0.5, 0.25])), ([3, 4], f32([2.0, 1.0]))], (0.5, 0.5), (0, 3)))
    cases.append(("same_ids", [([1, 2, 3], f32([0.5, 0.25, 0.1])), ([3, 2, 1], f32([2.0, 1.0, 0.5]))], (0.6, 0.4), (3, 3)))
    cases.append(("empty_list", [([], f32([])), ([3, 4], f32([2.0, 1.0]))], (0.5, 0.5), (3, 3)))
    cases.append(("one_entry_and_equal_scores", [([9], f32([0.3])), ([3, 4, 5], f32([2.0, 2.0, 2.0]))], (0.5, 0.5), (3, 3)))
    cases.append(("ties_keep_first_seen", [([5, 6, 7], f32([0.0, 0.0, 0.0])), ([8, 7], f32([0.0, 0.0]))], (1.0, 1.0), (0, 0)))
    cases.append(("negative_ip_and_weights", [([1, 2, 3], f32([-0.5, -2.0, -40.0])), ([2, 9], f32([-1.0, -7.0]))],
                  (-0.25, 0.0), (1, 1)))
    return cases


@pytest.mark.parametrize("case", fusion_cases(), ids=lambda c: c[0])
def test_score_fuse_lists_equals_the_restatement_bit_for_bit(case):
    _, lists, weights, norms = case
    got = score_fuse_lists(lists, weights, norms)
    # the restatement works on int64 ids: number the ids in first-seen order
    number = {}
    for ids, _ in lists:
        for i in ids:
            number.setdefault(i, len(number))
    name = {v: k for k, v in number.items()}
    fi, fs, fm = R.fuse([([number[i] for i in ids], sc) for ids, sc in lists], weights, norms)
    assert [g[0] for g in got] == [name[int(i)] for i in fi]
    assert np.array_equal(bits([g[1] for g in got]), bits(fs))
    assert [sum(1 << li for li in g[2]) for g in got] == fm.tolist()
    for (ids, sc), code in zip(lists, norms):
        assert np.array_equal(bits(normalise_scores(sc, code)), bits(R.normalise(sc, code)))


def test_math_atan_in_place_of_catan_moves_normalised_scores_by_less_than_1e_14():
    x = atan_sweep()
    x = x[np.abs(x) < 3e38].astype(np.float32)       # what a list can hold: finite fp32 scores
    for code in (R.ATAN, R.ATAN_DIST):
        ours = np.array(normalise_scores(x, code))
        libm = np.array(normalise_scores(x, code, atan=math.atan))
        assert np.abs(ours - libm).max() < 1e-14


def test_norm_codes_by_metric():
    assert [norm_code(m) for m in ("COSINE", "IP", "L2")] == [0, 1, 2]
    assert [norm_code(m, "minmax") for m in ("COSINE", "IP", "L2")] == [3, 3, 4]
    with pytest.raises(ValueError):
        norm_code("IP", "zscore")
    with pytest.raises(ValueError):
        normalise_scores([1.0], 5)


def test_config_validation():
    assert (RetrievalConfig().fusion, RetrievalConfig().score_normalization) == ("rrf", "activation")
    RetrievalConfig(fusion="weighted", score_normalization="minmax")
    for bad in ("RRF", "alpha", "", None, 1):
        with pytest.raises(ValueError):
            RetrievalConfig(fusion=bad)
        with pytest.raises(ValueError):
            RetrievalConfig(fusion="weighted", score_normalization=bad)


def test_profiles_and_pipeline_config_carry_both_fields():
    base = RetrievalConfig(fusion="weighted", score_normalization="minmax")
    profiles = HybridRetriever._build_default_profiles(base)
    assert set(profiles) == {"default", "faq", "troubleshooting", "summary", "analysis"}
    assert all((p.fusion, p.score_normalization) == ("weighted", "minmax") for p in profiles.values())
    assert all((p.fusion, p.score_normalization) == ("rrf", "activation")
               for p in HybridRetriever._build_default_profiles(RetrievalConfig()).values())
    assert (PipelineConfig().fusion, PipelineConfig().score_normalization) == ("rrf", "activation")
    from advanced_rag.pipeline import AdvancedRAGPipeline
    pipe = AdvancedRAGPipeline(config=PipelineConfig(fusion="weighted", score_normalization="minmax"), connect_to_milvus=False)
    assert (pipe.retriever.config.fusion, pipe.retriever.config.score_normalization) == ("weighted", "minmax")
    with pytest.raises(ValueError):
        AdvancedRAGPipeline(config=PipelineConfig(fusion="borda"), connect_to_milvus=False)


class Collection:
    def __init__(self, metric):
        self.metric = metric


class RecordingManager:
    """A duck-typed manager with every fusion entry point of the HBM one: records what the retriever calls."""

    def __init__(self, one_round=False, semantic_metric="COSINE"):
        self.calls = []
        self.collections = {"semantic_index": Collection(semantic_metric), "sparse_index": Collection("IP")}
        if one_round:
            self.hybrid_search = self._hybrid_search

    async def _generate_semantic_embedding(self, text):
        return np.ones(4, dtype=np.float32)

    async def _generate_sparse_embedding(self, text):
        return {0: 1.0}

    async def search(self, query_embedding, collection_name, top_k=20, filters=None, search_params=None):
        if collection_name == "semantic_index":
            return [{"id": "a", "_row": 0, "content": "x", "score": 0.75}, {"id": "b", "_row": 1, "content": "y", "score": 0.5}]
        return [{"id": "b", "_row": 1, "content": "y", "score": 11.0}, {"id": "c", "_row": 2, "content": "z", "score": 2.0}]

    async def _hybrid_search(self, dense, sparse, **kw):
        self.calls.append(("hybrid_search", tuple(sorted(kw))))
        self.kw = kw
        return None       # declined: the general path follows

    def fuse_rank_lists(self, rows, ids, weights, rrf_k=60):
        self.calls.append(("fuse_rank_lists", rows, ids, weights, rrf_k))
        raise RuntimeError("recorded")

    async def fuse_rank_lists_async(self, rows, ids, weights, rrf_k=60):
        self.calls.append(("fuse_rank_lists_async", rows, ids, weights, rrf_k))
        from advanced_rag.retrieval import rrf_rank_lists
        return rrf_rank_lists(ids, weights, rrf_k)

    def fuse_score_lists(self, rows, ids, scores, weights, norms):
        self.calls.append(("fuse_score_lists", rows, ids, scores, weights, norms))
        return score_fuse_lists(list(zip(ids, scores)), weights, norms)

    async def fuse_score_lists_async(self, rows, ids, scores, weights, norms):
        self.calls.append(("fuse_score_lists_async", rows, ids, scores, weights, norms))
        return score_fuse_lists(list(zip(ids, scores)), weights, norms)


def test_default_config_makes_the_fusion_calls_it_made_before():
    mgr = RecordingManager(one_round=True)
    out = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=5)).retrieve("plain statement", profile_hint="default"))
    assert [c[0] for c in mgr.calls] == ["hybrid_search", "fuse_rank_lists_async"]
    # the one-round request carries no fusion argument, the fusion call is RRF's with RRF's operands
    assert mgr.calls[0][1] == ("filters", "rrf_k", "semantic_params", "sparse_params", "top_k", "weights")
    assert mgr.calls[1][1:] == ([[0, 1], [1, 2], []], [["a", "b"], ["b", "c"], []], [0.7, 0.3, 0.2], 60)
    assert [h["id"] for h in out] == ["b", "a", "c"]
    # the synchronous entry point: fuse_rank_lists, never the score form
    mgr.calls.clear()
    r = HybridRetriever(mgr, RetrievalConfig(top_k=5))
    sem, spa = asyncio.run(mgr.search(None, "semantic_index")), asyncio.run(mgr.search(None, "sparse_index"))
    r._fuse_results(sem, spa)
    assert [c[0] for c in mgr.calls] == ["fuse_rank_lists"]


@pytest.mark.parametrize("normalization,metric,codes", [("activation", "COSINE", [0, 1, 0]), ("activation", "L2", [2, 1, 0]),
                                                        ("minmax", "COSINE", [3, 3, 3]), ("minmax", "L2", [4, 3, 3])])
def test_weighted_config_dispatches_to_the_score_fusion(normalization, metric, codes):
    # (the manager shows no domain collection: the third code comes from the request's search params, COSINE)
    mgr = RecordingManager(one_round=True, semantic_metric=metric)
    cfg = RetrievalConfig(top_k=5, fusion="weighted", score_normalization=normalization)
    r = HybridRetriever(mgr, cfg, weight_adapter=lambda q: (0.25, 0.5))
    out = asyncio.run(r.retrieve("plain statement", profile_hint="default"))
    assert [c[0] for c in mgr.calls] == ["hybrid_search", "fuse_score_lists_async"]
    assert mgr.kw["fusion"] == "weighted" and list(mgr.kw["norms"]) == codes[:2] and mgr.kw["weights"] == (0.25, 0.5)
    _, rows, ids, scores, weights, norms = mgr.calls[1]
    assert (rows, ids, scores) == ([[0, 1], [1, 2], []], [["a", "b"], ["b", "c"], []], [[0.75, 0.5], [11.0, 2.0], []])
    assert weights == [0.25, 0.5, 0.2] and norms == codes      # the adapter's per-request weights, as for RRF
    want = score_fuse_lists([(["a", "b"], [0.75, 0.5]), (["b", "c"], [11.0, 2.0]), ([], [])], [0.25, 0.5, 0.2], codes)
    assert [(h["id"], h["score"]) for h in out] == [(i, s) for i, s, _ in want]
    assert out[0]["retrieval_methods"] == [("semantic", "sparse", "domain")[li] for li in want[0][2]]
    # the synchronous entry point, and the host arithmetic of a manager without the device form
    mgr.calls.clear()
    sem, spa = asyncio.run(mgr.search(None, "semantic_index")), asyncio.run(mgr.search(None, "sparse_index"))
    fused = r._fuse_results(sem, spa)
    assert [c[0] for c in mgr.calls] == ["fuse_score_lists"]
    assert [(h["id"], h["score"]) for h in fused] == [(i, s) for i, s, _ in want]
