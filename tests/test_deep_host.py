"""Deep search, host side (no GPU): the window rule of a request (indexing.deep_window) and the host merge of per-shard
deep lists (shards.merge_deep_lists) against oracle.topk on the concatenated scores."""
import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag.constants import QUERY_MAX_WINDOW
from advanced_rag.indexing import deep_window
from advanced_rag.shards import merge_deep_lists


def test_the_window_limit_is_the_library_limit():
    assert QUERY_MAX_WINDOW == nat.HR_MAX_DEEP_K == 16384


@pytest.mark.parametrize("top_k,offset,want", [(1, 0, 1), (256, 0, 256), (257, 0, 257), (100, 200, 300), (1, 16383, 16384),
                                               (16384, 0, 16384), (np.int64(300), np.int32(5), 305)])
def test_deep_window_accepts(top_k, offset, want):
    w = deep_window(top_k, offset)
    assert w == want and type(w) is int


@pytest.mark.parametrize("top_k,offset,word", [(0, 0, "top_k"), (-3, 0, "top_k"), (1, -1, "offset"), (16385, 0, r"offset \+ top_k"),
                                               (16384, 1, r"offset \+ top_k"), (1, 16384, r"offset \+ top_k"), (True, 0, "top_k"),
                                               (10, False, "offset"), (10.0, 0, "top_k"), (10, 2.0, "offset"), ("10", 0, "top_k"),
                                               (10, None, "offset"), (np.float32(4), 0, "top_k"), (np.bool_(True), 0, "top_k")])
def test_deep_window_refuses(top_k, offset, word):
    with pytest.raises(ValueError, match=word):
        deep_window(top_k, offset)


def _shard_lists(scores, bounds, W, ascending):
    """Every shard's own list at depth W over its slice of `scores` (global rows), as a shard returns it."""
    ids, sc = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        s = scores[lo:hi]
        i, v = oracle.topk(-s if ascending else s, W, row_offset=lo)
        v = np.where(i >= 0, -v if ascending else v, np.float32(0)).astype(np.float32)
        ids.append(i[None, :])
        sc.append(v[None, :])
    return ids, sc


@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("W,offset", [(300, 0), (300, 299), (1000, 256), (700, 100)])
def test_merge_of_shard_lists_is_the_ranking_of_the_whole(ascending, W, offset):
    rng = np.random.default_rng(W + offset + ascending)
    # coarse scores: ties within and across shards, both signs, no zero (the oracle does not order -0 against +0)
    scores = (rng.integers(-40, 40, 2500) + 0.5).astype(np.float32) / 8
    if ascending:
        scores = np.abs(scores)
    bounds = [0, 900, 901, 1300, 2500]          # a one-row shard; 1300 .. 2500 alone is longer than W
    ids, sc = _shard_lists(scores, bounds, W, ascending)
    top_k = W - offset
    got_ids, got_sc = merge_deep_lists(ids, sc, top_k, offset, ascending)
    want_ids, want_sc = oracle.topk(-scores if ascending else scores, W)
    want_sc = -want_sc if ascending else want_sc
    assert got_ids.shape == (1, top_k) and got_sc.dtype == np.float32
    assert np.array_equal(got_ids[0], want_ids[offset:])
    assert np.array_equal(got_sc[0].view(np.uint32), want_sc[offset:].astype(np.float32).view(np.uint32))


def test_merge_pads_a_short_ranking():
    scores = np.linspace(1, 2, 50, dtype=np.float32)
    ids, sc = _shard_lists(scores, [0, 20, 50], 300, False)
    got_ids, got_sc = merge_deep_lists(ids, sc, 280, 20)
    want_ids, want_sc = oracle.topk(scores, 300)
    assert np.array_equal(got_ids[0], want_ids[20:]) and np.array_equal(got_sc[0], want_sc[20:])
    assert (got_ids[0, 30:] == -1).all() and (got_sc[0, 30:] == 0).all()
