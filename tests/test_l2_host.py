"""HR_METRIC_L2 on the host side: the ABI constant, the metric helper, the ascending merge, the manager's metric
handling (stub handles, no GPU) and the yardstick checking itself."""
import os
import re

import numpy as np
import pytest

from advanced_rag import _native as nat
from advanced_rag.indexing import MilvusIndexManager, ShardCollection, metric_code
from advanced_rag.shards import ShardSet, merge_lists

from l2_yardstick import bits, l2_dist_np, l2_dist_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree_on_the_metric_code():
    text = open(os.path.join(ROOT, "include", "hbmrag.h")).read()
    m = re.search(r"HR_METRIC_L2\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 2
    assert nat.HR_METRIC_L2 == 2
    assert (nat.HR_METRIC_IP, nat.HR_METRIC_COSINE) == (0, 1)
    assert "hr_merge_topk_asc_dev" in nat.EXPORTED_SYMBOLS and "hr_merge_topk_asc_dev" in text


def test_metric_helper_maps_three_names_and_rejects_the_rest():
    assert metric_code("L2") == nat.HR_METRIC_L2
    assert metric_code("IP") == nat.HR_METRIC_IP
    assert metric_code("COSINE") == nat.HR_METRIC_COSINE
    for bad in ("l2", "EUCLIDEAN", "", None, 2, "HAMMING"):
        with pytest.raises(ValueError):
            metric_code(bad)
    with pytest.raises(ValueError):
        MilvusIndexManager(connect=False, semantic_metric="JACCARD")
    with pytest.raises(ValueError):
        MilvusIndexManager(connect=False, domain_metric="l2")


def test_merge_lists_ascending():
    # shard 0 and shard 1 hold rows at EQUAL distances (0.5: ids 7 and 3; 2.0: ids 9 and 1), -1 padding in shard 1
    ids = [np.array([[7, 9, 20]], np.int64), np.array([[3, 1, -1]], np.int64)]
    sc = [np.array([[0.5, 2.0, 3.0]], np.float32), np.array([[0.5, 2.0, 0.0]], np.float32)]
    oi, os_ = merge_lists(ids, sc, 4, ascending=True)
    assert oi.tolist() == [[3, 7, 1, 9]]
    assert os_.tolist() == [[0.5, 0.5, 2.0, 2.0]]
    oi, os_ = merge_lists(ids, sc, 8, ascending=True)
    assert oi.tolist() == [[3, 7, 1, 9, 20, -1, -1, -1]]
    assert os_.tolist() == [[0.5, 0.5, 2.0, 2.0, 3.0, 0.0, 0.0, 0.0]]
    # a distance of exactly 0 is a hit, not padding
    oi, os_ = merge_lists([np.array([[4, -1]], np.int64), np.array([[2, 5]], np.int64)],
                          [np.array([[0.0, 0.0]], np.float32), np.array([[0.0, 1.0]], np.float32)], 3, ascending=True)
    assert oi.tolist() == [[2, 4, 5]] and os_.tolist() == [[0.0, 0.0, 1.0]]
    # the default stays (score desc, id asc)
    oi, _ = merge_lists(ids, sc, 3)
    assert oi.tolist() == [[20, 1, 9]]


class _Stub:
    """A shard handle as far as the host logic looks at one."""
    device, sparse_dim, num_rows, num_sparse_rows = 0, 0, 0, 0

    def __init__(self, metric=None):
        if metric is not None:
            self.metric = metric


def test_shardset_merges_an_l2_collection_ascending():
    class H(_Stub):
        def __init__(self, ids, sc):
            super().__init__(nat.HR_METRIC_L2)
            self._ids, self._sc, self.num_rows = ids, sc, 4

        def search_dense(self, q, k, *mask):
            return self._ids, self._sc

    a = H(np.array([[0, 1]], np.int64), np.array([[1.0, 4.0]], np.float32))
    b = H(np.array([[1, 0]], np.int64), np.array([[1.0, 2.0]], np.float32))
    s = ShardSet([a, b])
    s.rows_of = [np.array([0, 1, 2, 3], np.int64), np.array([10, 11, 12, 13], np.int64)]
    ids, sc = s.search_dense(np.zeros((1, 4), np.float32), 3)
    assert ids.tolist() == [[0, 11, 10]] and sc.tolist() == [[1.0, 1.0, 2.0]]


def test_search_params_follow_the_collection_metric():
    m = MilvusIndexManager(connect=False)
    for label in ("L2", "IP", "COSINE"):
        coll = ShardCollection(m, "semantic_index", "dense", _Stub(), 8, label)
        assert m._search_params(coll, None)["metric_type"] == label
        assert m._search_params(coll, {"metric_type": label, "params": {"ef": 8}})["metric_type"] == label
        other = "COSINE" if label != "COSINE" else "L2"
        with pytest.raises(ValueError):
            m._search_params(coll, {"metric_type": other})
    sparse = ShardCollection(m, "sparse_index", "sparse", _Stub(), 8, "IP")
    assert m._search_params(sparse, None)["metric_type"] == "IP"


def test_attach_shards_takes_the_label_from_the_handle():
    for metric, label in ((nat.HR_METRIC_L2, "L2"), (nat.HR_METRIC_IP, "IP"), (nat.HR_METRIC_COSINE, "COSINE"), (None, "COSINE")):
        m = MilvusIndexManager(connect=False, semantic_dim=8)
        m.attach_shards([_Stub(metric)])
        assert m.collections["semantic_index"].metric == label
        assert m._search_params(m.collections["semantic_index"], None)["metric_type"] == label


def test_manager_defaults_stay_cosine():
    m = MilvusIndexManager(connect=False)
    assert (m.semantic_metric, m.domain_metric) == ("COSINE", "COSINE")
    m = MilvusIndexManager(connect=False, semantic_metric="L2", domain_metric="IP")
    assert (m.semantic_metric, m.domain_metric) == ("L2", "IP")


@pytest.mark.parametrize("np_dtype", [np.float16, np.float32])
def test_yardstick_equals_a_scalar_loop(np_dtype):
    rng = np.random.default_rng(11)
    X = (rng.standard_normal((40, 37)) * 3).astype(np.float32).astype(np_dtype)
    X[5] = 0
    Q = rng.standard_normal((3, 37)).astype(np.float32)
    Q[2] = X[7].astype(np.float32)
    for q in Q:
        want = np.array([l2_dist_py(x, q) for x in X], np.float32)
        assert np.array_equal(bits(l2_dist_np(X, q)), bits(want))
    assert l2_dist_np(X, Q[2])[7] == 0.0
