"""advanced_rag/staging.py on the CPU: the float32 [B, dim] stack of mixed query payloads, the upload of a packed sparse
batch and the result-list buffers, as the batching front, the index manager and the engine use them."""
import numpy as np
import pytest

from advanced_rag.engine import pack_sparse_queries
from advanced_rag.staging import dense_rows_host, list_buffers, upload_sparse

torch = pytest.importorskip("torch")
DIM = 8
_RNG = np.random.default_rng(0)
_ROWS = _RNG.standard_normal((3, DIM))            # float64: the float32 cast is part of what is checked

PAYLOADS = {
    "float64_1d": lambda v: v.copy(),
    "float32_1x8": lambda v: v.astype(np.float32).reshape(1, DIM),
    "list": lambda v: v.tolist(),
    "cpu_tensor_requires_grad": lambda v: torch.tensor(v, requires_grad=True),
}


def _check(got, rows):
    want = np.stack([r.astype(np.float32) for r in rows])
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and got.shape == (len(rows), DIM)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", sorted(PAYLOADS))
def test_dense_rows_host_takes_every_payload_form(form, B):
    _check(dense_rows_host([PAYLOADS[form](v) for v in _ROWS[:B]], DIM), _ROWS[:B])
    _check(dense_rows_host([PAYLOADS[form](v) for v in _ROWS[:B]]), _ROWS[:B])        # no dim: no check, same rows


def test_dense_rows_host_takes_a_mix_of_forms_in_one_batch():
    forms = ("cpu_tensor_requires_grad", "float32_1x8", "list")
    _check(dense_rows_host([PAYLOADS[f](v) for f, v in zip(forms, _ROWS)], DIM), _ROWS)


@pytest.mark.parametrize("B", [1, 3])
def test_a_row_of_the_wrong_width_is_refused_with_the_shard_message(B):
    with pytest.raises(ValueError) as e:
        dense_rows_host([v[:7] for v in _ROWS[:B]], DIM)
    assert str(e.value) == "query dim 7 != shard dim 8"


def test_upload_sparse_keeps_dtypes_values_and_max_nnz():
    packed = pack_sparse_queries([(np.array([9, 2, 5]), np.array([0.5, 1.0, 0.25])), ((), ())], 0.0, 16)
    ptr, idx, val, max_nnz = upload_sparse(packed, "cpu")
    assert (ptr.dtype, idx.dtype, val.dtype) == (torch.int64, torch.int32, torch.float32)
    assert ptr.tolist() == [0, 3, 3] and idx.tolist() == [2, 5, 9] and val.tolist() == [1.0, 0.25, 0.5]
    for got, want in zip((ptr, idx, val), packed):
        assert np.array_equal(got.numpy(), want)
    assert max_nnz == packed[3] == 3


def test_list_buffers_shapes_dtypes_and_zero_flags():
    ids, scores, flags = list_buffers(3, 5, "cpu")
    assert (ids.shape, ids.dtype) == ((3, 5), torch.int64)
    assert (scores.shape, scores.dtype) == ((3, 5), torch.float32)
    assert (flags.shape, flags.dtype) == ((3,), torch.int32) and not flags.any()
