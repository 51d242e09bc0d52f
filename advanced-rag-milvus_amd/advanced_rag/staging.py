"""Staging of a query batch for the device searches, once for the batching front, the index manager and the engine: stack
the dense payloads into one float32 [B, dim] array, upload a packed sparse batch, allocate the result lists."""
from __future__ import annotations

import numpy as np


def dense_rows_host(payloads, dim=None) -> np.ndarray:
    """float32, C-contiguous [B, d] from B query payloads: numpy arrays of any float dtype and any shape that flattens to
    one row, Python sequences, torch tensors (CPU or CUDA, with or without requires_grad).  With `dim`, d must equal it."""
    rows = np.stack([np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float32).reshape(-1)
                     for x in payloads])
    if dim is not None and rows.shape[1] != dim:
        raise ValueError(f"query dim {rows.shape[1]} != shard dim {dim}")
    return rows


def dense_rows_device(payloads, dev, dim):
    """The same batch as a contiguous float32 [B, dim] tensor on `dev`: payloads that are ALL CUDA tensors (embedding table,
    encoder output) are stacked where they are, anything else takes dense_rows_host and one upload.  Both arms check the width."""
    import torch
    if all(getattr(x, "is_cuda", False) for x in payloads):
        q = torch.stack([x.reshape(-1).to(torch.float32) for x in payloads]).contiguous()
        if q.shape[1] != dim:
            raise ValueError(f"query dim {q.shape[1]} != shard dim {dim}")
        return q
    return torch.from_numpy(dense_rows_host(payloads, dim)).to(dev)


def csr_of_queries(queries):
    """B sparse queries [(indices, values)] -> their raw CSR (indptr int64 [B + 1], idx int32 [nnz], val float32 [nnz]), the
    entries as they came: nothing dropped, nothing sorted (engine.pack_sparse_queries does both, for the device forms)."""
    indptr = np.zeros(len(queries) + 1, dtype=np.int64)
    for b, (qi, qv) in enumerate(queries):
        if len(qi) != len(qv):
            raise ValueError(f"sparse query {b} has {len(qi)} indices and {len(qv)} values")
        indptr[b + 1] = indptr[b] + len(qi)
    if not indptr[-1]:
        return indptr, np.zeros(0, np.int32), np.zeros(0, np.float32)
    return (indptr, np.concatenate([np.asarray(qi, dtype=np.int32) for qi, _ in queries]),
            np.concatenate([np.asarray(qv, dtype=np.float32) for _, qv in queries]))


def upload_sparse(packed, dev):
    """engine.pack_sparse_queries' (indptr, idx, val, max_nnz) -> the three arrays as tensors on `dev`, max_nnz as it came."""
    import torch
    indptr, idx, val, max_nnz = packed
    return torch.from_numpy(indptr).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(val).to(dev), max_nnz


def list_buffers(B: int, k: int, dev):
    """(ids int64 [B, k], scores float32 [B, k], flags int32 [B]) for a device search to fill; the flags start at 0
    ("not proven"), the lists are uninitialised."""
    import torch
    return (torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
            torch.zeros((B,), dtype=torch.int32, device=dev))
