"""The rows' group keys in HBM: what `hr_group_select_dev`, `hr_group_select_n_dev` and the two group-mask kernels
(csrc/group.h) read.

Milvus groups a search on a scalar field server-side (`Collection.search(..., group_by_field=F)`).  Here the group keys of
a field (columns.PayloadColumns.group_keys: one int64 per row — an integer field as it is, the dictionary ordinal of a
string field's value) are mirrored onto the main shard's device the way device_tokens.py mirrors the token sets: uploaded
the first time a field is grouped on, extended in place by what later appends added, every row uploaded once.  Whatever
renumbers the rows (compact, load_snapshot, attach_shards) drops the mirror with the cached masks; it is rebuilt on first use.

A payload-free (synthetic) collection groups on what its hits show: doc_id = row // 10 and chunk_index = row % 10,
generated on the device.
"""
from __future__ import annotations

import threading
from typing import Any, Dict, Tuple

import numpy as np

from .columns import check_group_field

SYNTHETIC_GROUP_FIELDS = ("doc_id", "chunk_index")


def check_synthetic_group_field(field: str) -> str:
    check_group_field(field)
    if field not in SYNTHETIC_GROUP_FIELDS:
        raise ValueError("this shard was bulk-ingested without payload columns: only doc_id (= row // 10) and chunk_index "
                         f"(= row % 10) can be grouped on, not {[field]}")
    return field


def synthetic_group_keys(field: str, n: int) -> np.ndarray:
    """Host restatement of the generated keys of a payload-free collection."""
    rows = np.arange(n, dtype=np.int64)
    return rows // 10 if check_synthetic_group_field(field) == "doc_id" else rows % 10


def group_select_n_host(ids: np.ndarray, keys: np.ndarray, k_out: int, group_size: int):
    """numpy restatement of hr_group_select_n_dev for one list whose ids all lie in the key column: the valid prefix ends
    at the first id < 0.  -> (positions: one int array per selected group, the groups' keys, entries in the valid prefix)."""
    neg = np.flatnonzero(ids < 0)
    n = int(neg[0]) if neg.size else int(ids.shape[0])
    members: Dict[int, list] = {}          # insertion order = order of first appearance
    for i, k in enumerate(keys[ids[:n]].tolist()):
        at = members.get(k)
        if at is None:
            if len(members) == k_out:      # a group beyond the k_out-th: not selected, its members not counted
                continue
            at = members[k] = []
        if len(at) < group_size:
            at.append(i)
    return [np.asarray(at, dtype=np.int64) for at in members.values()], list(members), n


class DeviceGroupKeys:
    def __init__(self, columns, device: int):
        self.columns = columns                  # PayloadColumns, or None for a payload-free (synthetic) collection
        self.device = int(device)
        self._dev: Dict[str, Tuple[Any, int]] = {}   # field -> (int64 tensor with spare capacity, rows valid)
        self.stats = {"uploaded_bytes": 0, "host_build_s": 0.0}
        self._lock = threading.RLock()          # one caller grows the tensors at a time

    def tensor(self, field: str, n: int):
        """-> int64 CUDA tensor whose first n entries are the group keys of rows [0, n) for `field`.  Runs on the caller's
        current stream: a kernel enqueued behind it on that stream sees every row."""
        import time
        import torch
        dev = torch.device("cuda", self.device)
        with self._lock:
            cur, have = self._dev.get(field, (None, 0))
            if self.columns is None:
                check_synthetic_group_field(field)
                if cur is None or have < n:
                    rows = torch.arange(max(n, 1), dtype=torch.int64, device=dev)
                    cur = torch.div(rows, 10, rounding_mode="floor") if field == "doc_id" else rows % 10
                    self._dev[field] = (cur, n)
                    torch.cuda.current_stream(dev).synchronize()   # other threads read it on streams of their own
                return cur
            t0 = time.perf_counter()
            host = self.columns.group_keys(field)
            self.stats["host_build_s"] += time.perf_counter() - t0
            if host.shape[0] < n:
                raise ValueError(f"the payload columns hold {host.shape[0]} rows, the collection {n}")
            if cur is None or cur.shape[0] < n:
                cap = max(n, (cur.shape[0] * 3 // 2) if cur is not None else 0, 1024)
                grown = torch.empty(cap, dtype=torch.int64, device=dev)
                if cur is not None and have:
                    grown[:have] = cur[:have]
                cur = grown
            if have < n:
                part = np.ascontiguousarray(host[have:n])
                cur[have:n] = torch.from_numpy(part).to(dev)
                self.stats["uploaded_bytes"] += part.nbytes
                have = n
                torch.cuda.current_stream(dev).synchronize()       # other threads read it on streams of their own
            self._dev[field] = (cur, have)
            return cur

    @property
    def nbytes(self) -> int:
        """HBM held by the mirror (capacity, not only the valid part)."""
        return sum(t.numel() * t.element_size() for t, _ in self._dev.values())
