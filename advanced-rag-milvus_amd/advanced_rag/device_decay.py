"""The column a decay ranker reads, in HBM: what `hr_decay_rerank_dev` (csrc/decay.h) takes as d_col.

The INT64 / FLOAT fields (chunk_index, token_count, entropy, redundancy, domain_density) are the tensors the filter
evaluator already keeps (device_filters.DeviceFilters._column): no second copy.  The timestamp has no numeric form there —
filters compare its text through prefix keys — so its epoch seconds (columns.PayloadColumns.epoch_seconds, float64) get a
mirror of their own here, the way device_groups.DeviceGroupKeys mirrors the group keys: uploaded the first time a ranker
names the field, extended in place by what later appends added, every row uploaded once, 8 bytes per row.  Whatever
renumbers the rows (compact, load_snapshot, attach_shards) drops the mirror; it is rebuilt on first use.
"""
from __future__ import annotations

import threading
import time
from typing import Tuple

import numpy as np

from . import _native as nat
from .columns import INT_COLUMNS
from .decay import DECAY_FIELDS


def check_decay_field(field: str, synthetic: bool) -> str:
    """The field of a decay ranker on this collection, or ValueError: a payload-free (synthetic) collection has no
    timestamps and no scalar columns; only chunk_index (= row % 10) can be derived."""
    if field not in DECAY_FIELDS:
        raise ValueError(f"field must be one of {', '.join(DECAY_FIELDS)}, got {field!r}")
    if synthetic and field != "chunk_index":
        raise ValueError("this shard was bulk-ingested without payload columns: a decay ranker can read only chunk_index "
                         f"(= row % 10), not field={field!r}")
    return field


def host_values(columns, field: str, n_rows: int, rows: np.ndarray) -> np.ndarray:
    """float64 field value of every row of `rows` on the host (NaN for a row outside [0, n_rows)): what the restatement
    reads.  columns = PayloadColumns, or None for a payload-free collection."""
    rows = np.asarray(rows, dtype=np.int64)
    inside = (rows >= 0) & (rows < n_rows)
    at = np.where(inside, rows, 0)
    if columns is None:
        vals = (at % 10).astype(np.float64)
    elif field == "timestamp":
        vals = columns.epoch_seconds()[at] if n_rows else np.zeros(len(rows))
    else:
        vals = columns[field].array()[at].astype(np.float64) if n_rows else np.zeros(len(rows))
    return np.where(inside, vals, np.nan)


class DeviceDecayColumns:
    def __init__(self, columns, device: int):
        self.columns = columns                  # PayloadColumns, or None for a payload-free (synthetic) collection
        self.device = int(device)
        self._epoch = (None, 0)                 # (float64 tensor with spare capacity, rows valid)
        self.stats = {"uploaded_bytes": 0, "host_build_s": 0.0}
        self._lock = threading.RLock()          # one caller grows the tensor at a time

    def tensor(self, field: str, n: int, filters) -> Tuple[object, int]:
        """-> (CUDA tensor whose first n entries are the field's values of rows [0, n), its HR_COL_* kind).  Runs on the
        caller's current stream: a kernel enqueued behind it on that stream sees every row, and whatever was uploaded has
        arrived when the call returns (other threads read the tensors on streams of their own).  filters = the collection's
        DeviceFilters, owner of the INT64 / FLOAT columns."""
        if field != "timestamp":
            import torch
            with filters._lock:
                # _column queues the copy of rows it has not uploaded yet (and of the old rows when it grows) on the CURRENT
                # stream and records them as present at once.  Inside DeviceFilters.evaluate, its only caller so far, the
                # stream is drained before the lock is given up; here it must be too, or a filter evaluation on another
                # stream would find the rows "there" and read memory the copy has not reached
                before = {k: (id(v[0]), v[1]) for k, v in filters._dev.items()}
                t = filters._column(field, n)
                if {k: (id(v[0]), v[1]) for k, v in filters._dev.items()} != before:
                    torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()
            return t, nat.HR_COL_I64 if (field in INT_COLUMNS or self.columns is None) else nat.HR_COL_F32
        import torch
        dev = torch.device("cuda", self.device)
        with self._lock:
            cur, have = self._epoch
            t0 = time.perf_counter()
            host = self.columns.epoch_seconds()          # the first use parses every row on the host, once
            self.stats["host_build_s"] += time.perf_counter() - t0
            if host.shape[0] < n:
                raise ValueError(f"the payload columns hold {host.shape[0]} rows, the collection {n}")
            if cur is None or cur.shape[0] < n:
                cap = max(n, (cur.shape[0] * 3 // 2) if cur is not None else 0, 1024)
                grown = torch.empty(cap, dtype=torch.float64, device=dev)
                if cur is not None and have:
                    grown[:have] = cur[:have]
                cur = grown
            if have < n:
                part = np.ascontiguousarray(host[have:n])
                cur[have:n] = torch.from_numpy(part).to(dev)
                self.stats["uploaded_bytes"] += part.nbytes
                have = n
                torch.cuda.current_stream(dev).synchronize()       # other threads read it on streams of their own
            self._epoch = (cur, have)
            return cur, nat.HR_COL_F64

    @property
    def nbytes(self) -> int:
        """HBM held by the epoch mirror (capacity, not only the valid part)."""
        t = self._epoch[0]
        return t.numel() * t.element_size() if t is not None else 0
