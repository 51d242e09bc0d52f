"""The rows' token sets in HBM: what `hr_mmr_select_dev` (csrc/mmr.h) reads.

The reference diversifies a fused list on the token-Jaccard similarity of the hits' `content` (retrieval.py:493-516),
which it has on the host because every hit was formatted.  The one-round path formats only the hits it returns, so the
token sets (columns.TokenSetColumn: sorted int32 ids per row, CSR) are mirrored onto the main shard's device the way
device_filters.py mirrors the filter columns: uploaded on first use, extended in place by what later appends added,
every row uploaded once.  A payload-free (synthetic) collection formats `content` as "": its mirror has zero rows,
which the kernel reads as "every set empty".
"""
from __future__ import annotations

import threading
from typing import Any, Optional, Tuple

import numpy as np


class DeviceTokenSets:
    def __init__(self, columns, device: int, source=None):
        """source: PayloadColumns -> the host TokenSetColumn to mirror; None = `columns.token_sets()` (MMR's tokens).  The
        keyword filter (device_filters.py) mirrors `columns.word_sets()` through the same code."""
        self.columns = columns                  # PayloadColumns, or None for a payload-free (synthetic) collection
        self._source = source if source is not None else (lambda cols: cols.token_sets())
        self.device = int(device)
        self._indptr = None                     # int64 [capacity + 1], valid for rows <= _rows
        self._tok = None                        # int32 [capacity], valid below _used
        self._rows = 0
        self._used = 0
        self.stats = {"uploaded_bytes": 0, "host_build_s": 0.0}
        self._lock = threading.RLock()          # one caller grows the tensors at a time

    @staticmethod
    def _grown(torch, cur, need: int, valid: int, dtype, dev):
        if cur is not None and cur.shape[0] >= need:
            return cur
        cap = max(need, (cur.shape[0] * 3 // 2) if cur is not None else 0, 1024)
        grown = torch.empty(cap, dtype=dtype, device=dev)
        if cur is not None and valid:
            grown[:valid] = cur[:valid]
        return grown

    def tensors(self) -> Tuple[Optional[Any], Optional[Any], int]:
        """-> (indptr int64 CUDA tensor, tokens int32 CUDA tensor, rows); (None, None, 0) for a collection without
        contents.  Runs on the caller's current stream: a kernel enqueued behind it on that stream sees every row."""
        if self.columns is None:
            return None, None, 0
        import time
        import torch
        with self._lock:
            t0 = time.perf_counter()
            host = self._source(self.columns)
            self.stats["host_build_s"] += time.perf_counter() - t0
            n = len(host)
            if n == 0:
                return None, None, 0
            if n > self._rows:
                dev = torch.device("cuda", self.device)
                indptr, tok = host.indptr(), host.tokens()
                used = int(indptr[n])
                self._indptr = self._grown(torch, self._indptr, n + 1, self._rows + 1 if self._rows else 0, torch.int64, dev)
                self._tok = self._grown(torch, self._tok, max(used, 1), self._used, torch.int32, dev)
                part = np.ascontiguousarray(indptr[self._rows: n + 1])     # (rewrites indptr[_rows]: the same value)
                self._indptr[self._rows: n + 1] = torch.from_numpy(part).to(dev)
                self.stats["uploaded_bytes"] += part.nbytes
                if used > self._used:
                    part = np.ascontiguousarray(tok[self._used: used])
                    self._tok[self._used: used] = torch.from_numpy(part).to(dev)
                    self.stats["uploaded_bytes"] += part.nbytes
                self._rows, self._used = n, used
            return self._indptr, self._tok, self._rows

    @property
    def nbytes(self) -> int:
        """HBM held by the mirror (capacity, not only the valid part)."""
        return sum(t.numel() * t.element_size() for t in (self._indptr, self._tok) if t is not None)
