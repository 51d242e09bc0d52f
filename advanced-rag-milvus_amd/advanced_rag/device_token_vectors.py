"""The rows' token vectors in HBM: what `hr_maxsim_rerank_dev` (csrc/maxsim.h) reads.

columns.TokenVectorColumn (CSR over global rows: int64 indptr, fp16 [n_tok, token_dim]) is mirrored onto the main shard's
device the way device_tokens.DeviceTokenSets mirrors the token sets: uploaded on first use, extended in place by what
later appends added, every row uploaded once.  By construction the mirror holds 2 * token_dim bytes per token plus 8 per
row.  Whatever renumbers the rows (compact, load_snapshot, attach_shards) drops the mirror; it is rebuilt on next use.
"""
from __future__ import annotations

import threading
import time
from typing import Any, Optional, Tuple

import numpy as np


class DeviceTokenVectors:
    def __init__(self, columns, device: int):
        self.columns = columns                  # PayloadColumns with a token-vector column
        self.device = int(device)
        self._indptr = None                     # int64 [capacity + 1], valid for rows <= _rows
        self._val = None                        # fp16 [capacity, dim], valid below _used
        self._rows = 0
        self._used = 0
        self.stats = {"uploaded_bytes": 0, "host_build_s": 0.0}
        self._lock = threading.RLock()          # one caller grows the tensors at a time

    def tensors(self) -> Tuple[Optional[Any], Optional[Any], int]:
        """-> (indptr int64 CUDA tensor, values fp16 CUDA tensor [capacity, dim], rows); (None, None, 0) for a collection
        without rows.  Whatever was uploaded has arrived when the call returns: other threads read the tensors on streams
        of their own."""
        import torch
        with self._lock:
            t0 = time.perf_counter()
            host = self.columns.token_vectors()
            self.stats["host_build_s"] += time.perf_counter() - t0
            n = len(host) if host is not None else 0
            if n == 0:
                return None, None, 0
            if n > self._rows:
                dev = torch.device("cuda", self.device)
                indptr, val = host.indptr(), host.values()
                used = int(indptr[n])
                if self._indptr is None or self._indptr.shape[0] < n + 1:
                    grown = torch.empty(max(n + 1, (self._indptr.shape[0] * 3 // 2) if self._indptr is not None else 0, 1024),
                                        dtype=torch.int64, device=dev)
                    if self._indptr is not None and self._rows:
                        grown[: self._rows + 1] = self._indptr[: self._rows + 1]
                    self._indptr = grown
                if self._val is None or self._val.shape[0] < max(used, 1):
                    grown = torch.empty((max(used, (self._val.shape[0] * 3 // 2) if self._val is not None else 0, 1024), host.dim),
                                        dtype=torch.float16, device=dev)
                    if self._val is not None and self._used:
                        grown[: self._used] = self._val[: self._used]
                    self._val = grown
                part = np.ascontiguousarray(indptr[self._rows: n + 1])     # (rewrites indptr[_rows]: the same value)
                self._indptr[self._rows: n + 1] = torch.from_numpy(part).to(dev)
                self.stats["uploaded_bytes"] += part.nbytes
                if used > self._used:
                    part = np.ascontiguousarray(val[self._used: used])
                    self._val[self._used: used] = torch.from_numpy(part).to(dev)
                    self.stats["uploaded_bytes"] += part.nbytes
                self._rows, self._used = n, used
                torch.cuda.current_stream(dev).synchronize()
            return self._indptr, self._val, self._rows

    @property
    def nbytes(self) -> int:
        """HBM held by the mirror (capacity, not only the valid part)."""
        return sum(t.numel() * t.element_size() for t in (self._indptr, self._val) if t is not None)
