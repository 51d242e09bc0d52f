"""The rows' group keys in HBM: what `hr_group_select_dev`, `hr_group_select_n_dev` and the two group-mask kernels
(csrc/group.h) read — and the manager's blocking grouped search over them (grouped_search, on the device or the host form).

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
from typing import Any, Dict, List, Tuple

import numpy as np

from ._native import HR_MAX_TOPK   # importing the binding module does not load the library
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


def grouped_search(manager, path, top_k: int, filters, field: str, group_size: int, window: int):
    """The exact grouped ranking of ONE query (the manager's blocking loop; path: its indexing.SearchPath, window: its
    group_window(top_k, group_size)): for the first top_k groups of the collection's ranking R (filter expression and
    tombstones applied; groups ordered by their first row in R), the first min(group_size, members in R) rows of each
    -> (rows, scores), groups in group order, a group's rows adjacent and in R order.

    Phase 1 reads R a window of K' rows at a time through the host forms, which are exact, with a select that emits up
    to group_size members per group from the window in which the group first appears.  A window that holds top_k new
    groups, or fewer than K' rows (the search ran out of qualifying rows), ends the phase.  Otherwise every group of the
    window has been taken, so no other row of those groups can ever start a group: they leave the working mask and the
    next window is searched without them.  The remaining ranking is the old one minus rows that could not be selected, and
    every continuation removes at least one whole group, so the phase ends.  A window is a prefix of the masked ranking,
    so a group with group_size members in it is closed (they are its best), and so is every group of a window that was
    not full (the ranking ran out).  With group_size == 1 every selected group is closed at once: phase 1 is the answer.

    Phase 2 fills the open groups O: the base mask AND "key in O", one search of K2 = min(HR_MAX_TOPK, max(|O| *
    group_size, K')) rows.  Restricting R to some groups keeps its order, so a group's first rows in that list are
    its first rows in R.  A list that is not full closes every group; a full one spreads >= |O| * group_size rows over
    at most |O| groups, so one of them holds group_size and closes: at most |O| rounds (top_k * group_size <=
    HR_MAX_TOPK keeps K2 >= |O| * group_size)."""
    g = group_size
    count = manager._count
    be = (HostGroups if path.shard is None else DeviceGroups)(manager, path, filters, field)
    groups: List[list] = []            # [key, rows, scores, closed] in group order
    count("group_searches")
    mask = be.base
    while True:
        ids, sc = be.search(mask, window)
        count("group_rounds")
        at, keys, n_valid = be.select(ids, top_k - len(groups), g)
        for a, k in zip(at, keys):
            groups.append([k, ids[a], sc[a], len(a) == g or n_valid < window])
        if len(groups) == top_k or n_valid < window:
            break
        mask = be.drop(mask, keys)     # every group of the window was selected: none of their rows can be selected again
        count("group_continuations")
    open_ = [grp for grp in groups if not grp[3]]
    if open_:
        count("group_fill_searches")
    while open_:
        k2 = min(HR_MAX_TOPK, max(len(open_) * g, window))
        ids, sc = be.search(be.keep([grp[0] for grp in open_]), k2)
        count("group_fill_rounds")
        at, keys, n_valid = be.select(ids, len(open_), g)
        found = dict(zip(keys, at))
        for grp in open_:
            a = found.get(grp[0])
            if a is not None and len(a) >= len(grp[1]):      # (both are prefixes of the group's rows in R)
                grp[1], grp[2] = ids[a], sc[a]
            grp[3] = n_valid < k2 or len(grp[1]) == g
        still = [grp for grp in open_ if not grp[3]]
        if len(still) == len(open_):
            raise RuntimeError("grouping search: a full fill window closed no group")      # the pigeonhole step failed
        open_ = still
    if not groups:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate([grp[1] for grp in groups]), np.concatenate([grp[2] for grp in groups])


class HostGroups:
    """What grouped_search runs on when the masks are host arrays (several shards, the torchrun form, stand-in managers):
    numpy restatements of the kernels over boolean row masks.  Like DeviceGroups it offers base / search(mask, k) ->
    (ids [k], scores [k]) / select(ids, k_out, g) -> (positions per group, keys, valid entries) / drop(mask, keys) ->
    mask / keep(keys) -> base restricted to the keys."""

    def __init__(self, manager, path, filters, field: str):
        self.n = manager.num_rows
        self.keys = manager._host_group_keys(field)
        self.base = path.base(filters)                                           # cached and shared: never written here
        self.search = path.search

    def select(self, ids, k_out, g):
        return group_select_n_host(ids, self.keys, k_out, g)

    def _has_key(self, keys):
        return np.isin(self.keys[:self.n], np.asarray(keys, dtype=np.int64))

    def drop(self, mask, keys):
        gone = self._has_key(keys)
        return ~gone if mask is None else (mask[:self.n] & ~gone)

    def keep(self, keys):
        kept = self._has_key(keys)
        return kept if self.base is None else (self.base[:self.n] & kept)


class DeviceGroups:
    """What grouped_search runs on for one local GPU shard: hr_group_select_n_dev, hr_mask_drop_groups_dev,
    hr_mask_keep_groups_dev, masks in HBM.  The searches run on a stream of the library's own, so a mask kernel is
    synchronised before the next search; the one copy that reads a select's outputs back orders the select."""

    def __init__(self, manager, path, filters, field: str):
        import torch
        self.nat, self.n = manager._native, manager.num_rows
        self.dev = dev = torch.device("cuda", path.shard.device)
        with torch.cuda.device(dev):
            self.keys = manager._group_keys_on_device().tensor(field, self.n)
            self.base = path.base(filters)                                       # cached and shared: never written here
            self.work = [None, None]                                             # this query's drop mask and keep mask
            # what a select writes, in one buffer so that one copy reads it back: the groups' keys (int64 [K]), the positions
            # (int32 [K]: k_out * g <= K), the members per group (int32 [K]) and the number of groups (int32), K = HR_MAX_TOPK
            self.out = torch.empty(4 * HR_MAX_TOPK + 1, dtype=torch.int32, device=dev)
        self.search = path.search

    def select(self, ids, k_out, g):
        import torch
        K = HR_MAX_TOPK
        if not (k_out <= K and k_out * g <= K):      # (the request checks keep to it; the kernel itself would write more)
            raise ValueError(f"a group select writes at most HR_MAX_TOPK = {K} positions, got {k_out} * {g}")
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            d_ids = torch.from_numpy(ids).to(self.dev)
            out = self.out.data_ptr()
            self.nat.group_select_n_dev(d_ids.data_ptr(), 0, 1, len(ids), self.keys.data_ptr(), self.n, 0, k_out, g,
                                        out + 8 * K, out, out + 12 * K, out + 16 * K, 0, stream.cuda_stream)
            got = self.out.cpu().numpy()                                         # synchronises the stream
        keys, pos, cnt = got[:2 * K].view(np.int64), got[2 * K:3 * K].astype(np.int64), got[3 * K:]
        n_sel = int(cnt[K])
        neg = np.flatnonzero(ids < 0)
        return ([pos[o * g:o * g + int(cnt[o])] for o in range(n_sel)], keys[:n_sel].tolist(),
                int(neg[0]) if neg.size else len(ids))

    def _mask_op(self, op, slot, mask, keys):
        import torch
        from .device_filters import mask_bytes
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            if self.work[slot] is None:
                self.work[slot] = torch.empty(mask_bytes(self.n), dtype=torch.uint8, device=self.dev)
            d_set = torch.tensor(keys, dtype=torch.int64, device=self.dev)
            op(mask.data_ptr() if mask is not None else 0, self.work[slot].data_ptr(), self.n, self.keys.data_ptr(),
               d_set.data_ptr(), len(keys), stream.cuda_stream)
            stream.synchronize()      # the search reads the mask on a stream of its own
        return self.work[slot]

    def drop(self, mask, keys):
        return self._mask_op(self.nat.mask_drop_groups_dev, 0, mask, keys)

    def keep(self, keys):
        return self._mask_op(self.nat.mask_keep_groups_dev, 1, self.base, keys)


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
