"""A collection spread over several shard handles, searched as one.

The reference hides sharding behind the index manager: a collection is created
with `num_shards=4` and Milvus merges its segments server-side (reference
src/advanced_rag/indexing.py:234-239, :503-525).  `ShardSet` is the counterpart
for the in-HBM store: S shard handles (one per GPU of the node — or several on
one GPU, which is how the one-GPU tests exercise it), rows appended in balanced
pieces, every search run on all shards in parallel (one thread per shard: the
ctypes calls release the GIL and each handle owns its streams) and the S
per-shard lists merged by the same (score desc, global row asc) rule the kernels
use, so the answer is the one a single shard holding all rows would give.

Rows keep ONE global numbering (insertion order), which is what the host payload
columns are keyed by; each shard records which global rows it holds
(`rows_of[s]`, ascending — so a shard's local order is the global order and
per-shard lists stay exactly ordered after renumbering).  Row filters arrive as
a boolean array over global rows and are cut into per-shard bitmasks.
"""
from __future__ import annotations

import threading
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import wire
from ._native import HR_METRIC_L2   # a handle of that metric returns squared distances, smallest first
from .staging import csr_of_queries


def dense_ascending(handle) -> bool:
    """True when `handle`'s dense lists are distances (ascending): an L2 shard.  Handles without a `metric` (test stubs)
    are similarity shards."""
    return getattr(handle, "metric", None) == HR_METRIC_L2


def is_native_handle(handle) -> bool:
    """True for a libhbmrag shard (row masks are kept in its HBM, the device forms exist); False for a test stand-in."""
    return getattr(handle, "_h", None) is not None


def empty_lists(B: int, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """The [B, k] lists of a shard that holds no row: ids all -1, scores 0."""
    return np.full((B, k), -1, np.int64), np.zeros((B, k), np.float32)


def to_global(local_ids: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """A handle's lists of LOCAL rows -> global rows through its row map `rows`; the -1 padding stays -1."""
    if not len(rows):
        return np.full(local_ids.shape, -1, np.int64)
    return np.where(local_ids >= 0, rows[np.maximum(local_ids, 0)], -1).astype(np.int64)


def merge_lists(ids: Sequence[np.ndarray], scores: Sequence[np.ndarray], k: int,
                ascending: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """Merge per-shard top-k lists ([B,k] each, -1 padded) -> [B,k] by (score desc, id asc); with ascending=True (the
    distance lists of an L2 collection) by (score asc, id asc)."""
    all_ids = np.concatenate(ids, axis=1)
    all_sc = np.concatenate(scores, axis=1)
    B = all_ids.shape[0]
    out_ids = np.full((B, k), -1, dtype=np.int64)
    out_sc = np.zeros((B, k), dtype=np.float32)
    for b in range(B):
        live = np.nonzero(all_ids[b] >= 0)[0]
        key = all_sc[b][live].astype(np.float64)
        order = live[np.lexsort((all_ids[b][live], key if ascending else -key))][:k]
        out_ids[b, :len(order)] = all_ids[b][order]
        out_sc[b, :len(order)] = all_sc[b][order]
    return out_ids, out_sc


def merge_deep_lists(ids: Sequence[np.ndarray], scores: Sequence[np.ndarray], top_k: int, offset: int = 0,
                     ascending: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """Per-shard deep lists (each [B, W] at depth W = offset + top_k with offset 0, global rows, -1 padded) -> entries
    offset .. offset + top_k - 1 of their merge by (score desc or distance asc, row asc), [B, top_k], -1 / 0 padded.  A row
    of the collection's first W is among its own shard's first W, so the merge of the shards' lists is the collection's."""
    m_ids, m_sc = merge_lists(ids, scores, offset + top_k, ascending)
    return np.ascontiguousarray(m_ids[:, offset:]), np.ascontiguousarray(m_sc[:, offset:])


# ---- ranking keys on the host: the numpy twins of ord_f32 / rank_key (csrc/common.h) and deep_key_interval (csrc/deep.h)
KEY_EVERYTHING = (0, 2 ** 64 - 1)     # the open interval that holds every key of a finite score


def ord_f32(score) -> np.ndarray:
    """fp32 -> uint32 of the same order (+0.0 above -0.0): sign bit set = all bits flipped, else the sign bit set."""
    u = np.asarray(score, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def rank_key(score, row) -> np.ndarray:
    """The unique 64-bit ranking key of (score, row), row in 0 .. 2^32 - 1: (score desc, row asc) <=> key desc."""
    return (ord_f32(score).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(row).astype(np.uint64))


def cursor_key_interval(after, bounds, metric: str, row_offset: int = 0) -> Tuple[int, int]:
    """What the library makes of one query's cursor and range bounds (hr_search_*_deep_after): the open interval (lo, hi)
    of ranking keys a page is selected from, as Python integers.

    after = (score, id) of the last hit seen, or None: kept are the rows strictly after it — score worse, or score equal
    and id larger.  id is any integer, a position, not a row that has to exist: with id - row_offset below 0 every row of
    that score follows, beyond the 32-bit row space none does.  bounds = (radius, range_filter) as range_bounds() returns
    them, or None; a side may be None or infinite (unbounded).  Under L2 the cursor's score and the bounds are distances
    and are negated into the key domain.  A bound is first taken to the fp32 that cuts the fp32 scores where the float64
    does (_native.f32_bound); a zero bound is +0.0, so that -0.0 and +0.0 scores fall on the same side, while the cursor's
    score is used bit for bit.  ValueError: a non-finite cursor score, a NaN bound, an empty interval (range_bounds' rule)."""
    from ._native import f32_bound
    if metric not in ("L2", "IP", "COSINE"):
        raise ValueError(f"unknown metric_type {metric!r}")
    l2 = metric == "L2"
    lo, hi = KEY_EVERYTHING
    if bounds is not None:
        radius = (np.inf if l2 else -np.inf) if bounds[0] is None else float(bounds[0])
        range_filter = (-np.inf if l2 else np.inf) if bounds[1] is None else float(bounds[1])
        if radius != radius or range_filter != range_filter:
            raise ValueError("NaN range bound")
        radius, range_filter = float(f32_bound(radius, l2)[0]), float(f32_bound(range_filter, l2)[0])
        if (range_filter >= radius) if l2 else (radius >= range_filter):
            raise ValueError(f"empty range for {metric}: radius={radius}, range_filter={range_filter}")
        above, upto = (-radius, -range_filter) if l2 else (radius, range_filter)     # kept: above < score <= upto
        if above != -np.inf:
            lo = (int(ord_f32(np.float32(above) + np.float32(0.0))) << 32) | 0xFFFFFFFF     # x + 0.0: -0.0 becomes +0.0
        if upto != np.inf:
            hi = (int(ord_f32(np.float32(upto) + np.float32(0.0))) + 1) << 32
    if after is not None:
        with np.errstate(over="ignore"):
            score = np.float32(after[0])
        if not np.isfinite(score):
            raise ValueError(f"non-finite cursor score {after[0]!r}")
        top = int(ord_f32(-score if l2 else score)) << 32
        row = int(after[1]) - int(row_offset)
        hi = min(hi, top + (1 << 32) if row < 0 else top if row > 0xFFFFFFFF else top | (0xFFFFFFFF - row))
    return lo, hi


def page_after(ids: np.ndarray, scores: np.ndarray, k: int, after, bounds, ascending: bool) -> Tuple[np.ndarray, np.ndarray]:
    """The cursor forms restated on complete rankings: ids / scores [B, n] (-1 padded, in ranking order) -> the first k
    entries of each that lie inside the query's key interval, [B, k], -1 / 0 padded.  after = (scores [B], ids [B], has
    [B]) or None.  Used for shard stand-ins that rank on the host."""
    B = ids.shape[0]
    out_ids, out_sc = empty_lists(B, k)
    metric = "L2" if ascending else "IP"
    for b in range(B):
        cur = None if after is None or not after[2][b] else (after[0][b], after[1][b])
        lo, hi = cursor_key_interval(cur, bounds, metric)
        live = np.flatnonzero(ids[b] >= 0)
        key = rank_key(-scores[b][live] if ascending else scores[b][live], ids[b][live])
        take = live[(key > np.uint64(lo)) & (key < np.uint64(hi))][:k]
        out_ids[b, :len(take)], out_sc[b, :len(take)] = ids[b][take], scores[b][take]
    return out_ids, out_sc


class PartialAppend(RuntimeError):
    """A multi-shard append failed after some pieces had gone in: global rows [base, end) exist in the shards."""

    def __init__(self, base: int, end: int, cause: Exception):
        super().__init__(f"append stopped after rows [{base}, {end}): {cause}")
        self.base, self.end, self.cause = base, end, cause


class ShardSet:
    def __init__(self, handles: list):
        if not handles:
            raise ValueError("a ShardSet needs at least one shard handle")
        self.handles = list(handles)
        self.rows_of: List[np.ndarray] = [np.zeros(0, np.int64) for _ in handles]  # global row of each local row
        self._n = 0
        self._packed = None   # (filter array, {shard: packed mask}) of the filter used last
        # Searches with different filters run at the same time (the requests of one multi_search, each in its thread; the
        # shards of one search in the pool's threads).  The lock makes "look up or build" one step.  A search is handed a
        # raw device pointer into the entry, and another thread's filter may replace the entry while that search runs: each
        # thread keeps the entry it was handed last alive until it asks for the next one.
        self._packed_lock = threading.Lock()
        self._packed_held = threading.local()
        self._pool = ThreadPoolExecutor(max_workers=len(handles), thread_name_prefix="shard-") if len(handles) > 1 else None

    # ------------------------------------------------------------------ shape
    @property
    def n_shards(self) -> int:
        return len(self.handles)

    @property
    def first(self):
        return self.handles[0]

    @property
    def device(self) -> int:
        return self.handles[0].device

    @property
    def num_rows(self) -> int:
        return sum(h.num_rows for h in self.handles)

    @property
    def num_sparse_rows(self) -> int:
        return sum(h.num_sparse_rows for h in self.handles)

    @property
    def device_bytes(self) -> int:
        return sum(h.device_bytes for h in self.handles)

    # ------------------------------------------------------------------ ingest
    def _pieces(self, n: int) -> List[Tuple[int, int, int]]:
        """Cut a batch of n rows into contiguous pieces, one per shard, filling the emptiest shards first:
        -> [(shard, lo, hi)] with the pieces in row order."""
        S = self.n_shards
        if S == 1:
            return [(0, 0, n)]
        have = np.array([len(r) for r in self.rows_of], dtype=np.int64)
        target = (have.sum() + n + S - 1) // S
        want = np.maximum(target - have, 0)
        pieces, lo = [], 0
        for s in np.argsort(have, kind="stable"):
            take = int(min(want[s], n - lo))
            if take > 0:
                pieces.append((int(s), lo, lo + take))
                lo += take
        if lo < n:  # rounding leftovers: to the emptiest shard
            s = int(np.argmin(have))
            pieces.append((s, lo, n))
        return pieces

    def add(self, dense, sparse_csr=None, n: Optional[int] = None):
        """Append rows (dense [n, dim] and/or a CSR triple of n rows) to the shards; both parts of a row go to the
        same shard.  `dense` is a numpy array (host rows, uploaded) or a CUDA tensor already in the shard's storage
        dtype (an encoder's output: re-tiled device to device by hr_add_dense_raw_dev, no host hop).
        Returns (base, end, sparse_error): the global row range [base, end) and, if a shard refused
        the sparse part of its piece, that error — the piece then got EMPTY sparse rows instead, because the row
        number is the only join key between the dense rows, the sparse rows and the host payload columns.
        A dense failure part-way (say, one device out of memory) raises PartialAppend carrying the rows that did go
        in, so that the caller can keep its payload columns aligned with them."""
        n = dense.shape[0] if dense is not None else (len(sparse_csr[0]) - 1 if sparse_csr is not None else int(n or 0))
        base = self._n
        sparse_error = None
        on_device = dense is not None and hasattr(dense, "is_cuda")
        for s, lo, hi in self._pieces(n):
            h = self.handles[s]
            if dense is not None:
                try:
                    if on_device:
                        self._add_dense_device(h, dense[lo:hi])
                    else:
                        h.add_dense(dense[lo:hi])
                except Exception as e:
                    if self._n > base:   # earlier pieces are in: tell the caller how many rows the set gained
                        raise PartialAppend(base, self._n, e) from e
                    raise
            if sparse_csr is not None:
                ptr, idx, val = sparse_csr
                ptr = np.asarray(ptr, dtype=np.int64)
                try:
                    h.add_sparse(ptr[lo:hi + 1], idx, val)  # hr_add_sparse reads idx/val at absolute indptr positions
                except Exception as e:  # keep the numbering aligned, report
                    sparse_error = e
                    h.add_sparse(np.zeros(hi - lo + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
            self.rows_of[s] = np.concatenate([self.rows_of[s], np.arange(base + lo, base + hi, dtype=np.int64)])
            self._n = base + hi  # pieces are in row order: a failure further on leaves a consistent prefix
        return base, base + n, sparse_error

    @staticmethod
    def _add_dense_device(h, rows):
        """rows: CUDA tensor [m, dim] in the shard's storage dtype (fp16 / fp32); copied to the shard's GPU if needed."""
        import torch
        want = torch.float16 if h.dtype == 1 else torch.float32
        if rows.dtype != want:
            raise ValueError(f"device rows are {rows.dtype}, the shard stores {want}")
        if rows.dim() != 2 or rows.shape[1] != h.dim:
            raise ValueError(f"rows must be [n,{h.dim}], got {tuple(rows.shape)}")
        if rows.device.index != h.device:
            rows = rows.to(f"cuda:{h.device}")
        rows = rows.contiguous()
        stream = torch.cuda.current_stream(rows.device)
        h.add_dense_dev(rows.data_ptr(), rows.shape[0], stream.cuda_stream)   # synchronises the stream before it returns

    def finalize(self):
        for h in self.handles:
            h.finalize()

    def compact(self, keep_global: np.ndarray, d_keep: int = 0) -> int:
        """Remove the rows whose entry of `keep_global` (boolean, over GLOBAL rows) is False from every shard for good
        (hr_compact) and renumber the survivors: new global row = kept rows before it.  Returns the rows left.
        d_keep: the same mask packed in HBM; used instead of an upload when the set is one native shard whose local rows
        are the global rows.  While the shards are processed every row map is cut down but keeps the OLD numbers; the maps
        are renumbered only after the last shard has succeeded.  If a shard fails the error is raised with the set still
        consistent under the old numbering: the shards done so far have merely lost rows the mask hides anyway.
        A maintenance call: no search may run meanwhile."""
        keep = np.asarray(keep_global, dtype=bool)
        if keep.ndim != 1 or any(len(r) and int(r[-1]) >= len(keep) for r in self.rows_of):
            raise ValueError(f"keep mask covers {keep.shape} rows, the set holds rows up to {self._n}")
        self._packed = None     # packed copies of filters are cut by local row: stale from the first shard on
        for s, h in enumerate(self.handles):
            rows = self.rows_of[s]
            own = keep[rows]
            if own.all():
                continue
            if d_keep and self.n_shards == 1 and is_native_handle(h) and np.array_equal(rows, np.arange(len(rows))):
                h.compact(d_keep=d_keep)
            else:
                h.compact(own)
            self.rows_of[s] = rows[own]
        new_of = np.cumsum(keep, dtype=np.int64) - 1
        self.rows_of = [new_of[r] for r in self.rows_of]
        self._n = int(np.count_nonzero(keep[:self._n]))
        return self._n

    def close(self):
        for h in self.handles:
            h.close()
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    # ------------------------------------------------------------------ search
    def _local_mask(self, s: int, keep: Optional[np.ndarray]):
        """Shard s's packed row mask of a boolean filter over GLOBAL rows -> positional arguments (rowmask, d_rowmask)
        of the handle's search.  Cut out and packed ONCE per filter (the manager hands the same array object for the
        same expression) and, for real shard handles, uploaded once: later searches with that filter pass a device
        pointer — no gather over the rows and no N/8-byte upload per search."""
        if keep is None:
            return ()
        with self._packed_lock:
            ent = self._packed
            if ent is None or ent[0] is not keep:
                self._packed = ent = (keep, {})
            hit = ent[1].get(s)
            if hit is None:
                own = keep if (self.n_shards == 1 and len(self.rows_of[0]) == len(keep)) else keep[self.rows_of[s]]
                packed = np.packbits(own, bitorder="little")
                h = self.handles[s]
                if is_native_handle(h):   # keep the mask in its HBM
                    import torch
                    hit = (None, torch.from_numpy(packed).to(f"cuda:{h.device}"))
                else:
                    hit = (packed, None)
                ent[1][s] = hit
        self._packed_held.hit = hit   # the caller's search reads the device copy by address after the entry may be gone
        packed, dev = hit
        return (packed,) if dev is None else (None, dev.data_ptr())

    def _fan_out(self, fn):
        if self._pool is None:
            return [fn(0)]
        return list(self._pool.map(fn, range(self.n_shards)))

    @property
    def dense_ascending(self) -> bool:
        return dense_ascending(self.handles[0])

    def _gather(self, parts, k: int, ascending: bool = False):
        if self.n_shards == 1:
            return parts[0]
        ids = [to_global(li, self.rows_of[s]) for s, (li, _) in enumerate(parts)]
        return merge_lists(ids, [sc for _, sc in parts], k, ascending)

    def search_dense(self, q: np.ndarray, k: int, keep: Optional[np.ndarray] = None, bounds=None):
        """q [B, dim] float32; keep = boolean filter over GLOBAL rows (or None) -> (ids [B,k] global rows, scores).
        bounds = (radius, range_filter) of a range search, numbers or one per query: every shard's range form gets them, and
        the merge is the usual one (the per-shard lists are in range already)."""
        def one(s):
            if self.handles[s].num_rows == 0:
                return empty_lists(np.atleast_2d(q).shape[0], k)
            if bounds is not None:
                return self.handles[s].search_dense_range(q, k, bounds[0], bounds[1], *self._local_mask(s, keep))
            return self.handles[s].search_dense(q, k, *self._local_mask(s, keep))
        return self._gather(self._fan_out(one), k, self.dense_ascending)

    def search_sparse(self, queries, k: int, drop_ratio: float = 0.0, keep: Optional[np.ndarray] = None):
        def one(s):
            if self.handles[s].num_sparse_rows == 0:
                return empty_lists(len(queries), k)
            return self.handles[s].search_sparse(queries, k, drop_ratio, *self._local_mask(s, keep))
        return self._gather(self._fan_out(one), k)

    @staticmethod
    def _deep_of(handle, name: str):
        """A handle's deep form at depth W, offset 0.  A libhbmrag shard has one; a test stand-in that ranks on the host takes
        any k through its plain form."""
        deep = getattr(handle, name + "_deep", None)
        if deep is not None:
            return lambda x, W, *rest: deep(x, W, 0, *rest)
        return getattr(handle, name)

    def _deep(self, name: str, rows_attr: str, B: int, k: int, offset: int, ascending: bool, call):
        """Every shard's list at depth W = offset + k (call(form, s) -> its lists), merged and cut on the host."""
        W = offset + k

        def one(s):
            if getattr(self.handles[s], rows_attr) == 0:
                return empty_lists(B, W)
            return call(self._deep_of(self.handles[s], name), s)
        parts = self._fan_out(one)
        ids = [li if self.n_shards == 1 else to_global(li, self.rows_of[s]) for s, (li, _) in enumerate(parts)]
        return merge_deep_lists(ids, [sc for _, sc in parts], k, offset, ascending)

    def search_dense_deep(self, q: np.ndarray, k: int, offset: int = 0, keep: Optional[np.ndarray] = None):
        """Deep search (offset + k <= HR_MAX_DEEP_K): entries offset .. offset + k - 1 of the collection's exact ranking.
        One libhbmrag shard cuts the window on the device; several shards return their lists at depth offset + k, merged by
        (score desc or distance asc, global row asc) and cut on the host."""
        h = self.handles[0]
        if self.n_shards == 1 and hasattr(h, "search_dense_deep") and h.num_rows:
            return h.search_dense_deep(q, k, offset, *self._local_mask(0, keep))
        return self._deep("search_dense", "num_rows", np.atleast_2d(q).shape[0], k, offset, self.dense_ascending,
                          lambda form, s: form(q, offset + k, *self._local_mask(s, keep)))

    def search_sparse_deep(self, queries, k: int, offset: int = 0, drop_ratio: float = 0.0, keep: Optional[np.ndarray] = None):
        h = self.handles[0]
        if self.n_shards == 1 and hasattr(h, "search_sparse_deep") and h.num_sparse_rows:
            return h.search_sparse_deep(queries, k, offset, drop_ratio, *self._local_mask(0, keep))
        return self._deep("search_sparse", "num_sparse_rows", len(queries), k, offset, False,
                          lambda form, s: form(queries, offset + k, drop_ratio, *self._local_mask(s, keep)))

    # ---- the search iterator's page: the first k entries of the ranking strictly after a cursor (hr_search_*_deep_after)
    @staticmethod
    def _cursor(after, B: int):
        """after = None or (scores, rows[, has]) per query -> None or three arrays [B] (float32, int64 GLOBAL rows, bool)."""
        if after is None:
            return None
        has = np.ones(B, bool) if len(after) < 3 or after[2] is None else np.broadcast_to(np.asarray(after[2], dtype=bool), (B,))
        return (np.broadcast_to(np.asarray(after[0], dtype=np.float32), (B,)),
                np.broadcast_to(np.asarray(after[1], dtype=np.int64), (B,)), has)

    def _after(self, name: str, rows_attr: str, B: int, k: int, after, bounds, ascending: bool, call, full):
        """Every shard's page behind the SAME cursor, translated into the shard's own ids (the last of its rows at or before
        the cursor's global row: rows_of is ascending), merged on the host.  A row among the first k of the collection after
        the cursor is among the first k of its own shard after it (the argument of merge_deep_lists), so the merge is exact.
        call(form, s, after_s) -> the shard's page; a stand-in without the cursor form ranks all its n rows (full(form, s, n),
        as _deep_of) and the page is cut on the host (page_after)."""
        after = self._cursor(after, B)

        def one(s):
            h = self.handles[s]
            n = getattr(h, rows_attr)
            if n == 0:
                return empty_lists(B, k)
            mine = after
            if after is not None and self.n_shards > 1:
                local = np.searchsorted(self.rows_of[s], after[1], side="right") - 1 + int(getattr(h, "row_offset", 0))
                mine = (after[0], local.astype(np.int64), after[2])
            form = getattr(h, name + "_deep_after", None)
            if form is not None:
                return call(form, s, mine)
            ids, sc = full(self._deep_of(h, name), s, n)
            return page_after(ids, sc, k, mine, bounds, ascending)
        parts = self._fan_out(one)
        if self.n_shards == 1:
            return parts[0]
        ids = [to_global(li, self.rows_of[s]) for s, (li, _) in enumerate(parts)]
        return merge_lists(ids, [sc for _, sc in parts], k, ascending)

    def search_dense_deep_after(self, q: np.ndarray, k: int, after=None, bounds=None, keep: Optional[np.ndarray] = None):
        """The first k <= HR_MAX_DEEP_K entries of the dense ranking strictly after the cursor after = (scores [B], GLOBAL rows
        [B][, has [B]]) (None: from the top), cut to bounds = (radius, range_filter) when given.  The cursor is a position:
        its row need not exist (any more).  One shard: the call passed through; several: _after."""
        return self._after("search_dense", "num_rows", np.atleast_2d(q).shape[0], k, after, bounds, self.dense_ascending,
                           lambda form, s, a: form(q, k, a, bounds, *self._local_mask(s, keep)),
                           lambda form, s, n: form(q, n, *self._local_mask(s, keep)))

    def search_sparse_deep_after(self, queries, k: int, after=None, drop_ratio: float = 0.0, keep: Optional[np.ndarray] = None):
        return self._after("search_sparse", "num_sparse_rows", len(queries), k, after, None, False,
                           lambda form, s, a: form(queries, k, a, drop_ratio, *self._local_mask(s, keep)),
                           lambda form, s, n: form(queries, n, drop_ratio, *self._local_mask(s, keep)))

    # ------------------------------------------------------------------ read path
    def _locate(self, global_rows):
        """`rows_of` inverted: -> (the rows as int64 [n], per shard (positions in the request, local rows)).  A row no
        shard holds: ValueError."""
        g = np.ascontiguousarray(global_rows, dtype=np.int64).reshape(-1)
        parts, found = [], np.zeros(g.shape[0], dtype=bool)
        for s, rows in enumerate(self.rows_of):      # ascending per shard: a binary search inverts it
            at = np.searchsorted(rows, g)
            hit = at < len(rows)
            hit[hit] = rows[at[hit]] == g[hit]
            parts.append((np.flatnonzero(hit), at[hit]))
            found |= hit
        if not found.all():
            raise ValueError(f"row {int(g[np.flatnonzero(~found)[0]])} is not in this collection ({self._n} rows)")
        return g, parts

    def get_dense_rows(self, global_rows) -> np.ndarray:
        """The stored vectors of the given GLOBAL rows (any order, repeats allowed) as float32 [n, dim], in request order:
        `rows_of` inverted gives shard and local row, every shard gathers its part (hr_get_dense_rows, in parallel through
        the pool) and the parts are scattered back.  A row no shard holds: ValueError."""
        g, parts = self._locate(global_rows)

        def one(s):
            where, local = parts[s]
            if not len(where):
                return None
            h = self.handles[s]
            return h.get_dense_rows(local + int(getattr(h, "row_offset", 0)))
        got = self._fan_out(one)
        dim = next((v.shape[1] for v in got if v is not None), int(getattr(self.handles[0], "dim", 0)))
        out = np.empty((g.shape[0], dim), dtype=np.float32)
        for (where, _), v in zip(parts, got):
            if v is not None:
                out[where] = v
        return out

    def get_sparse_rows(self, global_rows) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The stored sparse rows of the given GLOBAL rows (any order, repeats allowed) as one CSR in request order
        (indptr int64 [n + 1], indices int32, values float32): the inversion and the fan-out of get_dense_rows, every
        shard's ragged part (hr_get_sparse_rows) stitched in.  A row no shard holds: ValueError.  A row whose shard has
        fewer sparse rows than dense ones (appended without a sparse payload: local row >= num_sparse_rows) is empty."""
        g, parts = self._locate(global_rows)

        def one(s):
            where, local = parts[s]
            if not len(where):
                return None
            h = self.handles[s]
            stored = local < int(h.num_sparse_rows)
            ptr, idx, val = h.get_sparse_rows(local[stored] + int(getattr(h, "row_offset", 0)))
            lens = np.zeros(len(where), dtype=np.int64)
            lens[stored] = np.diff(ptr)
            return lens, idx, val
        got = self._fan_out(one)
        lens = np.zeros(g.shape[0], dtype=np.int64)
        for (where, _), v in zip(parts, got):
            if v is not None:
                lens[where] = v[0]
        indptr = np.zeros(g.shape[0] + 1, dtype=np.int64)
        np.cumsum(lens, out=indptr[1:])
        indices, values = np.empty(int(indptr[-1]), dtype=np.int32), np.empty(int(indptr[-1]), dtype=np.float32)
        for (where, _), v in zip(parts, got):
            if v is None or not len(v[1]):
                continue
            n_of = v[0]          # the part's entries lie back to back in the order of `where`: entry -> its place in the whole
            dst = np.repeat(indptr[where] - (np.cumsum(n_of) - n_of), n_of) + np.arange(len(v[1]), dtype=np.int64)
            indices[dst], values[dst] = v[1], v[2]
        return indptr, indices, values

    # ------------------------------------------------------------------ snapshot
    def save(self, path_of_shard) -> None:
        """path_of_shard(s) -> file for shard s."""
        for s, h in enumerate(self.handles):
            h.save(path_of_shard(s))

    def row_maps(self) -> List[np.ndarray]:
        return [r.copy() for r in self.rows_of]

    def adopt(self, handles: list, rows_of: Sequence[np.ndarray]):
        """Replace the shards by loaded ones (snapshot resume)."""
        for h in self.handles:
            h.close()
        self.handles = list(handles)
        self.rows_of = [np.asarray(r, dtype=np.int64) for r in rows_of]
        self._n = int(sum(len(r) for r in self.rows_of))


class MaskCache:
    """The row filters a CollectiveShardSet has sent round: MAX_MASKS entries, first in first out.  Every rank `put`s the
    same mask ids in the same order, so the ranks evict alike and rank 0's `lookup` knows what the others still hold.  An
    entry is this rank's boolean slice of the mask and, made on first use by a hybrid round, its packed copy on the device;
    they leave together."""

    def __init__(self, capacity: int):
        self.capacity = capacity
        self._entries = {}          # mask id -> [boolean slice, device copy | None], oldest first
        self._ids = {}              # rank 0: id(filter array) -> (mask id, the array: keeps the id() unique)
        self._next_id = 1

    def lookup(self, keep: Optional[np.ndarray]):
        """rank 0: (mask id, 1 if the mask must travel with this round, its packed bytes or None) of a filter array; the
        id 0 is "no filter"."""
        if keep is None:
            return 0, 0, None
        ent = self._ids.get(id(keep))
        if ent is not None and ent[0] in self._entries:
            return ent[0], 0, None
        mask_id = self._next_id
        self._next_id += 1
        self._ids = {key: v for key, v in self._ids.items() if v[0] in self._entries}
        self._ids[id(keep)] = (mask_id, keep)
        return mask_id, 1, np.packbits(np.asarray(keep, dtype=bool), bitorder="little")

    def put(self, mask_id: int, bits_slice: np.ndarray):
        if len(self._entries) >= self.capacity:
            self._entries.pop(next(iter(self._entries)))
        self._entries[mask_id] = [bits_slice, None]

    def get(self, mask_id: int) -> np.ndarray:
        return self._entries[mask_id][0]

    def device(self, mask_id: int, upload):
        """The entry's device copy: upload(boolean slice), made once."""
        ent = self._entries[mask_id]
        if ent[1] is None:
            ent[1] = upload(ent[0])
        return ent[1]

    def __contains__(self, mask_id: int) -> bool:
        return mask_id in self._entries

    def clear(self):
        self._entries.clear()
        self._ids.clear()


class CollectiveShardSet:
    """The torchrun form: one PROCESS per GPU, each owning the shard of a contiguous global row range, searched as one
    collection from rank 0 — the reference's `num_shards` are invisible to the caller and cost it one RPC
    (indexing.py:232-239, :439-551); here a round of searches costs TWO collectives:

      1. ONE broadcast of a fixed-size packet: every rank learns what to search;
      2. every rank runs the dense and / or the sparse search of the round on its shard (device forms on a GPU shard,
         unproven lists repaired locally through the host form);
      3. ONE gather of the packed per-rank lists (both modalities) to rank 0, which merges them by (score desc, row asc).

    The packet (wire.py holds the layout; no position is spelt out here) is a header — the op, the op's fields, the mask
    triple, the payload's byte count — and a payload of typed sections, 8-byte items first:

      OP_ROUND   Bd, Bs, k, dim, nnz, drop + mask_id, mask_new, mask_len;  sparse indptr [Bs + 1], dense queries [Bd, dim],
                 sparse indices [nnz], sparse values [nnz]
      OP_HYBRID  B, top_k, dim, nnz, rrf_k, max_nnz + the mask triple;  indptr [B + 1], fusion weights [B, 3], dense
                 queries [B, dim], indices [nnz], values [nnz]
      OP_ADD     nrows, dim, has_dense, has_sparse, nnz;  no payload (the batch follows in broadcasts of its own)
      OP_SAVE    no fields;  the ranks' shard paths, one per line
      OP_FLUSH, OP_ROWMAPS, OP_STOP   neither

    A round carries the searches of one or many retrieve() calls (the manager's batching front packs concurrent
    callers), so a lone retrieve() = 1 broadcast + 1 gather.  A filter's packed row mask travels ONCE, in an extra
    broadcast of the round that first uses it; every rank keeps its slice under the mask's id (MaskCache: first in first
    out, the same order on all ranks).  Rank 0 validates and packs the whole round BEFORE the first collective, and
    rounds are serialised by a lock, so every rank sees the same sequence.  Collectives are torch.distributed's (backend
    "nccl" = RCCL over xGMI on a GPU node; "gloo" in the CPU tests and one-GPU rehearsals).

    Who is guaranteed to reach the collective.  A search round (OP_ROUND) and every control operation: a rank whose own
    part fails still enters the gather / the status all-reduce, with empty lists and an error flag that rank 0 raises, so
    nobody is left waiting.  A hybrid round (OP_HYBRID) is NOT: its collective is the all-gather inside the engine's
    search, and a rank that raises before it (a mask shorter than its rows, say) never enters it — the other ranks wait.

    Two forms of the local shard (a local ShardSet of one handle).  Pre-built: the rank filled its shard itself with one
    contiguous global row range; the handle carries the numbers (ShardHandle.set_row_offset(first_row)) and `first_row`
    says where the rank's rows sit in a global filter mask.  Ingested (`local_ids=True`): the handle numbers its rows from
    0, `local.rows_of[0]` maps them to global rows, and the collection grows through the COLLECTIVE control operations —
    add (the batch is broadcast, every rank keeps one contiguous block of it), finalize, save (every rank writes its own
    shard file), row_maps (one gather) — which rank 0 calls while the other ranks sit in serve(); each is one control
    packet + its payload broadcasts + one all-reduce of a status flag, so that rank 0 hears of a failure anywhere."""

    PACKET_BYTES = wire.PACKET_BYTES
    MAX_MASKS = 8
    hybrid_on_device = True         # False: retrieve() takes the two-searches-then-fuse rounds through the host forms (round 3)

    def __init__(self, local: ShardSet, first_row: int, dist, group=None, device=None, local_ids: bool = False):
        import threading

        import torch
        self.torch, self.dist, self.group = torch, dist, group
        self.local, self.first_row = local, int(first_row)
        # local_ids: the local handle numbers its rows from 0 and `local.rows_of[0]` says which global row each one is — the
        # form a collection INGESTED through this set takes (round 4: `add` is collective, every batch is cut into one
        # block per rank, so a rank's rows are no longer one contiguous global range).  Otherwise (a shard built by the rank
        # itself, hr_set_row_offset(first_row)) the handle already returns global rows of a contiguous range.
        self.local_ids = bool(local_ids)
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.dev = torch.device(device) if device is not None else (
            torch.device("cuda", local.device) if dist.get_backend(group) == "nccl" else torch.device("cpu"))
        self._lock = threading.Lock()
        n = torch.tensor([local.num_rows, local.num_sparse_rows], dtype=torch.int64, device=self.dev)
        dist.all_reduce(n, group=group)
        self._n_rows, self._n_sparse = int(n[0]), int(n[1])
        self._packet = torch.zeros(self.PACKET_BYTES, dtype=torch.uint8, device=self.dev)
        self._masks = MaskCache(self.MAX_MASKS)
        self.n_collectives = 0      # broadcasts + gathers issued (tests count them)
        self._side = None           # one worker thread: the dense search of a round that also carries sparse queries
        self._hyb_engines = {}      # (top_k, rrf_k) -> engine.HybridSearchEngine over the group (hybrid rounds on the device)
        self._serving = False
        # what every rank runs when a packet of that op arrives: handler(fields, packet bytes, **what only rank 0 has)
        self._handlers = {wire.OP_ROUND: self._op_round, wire.OP_HYBRID: self._op_hybrid, wire.OP_ADD: self._op_add,
                          wire.OP_FLUSH: self._op_flush, wire.OP_SAVE: self._op_save, wire.OP_ROWMAPS: self._op_rowmaps,
                          wire.OP_STOP: self._op_stop}

    # shape, as ShardSet
    n_shards = property(lambda self: self.world)
    first = property(lambda self: self.local.first)
    device = property(lambda self: self.local.device)
    num_rows = property(lambda self: self._n_rows)
    num_sparse_rows = property(lambda self: self._n_sparse)
    rows_of = property(lambda self: self.local.rows_of)

    def close(self):
        self.local.close()

    def compact(self, keep_global, d_keep: int = 0):
        """Not in the torchrun form: every rank would have to compact its shard and renumber in step."""
        raise NotImplementedError("compaction of a torchrun collection (CollectiveShardSet) is not implemented")

    def get_dense_rows(self, global_rows):
        """Not in the torchrun form: the rows would have to travel from the ranks that hold them."""
        raise NotImplementedError("reading stored vectors back from a torchrun collection (CollectiveShardSet) is not implemented")

    def get_sparse_rows(self, global_rows):
        """Not in the torchrun form, as for the dense vectors."""
        raise NotImplementedError("reading stored sparse vectors back from a torchrun collection (CollectiveShardSet) is not implemented")

    def _global_rows(self) -> np.ndarray:
        """Global row of every local row of this rank."""
        if self.local_ids:
            return self.local.rows_of[0]
        return np.arange(self.first_row, self.first_row + max(self.local.num_rows, self.local.num_sparse_rows), dtype=np.int64)

    # ------------------------------------------------------------------ protocol
    def _bcast(self, t):
        self.n_collectives += 1
        self.dist.broadcast(t, src=0, group=self.group)
        return t

    def _send_packet(self, body: Optional[np.ndarray]) -> np.ndarray:
        """ONE broadcast of the fixed-size packet; returns the bytes in use (header + payload) as numpy on every rank."""
        t = self.torch
        if self.rank == 0:
            self._packet[: body.size].copy_(t.from_numpy(body))
        self._bcast(self._packet)
        if self.rank == 0:
            return body
        n = wire.unpack_header(self._packet[: wire.HEADER_BYTES].cpu().numpy())[2]
        return self._packet[: wire.HEADER_BYTES + n].cpu().numpy()

    def _dispatch(self, body: Optional[np.ndarray], **rank0):
        """Both sides of one packet: rank 0 sends `body` (the workers pick it up in serve()), every rank reads the header
        and runs the op's handler; `rank0` is what only the sender has (a new mask's bytes, the batch of an add)."""
        pkt = self._send_packet(body)
        op, fields, _ = wire.unpack_header(pkt)
        return self._handlers[op](fields, pkt, **rank0)

    def _control(self, op: int, fields=(), blob: bytes = b"", **rank0):
        """rank 0, under the lock: one control operation = its packet (header fields + an optional byte blob), then the
        handler every rank runs."""
        return self._dispatch(wire.pack(op, fields, [np.frombuffer(blob, dtype=np.uint8)], self.PACKET_BYTES), **rank0)

    @staticmethod
    def _guarded(fn):
        """Run this rank's part of a collective operation -> (result, None) or (None, the exception): a rank that fails
        must still reach the collective that follows, nobody may be left waiting in it."""
        try:
            return fn(), None
        except Exception as e:
            return None, e

    def _log_worker_failure(self, what: str, err: Optional[Exception]):
        """A worker rank has nobody to raise to: its error goes to the log, rank 0 learns of it through the collective."""
        if err is not None and self.rank != 0:
            import logging
            logging.getLogger(__name__).error("rank %d failed %s: %s", self.rank, what, err)

    def _status(self, err: Optional[Exception]):
        """Every rank reports whether its part of a control operation worked; rank 0 raises if any did not."""
        t = self.torch
        flag = t.tensor([0 if err is None else 1], dtype=t.int64, device=self.dev)
        self.n_collectives += 1
        self.dist.all_reduce(flag, group=self.group)
        self._log_worker_failure("a collective control operation", err)
        if self.rank == 0:
            if err is not None:
                raise err
            if int(flag.item()):
                raise RuntimeError("a collective control operation failed on another rank (see its log)")

    # ------------------------------------------------------------------ collective control operations (rank 0 calls, the others serve())
    def add(self, dense, sparse_csr=None, n: Optional[int] = None):
        """Collective append (rank 0 calls it with the batch, the other ranks are in serve()): the batch travels in ONE
        broadcast per part (dense rows, CSR), every rank keeps the contiguous block shard_range(n, rank, world) of it and
        records which global rows those are (reference: Milvus spreads an insert over its `num_shards`,
        indexing.py:234-239, :264-437).  Same return value as ShardSet.add.  Needs `local_ids`."""
        if not self.local_ids:
            raise RuntimeError("this shard set was attached with pre-built contiguous shards; collective ingest needs local_ids=True")
        with self._lock:
            if dense is not None and hasattr(dense, "detach"):
                dense = dense.detach().float().cpu().numpy()
            nrows = dense.shape[0] if dense is not None else (len(sparse_csr[0]) - 1 if sparse_csr is not None else int(n or 0))
            if sparse_csr is not None:      # positions from 0 and exactly nnz entries: the receivers size their buffers by it
                ptr = np.asarray(sparse_csr[0], dtype=np.int64)
                sparse_csr = (ptr - ptr[0], np.asarray(sparse_csr[1])[ptr[0]:ptr[-1]], np.asarray(sparse_csr[2])[ptr[0]:ptr[-1]])
            fields = dict(nrows=nrows, dim=0 if dense is None else dense.shape[1], has_dense=dense is not None,
                          has_sparse=sparse_csr is not None, nnz=0 if sparse_csr is None else sparse_csr[0][-1])
            return self._control(wire.OP_ADD, fields, dense=dense, sparse_csr=sparse_csr)

    def _op_add(self, f, pkt, dense=None, sparse_csr=None):
        from .engine import shard_range
        t = self.torch
        nrows, has_dense, has_sparse = f.nrows, bool(f.has_dense), bool(f.has_sparse)
        base = self._n_rows if has_dense or not has_sparse else self._n_sparse

        def bcast_array(arr, count, dtype):
            buf = (t.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to(self.dev) if self.rank == 0
                   else t.empty(count, dtype=getattr(t, np.dtype(dtype).name), device=self.dev))
            return self._bcast(buf.reshape(-1)).cpu().numpy()

        def my_part():
            d = bcast_array(dense, nrows * f.dim, np.float32).reshape(nrows, f.dim) if has_dense else None
            csr = None
            if has_sparse:
                ptr = bcast_array(sparse_csr[0] if self.rank == 0 else None, nrows + 1, np.int64)
                idx = bcast_array(sparse_csr[1] if self.rank == 0 else None, f.nnz, np.int32) if f.nnz else np.zeros(0, np.int32)
                val = bcast_array(sparse_csr[2] if self.rank == 0 else None, f.nnz, np.float32) if f.nnz else np.zeros(0, np.float32)
                csr = (ptr, idx, val)
            lo, hi = shard_range(nrows, self.rank, self.world)
            # the global row numbers are taken on every rank BEFORE the local append: a rank whose append fails leaves a
            # hole (rows no search returns) instead of ranks that disagree about the numbering
            if has_dense or not has_sparse:
                self._n_rows += nrows
            if has_sparse or not has_dense:
                self._n_sparse += nrows
            self._masks.clear()          # row slices of cached filters are stale on every rank
            sparse_err = None
            if hi > lo:
                piece_csr = None if csr is None else (csr[0][lo:hi + 1], csr[1], csr[2])
                b0 = self.local._n
                _, _, sparse_err = self.local.add(None if d is None else d[lo:hi], piece_csr, hi - lo)
                self.local.rows_of[0][b0:] = np.arange(base + lo, base + hi, dtype=np.int64)   # global rows of the block
            return base, base + nrows, sparse_err

        out, err = self._guarded(my_part)
        try:
            self._status(err)
        except Exception as e:
            # the row numbers [base, base + nrows) are taken on every rank whatever failed: the caller keeps its payload
            # columns aligned with them (the failing rank's block stays a hole no search returns)
            raise PartialAppend(base, base + nrows, e) from e
        return out

    def finalize(self):
        """Flush every rank's shard (rank 0 calls it; a rank in serve() flushes when the packet arrives)."""
        if self.rank != 0 or not self.local_ids:
            self.local.finalize()
            return
        with self._lock:
            self._control(wire.OP_FLUSH)

    def _op_flush(self, f, pkt):
        self._status(self._guarded(self.local.finalize)[1])

    def save(self, path_of_shard) -> None:
        """Every rank writes its shard to path_of_shard(rank) (rank 0 calls it; the paths travel in the control packet)."""
        with self._lock:
            self._control(wire.OP_SAVE, blob="\n".join(path_of_shard(r) for r in range(self.world)).encode("utf-8"))

    def _op_save(self, f, pkt):
        def my_part():
            mine = wire.payload(pkt).tobytes().decode("utf-8").split("\n")[self.rank]
            self.local.save(lambda s: mine)
        self._status(self._guarded(my_part)[1])

    def row_maps(self):
        """The global rows every rank's shard holds, in rank order (rank 0 calls it: one gather)."""
        with self._lock:
            return self._control(wire.OP_ROWMAPS)

    def _op_rowmaps(self, f, pkt):
        rows = self._global_rows()
        parts = [None] * self.world if self.rank == 0 else None
        self.n_collectives += 1
        self.dist.gather_object(rows, parts, dst=0, group=self.group)
        return [np.asarray(r, dtype=np.int64) for r in parts] if self.rank == 0 else None

    def stop_workers(self):
        with self._lock:
            self._control(wire.OP_STOP)

    def _op_stop(self, f, pkt):
        self._serving = False
        if self._side is not None:
            self._side.shutdown(wait=False)
            self._side = None

    # ------------------------------------------------------------------ ranks > 0
    def serve(self):
        """Answer rank 0's packets until it sends OP_STOP."""
        self._serving = True
        while self._serving:
            self._dispatch(None)

    # ------------------------------------------------------------------ search rounds
    def round(self, dense_q: Optional[np.ndarray], sparse_queries, k: int, drop_ratio: float = 0.0, keep: Optional[np.ndarray] = None):
        """One round = one broadcast + one gather: dense_q [Bd, dim] and / or Bs sparse queries, all with the same k and
        filter -> ((dense ids, scores) | None, (sparse ids, scores) | None), global rows, merged over the ranks.  Raises
        BEFORE any collective if the round cannot be packed."""
        fields = dict(Bd=0, Bs=0, k=k, dim=0, nnz=0, drop=drop_ratio)
        ptr = idx = val = None
        if dense_q is not None:
            dense_q = np.ascontiguousarray(np.atleast_2d(dense_q), dtype=np.float32)
            fields.update(Bd=dense_q.shape[0], dim=dense_q.shape[1] if dense_q.shape[0] else 0)
        if sparse_queries is not None and len(sparse_queries):
            ptr, idx, val = csr_of_queries(sparse_queries)
            fields.update(Bs=len(sparse_queries), nnz=idx.size)
        sections = [a for a in (ptr, dense_q if fields["Bd"] else None, idx, val) if a is not None]   # 8-byte items first
        with self._lock:
            mask_id, mask_new, mask_bytes = self._masks.lookup(keep)
            body = wire.pack(wire.OP_ROUND, {**fields, **wire.mask_fields(mask_id, mask_new, mask_bytes)}, sections, self.PACKET_BYTES)
            return self._dispatch(body, mask_bytes=mask_bytes)

    def search_dense(self, q: np.ndarray, k: int, keep: Optional[np.ndarray] = None, bounds=None):
        if bounds is not None:
            raise NotImplementedError("range search is not built for the torchrun form: a round's packet carries no bounds")
        return self.round(q, None, k, 0.0, keep)[0]

    def search_sparse(self, queries, k: int, drop_ratio: float = 0.0, keep: Optional[np.ndarray] = None):
        return self.round(None, list(queries), k, drop_ratio, keep)[1]

    def _mask_slice(self, f, mask_bytes_rank0):
        """This rank's boolean slice of the round's filter (None = no filter); receives a new mask if the round carries one."""
        t = self.torch
        if f.mask_id == 0:
            return None
        if f.mask_new:
            buf = t.from_numpy(mask_bytes_rank0).to(self.dev) if self.rank == 0 else t.empty(f.mask_len, dtype=t.uint8, device=self.dev)
            bits = np.unpackbits(self._bcast(buf).cpu().numpy(), bitorder="little").astype(bool)
            rows = self._global_rows()
            if rows.size and bits.size <= int(rows.max()):
                raise ValueError(f"filter mask covers {bits.size} rows, this rank holds rows up to {int(rows.max()) + 1}")
            self._masks.put(f.mask_id, bits[rows])
        return self._masks.get(f.mask_id)

    def _local_round(self, f, pkt: np.ndarray, keep_local):
        """Run this rank's part of a round -> [(ids, scores)] per modality in the round, global rows."""
        s = wire.Sections(pkt)
        out = []
        dense_job = None
        if f.Bs:
            ptr = s.take(f.Bs + 1, np.int64)
        if f.Bd:
            q = s.take(f.Bd * f.dim, np.float32).reshape(f.Bd, f.dim)
            # the slice object itself when it fits: the local ShardSet keeps a filter's packed (device) mask by identity
            kd = None if keep_local is None else (keep_local if keep_local.size == self.local.num_rows else keep_local[: self.local.num_rows])
            if f.Bs:   # both modalities in the round: the dense search runs beside the sparse one (ctypes releases the GIL)
                if self._side is None:
                    self._side = ThreadPoolExecutor(max_workers=1, thread_name_prefix="round-dense-")
                dense_job = self._side.submit(self.local.search_dense, q, f.k, kd)
                out.append(None)
            else:
                out.append(self.local.search_dense(q, f.k, kd))
        if f.Bs:
            idx, val = s.take(f.nnz, np.int32), s.take(f.nnz, np.float32)
            queries = [(idx[ptr[b]:ptr[b + 1]], val[ptr[b]:ptr[b + 1]]) for b in range(f.Bs)]
            ks = None if keep_local is None else (keep_local if keep_local.size == self.local.num_sparse_rows
                                                  else keep_local[: self.local.num_sparse_rows])
            try:
                out.append(self.local.search_sparse(queries, f.k, f.drop, ks))
            finally:
                if dense_job is not None:   # never leave the side thread running into the next round
                    dense_err = dense_job.exception()
            if dense_job is not None:
                if dense_err is not None:
                    raise dense_err
                out[0] = dense_job.result()
        if self.local_ids:
            out = [(to_global(li, self.local.rows_of[0]), sc) for li, sc in out]
        return out

    def _op_round(self, f, pkt, mask_bytes=None):
        """Every rank's part of a search round after rank 0 has packed it.  Returns the merged lists on rank 0."""
        t = self.torch
        n_vals = (f.Bd + f.Bs) * f.k
        mine, err = self._guarded(lambda: wire.pack_lists(self._local_round(f, pkt, self._mask_slice(f, mask_bytes)), n_vals))
        mine_t = t.from_numpy(wire.pack_lists(None, n_vals) if err is not None else mine).to(self.dev)
        parts = [t.empty_like(mine_t) for _ in range(self.world)] if self.rank == 0 else None
        self.n_collectives += 1
        self.dist.gather(mine_t, parts, dst=0, group=self.group)
        self._log_worker_failure("its part of a search round", err)
        if self.rank != 0:
            return None
        if err is not None:
            raise err
        bad, lists = wire.unpack_lists([p.cpu().numpy() for p in parts], (f.Bd, f.Bs), f.k)
        if bad:
            raise RuntimeError(f"search round failed on rank(s) {bad}")
        return [None if m is None else merge_lists(m[0], m[1], f.k, asc)
                for m, asc in zip(lists, (self.local.dense_ascending, False))]

    # ------------------------------------------------------------------ hybrid rounds on the device
    @property
    def supports_hybrid_round(self) -> bool:
        """The device form of a hybrid round needs real shards whose handles return GLOBAL rows (pre-built contiguous
        shards: the engine merges the ranks' lists by the ids the scans wrote) and the sparse modality."""
        h = self.local.first
        return self.hybrid_on_device and not self.local_ids and is_native_handle(h) and getattr(h, "sparse_dim", 0) > 0

    def round_hybrid(self, dense_q: np.ndarray, sparse_queries, top_k: int, drop_ratio: float, rrf_k: int,
                     weights: np.ndarray, keep: Optional[np.ndarray] = None):
        """rank 0: the dense search (2 x top_k), the sparse search (2 x top_k) and their rank fusion for B requests as ONE
        collective round on the device: the packet (queries, CSR, per-request weights) is broadcast, every rank runs
        hr_search_hybrid_dev on its shard with pointers INTO the packet, the per-rank lists travel in the engine's one
        all-gather and every rank merges + fuses them in one launch (engine.HybridSearchEngine with the process group: the
        path bench.py times) — under nccl nothing but the 128-byte header and rank 0's answer crosses the host.
        -> dict of numpy arrays: fused_ids / fused_scores / fused_methods [B, top_k], fused_n [B], list_ids /
        list_scores [2, B, k'], proven [B] (False: some rank could not prove a list — the caller redoes that request
        through the host forms)."""
        from .engine import pack_sparse_queries
        dense_q = np.ascontiguousarray(np.atleast_2d(dense_q), dtype=np.float32)
        B, dim = dense_q.shape
        h = self.local.first
        if dim != h.dim:
            raise ValueError(f"query dim {dim} != shard dim {h.dim}")
        ptr, idx, val, max_nnz = pack_sparse_queries(list(sparse_queries), float(drop_ratio), h.sparse_dim)
        if len(ptr) != B + 1 or not idx.size:
            raise ValueError("a hybrid round needs one non-empty sparse query per dense query")
        w = np.zeros((B, 3), dtype=np.float64)
        w[:, :2] = np.asarray(weights, dtype=np.float64).reshape(B, 2)
        with self._lock:
            mask_id, mask_new, mask_bytes = self._masks.lookup(keep)
            fields = dict(B=B, top_k=top_k, dim=dim, nnz=idx.size, rrf_k=rrf_k, max_nnz=max_nnz,
                          **wire.mask_fields(mask_id, mask_new, mask_bytes))
            body = wire.pack(wire.OP_HYBRID, fields, [ptr.astype(np.int64), w, dense_q, idx.astype(np.int32), val.astype(np.float32)],
                             self.PACKET_BYTES)
            return self._dispatch(body, mask_bytes=mask_bytes)

    def _op_hybrid(self, f, pkt: np.ndarray, mask_bytes=None):
        """Every rank's part of a hybrid round (collective: the engine's all-gather is inside)."""
        from .engine import EngineConfig, HybridSearchEngine
        t = self.torch
        keep_local = self._mask_slice(f, mask_bytes)
        dev = t.device("cuda", self.local.first.device)
        eng = self._hyb_engines.get((f.top_k, f.rrf_k))
        if eng is None:
            if len(self._hyb_engines) >= 8:
                self._hyb_engines.clear()
            eng = self._hyb_engines[(f.top_k, f.rrf_k)] = HybridSearchEngine(
                self.local.first, EngineConfig(top_k=f.top_k, rrf_k=f.rrf_k, enable_reranking=False), process_group=self.group, device=str(dev))
        # the operands are views of the packet where it lives on the device (nccl), of an upload of its host copy otherwise
        s = wire.Sections(self._packet if self._packet.is_cuda else t.from_numpy(pkt).to(dev))
        ptr = s.take(f.B + 1, np.int64)
        wq = s.take(f.B * 3, np.float64).view(f.B, 3)
        q = s.take(f.B * f.dim, np.float32).view(f.B, f.dim)
        idx, val = s.take(f.nnz, np.int32), s.take(f.nnz, np.float32)
        mask = None if keep_local is None else self._masks.device(
            f.mask_id, lambda bits: t.from_numpy(np.packbits(bits, bitorder="little")).to(dev))
        with t.cuda.device(dev):
            b = eng.search(q, (ptr, idx, val, f.max_nnz), rowmask=mask, weights=wq)
            t.cuda.current_stream(dev).synchronize()      # the packet may be rewritten by the next round
        if self.rank != 0:
            return None
        out = {k: b[k].cpu().numpy() for k in ("fused_ids", "fused_scores", "fused_methods", "fused_n", "list_ids", "list_scores")}
        out["proven"] = b["agg_flags"].cpu().numpy().min(axis=0) == 1
        return out
