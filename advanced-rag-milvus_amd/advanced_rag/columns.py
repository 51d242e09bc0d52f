"""Append-only payload columns of a collection, keyed by global row.

The reference keeps the scalar fields of its schema (indexing.py:191-225: id / chunk_id, doc_id, content,
chunk_index, token_count, entropy, redundancy, domain_density, timestamp, metadata_json) inside Milvus; here they
stay on the host — the GPU only ever sees row numbers — in arrow-style columns:

  * numeric fields: one growable numpy array each (int64 / float32, amortised O(batch) appends);
  * string fields: one growable UTF-8 byte buffer + int64 offsets each — no Python object per row, so ten million
    rows of ids and doc ids cost a few hundred MB instead of GBs of str objects, and nothing is rebuilt after an append.

For filter expressions (filters.py / device_filters.py) a string column can hand out an ORDER-PRESERVING 16-byte
prefix key per row (two big-endian uint64 words of the zero-padded UTF-8 bytes; UTF-8 byte order is code-point
order): `key < key(v)` decides `s < v` for every row whose first 16 bytes differ from v's, and only the rows that tie
on the prefix need the full strings.  Keys are built lazily, per column, on first use, and extended by later appends.

For MMR diversification on the device (csrc/mmr.h) the `content` column can hand out its rows' TOKEN SETS
(`TokenSetColumn`): the reference compares `set(content.lower().split())` of two hits; here every distinct token of the
collection gets an int32 id and a row keeps its ids, sorted — built lazily as well, and never part of a snapshot.

For grouping search (csrc/group.h) every groupable field hands out an int64 GROUP KEY per row (`GroupKeyColumn`): an
integer field is its own key; the value of a string field gets its ordinal in a collection-wide dictionary, in first-seen
order — equal keys mean equal values.  Built lazily, extended by later appends, gathered (never renumbered) by compact(),
and never part of a snapshot: the TokenSetColumn pattern.

For the decay ranker (csrc/decay.h) the `timestamp` column hands out EPOCH SECONDS per row (`PayloadColumns.epoch_seconds`):
a float64 derived from the ISO text by decay.epoch_seconds, NaN where the text is empty or no ISO time.  The same pattern:
built on first use, extended by appends, gathered by compact(), never part of a snapshot.
"""
from __future__ import annotations

import threading
from typing import Any, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

STRING_COLUMNS = ("id", "doc_id", "content", "timestamp", "metadata_json")
INT_COLUMNS = ("chunk_index", "token_count")
FLOAT_COLUMNS = ("entropy", "redundancy", "domain_density")
KEY_BYTES = 16
GROUP_STRING_FIELDS = {"doc_id": "doc_id", "id": "id", "chunk_id": "id", "timestamp": "timestamp"}   # field -> column


def check_group_field(field) -> str:
    """The field of a grouping search, or ValueError: float fields cannot be grouped on (Milvus refuses them too), and a
    field the schema does not have, or whose values are free text (content, metadata_json), is unknown."""
    if field in FLOAT_COLUMNS:
        raise ValueError(f"group_by_field {field!r} is a float field: grouping needs an integer or a string field")
    if field not in INT_COLUMNS and field not in GROUP_STRING_FIELDS:
        raise ValueError(f"unknown group_by_field: {field!r} (expected one of "
                         f"{', '.join(sorted(set(INT_COLUMNS) | set(GROUP_STRING_FIELDS)))})")
    return field


def _keep_mask(keep, n: int) -> np.ndarray:
    keep = np.asarray(keep, dtype=bool)
    if keep.shape != (n,):
        raise ValueError(f"keep mask has shape {keep.shape}, the column holds {n} rows")
    return keep


def _gather_csr(off: np.ndarray, data: np.ndarray, keep: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The rows of a CSR (off [n + 1], data) that `keep` names -> (new offsets from 0, their data back to back)."""
    lens = (off[1:] - off[:-1])[keep]
    new_off = np.zeros(lens.shape[0] + 1, dtype=np.int64)
    np.cumsum(lens, out=new_off[1:])
    # element e of the output lies in kept row j: it comes from start[j] + (e - new_off[j])
    shift = np.repeat(off[:-1][keep] - new_off[:-1], lens)
    return new_off, data[np.arange(int(new_off[-1]), dtype=np.int64) + shift]


def _grown(arr: np.ndarray, need: int) -> np.ndarray:
    if need <= arr.shape[0]:
        return arr
    cap = max(need, arr.shape[0] + arr.shape[0] // 2, 1024)
    out = np.empty(cap, dtype=arr.dtype)
    out[: arr.shape[0]] = arr
    return out


class NumericColumn:
    def __init__(self, dtype):
        self._a = np.empty(0, dtype=dtype)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def append(self, v) -> None:
        self._a = _grown(self._a, self._n + 1)
        self._a[self._n] = v
        self._n += 1

    def extend(self, values) -> None:
        vals = np.asarray(values if isinstance(values, np.ndarray) else list(values), dtype=self._a.dtype)
        self._a = _grown(self._a, self._n + vals.shape[0])
        self._a[self._n: self._n + vals.shape[0]] = vals
        self._n += vals.shape[0]

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.array()[i].tolist()
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._a[i].item()      # Python int / float (a float32 value as the float that equals it)

    def __iter__(self) -> Iterator:
        return iter(self.array().tolist())

    def __eq__(self, other) -> bool:
        return list(self) == list(other)

    def compact(self, keep: np.ndarray) -> None:
        """Drop the rows whose entry of the boolean `keep` is False; the others move up in order."""
        self._a = self._a[: self._n][_keep_mask(keep, self._n)]
        self._n = self._a.shape[0]

    def array(self) -> np.ndarray:
        """The column as a numpy view (no copy): what the filters compare against."""
        return self._a[: self._n]

    def tolist(self) -> list:
        return self.array().tolist()

    @property
    def nbytes(self) -> int:
        return self._a.nbytes


class StringColumn:
    def __init__(self):
        self._buf = np.empty(0, dtype=np.uint8)
        self._used = 0
        self._off = np.zeros(1, dtype=np.int64)   # _off[r] .. _off[r + 1] = bytes of row r
        self._n = 0
        self._keys: Optional[np.ndarray] = None   # [cap, 2] uint64 prefix keys, valid for rows < _n_keyed
        self._n_keyed = 0

    def __len__(self) -> int:
        return self._n

    def append(self, v) -> None:
        self.extend((v,))

    def extend(self, values: Iterable) -> None:
        enc = [str(v).encode("utf-8") for v in values]
        if not enc:
            return
        lens = np.fromiter((len(b) for b in enc), dtype=np.int64, count=len(enc))
        total = int(lens.sum())
        self._buf = _grown(self._buf, self._used + total)
        self._buf[self._used: self._used + total] = np.frombuffer(b"".join(enc), dtype=np.uint8)
        self._off = _grown(self._off, self._n + len(enc) + 1)
        np.cumsum(lens, out=self._off[self._n + 1: self._n + len(enc) + 1])
        self._off[self._n + 1: self._n + len(enc) + 1] += self._used
        self._used += total
        self._n += len(enc)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._buf[self._off[i]: self._off[i + 1]].tobytes().decode("utf-8")

    def __iter__(self) -> Iterator[str]:
        whole = self._buf[: self._used].tobytes()
        off = self._off
        return (whole[off[i]: off[i + 1]].decode("utf-8") for i in range(self._n))

    def __eq__(self, other) -> bool:
        return list(self) == list(other)

    def tolist(self) -> List[str]:
        return list(self)

    def compact(self, keep: np.ndarray) -> None:
        """Drop the rows whose entry of the boolean `keep` is False: the byte buffer is gathered and the offsets are
        rebuilt; the prefix keys are gathered with them."""
        keep = _keep_mask(keep, self._n)
        self._off, self._buf = _gather_csr(self._off[: self._n + 1], self._buf, keep)
        if self._keys is not None:
            self._keys = self._keys[: self._n_keyed][keep[: self._n_keyed]]
            self._n_keyed = self._keys.shape[0]
        self._used = int(self._off[-1])
        self._n = self._off.shape[0] - 1

    def as_str_array(self) -> np.ndarray:
        """numpy unicode array (fixed width = the longest row): only for small collections and tests."""
        return np.asarray(self.tolist(), dtype=str) if self._n else np.zeros(0, dtype=str)

    @property
    def nbytes(self) -> int:
        return self._buf.nbytes + self._off.nbytes + (self._keys.nbytes if self._keys is not None else 0)

    # -- order-preserving prefix keys --------------------------------------------------------------------------
    @staticmethod
    def key_of(value: str) -> Tuple[int, int]:
        b = value.encode("utf-8")[:KEY_BYTES].ljust(KEY_BYTES, b"\0")
        return int.from_bytes(b[:8], "big"), int.from_bytes(b[8:], "big")

    def keys(self) -> np.ndarray:
        """[n, 2] uint64: big-endian words of the first 16 bytes of every row, zero padded."""
        n = self._n
        if self._keys is None:
            self._keys, self._n_keyed = np.empty((max(n, 1024), 2), dtype=np.uint64), 0
        if self._keys.shape[0] < n:
            grown = np.empty((max(n, self._keys.shape[0] * 3 // 2), 2), dtype=np.uint64)
            grown[: self._n_keyed] = self._keys[: self._n_keyed]
            self._keys = grown
        step = 1 << 20       # bounded temporaries: 16 MB of gathered bytes per piece
        for a in range(self._n_keyed, n, step):
            b = min(n, a + step)
            start, end = self._off[a:b], self._off[a + 1: b + 1]
            pos = start[:, None] + np.arange(KEY_BYTES, dtype=np.int64)[None, :]
            valid = pos < end[:, None]
            if self._used:
                raw = self._buf[np.minimum(pos, self._used - 1)]
                raw[~valid] = 0
            else:
                raw = np.zeros((b - a, KEY_BYTES), dtype=np.uint8)
            self._keys[a:b] = np.ascontiguousarray(raw).view(">u8").astype(np.uint64)
        self._n_keyed = n
        return self._keys[:n]

    def compare_rows(self, rows: np.ndarray, op: str, value: str) -> np.ndarray:
        """Exact `row OP value` for the given rows (the ones a prefix key could not decide)."""
        vb = value.encode("utf-8")
        out = np.empty(len(rows), dtype=bool)
        whole = self._buf
        for i, r in enumerate(np.asarray(rows, dtype=np.int64).tolist()):
            s = whole[self._off[r]: self._off[r + 1]].tobytes()
            out[i] = {"==": s == vb, "!=": s != vb, "<": s < vb, "<=": s <= vb, ">": s > vb, ">=": s >= vb}[op]
        return out


    def member_rows(self, rows: np.ndarray, values: Sequence[str]) -> np.ndarray:
        """Exact `row in values` for the given rows: compare_rows' counterpart for a membership list."""
        members = {v.encode("utf-8") for v in values}
        whole = self._buf
        return np.fromiter((whole[self._off[r]: self._off[r + 1]].tobytes() in members
                            for r in np.asarray(rows, dtype=np.int64).tolist()), dtype=bool, count=len(rows))


class TokenSetColumn:
    """Append-only CSR over global rows: row r holds the sorted, unique int32 ids of `set(content.lower().split())`
    (Python's own lower / split: Unicode case mapping and whitespace are the reference's, retrieval.py:495).  Ids come
    from one dictionary per collection, token -> id in first-seen order: equal ids mean equal tokens (nothing is hashed).
    Rows are tokenised once; an id, once given, never changes."""
    MAX_TOKENS = (1 << 31) - 1     # ids are int32

    def __init__(self, tokenizer=None):
        """tokenizer: text -> iterable of tokens (duplicates allowed); None = the reference's `text.lower().split()`.  The
        keyword filter's column (PayloadColumns.word_sets) passes filters.analyze."""
        self._tokenize = tokenizer if tokenizer is not None else (lambda text: text.lower().split())
        self.ids: Dict[str, int] = {}
        self._indptr = np.zeros(1, dtype=np.int64)
        self._tok = np.empty(0, dtype=np.int32)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def extend(self, contents: Iterable[str]) -> None:
        ids, rows, lens, tokenize = self.ids, [], [], self._tokenize
        for text in contents:
            row = []
            for t in dict.fromkeys(tokenize(text)):      # distinct tokens in the order of their first occurrence
                i = ids.get(t)
                if i is None:
                    if len(ids) >= self.MAX_TOKENS:
                        raise ValueError(f"more than {self.MAX_TOKENS} distinct tokens: token ids are int32")
                    i = ids[t] = len(ids)
                row.append(i)
            row.sort()
            rows.extend(row)
            lens.append(len(row))
        if not lens:
            return
        used = int(self._indptr[self._n])
        self._tok = _grown(self._tok, used + len(rows))
        self._tok[used: used + len(rows)] = rows
        self._indptr = _grown(self._indptr, self._n + len(lens) + 1)
        np.cumsum(lens, out=self._indptr[self._n + 1: self._n + len(lens) + 1])
        self._indptr[self._n + 1: self._n + len(lens) + 1] += used
        self._n += len(lens)

    def compact(self, keep: np.ndarray) -> None:
        """Drop the rows whose entry of the boolean `keep` is False.  The dictionary stays: an id never changes."""
        keep = _keep_mask(keep, self._n)
        self._indptr, self._tok = _gather_csr(self._indptr[: self._n + 1], self._tok, keep)
        self._n = self._indptr.shape[0] - 1

    def sync(self, content: "StringColumn") -> "TokenSetColumn":
        """Tokenise the rows of `content` this column does not hold yet."""
        step = 1 << 16       # bounded temporaries
        for a in range(self._n, len(content), step):
            self.extend(content[a: min(len(content), a + step)])
        return self

    def indptr(self) -> np.ndarray:
        """int64 [rows + 1] view (no copy)."""
        return self._indptr[: self._n + 1]

    def tokens(self) -> np.ndarray:
        """int32 view of every row's ids, row after row (no copy)."""
        return self._tok[: int(self._indptr[self._n])]

    def row(self, r: int) -> np.ndarray:
        if not 0 <= r < self._n:
            raise IndexError(r)
        return self._tok[self._indptr[r]: self._indptr[r + 1]]

    @property
    def nbytes(self) -> int:
        return self._indptr.nbytes + self._tok.nbytes


class TokenVectorColumn:
    """Append-only CSR over global rows: row r holds T_r >= 0 token vectors of `dim` fp16 elements, the stored bits of the
    late-interaction rerank (csrc/maxsim.h).  A row appended without vectors has T_r = 0.  Values are kept flat (one
    growable fp16 buffer, 3/2 growth) and handed out as [n_tok, dim] views."""

    def __init__(self, dim: int):
        self.dim = int(dim)
        self._indptr = np.zeros(1, dtype=np.int64)
        self._val = np.empty(0, dtype=np.float16)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def extend(self, indptr: np.ndarray, values: np.ndarray) -> None:
        """Append len(indptr) - 1 rows: indptr int64 non-decreasing from 0, values fp16 [indptr[-1], dim] (checked by the
        caller: indexing.MilvusIndexManager._checked_token_vectors)."""
        indptr = np.asarray(indptr, dtype=np.int64)
        rows = indptr.shape[0] - 1
        if rows <= 0:
            return
        used, add = int(self._indptr[self._n]), int(indptr[-1])
        self._val = _grown(self._val, (used + add) * self.dim)
        self._val[used * self.dim: (used + add) * self.dim] = np.asarray(values, dtype=np.float16).reshape(-1)[: add * self.dim]
        self._indptr = _grown(self._indptr, self._n + rows + 1)
        self._indptr[self._n + 1: self._n + rows + 1] = indptr[1:] + used
        self._n += rows

    def pad_to(self, n_rows: int) -> "TokenVectorColumn":
        """Rows this column does not hold yet, up to n_rows, get no vectors."""
        if n_rows > self._n:
            self._indptr = _grown(self._indptr, n_rows + 1)
            self._indptr[self._n + 1: n_rows + 1] = self._indptr[self._n]
            self._n = n_rows
        return self

    def compact(self, keep: np.ndarray) -> None:
        """Drop the rows whose entry of the boolean `keep` is False; every survivor keeps its vectors."""
        keep = _keep_mask(keep, self._n)
        self._indptr, val = _gather_csr(self._indptr[: self._n + 1], self.values(), keep)
        self._val = np.ascontiguousarray(val).reshape(-1)
        self._n = self._indptr.shape[0] - 1

    def indptr(self) -> np.ndarray:
        """int64 [rows + 1] view (no copy)."""
        return self._indptr[: self._n + 1]

    def values(self) -> np.ndarray:
        """fp16 [n_tok, dim] view of every row's vectors, row after row (no copy)."""
        used = int(self._indptr[self._n])
        return self._val[: used * self.dim].reshape(used, self.dim)

    def row(self, r: int) -> np.ndarray:
        if not 0 <= r < self._n:
            raise IndexError(r)
        return self.values()[self._indptr[r]: self._indptr[r + 1]]

    def gather(self, rows) -> Tuple[np.ndarray, np.ndarray]:
        """(indptr from 0, values) of the given rows in the given order; a row outside the column has no vectors.  Bounded
        by what the rows hold, not by the column."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        ok = (rows >= 0) & (rows < self._n)
        at = np.where(ok, rows, 0)
        beg = np.where(ok, self._indptr[at], 0)
        cnt = np.where(ok, self._indptr[at + 1] - self._indptr[at], 0) if self._n else np.zeros(len(rows), dtype=np.int64)
        out = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(cnt, out=out[1:])
        take = np.repeat(beg - out[:-1], cnt) + np.arange(int(out[-1]), dtype=np.int64)
        return out, self.values()[take]

    @property
    def nbytes(self) -> int:
        return self._indptr.nbytes + self._val.nbytes


class GroupKeyColumn:
    """Append-only int64 group key per global row of one string column: the ordinal of the row's value in one dictionary
    per collection and field, value -> ordinal in first-seen order.  Rows are keyed once; an ordinal, once given, never
    changes (compact() gathers the keys and keeps the dictionary), so equal keys stay equal and distinct ones distinct."""

    def __init__(self):
        self.ordinals: Dict[str, int] = {}
        self._keys = np.empty(0, dtype=np.int64)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def extend(self, values: Iterable[str]) -> None:
        ordinals = self.ordinals
        new = [ordinals.setdefault(v, len(ordinals)) for v in values]
        if not new:
            return
        self._keys = _grown(self._keys, self._n + len(new))
        self._keys[self._n: self._n + len(new)] = new
        self._n += len(new)

    def compact(self, keep: np.ndarray) -> None:
        """Drop the rows whose entry of the boolean `keep` is False.  The dictionary stays: an ordinal never changes."""
        self._keys = self._keys[: self._n][_keep_mask(keep, self._n)]
        self._n = self._keys.shape[0]

    def sync(self, column: "StringColumn") -> "GroupKeyColumn":
        """Key the rows of `column` this column does not hold yet."""
        step = 1 << 16       # bounded temporaries
        for a in range(self._n, len(column), step):
            self.extend(column[a: min(len(column), a + step)])
        return self

    def array(self) -> np.ndarray:
        """int64 [rows] view (no copy)."""
        return self._keys[: self._n]

    @property
    def nbytes(self) -> int:
        return self._keys.nbytes


class EpochColumn:
    """Append-only float64 per global row of the timestamp column: decay.epoch_seconds of the row's text (seconds since
    1970-01-01 UTC; NaN = the row has no time).  Rows are parsed once."""

    def __init__(self):
        self._a = np.empty(0, dtype=np.float64)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def extend(self, texts: Iterable[str]) -> None:
        from .decay import epoch_seconds
        new = [epoch_seconds(t) for t in texts]
        if not new:
            return
        self._a = _grown(self._a, self._n + len(new))
        self._a[self._n: self._n + len(new)] = new
        self._n += len(new)

    def compact(self, keep: np.ndarray) -> None:
        """Drop the rows whose entry of the boolean `keep` is False; the others move up in order."""
        self._a = self._a[: self._n][_keep_mask(keep, self._n)]
        self._n = self._a.shape[0]

    def sync(self, column: "StringColumn") -> "EpochColumn":
        """Parse the rows of `column` this column does not hold yet."""
        step = 1 << 16       # bounded temporaries
        for a in range(self._n, len(column), step):
            self.extend(column[a: min(len(column), a + step)])
        return self

    def array(self) -> np.ndarray:
        """float64 [rows] view (no copy)."""
        return self._a[: self._n]

    @property
    def nbytes(self) -> int:
        return self._a.nbytes


class PayloadColumns:
    """dict-like: columns["id"][row], columns["entropy"].array(), len(columns["id"])."""

    def __init__(self):
        self._c: Dict[str, Any] = {k: StringColumn() for k in STRING_COLUMNS}
        self._c.update({k: NumericColumn(np.int64) for k in INT_COLUMNS})
        self._c.update({k: NumericColumn(np.float32) for k in FLOAT_COLUMNS})
        self._token_sets: Optional[TokenSetColumn] = None    # derived from "content" on first use; not a payload field
        self._word_sets: Optional[TokenSetColumn] = None     # the same under filters.analyze: what TEXT_MATCH reads
        self._word_lock = threading.Lock()                   # the build and the extension are read-modify-write
        self._group_keys: Dict[str, GroupKeyColumn] = {}     # string column -> its rows' group keys, on first use
        # the lazy build and the extension of a group-key column are read-modify-write: the searches of one request run in
        # different threads (a sharded manager has no front) and ask for the same field at once
        self._group_lock = threading.Lock()
        self._epoch: Optional[EpochColumn] = None            # derived from "timestamp" on first use (the decay ranker's field)
        self._epoch_lock = threading.Lock()
        self._token_vectors: Optional[TokenVectorColumn] = None   # the late-interaction store, when the manager has a token_dim
        self._tokvec_lock = threading.Lock()

    def __getitem__(self, name: str):
        return self._c["id" if name == "chunk_id" else name]

    def __contains__(self, name: str) -> bool:
        return name == "chunk_id" or name in self._c

    def __iter__(self):
        return iter(self._c)

    def items(self):
        return self._c.items()

    def keys(self):
        return self._c.keys()

    def __len__(self) -> int:
        return len(self._c)

    @property
    def n_rows(self) -> int:
        return len(self._c["id"])

    @property
    def nbytes(self) -> int:
        return sum(c.nbytes for c in self._c.values())

    def token_sets(self) -> TokenSetColumn:
        """The token sets of every row's content: built on first use, extended by what later appends added."""
        if self._token_sets is None:
            self._token_sets = TokenSetColumn()
        return self._token_sets.sync(self._c["content"])

    def word_sets(self) -> TokenSetColumn:
        """The WORD sets of every row's content, what TEXT_MATCH filters on: a second TokenSetColumn whose tokenizer is
        filters.analyze (the BM25 words: "timeout," is "timeout"), with a dictionary of its own (`.ids`, word -> id in
        first-seen order; an id never changes).  Built on first use — the host tokenises every row once —, extended by
        what later appends added, gathered by compact(), never part of a snapshot."""
        with self._word_lock:
            if self._word_sets is None:
                from .filters import analyze
                self._word_sets = TokenSetColumn(analyze)
            return self._word_sets.sync(self._c["content"])

    def group_keys(self, field: str) -> np.ndarray:
        """int64 group key of every row for a grouping search on `field` (a view, no copy): the column itself for an
        integer field, dictionary ordinals (GroupKeyColumn) for a string field — built on first use, extended by what
        later appends added.  ValueError for a float or an unknown field."""
        check_group_field(field)
        if field in INT_COLUMNS:
            return self._c[field].array()
        name = GROUP_STRING_FIELDS[field]
        with self._group_lock:
            col = self._group_keys.get(name)
            if col is None:
                col = self._group_keys[name] = GroupKeyColumn()
            return col.sync(self._c[name]).array()

    def epoch_seconds(self) -> np.ndarray:
        """float64 seconds since 1970-01-01 UTC of every row's timestamp (a view, no copy; NaN where the text is empty or
        no ISO time): what the decay ranker reads for field="timestamp".  Built on first use — the host parses every row
        once —, extended by what later appends added, gathered by compact(), never part of a snapshot."""
        with self._epoch_lock:
            if self._epoch is None:
                self._epoch = EpochColumn()
            return self._epoch.sync(self._c["timestamp"]).array()

    def enable_token_vectors(self, dim: int, reset: bool = False) -> None:
        """Give the collection a token-vector column of `dim` elements per vector (rows so far have none); reset = drop
        the vectors a column of that dim already holds."""
        with self._tokvec_lock:
            if reset or self._token_vectors is None or self._token_vectors.dim != int(dim):
                self._token_vectors = TokenVectorColumn(dim)

    def token_vectors(self) -> Optional[TokenVectorColumn]:
        """The token vectors of every row (None when the collection keeps none): rows appended without vectors are padded
        with T_r = 0 here, so the column always covers n_rows.  Gathered by compact(), never part of a snapshot."""
        with self._tokvec_lock:
            return None if self._token_vectors is None else self._token_vectors.pad_to(self.n_rows)

    def extend_token_vectors(self, base: int, indptr: np.ndarray, values: np.ndarray) -> None:
        """The vectors of the rows appended at global row `base` (rows before it that have none yet are padded)."""
        with self._tokvec_lock:
            col = self._token_vectors.pad_to(base)
            if len(col) != base:
                raise ValueError(f"token vectors for row {base} arrive after row {len(col)} was written")
            col.extend(indptr, values)

    def compact(self, keep: np.ndarray) -> None:
        """Drop the rows whose entry of the boolean `keep` (one per row) is False from every column, one column at a
        time (the peak extra memory is one column), and from the token sets and the group keys as far as they are built."""
        keep = _keep_mask(keep, self.n_rows)
        with self._tokvec_lock:
            if self._token_vectors is not None:
                self._token_vectors.pad_to(self.n_rows).compact(keep)
        for col in self._c.values():
            col.compact(keep)
        if self._token_sets is not None:
            n = len(self._token_sets)
            self._token_sets.compact(keep[:n])
        with self._word_lock:
            if self._word_sets is not None:
                self._word_sets.compact(keep[:len(self._word_sets)])
        with self._group_lock:
            for col in self._group_keys.values():
                col.compact(keep[:len(col)])
        with self._epoch_lock:
            if self._epoch is not None:
                self._epoch.compact(keep[:len(self._epoch)])

    def filter_columns(self) -> Dict[str, np.ndarray]:
        """What filters.evaluate takes: numpy arrays per field (string fields as unicode arrays — fine for small
        collections; large ones go through device_filters, which never materialises them)."""
        out = {k: self._c[k].array() for k in INT_COLUMNS + FLOAT_COLUMNS}
        for k in ("id", "doc_id", "timestamp"):
            out[k] = self._c[k].as_str_array()
        out["chunk_id"] = out["id"]
        return out
