"""Filter expressions evaluated on the GPU over HBM-resident scalar columns.

The reference hands `expr` to Milvus (indexing.py:503-525) which evaluates it server-side over the scalar fields of
the schema (indexing.py:191-225).  Here the payload columns live on the host (columns.py) and a COPY of the
filterable ones lives in HBM — uploaded the first time a field is filtered on, extended by what later appends
added — so that an expression becomes one `hr_filter_eval_dev` launch (a conjunction of comparisons) or one
`hr_filter_eval_expr_dev` launch (`in` lists, or, not, parentheses: leaves, sorted sets and a postfix program) that writes the packed row mask the search
kernels take (no row-sized transfer in either direction; the first filtered request at 10M rows took 44 ms on the
host, the mask was re-uploaded with every search).

A keyword leaf, TEXT_MATCH(content, "words"), reads the rows' WORD SETS instead of a scalar column: a CSR of int32 word ids
(columns.PayloadColumns.word_sets, mirrored by device_tokens.DeviceTokenSets and owned here, so it goes wherever this object
goes).  The query's words are looked up in the collection's dictionary on the host and travel like an `in` set.

Strings (doc_id, chunk_id, timestamp) are compared through order-preserving 16-byte prefix keys; the rare rows whose
first 16 bytes equal the literal's come back in an "undecided" mask and are settled here on the full strings.
`filters.evaluate` (numpy, host) is the restatement the tests hold this against, bit for bit.
"""
from __future__ import annotations

import threading
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _native as nat
from . import filters as _filters
from .columns import FLOAT_COLUMNS, INT_COLUMNS, StringColumn

_STRING_FIELDS = {"id": "id", "chunk_id": "id", "doc_id": "doc_id", "timestamp": "timestamp"}


def mask_bytes(n_rows: int) -> int:
    return 8 * ((n_rows + 63) // 64)


def unpack_mask(mask_u8, n_rows: int):
    """uint8 CUDA tensor of packed bits -> bool CUDA tensor [n_rows]."""
    import torch
    shifts = torch.arange(8, device=mask_u8.device, dtype=torch.uint8)
    return ((mask_u8[:, None] >> shifts[None, :]) & 1).reshape(-1)[:n_rows].bool()


def pack_mask(keep, n_rows: int):
    """bool CUDA tensor [n_rows] -> uint8 CUDA tensor of mask_bytes(n_rows) packed bits."""
    import torch
    padded = torch.zeros(mask_bytes(n_rows) * 8, dtype=torch.uint8, device=keep.device)
    padded[:n_rows] = keep.to(torch.uint8)
    weights = (1 << torch.arange(8, device=keep.device, dtype=torch.int32))
    return (padded.view(-1, 8).to(torch.int32) * weights[None, :]).sum(dim=1).to(torch.uint8)


class _Program:
    """What an expression beyond the flat conjunction carries besides its leaves: the postfix codes over them, the tree
    (undecided rows are settled on it) and the device tensors of the leaves' sets (alive until the stream has passed)."""

    def __init__(self, codes: List[int], tree, sets: list):
        self.codes, self.tree, self.sets = codes, tree, sets


class DeviceFilters:
    def __init__(self, columns, device: int):
        self.columns = columns                  # PayloadColumns, or None for a payload-free (synthetic) collection
        self.device = int(device)
        self._dev: Dict[str, Tuple[Any, int]] = {}   # column -> (device tensor with spare capacity, rows uploaded)
        # expr_evaluations: the evaluations among them that took hr_filter_eval_expr_dev (anything but a flat conjunction)
        # match_leaves: the TEXT_MATCH leaves among the evaluated expressions
        self.stats = {"evaluations": 0, "expr_evaluations": 0, "undecided_rows": 0, "uploaded_bytes": 0, "match_leaves": 0}
        self._words = None                      # DeviceTokenSets over columns.word_sets(): built by the first TEXT_MATCH
        # one evaluation at a time: the column tensors are owned by `_dev` alone, so a second thread that re-uploads a
        # column (the dense and the sparse search of an uncoalesced retrieve() evaluate a new expression concurrently)
        # would free the tensor the first thread's kernel is about to read
        self._lock = threading.RLock()

    # ------------------------------------------------------------------ columns in HBM
    def _tensor(self, name: str, host_rows, n: int, width: int = 1):
        """Device copy of a host column, valid for rows < n: uploads only what is not there yet."""
        import torch
        dev = torch.device("cuda", self.device)
        cur, have = self._dev.get(name, (None, 0))
        if cur is None or cur.shape[0] < n:
            cap = max(n, (cur.shape[0] * 3 // 2) if cur is not None else 0, 1024)
            shape = (cap, width) if width > 1 else (cap,)
            grown = torch.empty(shape, dtype=torch.int64 if host_rows(0, 0).dtype.kind in "iu" else torch.float32, device=dev)
            if cur is not None and have:
                grown[:have] = cur[:have]
            cur = grown
        if have < n:
            part = np.ascontiguousarray(host_rows(have, n))
            if part.dtype == np.uint64:
                part = part.view(np.int64)       # same bits; the kernel compares them as unsigned
            cur[have:n] = torch.from_numpy(part).to(dev)
            self.stats["uploaded_bytes"] += part.nbytes
        self._dev[name] = (cur, n)
        return cur

    def _column(self, field: str, n: int):
        if self.columns is None:   # payload-free rows: what the synthetic id encodes (chunk_index = row % 10)
            import torch
            cur, have = self._dev.get("chunk_index", (None, 0))
            if cur is None or have < n:
                cur = torch.arange(n, dtype=torch.int64, device=torch.device("cuda", self.device)) % 10
                self._dev["chunk_index"] = (cur, n)
            return cur
        if field in _STRING_FIELDS:
            col = self.columns[_STRING_FIELDS[field]]
            return self._tensor("key:" + _STRING_FIELDS[field], lambda a, b: col.keys()[a:b], n, width=2)
        col = self.columns[field]
        return self._tensor(field, lambda a, b: col.array()[a:b], n)

    def _word_sets(self, stream):
        """-> (indptr int64 CUDA tensor [rows + 1], word ids int32 CUDA tensor or None, rows) of the word mirror, what
        later appends added uploaded on `stream`: the kernel that follows on that stream sees every row."""
        import torch
        from .device_tokens import DeviceTokenSets
        if self._words is None:
            self._words = DeviceTokenSets(self.columns, self.device, source=lambda cols: cols.word_sets())
        before = self._words.stats["uploaded_bytes"]
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", self.device))):
            indptr, tok, rows = self._words.tensors()
            if indptr is None:       # a collection without a row: one offset, no word
                indptr = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", self.device))
        self.stats["uploaded_bytes"] += self._words.stats["uploaded_bytes"] - before
        return indptr, tok, rows

    @property
    def word_mirror_bytes(self) -> int:
        """HBM the word mirror holds (0 before the first TEXT_MATCH)."""
        return self._words.nbytes if self._words is not None else 0

    def _match_ids(self, field: str, text: str) -> np.ndarray:
        """The query words of TEXT_MATCH(field, text) as the kernel searches them: their ids in the collection's
        dictionary, ascending, each once; a word no row holds has no id and is dropped (it can match nothing)."""
        if self.columns is None:
            raise ValueError("this shard was bulk-ingested without payload columns: only chunk_index (= row % 10) "
                             f"can be filtered on, not {[field]}")
        if field not in _filters.TEXT_FIELDS:
            raise ValueError(f"TEXT_MATCH analyses only the field content, not {field}, in filter term: TEXT_MATCH({field}, ...)")
        ids = self.columns.word_sets().ids      # the first use tokenises every row on the host, once
        return np.asarray(sorted({ids[w] for w in set(_filters.analyze(text)) if w in ids}), dtype=np.int32)

    # ------------------------------------------------------------------ expression -> terms
    def _term(self, field: str, op: str, value) -> Tuple["nat.FilterTerm", Optional[Tuple[str, str, str]]]:
        """One comparison as the kernel takes it (no column pointer yet) and, for a string field, what settles its ties."""
        if self.columns is None and field != "chunk_index":
            raise ValueError("this shard was bulk-ingested without payload columns: only chunk_index (= row % 10) "
                             f"can be filtered on, not {[field]}")
        t = nat.FilterTerm()
        t.op = nat.FILTER_OPS[op]
        if field in INT_COLUMNS:
            if isinstance(value, str):
                raise ValueError(f"field {field} is numeric; got string {value!r}")
            value = _filters.numeric_literal(field, op, value, "i")   # ctypes would wrap an int beyond int64 silently
            if isinstance(value, float):
                t.kind, t.dval = nat.HR_COL_I64_VS_F64, value
            else:
                t.kind, t.ival = nat.HR_COL_I64, value
        elif field in FLOAT_COLUMNS:
            if isinstance(value, str):
                raise ValueError(f"field {field} is numeric; got string {value!r}")
            t.kind, t.fval = nat.HR_COL_F32, float(_filters.numeric_literal(field, op, value, "f"))
        elif field in _STRING_FIELDS:
            if not isinstance(value, str):
                raise ValueError(f"field {field} is a string column; got {value!r}")
            t.kind = nat.HR_COL_STR16
            t.key[0], t.key[1] = StringColumn.key_of(value)
            return t, (_STRING_FIELDS[field], op, value)
        else:
            raise ValueError(f"unknown filter field: {field}")
        return t, None

    def _terms(self, expr: str, n: int, stream=None):
        """-> (terms, string_terms) for a flat conjunction of comparisons (hr_filter_eval_dev, as ever), or
        (leaves, _Program) for every other expression (hr_filter_eval_expr_dev)."""
        # every term is checked and built before the first column is touched: an expression that is refused (a literal
        # that would wrap in its field, a type mismatch, an unknown field, too many terms) uploads nothing
        flat, tree = _filters.lower(expr)
        if tree is None:
            terms, string_terms, fields = [], [], []
            for field, op, value in flat:
                t, settle = self._term(field, op, value)
                if settle is not None:
                    string_terms.append(settle)
                terms.append(t)
                fields.append(field)
            if len(terms) > 16:
                raise ValueError("a filter expression may hold up to 16 terms")
            for t, field in zip(terms, fields):
                t.col = self._column(field, n).data_ptr()
            return terms, string_terms
        leaves, fields, sets, program = [], [], [], []

        def emit(node):
            if node[0] in ("and", "or"):
                emit(node[1])
                emit(node[2])
                program.append(nat.HR_FILTER_AND if node[0] == "and" else nat.HR_FILTER_OR)
            elif node[0] == "not":
                emit(node[1])
                program.append(nat.HR_FILTER_NOT)
            else:
                program.append(len(leaves))
                leaf, members = nat.FilterLeaf(), None
                if node[0] == "cmp":
                    leaf.term = self._term(node[1], node[2], node[3])[0]
                elif node[0] == "match":
                    members = self._match_ids(node[1], node[2])
                    leaf.term.kind, leaf.term.op, leaf.term.ival = nat.HR_COL_TOKENS, nat.HR_OP_MATCH, int(node[3])
                    leaf.n_set = members.shape[0]
                else:
                    leaf.term.op, members = nat.HR_OP_IN, self._members(node[1], node[2])
                    leaf.term.kind = {np.int64: nat.HR_COL_I64, np.float32: nat.HR_COL_F32, np.uint64: nat.HR_COL_STR16}[members.dtype.type]
                    leaf.n_set = members.shape[0]
                leaves.append(leaf)
                fields.append(node[1])
                sets.append(members)

        emit(tree)
        set_bytes = sum((m.nbytes + 15) // 16 * 16 for m in sets if m is not None)
        if len(leaves) > nat.HR_MAX_FILTER_TERMS:
            raise ValueError(f"a filter expression may hold up to {nat.HR_MAX_FILTER_TERMS} terms (an `in` list is one term)")
        if len(program) > nat.HR_MAX_FILTER_PROGRAM:
            raise ValueError(f"a filter expression may hold up to {nat.HR_MAX_FILTER_PROGRAM} terms and operators together")
        if set_bytes > nat.HR_MAX_FILTER_SET_BYTES:
            raise ValueError("the `in` lists of one filter expression may hold up to 4096 strings or 8192 integers together, "
                             "the TEXT_MATCH texts 16384 words "
                             f"({nat.HR_MAX_FILTER_SET_BYTES} bytes of members; this one has {set_bytes})")
        import torch
        dev = torch.device("cuda", self.device)
        for i, (leaf, field) in enumerate(zip(leaves, fields)):
            if leaf.term.op == nat.HR_OP_MATCH:
                indptr, tok, rows = self._word_sets(stream)
                leaf.term.col, leaf.term.key[0], leaf.term.key[1] = indptr.data_ptr(), tok.data_ptr() if tok is not None else 0, rows
                sets.append(indptr)              # (an own tensor for an empty collection) alive as long as the sets
            else:
                leaf.term.col = self._column(field, n).data_ptr()
            if sets[i] is not None and sets[i].shape[0]:
                m = sets[i]
                sets[i] = torch.from_numpy(m.view(np.int64) if m.dtype == np.uint64 else m).to(dev)   # lives until the stream is synchronised
                leaf.set = sets[i].data_ptr()
        return leaves, _Program(program, tree, sets)

    def _members(self, field: str, values) -> np.ndarray:
        """The set of `field in values` as the kernel searches it: sorted, without duplicates; int64, float32 (no NaN,
        -0.0 folded into 0.0) or [n, 2] uint64 prefix keys in lexicographic order (literals that share their first 16
        bytes are one key: such a row is undecided either way)."""
        if self.columns is None and field != "chunk_index":
            raise ValueError("this shard was bulk-ingested without payload columns: only chunk_index (= row % 10) "
                             f"can be filtered on, not {[field]}")
        if field in INT_COLUMNS:
            return np.unique(np.asarray(_filters.list_members(field, values, "i"), dtype=np.int64))
        if field in FLOAT_COLUMNS:
            m = np.asarray(_filters.list_members(field, values, "f"), dtype=np.float32)
            return np.unique(m[m == m] + np.float32(0.0))       # x + 0.0: -0.0 becomes 0.0, everything else stays
        if field in _STRING_FIELDS:
            keys = sorted({StringColumn.key_of(v) for v in _filters.list_members(field, values, "s")})
            return np.asarray(keys, dtype=np.uint64).reshape(-1, 2)
        raise ValueError(f"unknown filter field: {field}")

    def _settle(self, tree, rows: np.ndarray) -> np.ndarray:
        """The whole tree on the given rows, string leaves on the full strings: which undecided rows pass."""
        def leaf(node):
            field = node[1]
            if node[0] == "match":
                content = self.columns["content"]
                return _filters.match_rows([content[int(r)] for r in rows], node[2], node[3])
            if field in _STRING_FIELDS:
                col = self.columns[_STRING_FIELDS[field]]
                return col.member_rows(rows, node[2]) if node[0] == "in" else col.compare_rows(rows, node[2], node[3])
            values = rows % 10 if self.columns is None else self.columns[field].array()[rows]
            return _filters._leaf_mask(node, {field: values})
        return _filters.evaluate_tree(tree, leaf)

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, expr: Optional[str], n_rows: int, deleted: Optional[np.ndarray] = None, stream=None):
        """-> (uint8 CUDA tensor of mask_bytes(n_rows) packed bits, rows kept).  expr None = tombstones only."""
        with self._lock:
            return self._evaluate_locked(expr, n_rows, deleted, stream)

    def _evaluate_locked(self, expr, n_rows, deleted, stream):
        import torch
        dev = torch.device("cuda", self.device)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        terms, settle = self._terms(expr, n_rows, st) if expr else ([], [])
        program = settle if isinstance(settle, _Program) else None
        mask = torch.empty(mask_bytes(n_rows), dtype=torch.uint8, device=dev)
        und = torch.empty(mask_bytes(n_rows), dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        d_del = None
        if deleted is not None and deleted[:n_rows].any():
            bits = np.zeros(mask_bytes(n_rows), dtype=np.uint8)
            packed = np.packbits(deleted[:n_rows], bitorder="little")
            bits[: packed.size] = packed
            d_del = torch.from_numpy(bits).to(dev)
        with torch.cuda.stream(st):   # the read-backs and the fix-ups below are ordered behind the kernel on ITS stream
            if program is None:
                nat.filter_eval_dev(terms, n_rows, d_del.data_ptr() if d_del is not None else 0, mask.data_ptr(), und.data_ptr(),
                                    counts.data_ptr(), st.cuda_stream)
            else:
                nat.filter_eval_expr_dev(terms, program.codes, n_rows, d_del.data_ptr() if d_del is not None else 0, mask.data_ptr(),
                                         und.data_ptr(), counts.data_ptr(), st.cuda_stream)
                self.stats["expr_evaluations"] += 1
                self.stats["match_leaves"] += sum(1 for leaf in terms if leaf.term.op == nat.HR_OP_MATCH)
            kept, undecided = (int(x) for x in counts.cpu().tolist())   # synchronises the stream (the sets may go after it)
            self.stats["evaluations"] += 1
            if undecided:
                # rows that tie with a literal on the first 16 bytes.  A conjunction: every other term has already passed
                # them; settle the string terms on the full strings (host) and switch the survivors on.  Any other tree
                # is evaluated whole on those rows.
                self.stats["undecided_rows"] += undecided
                rows = np.nonzero(np.unpackbits(und.cpu().numpy(), bitorder="little")[:n_rows])[0]
                if program is None:
                    ok = np.ones(rows.shape[0], dtype=bool)
                    for col_name, op, value in settle:
                        ok &= self.columns[col_name].compare_rows(rows, op, value)
                else:
                    ok = self._settle(program.tree, rows)
                rows = rows[ok]
                kept += int(rows.shape[0])
                for b in range(8):   # rows with the same bit position touch distinct bytes: plain indexed updates
                    sel = rows[(rows & 7) == b]
                    if sel.size:
                        idx = torch.from_numpy(sel >> 3).to(dev)
                        mask[idx] = mask[idx] | (1 << b)
                # the mask is cached and handed to searches on OTHER streams (the front's dense / sparse / hybrid streams,
                # the host view of _row_mask): only a finished mask may leave this function
                st.synchronize()
        return mask, kept
