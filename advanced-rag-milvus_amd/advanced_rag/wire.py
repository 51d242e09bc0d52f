"""The wire format of a collection that spans ranks (shards.CollectiveShardSet): pure functions over numpy arrays, torch
only where a caller hands a tensor in.  Private to the ranks of one run — nothing is stored in this format.

A packet is HEADER int64 words followed by a payload of typed sections:

    word 0                  the op (OP_*)
    words 1 ..              the op's fields, in the order of FIELDS[op]
    words HEADER-4 .. -2    mask_id, mask_new, mask_len — of every op that carries a row filter (FILTERED)
    word HEADER-1           the payload's byte count, for every op

`pack` writes a packet and `unpack_header` reads its header back by field name; `Sections` walks the payload.  The lists
travelling back to rank 0 are one int64 vector per rank: `pack_lists` / `unpack_lists`."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Mapping, Optional, Sequence

import numpy as np

HEADER = 16                     # int64 words
HEADER_BYTES = HEADER * 8
PACKET_BYTES = 1 << 20          # header + queries of one round (128 x (768-d dense + 100-term sparse) = 0.5 MB)

OP_STOP, OP_ROUND, OP_ADD, OP_FLUSH, OP_SAVE, OP_ROWMAPS, OP_HYBRID = range(7)
OP_NAMES = {OP_STOP: "stop", OP_ROUND: "round", OP_ADD: "add", OP_FLUSH: "flush", OP_SAVE: "save", OP_ROWMAPS: "row_maps",
            OP_HYBRID: "hybrid"}
FIELDS = {
    OP_ROUND: ("Bd", "Bs", "k", "dim", "nnz", "drop"),
    OP_HYBRID: ("B", "top_k", "dim", "nnz", "rrf_k", "max_nnz"),
    OP_ADD: ("nrows", "dim", "has_dense", "has_sparse", "nnz"),
}
MASK_FIELDS = ("mask_id", "mask_new", "mask_len")
FILTERED = (OP_ROUND, OP_HYBRID)
FLOAT_FIELDS = ("drop",)        # travel as the bits of a float64
_MASK_WORD = HEADER - 1 - len(MASK_FIELDS)
assert all(1 + len(names) <= _MASK_WORD for names in FIELDS.values())


def float_bits(x: float) -> int:
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def bits_float(w: int) -> float:
    return float(np.array([w], dtype=np.int64).view(np.float64)[0])


def _layout(op: int):
    """[(word, field name)] of an op's header."""
    words = list(enumerate(FIELDS.get(op, ()), 1))
    return words + list(enumerate(MASK_FIELDS, _MASK_WORD)) if op in FILTERED else words


def mask_fields(mask_id: int, is_new, packed: Optional[np.ndarray]) -> dict:
    """MaskCache.lookup's answer as the header's mask triple."""
    return {"mask_id": int(mask_id), "mask_new": int(is_new), "mask_len": 0 if packed is None else int(packed.size)}


def pack(op: int, fields: Mapping = (), sections: Sequence[np.ndarray] = (), limit: int = PACKET_BYTES) -> np.ndarray:
    """One packet as uint8: the header of `op` with `fields` by name (an absent mask triple means "no filter"), then the
    `sections` in order, each as its own bytes.  The ONE place that holds a packet to its size: raises ValueError, before
    anything can have been sent."""
    fields = dict(fields)
    layout = _layout(op)
    unknown = set(fields) - {name for _, name in layout}
    if unknown:
        raise KeyError(f"{OP_NAMES[op]} packet has no field(s) {sorted(unknown)}")
    hdr = np.zeros(HEADER, dtype=np.int64)
    hdr[0] = op
    for word, name in layout:
        v = fields.get(name, 0) if name in MASK_FIELDS else fields[name]
        hdr[word] = float_bits(v) if name in FLOAT_FIELDS else int(v)
    raw = [np.ascontiguousarray(s).reshape(-1).view(np.uint8) for s in sections]
    hdr[HEADER - 1] = sum(r.size for r in raw)
    need = HEADER_BYTES + int(hdr[HEADER - 1])
    if need > limit:
        raise ValueError(f"a {OP_NAMES[op]} packet of {need} bytes was asked for; the packet holds {limit}")
    return np.concatenate([hdr.view(np.uint8)] + raw)


def unpack_header(buf: np.ndarray):
    """-> (op, fields, payload_bytes) of a packet's first HEADER_BYTES bytes; `fields` has one attribute per field name."""
    hdr = np.ascontiguousarray(buf[: HEADER_BYTES]).view(np.int64)
    op = int(hdr[0])
    fields = SimpleNamespace(**{name: bits_float(hdr[word]) if name in FLOAT_FIELDS else int(hdr[word])
                                for word, name in _layout(op)})
    return op, fields, int(hdr[HEADER - 1])


def payload(buf: np.ndarray) -> np.ndarray:
    """The payload bytes of a packet (a control op's blob)."""
    return buf[HEADER_BYTES: HEADER_BYTES + unpack_header(buf)[2]]


class Sections:
    """A cursor over a packet's payload: take(count, dtype) is the next `count` items as a typed view, no copy.  `buf` is
    the packet as a numpy uint8 array or a torch uint8 tensor (CPU or CUDA) — the views are then of the same kind.  The
    writer lays 8-byte items first; take() holds it to that: a view must start at a multiple of its item size."""

    def __init__(self, buf, start: int = HEADER_BYTES):
        self.buf, self.off = buf, start

    def take(self, count: int, dtype):
        dtype = np.dtype(dtype)
        assert self.off % dtype.itemsize == 0, f"a {dtype.name} section at byte {self.off} of the packet is misaligned"
        raw = self.buf[self.off: self.off + count * dtype.itemsize]
        if raw.shape[0] != count * dtype.itemsize:
            raise ValueError(f"the packet ends {count * dtype.itemsize - raw.shape[0]} bytes before its {dtype.name} section does")
        self.off += count * dtype.itemsize
        if isinstance(raw, np.ndarray):
            return raw.view(dtype)
        import torch
        return raw.view(getattr(torch, dtype.name))


def pack_lists(lists, n_vals: int) -> np.ndarray:
    """A rank's answer to a round as int64 [1 + 2 * n_vals]: a status word (0 = ok), the ids of every list, then the
    score BITS of every list (float32 as int32, widened: every bit survives, NaN payloads and -0.0 included).  `lists` is
    [(ids [B, k], scores [B, k])] per modality in the round, n_vals their total length; None = this rank failed (status 1,
    ids all -1)."""
    out = np.zeros(1 + 2 * n_vals, dtype=np.int64)
    if lists is None:
        out[0] = 1
        out[1: 1 + n_vals] = -1
        return out
    out[1: 1 + n_vals] = np.concatenate([ids.reshape(-1) for ids, _ in lists])
    out[1 + n_vals:] = np.concatenate([sc.reshape(-1) for _, sc in lists]).astype(np.float32).view(np.int32)
    return out


def unpack_lists(parts: Sequence[np.ndarray], Bs_per_modality: Sequence[int], k: int):
    """The ranks' pack_lists vectors -> (ranks that failed, per modality None (no query of it in the round) or
    ([ids [B, k] per rank], [scores [B, k] per rank])).  With a failed rank the lists are not decoded."""
    bad = [r for r, p in enumerate(parts) if p[0] != 0]
    if bad:
        return bad, None
    n_vals = sum(Bs_per_modality) * k
    out, o = [], 1
    for B in Bs_per_modality:
        if not B:
            out.append(None)
            continue
        out.append(([p[o: o + B * k].reshape(B, k) for p in parts],
                    [p[n_vals + o: n_vals + o + B * k].astype(np.int32).view(np.float32).reshape(B, k) for p in parts]))
        o += B * k
    return bad, out
