"""The wire format of the collective shard set (advanced_rag/wire.py) and the small pieces that go with it (the mask
cache, the raw CSR of a query batch, the renumbering of lists) — no process group, no GPU."""
import itertools

import numpy as np
import pytest

from advanced_rag import wire
from advanced_rag.shards import CollectiveShardSet, MaskCache, empty_lists, to_global
from advanced_rag.staging import csr_of_queries

MASK = dict(mask_id=7, mask_new=1, mask_len=12_345)
NO_MASK = dict(mask_id=0, mask_new=0, mask_len=0)


def _header_cases():
    for Bd, Bs, drop, mask in itertools.product((0, 1, 128), (0, 1, 128), (0.0, 0.2, 1.0), (None, MASK)):
        yield wire.OP_ROUND, dict(Bd=Bd, Bs=Bs, k=256, dim=768 if Bd else 0, nnz=0, drop=drop), mask, 0
    for B, mask in itertools.product((1, 128), (None, MASK)):
        yield wire.OP_HYBRID, dict(B=B, top_k=256, dim=1, nnz=2 ** 31 + 1, rrf_k=60, max_nnz=100), mask, 40
    yield wire.OP_ADD, dict(nrows=2 ** 33, dim=4096, has_dense=1, has_sparse=0, nnz=0), None, 0
    yield wire.OP_ADD, dict(nrows=0, dim=0, has_dense=0, has_sparse=1, nnz=2 ** 40), None, 0
    for op in (wire.OP_STOP, wire.OP_FLUSH, wire.OP_ROWMAPS):
        yield op, {}, None, 0
    yield wire.OP_SAVE, {}, None, 77


def test_header_round_trip_for_every_op():
    seen = set()
    for op, fields, mask, n_payload in _header_cases():
        seen.add(op)
        blob = np.arange(n_payload, dtype=np.uint8)
        body = wire.pack(op, {**fields, **(mask or {})}, [blob])
        assert body.dtype == np.uint8 and body.size == wire.HEADER * 8 + n_payload
        want = dict(fields, **((mask or NO_MASK) if op in wire.FILTERED else {}))
        # the packet as a receiver holds it: junk after the body, which decoding must not look at
        packet = np.full(wire.PACKET_BYTES, 0xA5, dtype=np.uint8)
        packet[: body.size] = body
        for buf in (body, packet, body[: wire.HEADER * 8]):
            got_op, got, got_n = wire.unpack_header(buf)
            assert (got_op, vars(got), got_n) == (op, want, n_payload), (op, fields)
        assert all(type(v) is (float if name in wire.FLOAT_FIELDS else int) for name, v in vars(got).items())
        assert np.array_equal(wire.payload(packet), blob)
    assert seen == set(wire.OP_NAMES)


def test_header_layout_is_the_declared_one():
    """The op in word 0, the payload's byte count in the last word of every op, the mask triple in the same three words
    of every op that carries a filter; a field is read where it was written, by name."""
    words, mask = {}, dict(mask_id=701, mask_new=702, mask_len=703)
    for op, fields in ((wire.OP_ROUND, dict(Bd=1, Bs=2, k=3, dim=4, nnz=5, drop=0.5)),
                       (wire.OP_HYBRID, dict(B=1, top_k=2, dim=3, nnz=4, rrf_k=5, max_nnz=6))):
        hdr = wire.pack(op, {**fields, **mask}, [np.zeros(9, np.uint8)])[: wire.HEADER * 8].view(np.int64)
        assert hdr[0] == op and hdr[wire.HEADER - 1] == 9
        words[op] = [int(np.nonzero(hdr == v)[0][0]) for v in mask.values()]
        got = vars(wire.unpack_header(hdr.view(np.uint8))[1])
        assert got == {**fields, **mask}               # distinct values: a swapped pair of positions would show
    assert words[wire.OP_ROUND] == words[wire.OP_HYBRID]
    assert wire.pack(wire.OP_STOP).view(np.int64)[wire.HEADER - 1] == 0
    assert wire.bits_float(wire.float_bits(0.2)) == 0.2 and wire.float_bits(0.0) == 0
    with pytest.raises(KeyError):
        wire.pack(wire.OP_ADD, dict(nrows=1, dim=1, has_dense=1, has_sparse=0, nnz=0, mask_id=3))    # an add carries no filter
    with pytest.raises(KeyError):
        wire.pack(wire.OP_ROUND, dict(Bd=1, Bs=0, k=1, dim=1, nnz=0))                                # a field left out


def _round_sections(rng, B, dim, nnz):
    ptr = np.linspace(0, nnz, B + 1).astype(np.int64)
    return [("ptr", ptr), ("dense", rng.standard_normal((B, dim)).astype(np.float32)),
            ("idx", rng.integers(0, 1000, nnz).astype(np.int32)), ("val", rng.random(nnz).astype(np.float32))]


def _hybrid_sections(rng, B, dim, nnz):
    ptr, dense, idx, val = _round_sections(rng, B, dim, nnz)
    return [ptr, ("weights", rng.random((B, 3))), dense, idx, val]


@pytest.mark.parametrize("op,fields,layout", [
    (wire.OP_ROUND, dict(Bd=0, Bs=0, k=1, dim=0, nnz=0, drop=0.0), _round_sections),
    (wire.OP_HYBRID, dict(B=0, top_k=1, dim=0, nnz=0, rrf_k=1, max_nnz=0), _hybrid_sections)], ids=["round", "hybrid"])
@pytest.mark.parametrize("B,dim,nnz", [(1, 1, 1), (1, 48, 7), (3, 1, 5), (3, 48, 31)])
def test_sections_read_the_same_from_numpy_and_torch(op, fields, layout, B, dim, nnz):
    import torch
    sections = layout(np.random.default_rng(B * 100 + dim + nnz), B, dim, nnz)
    body = wire.pack(op, fields, [a for _, a in sections])
    assert wire.unpack_header(body)[2] == sum(a.nbytes for _, a in sections)
    as_np, as_torch = wire.Sections(body), wire.Sections(torch.from_numpy(body.copy()))
    for name, a in sections:
        got_np, got_t = as_np.take(a.size, a.dtype), as_torch.take(a.size, a.dtype)
        assert isinstance(got_np, np.ndarray) and isinstance(got_t, torch.Tensor)
        assert got_np.dtype == a.dtype and got_t.numpy().dtype == a.dtype, name
        assert np.array_equal(got_np, a.reshape(-1)) and np.array_equal(got_t.numpy(), a.reshape(-1)), name
    assert as_np.off == as_torch.off == body.size
    with pytest.raises(ValueError):
        as_np.take(1, np.uint8)                       # nothing is read past the packet's end


def test_sections_refuse_a_misaligned_view():
    import torch
    body = wire.pack(wire.OP_SAVE, {}, [np.arange(3, dtype=np.int32), np.arange(1, dtype=np.int64)])
    for buf in (body, torch.from_numpy(body)):
        s = wire.Sections(buf)
        assert np.array_equal(np.asarray(s.take(3, np.int32)), [0, 1, 2])
        with pytest.raises(AssertionError):
            s.take(1, np.int64)


def test_size_limit_is_checked_in_pack():
    room = wire.PACKET_BYTES - wire.HEADER * 8
    body = wire.pack(wire.OP_SAVE, {}, [np.zeros(room - 3, np.uint8), np.zeros(3, np.uint8)])
    assert body.size == wire.PACKET_BYTES == CollectiveShardSet.PACKET_BYTES
    with pytest.raises(ValueError, match=rf"save packet of {wire.PACKET_BYTES + 1} bytes .* holds {wire.PACKET_BYTES}\b"):
        wire.pack(wire.OP_SAVE, {}, [np.zeros(room - 3, np.uint8), np.zeros(4, np.uint8)])
    with pytest.raises(ValueError, match="round packet"):
        wire.pack(wire.OP_ROUND, dict(Bd=1, Bs=0, k=1, dim=room // 4 + 1, nnz=0, drop=0.0), [np.zeros(room // 4 + 1, np.float32)])


def test_lists_keep_every_score_bit():
    k = 6
    bits = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x7FC00123, 0xFFC0FEED,        # -0.0, +-inf, subnormal, NaNs
                     0x3F800000, 0x00000000, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800001], dtype=np.uint32)
    dense = (np.array([[5, 2 ** 40, 3, -1, -1, -1], [0, 1, 2, 3, 4, 2 ** 62]], np.int64), bits.view(np.float32).reshape(2, k))
    sparse = (np.array([[9, -1, -1, -1, -1, -1]], np.int64), np.array([[1.5, 0, 0, 0, 0, 0]], np.float32))
    other = (dense[0] + 1, dense[1][::-1].copy())
    for lists, Bs in (([dense, sparse], (2, 1)), ([dense], (2, 0)), ([sparse], (0, 1))):
        n_vals = sum(Bs) * k
        parts = [wire.pack_lists(lists, n_vals), wire.pack_lists([other] + lists[1:] if Bs[0] else lists, n_vals)]
        assert all(p.dtype == np.int64 and p.shape == (1 + 2 * n_vals,) for p in parts)
        bad, got = wire.unpack_lists(parts, Bs, k)
        assert bad == [] and len(got) == 2
        want = iter(lists)
        for m, B in zip(got, Bs):
            if not B:
                assert m is None
                continue
            ids, scores = next(want)
            assert np.array_equal(m[0][0], ids) and m[1][0].dtype == np.float32
            assert np.array_equal(m[1][0].view(np.uint32), scores.view(np.uint32))
        if Bs[0]:
            assert np.array_equal(got[0][0][1], other[0]) and np.array_equal(got[0][1][1].view(np.uint32), other[1].view(np.uint32))
    failed = wire.pack_lists(None, 18)
    assert failed[0] == 1 and (failed[1:19] == -1).all()
    assert wire.unpack_lists([wire.pack_lists([dense, sparse], 18), failed], (2, 1), k)[0] == [1]
    assert wire.unpack_lists([failed, failed, wire.pack_lists([dense, sparse], 18)], (2, 1), k)[0] == [0, 1]


def test_mask_cache_is_first_in_first_out_and_evicts_both_halves():
    n = CollectiveShardSet.MAX_MASKS
    cache = MaskCache(n)
    assert cache.lookup(None) == (0, 0, None)
    filters = [np.arange(50) % (i + 2) == 0 for i in range(n + 2)]
    ids, made = [], []

    def upload(bits):
        made.append(bits)
        return ("device copy of", id(bits))

    for f in filters:
        mask_id, is_new, packed = cache.lookup(f)
        assert is_new == 1 and mask_id not in ids and mask_id != 0
        assert np.array_equal(np.unpackbits(packed, bitorder="little")[:50].astype(bool), f)
        cache.put(mask_id, f[10:30])
        assert cache.device(mask_id, upload) == ("device copy of", id(cache.get(mask_id)))
        if ids and ids[0] in cache:
            cache.get(ids[0])                         # a read does not renew an entry: first in first out, not LRU
        ids.append(mask_id)
    assert len(made) == n + 2
    assert [i in cache for i in ids] == [False, False] + [True] * n
    for gone in ids[:2]:
        with pytest.raises(KeyError):
            cache.get(gone)
        with pytest.raises(KeyError):                 # the device half went with the slice
            cache.device(gone, upload)
    for i, f in zip(ids[2:], filters[2:]):
        assert cache.lookup(f) == (i, 0, None)        # live: known, nothing to send
        assert np.array_equal(cache.get(i), f[10:30])
        assert cache.device(i, upload)[0] == "device copy of" and len(made) == n + 2      # made once
    mask_id, is_new, packed = cache.lookup(filters[0])        # evicted: travels again, under a fresh id
    assert is_new == 1 and mask_id not in ids and packed is not None
    cache.put(mask_id, filters[0][10:30])
    assert ids[2] not in cache and ids[3] in cache            # and pushes out the oldest
    cache.clear()
    assert not any(i in cache for i in ids + [mask_id])
    assert cache.lookup(filters[-1])[1] == 1


def test_csr_of_queries():
    ptr, idx, val = csr_of_queries([])
    assert ptr.tolist() == [0] and idx.shape == val.shape == (0,)
    assert (ptr.dtype, idx.dtype, val.dtype) == (np.int64, np.int32, np.float32)
    ptr, idx, val = csr_of_queries([([7, 3], [0.5, 0.25]), ([], []), (np.array([3], np.int64), np.array([2.0]))])
    assert ptr.tolist() == [0, 2, 2, 3] and idx.tolist() == [7, 3, 3] and val.tolist() == [0.5, 0.25, 2.0]   # as they came
    assert (ptr.dtype, idx.dtype, val.dtype) == (np.int64, np.int32, np.float32)
    ptr, idx, val = csr_of_queries([([], []), ([], [])])
    assert ptr.tolist() == [0, 0, 0] and (idx.dtype, val.dtype, idx.size, val.size) == (np.int32, np.float32, 0, 0)
    with pytest.raises(ValueError, match="query 1"):
        csr_of_queries([([1], [1.0]), ([1, 2], [1.0])])
    with pytest.raises(ValueError):
        csr_of_queries([([1], [1.0, 2.0]), ([1, 2], [1.0])])      # equal totals do not hide it


def test_to_global_and_empty_lists():
    rows = np.array([10, 20, 35], np.int64)
    got = to_global(np.array([[2, 0, -1], [-1, -1, -1]], np.int64), rows)
    assert got.dtype == np.int64 and got.tolist() == [[35, 10, -1], [-1, -1, -1]]
    got = to_global(np.array([[0, -1]], np.int64), np.zeros(0, np.int64))
    assert got.dtype == np.int64 and got.tolist() == [[-1, -1]]
    ids, scores = empty_lists(3, 4)
    assert ids.shape == scores.shape == (3, 4) and (ids == -1).all() and not scores.any()
    assert (ids.dtype, scores.dtype) == (np.int64, np.float32)
