"""The kernels in FRONT of the scan — bm25_encode_kernel, hash_tokenize_kernel (csrc/text.h), add_layernorm_f16_kernel<NC>,
embed_layernorm_f16_kernel<NC> (csrc/encoder_ops.h) — at the byte-class, length, capacity, packing and value edges the tests
that arrived with them never reach.  The cases and references are in tests/text_front_refs.py; tests/test_text_front_refs_host.py
shows on the CPU that the cases have the properties they are named after.

A  BM25 payloads, bit for bit against BM25SparseEncoder.encode_document, straight through the entry point (idx, val, nnz, flags on
   sentinel-filled buffers with a guard row on either side) and through encode_documents_csr(device=...).
B  The hash tokenizer, identical to HashTokenizer on the host, through .batch(device=...) and through the entry point.
C  The LayerNorm pair against fp64 LayerNorm of the fp16-rounded sum, with the unfused fp16 path on the same GPU as the
   yardstick (encoder_refs.yardstick_ok: max E_k <= 2 max E_u + u, mean E_k <= 2 mean E_u); constant rows, poisoned rows,
   aliasing and clamped ids bitwise.  Every output buffer is NaN-filled with 16 guard rows behind the last row.
D  The 65 536-slot histogram (128 KiB of dynamic LDS) on a second device first, in a fresh process.

Every buffer a kernel writes is prefilled: -7 for integers, NaN for floats."""
import os
import subprocess
import sys

import numpy as np
import pytest

import encoder_refs as R
import text_front_refs as F

torch = pytest.importorskip("torch")
from advanced_rag.encoders import HashTokenizer  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
S = F.INT_SENTINEL
NAN32 = torch.full((1,), NAN, dtype=torch.float32).numpy().view(np.uint32)[0]
NAN16 = torch.full((1,), NAN, dtype=torch.float16).numpy().view(np.uint16)[0]
GUARD_ROWS = 16


def _stream(dev="cuda:0"):
    return torch.cuda.current_stream(torch.device(dev)).cuda_stream


# =========================================================================================================== A. BM25
def _bm25_direct(enc, docs, cap, dev="cuda:0"):
    """hr_bm25_encode_dev on sentinel-filled buffers of n + 2 rows (row 0 and row n + 1 are guards) -> the four host arrays,
    guards included (val as its uint32 bits)"""
    from advanced_rag import _native as nat
    text, off = F.pack(docs)
    n = len(docs)
    with torch.cuda.device(torch.device(dev)):
        d_text = torch.frombuffer(bytearray(text or b"\0"), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(off).to(dev)
        idx = torch.full((n + 2, cap), S, dtype=torch.int32, device=dev)
        val = torch.full((n + 2, cap), NAN, dtype=torch.float32, device=dev)
        nnz = torch.full((n + 2,), S, dtype=torch.int32, device=dev)
        flags = torch.full((n + 2,), S, dtype=torch.int32, device=dev)
        nat.bm25_encode_dev(d_text.data_ptr(), d_off.data_ptr(), n, enc.sparse_dim, enc.k1, enc.b, enc.avgdl, cap,
                            idx[1:].data_ptr(), val[1:].data_ptr(), nnz[1:].data_ptr(), flags[1:].data_ptr(), _stream(dev))
        torch.cuda.synchronize()
        return idx.cpu().numpy(), val.cpu().numpy().view(np.uint32), nnz.cpu().numpy(), flags.cpu().numpy()


def _hold_bm25(enc, docs, cap, dev="cuda:0", label=""):
    """Every document of the batch against the host encoder: flag, nnz, indices, weight bits; the cells behind nnz, the rows
    of handed-back documents and both guard rows keep the sentinel.  -> (idx, val bits, nnz, flags) of the real rows"""
    idx, val, nnz, flags = _bm25_direct(enc, docs, cap, dev)
    for g in (0, len(docs) + 1):
        assert np.all(idx[g] == S) and np.all(val[g] == NAN32) and nnz[g] == S and flags[g] == S, (label, "guard row", g)
    idx, val, nnz, flags = idx[1:-1], val[1:-1], nnz[1:-1], flags[1:-1]
    for i, doc in enumerate(docs):
        raw = F.as_bytes(doc)
        ascii_doc = all(c < 0x80 for c in raw)
        w_idx, w_val = F.bm25_want(enc, doc) if ascii_doc else (np.zeros(0, np.int32), np.zeros(0, np.uint32))
        flag = F.bm25_flag(doc, len(w_idx), cap)
        where = (label, i, raw[:24])
        assert flags[i] == flag, where + (int(flags[i]), flag)
        if flag:
            assert nnz[i] == 0 and np.all(idx[i] == S) and np.all(val[i] == NAN32), where
            continue
        k = len(w_idx)
        assert nnz[i] == k, where + (int(nnz[i]), k)
        assert np.array_equal(idx[i, :k], w_idx), where
        assert np.array_equal(val[i, :k], w_val), where
        assert np.all(idx[i, k:] == S) and np.all(val[i, k:] == NAN32), where
    return idx, val, nnz, flags


def _hold_wrapper(enc, texts, label=""):
    ptr, idx, val = enc.encode_documents_csr(texts, device="cuda:0")
    assert ptr.shape == (len(texts) + 1,) and ptr[0] == 0 and ptr[-1] == idx.shape[0] == val.shape[0], label
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == np.float32, label
    for i, t in enumerate(texts):
        want = enc.encode_document(t)
        assert idx[ptr[i]:ptr[i + 1]].tolist() == want["indices"], (label, i, t[:24])
        assert np.array_equal(val[ptr[i]:ptr[i + 1]].view(np.uint32), np.asarray(want["values"], np.float32).view(np.uint32)), (label, i)


@pytest.mark.parametrize("dim", [1000, 65536, 37])
def test_bm25_byte_classes(gpu, dim):
    """A1: every byte below 0x80 between, before, after and without letters — one batch of 512 documents"""
    docs = F.byte_class_docs()
    enc = F.bm25_encoder(dim)
    _, _, nnz, _ = _hold_bm25(enc, docs, 2, label=f"byte classes, dim {dim}")
    assert set(nnz.tolist()) == {0, 1, 2}
    _hold_wrapper(enc, docs, f"byte classes, dim {dim}")


@pytest.mark.parametrize("dim", F.LENGTH_EDGE_DIMS)
def test_bm25_length_edge(gpu, dim):
    """A2: 65 535 bytes (32 768 tokens in one slot; one token; two words in the two halves of one histogram word) are encoded,
    65 536 bytes are handed back untouched — and come out of the wrapper equal to the host's row"""
    docs = F.length_edge_docs(dim)
    enc = F.bm25_encoder(dim)
    _, _, nnz, flags = _hold_bm25(enc, docs, 4, label=f"length edge, dim {dim}")
    assert flags.tolist() == [0, 0, 2, 0] and nnz.tolist() == [1, 1, 0, 3]
    _hold_wrapper(enc, docs, f"length edge, dim {dim}")


@pytest.mark.parametrize("dim", F.VOCAB_DIMS)
def test_bm25_vocabulary_shapes(gpu, dim):
    """A3: the slots 0, 1, dim - 2, dim - 1 and, up to 513, a document on every slot (nnz = dim = cap at 513)"""
    docs = F.vocab_docs(dim)
    enc = F.bm25_encoder(dim)
    _, _, nnz, flags = _hold_bm25(enc, docs, F.vocab_cap(dim), label=f"vocabulary {dim}")
    assert not flags.any() and nnz[0] == len(F.corner_slots(dim)) and (len(docs) == 1 or nnz[1] == dim)
    _hold_wrapper(enc, docs, f"vocabulary {dim}")


@pytest.mark.parametrize("cap", F.CAPS)
def test_bm25_cap_edge(gpu, cap):
    """A4: exactly cap slots fill the row to its last cell; cap + 1 are handed back and the row keeps the sentinel"""
    enc = F.bm25_encoder(F.CAP_DIM)
    _, _, nnz, flags = _hold_bm25(enc, F.cap_docs(cap), cap, label=f"cap {cap}")
    assert flags.tolist() == [0, 2, 0] and nnz.tolist() == [cap, 0, cap]


@pytest.mark.parametrize("batch", range(len(F.SEAM_BATCHES)))
def test_bm25_document_seams(gpu, batch):
    """A5: documents packed with no separator — no token joins across a seam, empty documents at either end"""
    docs = F.SEAM_BATCHES[batch]
    for dim in (1000, 2):
        enc = F.bm25_encoder(dim)
        _hold_bm25(enc, docs, 4, label=f"seams {batch}")
        _hold_wrapper(enc, docs, f"seams {batch}")


def test_bm25_flagged_documents_leave_their_neighbours_alone(gpu):
    """A6: a document of the single byte 0x80, one of 0xFF and one with a UTF-8 pair between ASCII documents: flag 1, nnz 0, and
    the other rows equal those of the batch in which the flagged documents are empty"""
    enc = F.bm25_encoder(1000)
    got = _hold_bm25(enc, list(F.FLAG_DOCS), 8, label="flags in company")
    blank = _hold_bm25(enc, F.flag_docs_blanked(), 8, label="flags blanked")
    assert got[3].tolist() == [0, 1, 0, 1, 0, 1, 0] and not blank[3].any()
    for i in (0, 2, 4, 6):
        assert all(np.array_equal(a[i], b[i]) for a, b in zip(got[:3], blank[:3])), i


def test_bm25_parameters(gpu):
    """A7: k1 = 0, b = 0, b = 1 and avgdl of 1 / 1000 and 5 000: the weights stay bit-exact"""
    for k1, b in F.PARAMS:
        _hold_bm25(F.bm25_encoder(1000, k1, b), list(F.PARAM_DOCS), 16, label=f"k1 {k1} b {b}")
    for enc in F.avgdl_encoders(1000):
        _hold_bm25(enc, list(F.PARAM_DOCS), 16, label=f"avgdl {enc.avgdl}")
        _hold_wrapper(enc, list(F.PARAM_DOCS), f"avgdl {enc.avgdl}")


def test_bm25_wrapper_batches(gpu):
    """A8: every document flagged; only empty strings; 65 537 slots (the host route); mixed batches keep their order"""
    enc = F.bm25_encoder(1000)
    _hold_wrapper(enc, ["café", "naïve déjà vu", "ü"], "all flagged")
    ptr, idx, val = enc.encode_documents_csr(["", "", ""], device="cuda:0")
    assert ptr.tolist() == [0, 0, 0, 0] and idx.shape == (0,) and val.shape == (0,)
    mixed = ["first doc", "déjà vu", "", "third third", "a " * 32768, "ß", "last_one 9", "x" * 70000, "tail"]
    _hold_wrapper(enc, mixed, "mixed")
    _hold_wrapper(enc, mixed[::-1], "mixed, reversed")
    _hold_wrapper(F.bm25_encoder(65537), mixed + F.vocab_docs(65536), "host route")


# ====================================================================================================== B. tokenizer
def _tok_direct(vocab, max_len, docs):
    """hr_hash_tokenize_dev on a sentinel-filled [n + 2][max_len] buffer -> ids, lens, flags on the host, guards included"""
    from advanced_rag import _native as nat
    text, off = F.pack(docs)
    n = len(docs)
    d_text = torch.frombuffer(bytearray(text or b"\0"), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(off).cuda()
    ids = torch.full((n + 2, max_len), S, dtype=torch.int64, device="cuda")
    lens = torch.full((n + 2,), S, dtype=torch.int32, device="cuda")
    flags = torch.full((n + 2,), S, dtype=torch.int32, device="cuda")
    nat.hash_tokenize_dev(d_text.data_ptr(), d_off.data_ptr(), n, max_len, vocab, ids[1:].data_ptr(), lens[1:].data_ptr(),
                          flags[1:].data_ptr(), _stream())
    torch.cuda.synchronize()
    return ids.cpu().numpy(), lens.cpu().numpy(), flags.cpu().numpy()


def _hold_tok(vocab, max_len, docs, label=""):
    """The entry point against HashTokenizer.encode: CLS ids SEP then zeros to the end of the row, lens, flags; a text with a
    byte >= 0x80 has flag 1 and lens 0; the guard rows keep the sentinel.  -> the real rows"""
    ids, lens, flags = _tok_direct(vocab, max_len, docs)
    for g in (0, len(docs) + 1):
        assert np.all(ids[g] == S) and lens[g] == S and flags[g] == S, (label, "guard row", g)
    ids, lens, flags = ids[1:-1], lens[1:-1], flags[1:-1]
    plain = [i for i, d in enumerate(docs) if all(c < 0x80 for c in F.as_bytes(d))]
    want, want_lens = F.tok_rows(HashTokenizer(vocab, max_len), [F.as_bytes(docs[i]).decode("ascii") for i in plain])
    for k, i in enumerate(plain):
        where = (label, vocab, max_len, i, F.as_bytes(docs[i])[:24])
        assert flags[i] == 0 and lens[i] == want_lens[k], where + (int(lens[i]), int(want_lens[k]))
        assert np.array_equal(ids[i], want[k]), where
    for i in set(range(len(docs))) - set(plain):
        assert flags[i] == 1 and lens[i] == 0, (label, i)
    return ids, lens, flags


def _hold_batch(vocab, max_len, texts, label=""):
    got = HashTokenizer(vocab, max_len).batch(texts, device="cuda:0")
    want = HashTokenizer(vocab, max_len).batch(texts, device="cpu")
    assert got[0].is_cuda
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g.cpu(), w), (label, vocab, max_len)


def test_tokenizer_byte_classes(gpu):
    """B1: a byte that is neither word nor space is a token of its own; tab .. carriage return, the blank and 0x1c .. 0x1f are not"""
    docs = F.byte_class_docs()
    ids, lens, _ = _hold_tok(30522, 16, docs, "byte classes")
    for c in F.SPACE_BYTES:
        assert lens[4 * c: 4 * c + 4].tolist() == [4, 2, 3, 3], c
    _hold_batch(30522, 16, docs, "byte classes")


@pytest.mark.parametrize("max_len", [512, 16])
def test_tokenizer_every_byte_a_token(gpu, max_len):
    """B2: '!' * n and 'a!' * n — every thread's count is its slice's length, the prefix sum carries across all four waves"""
    docs = ["!" * n for n in F.EVERY_BYTE_NS] + ["a!" * n for n in F.EVERY_BYTE_NS]
    _, lens, _ = _hold_tok(30522, max_len, docs, "every byte a token")
    assert lens.tolist() == [min(n, max_len - 2) + 2 for n in F.EVERY_BYTE_NS] + [min(2 * n, max_len - 2) + 2 for n in F.EVERY_BYTE_NS]
    _hold_batch(30522, max_len, docs, "every byte a token")


@pytest.mark.parametrize("max_len", [512, 16, 100])
def test_tokenizer_slice_edges(gpu, max_len):
    """B3: tokens that start on the first byte of a thread's slice, end on its last byte or run across slices"""
    docs = [F.slice_edge_text(n) for n in F.SLICE_LENGTHS]
    _hold_tok(30522, max_len, docs, "slice edges")
    _hold_batch(30522, max_len, docs, "slice edges")
    text, cut = F.long_word_text()
    _hold_tok(30522, cut, [text, "x", text], "long word kept last")
    _hold_batch(30522, cut, [text], "long word kept last")


@pytest.mark.parametrize("max_len", F.TRUNC_MAX_LENS)
def test_tokenizer_truncation(gpu, max_len):
    """B4: room - 1, room and room + 1 tokens; SEP sits at 1 + min(tokens, room), zeros behind it in a sentinel-filled row"""
    docs = F.truncation_texts(max_len)
    ids, lens, _ = _hold_tok(30522, max_len, docs, "truncation")
    room = max_len - 2
    for r, n_tok in zip(ids, (room - 1, room, room + 1)):
        assert r[0] == 101 and r[1 + min(n_tok, room)] == 102 and np.all(r[2 + min(n_tok, room):] == 0)
    assert lens.tolist() == [max_len - 1, max_len, max_len]
    _hold_batch(30522, max_len, docs, "truncation")


@pytest.mark.parametrize("vocab", F.VOCABS)
def test_tokenizer_vocabularies(gpu, vocab):
    """B5: 1001 (every id is 1000), 1002, 30 522"""
    docs = list(F.SEAM_BATCHES[0]) + [F.token_run(40), F.slice_edge_text(513)] + F.byte_class_docs()[128:256]
    ids, _, _ = _hold_tok(vocab, 64, docs, "vocabulary")
    if vocab == 1001:
        assert set(np.unique(ids).tolist()) == {0, 101, 102, 1000}
    _hold_batch(vocab, 64, docs, "vocabulary")


def test_tokenizer_seams_and_flags(gpu):
    """B6: no token joins across a seam; a non-ASCII text gets flag 1 and lens 0 and leaves its neighbours' rows as they are
    without it; .batch then takes the host path"""
    for batch in F.SEAM_BATCHES:
        _hold_tok(30522, 16, batch, "seams")
        _hold_batch(30522, 16, batch, "seams")
    company = ["abc def", b"\x80", "ghi!", b"caf\xc3\xa9 au lait", "end", b"\xff", "Z_9 ?"]
    got = _hold_tok(30522, 16, company, "flags in company")
    alone = _hold_tok(30522, 16, [d for d in company if isinstance(d, str)], "flags left out")
    assert got[2].tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert np.array_equal(got[0][::2], alone[0]) and np.array_equal(got[1][::2], alone[1])
    tok = HashTokenizer(30522, 16)
    texts = ["plain", "ünïcode", "x y"]
    assert tok._batch_on_device(texts, torch.device("cuda:0")) is None
    got, want = tok.batch(texts, device="cuda:0"), tok.batch(texts, device="cpu")
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


# ====================================================================================================== C. LayerNorm
def _dev_rows(a):
    """a [rows][hidden] fp16 on the host -> a device buffer of rows + 16 rows, NaN behind the real ones"""
    buf = torch.full((a.shape[0] + GUARD_ROWS, a.shape[1]), NAN, dtype=torch.float16, device="cuda")
    buf[: a.shape[0]] = torch.from_numpy(a).cuda()
    return buf


def _guards_kept(out, rows, label):
    tail = out[rows:].cpu().numpy().view(np.uint16)
    assert tail.shape[0] == GUARD_ROWS and np.all(tail == NAN16), (label, "rows behind the last row were written")


def _add_ln(x, res, gamma, beta, eps, alias=None):
    """hr_add_layernorm_f16_dev -> fp16 [rows][hidden] on the host.  out is a NaN-filled buffer with 16 guard rows, or (alias =
    'x' / 'res') the input buffer itself, whose 16 trailing rows are NaN as well."""
    from advanced_rag import _native as nat
    rows, hidden = x.shape
    dx = _dev_rows(x)
    dres = _dev_rows(res) if res is not None else None
    g, b = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    out = dx if alias == "x" else dres if alias == "res" else torch.full((rows + GUARD_ROWS, hidden), NAN, dtype=torch.float16, device="cuda")
    nat.add_layernorm_f16_dev(dx.data_ptr(), dres.data_ptr() if dres is not None else 0, g.data_ptr(), b.data_ptr(), out.data_ptr(),
                              rows, hidden, eps, _stream())
    torch.cuda.synchronize()
    _guards_kept(out, rows, ("add_layernorm", rows, hidden, alias))
    return out[:rows].cpu().numpy()


def _add_ln_unfused(x, res, gamma, beta, eps):
    """the ops the kernel replaces, as the unfused fp16 module runs them on the same GPU: fp16 add, F.layer_norm on halves"""
    h = torch.from_numpy(x).cuda()
    if res is not None:
        h = h + torch.from_numpy(res).cuda()
    return torch.nn.functional.layer_norm(h, (x.shape[1],), torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda(), eps).cpu().numpy()


def _yardstick(label, got, plain, want):
    assert np.isfinite(got).all() and np.isfinite(want).all(), label
    e_k, e_u = np.abs(got.astype(np.float64) - want), np.abs(plain.astype(np.float64) - want)
    ok, (mk, mu, ak, au), u = R.yardstick_ok(e_k, e_u, float(np.abs(want).max()))
    print(f"layernorm {label}: max E_k {mk:.3e}  max E_u {mu:.3e}  mean E_k {ak:.3e}  mean E_u {au:.3e}  u {u:.2e}")
    assert ok, (label, mk, mu, ak, au, u)


def _hold_add_ln(label, x, res, eps):
    gamma, beta = F.ln_params(x.shape[1])
    want = F.ln_ref(F.fp16_add(x, res) if res is not None else x, gamma, beta, eps)
    _yardstick(label, _add_ln(x, res, gamma, beta, eps), _add_ln_unfused(x, res, gamma, beta, eps), want)


@pytest.mark.parametrize("with_residual", [True, False])
@pytest.mark.parametrize("regime", F.LN_REGIMES)
def test_add_layernorm_value_regimes(gpu, regime, with_residual):
    """C1: unit, offset rows, outlier dimensions, small variance — and rows a few fp16 ulps around 8 and 30, where a one-pass
    variance has no digit left — with and without the residual, 37 rows of 384"""
    x, res = F.ln_inputs(regime)
    _hold_add_ln(f"{regime}{' + residual' if with_residual else ''}", x, res if with_residual else None, 1e-12)


@pytest.mark.parametrize("eps", F.EPS_VALUES)
def test_add_layernorm_honours_eps(gpu, eps):
    """C2: the small-variance regime at eps 1e-12, 1e-5 and 1 (the three references lie more than 10 u apart); the embedding
    kernel on tables scaled down to the same variance"""
    x, res = F.ln_inputs("small_variance")
    _hold_add_ln(f"small_variance eps {eps:g}", x, res, eps)
    small = [(2e-3 * t.astype(np.float64)).astype(np.float16) for t in F.embed_tables(F.LN_HIDDEN)]   # variance ~ 3e-6
    _hold_embed_ln(f"embedding small tables eps {eps:g}", *F.embed_ids(5, 7), *small, eps)


@pytest.mark.parametrize("chunks", F.DISPATCH_CHUNKS)
def test_add_layernorm_dispatch_and_row_edges(gpu, chunks):
    """C3: both sides of every NC dispatch edge (16 | 17, 32 | 33, 48 | 49, 64 | 65 chunks) and of the 16 rows of a block"""
    for rows in F.ROW_EDGES:
        x, res = F.unit_inputs(rows, 8 * chunks)
        _hold_add_ln(f"hidden {8 * chunks} rows {rows}", x, res, 1e-12)
        ids, types = F.embed_ids(rows, 1)
        _hold_embed_ln(f"embedding hidden {8 * chunks} rows {rows}", ids, types, *F.embed_tables(8 * chunks), 1e-12)


@pytest.mark.parametrize("hidden", F.CONSTANT_WIDTHS)
def test_constant_rows_return_beta_bit_for_bit(gpu, hidden):
    """C4: rows of one fp16 constant (0, 2, -0.5, 0.1, 3.3, 30, -30).  The kernels' fp32 mean of such a row is the constant
    itself (text_front_refs.emulated_mean: lane sums, the 16-lane sum and the product with the rounded 1 / n are all exact), so
    x - mean = 0 and the output is beta, whatever gamma and eps are."""
    x = F.constant_rows(hidden)
    gamma, beta = F.ln_params(hidden)
    want = np.broadcast_to(beta.view(np.uint16), x.shape)
    for res in (None, np.zeros_like(x)):
        got = _add_ln(x, res, gamma, beta, 1e-12)
        assert np.array_equal(got.view(np.uint16), want), (hidden, res is None, np.abs(got.astype(np.float64) - beta).max())
    # the embedding kernel: a constant word row, zero position and segment rows
    ids = (np.arange(x.shape[0], dtype=np.int64) % len(F.CONSTANTS))[None, :]
    word = F.constant_rows(hidden, len(F.CONSTANTS))
    zeros = np.zeros((x.shape[0], hidden), dtype=np.float16)
    got = _embed_ln(ids, np.zeros_like(ids), word, zeros, zeros[:1], gamma, beta, 1e-12)
    assert np.array_equal(got.view(np.uint16), want), hidden


def _hold_no_bleed(clean, got, bad_rows, label):
    bad = np.zeros(clean.shape[0], dtype=bool)
    bad[list(bad_rows)] = True
    assert not np.isfinite(got[bad]).any(), (label, "poisoned rows must come out non-finite")
    assert np.isfinite(clean).all() and np.array_equal(got[~bad].view(np.uint16), clean[~bad].view(np.uint16)), (label, "a neighbour changed")


def test_rows_do_not_bleed(gpu):
    """C5: a NaN row and a row that overflows fp16 in x + res (60 000 + 60 000) come out non-finite; every other row keeps its
    bits — in both kernels.  The 16 rows behind the last row keep the sentinel at 1, 15, 17 and 33 rows (checked on every
    launch of this file)."""
    gamma, beta = F.ln_params(F.LN_HIDDEN)
    for regime in ("unit", "offset_rows"):
        x, res = F.ln_inputs(regime)
        px, pres = F.poisoned(x, res)
        _hold_no_bleed(_add_ln(x, res, gamma, beta, 1e-12), _add_ln(px, pres, gamma, beta, 1e-12), (F.NAN_ROW, F.OVERFLOW_ROW), regime)
    for rows in (1, 15, 17, 33):
        x, res = F.ln_inputs("unit", rows)
        assert np.isfinite(_add_ln(x, res, gamma, beta, 1e-12)).all()
        ids, types = F.embed_ids(rows, 1)
        assert np.isfinite(_embed_ln(ids, types, *F.embed_tables(F.LN_HIDDEN), gamma, beta, 1e-12)).all()
    # the embedding kernel: word row 7 is NaN; word row 9 and segment row 2 hold 60 000
    word, pos, seg = F.embed_tables(F.LN_HIDDEN, n_seg=3)
    word[7], word[9], seg[2] = np.nan, F.OVERFLOW_VALUE, F.OVERFLOW_VALUE
    ids, types = F.embed_ids(5, 7)
    ids[ids == 7], ids[ids == 9] = 8, 10
    clean = _embed_ln(ids, types, word, pos, seg, gamma, beta, 1e-12)
    p_ids, p_types = ids.copy(), types.copy()
    p_ids.reshape(-1)[F.NAN_ROW], p_ids.reshape(-1)[F.OVERFLOW_ROW], p_types.reshape(-1)[F.OVERFLOW_ROW] = 7, 9, 2
    _hold_no_bleed(clean, _embed_ln(p_ids, p_types, word, pos, seg, gamma, beta, 1e-12), (F.NAN_ROW, F.OVERFLOW_ROW), "embedding")


@pytest.mark.parametrize("rows,hidden", [(37, 384), (17, 1024), (1, 8), (33, 136)])
def test_add_layernorm_output_may_alias_either_input(gpu, rows, hidden):
    """C6: out == res and out == x give the bits of the out-of-place call"""
    x, res = F.unit_inputs(rows, hidden)
    gamma, beta = F.ln_params(hidden)
    want = _add_ln(x, res, gamma, beta, 1e-12).view(np.uint16)
    assert np.array_equal(_add_ln(x, res, gamma, beta, 1e-12, alias="res").view(np.uint16), want)
    assert np.array_equal(_add_ln(x, res, gamma, beta, 1e-12, alias="x").view(np.uint16), want)
    assert np.array_equal(_add_ln(x, None, gamma, beta, 1e-12, alias="x").view(np.uint16), _add_ln(x, None, gamma, beta, 1e-12).view(np.uint16))


# ------------------------------------------------------------------------------------------------------- embedding
def _embed_ln(ids, types, word, pos, seg, gamma, beta, eps):
    """hr_embed_layernorm_f16_dev -> fp16 [n_seq * T][hidden] on the host (NaN-filled output, 16 guard rows)"""
    from advanced_rag import _native as nat
    n_seq, T = ids.shape
    hidden = word.shape[1]
    rows = n_seq * T
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ids, types, word, pos, seg, gamma, beta)]
    out = torch.full((rows + GUARD_ROWS, hidden), NAN, dtype=torch.float16, device="cuda")
    nat.embed_layernorm_f16_dev(*(t.data_ptr() for t in dev), out.data_ptr(), n_seq, T, hidden, eps, word.shape[0], seg.shape[0], _stream())
    torch.cuda.synchronize()
    _guards_kept(out, rows, ("embed_layernorm", n_seq, T, hidden))
    return out[:rows].cpu().numpy()


def _embed_unfused(ids, types, word, pos, seg, gamma, beta, eps):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    h = (d(word)[d(ids)] + d(pos)[: ids.shape[1]][None]) + d(seg)[d(types)]                # fp16, rounded after each add
    return torch.nn.functional.layer_norm(h, (word.shape[1],), d(gamma), d(beta), eps).reshape(-1, word.shape[1]).cpu().numpy()


def _hold_embed_ln(label, ids, types, word, pos, seg, eps):
    gamma, beta = F.ln_params(word.shape[1])
    want = F.ln_ref(F.embed_chain(word, pos, seg, ids, types), gamma, beta, eps).reshape(-1, word.shape[1])
    got = _embed_ln(ids, types, word, pos, seg, gamma, beta, eps)
    _yardstick(label, got, _embed_unfused(ids, types, word, pos, seg, gamma, beta, eps), want)
    return got, want


@pytest.mark.parametrize("n_seq,T", F.EMBED_SHAPES)
def test_embed_layernorm_shapes_and_clamping(gpu, n_seq, T):
    """C7: T = 1, 7, 17 and 512 with row counts off the 16-row grid (at T = 512 every count is a multiple of 16), distinct
    position rows, ids 0 and n_word - 1; ids -5 and n_word + 9 and types -3 and 7 equal the clamped call bit for bit; one
    segment row"""
    gamma, beta = F.ln_params(F.LN_HIDDEN)
    ids, types = F.embed_ids(n_seq, T)
    tables = F.embed_tables(F.LN_HIDDEN)
    got, _ = _hold_embed_ln(f"embedding n_seq {n_seq} T {T}", ids, types, *tables, 1e-12)
    wild_i, wild_t = ids.copy(), types.copy()
    wild_i.reshape(-1)[[1, 2]] = [-5, F.N_WORD + 9]
    wild_t.reshape(-1)[[1, 3]] = [-3, 7]
    clamped = _embed_ln(wild_i.clip(0, F.N_WORD - 1), wild_t.clip(0, 1), *tables, gamma, beta, 1e-12)
    assert np.array_equal(_embed_ln(wild_i, wild_t, *tables, gamma, beta, 1e-12).view(np.uint16), clamped.view(np.uint16))
    assert not np.array_equal(clamped[1:4].view(np.uint16), got[1:4].view(np.uint16))      # the planted ids do change the rows
    one = F.embed_tables(F.LN_HIDDEN, n_seg=1)
    got_one, _ = _hold_embed_ln(f"embedding n_seq {n_seq} T {T}, one segment", ids, np.zeros_like(types), *one, 1e-12)
    assert np.array_equal(_embed_ln(ids, wild_t, *one, gamma, beta, 1e-12).view(np.uint16), got_one.view(np.uint16))


@pytest.mark.parametrize("regime", ["order", "order_planted"])
def test_embed_layernorm_adds_in_the_order_of_the_unfused_module(gpu, regime):
    """C7: fp16(fp16(word + pos) + seg), not word + (pos + seg).  `order` (word N(0, 8), pos and seg N(0, 0.01)): the two orders
    differ in more than a tenth of the elements; the kernel is held to the chain's reference by the yardstick and the share of
    elements nearer to the other order's reference is printed.  `order_planted`: the chain returns the word rows exactly and
    the other order moves a third of the elements by 2, a tenth of an output unit — far outside the yardstick."""
    ids, types = F.embed_ids(5, 7)
    word, pos, seg = F.embed_tables(F.LN_HIDDEN, regime=regime)
    gamma, beta = F.ln_params(F.LN_HIDDEN)
    got, want = _hold_embed_ln(f"embedding {regime}", ids, types, word, pos, seg, 1e-12)
    other = F.ln_ref(F.embed_other_order(word, pos, seg, ids, types), gamma, beta, 1e-12).reshape(want.shape)
    g = got.astype(np.float64)
    nearer = np.abs(g - other) < np.abs(g - want)
    apart = (F.embed_chain(word, pos, seg, ids, types) != F.embed_other_order(word, pos, seg, ids, types)).reshape(want.shape)
    print(f"embedding {regime}: {float(nearer.mean()):.4f} of all elements and {float(nearer[apart].mean()):.4f} of the {int(apart.sum())} "
          f"whose sums differ are nearer to the reference of word + (pos + seg)")


# =================================================================================================== D. second device
def _second_device_child():
    """runs in a fresh process: the 65 536-slot cases on cuda:1 BEFORE cuda:0 has launched the kernel, then on cuda:0"""
    enc = F.bm25_encoder(65536)
    docs = F.vocab_docs(65536) + F.length_edge_docs(65536)
    for dev in ("cuda:1", "cuda:0"):
        _, _, nnz, flags = _hold_bm25(enc, docs, 4, dev=dev, label=f"65 536 slots on {dev}")
        assert flags.tolist() == [0, 0, 0, 2, 0] and nnz.tolist() == [4, 1, 1, 0, 3], dev
        print(f"bm25 at 65 536 slots on {dev}: ok")


def test_bm25_widest_histogram_on_a_second_device_first(gpu):
    """D: hr_bm25_encode_dev raises the kernel's dynamic-LDS limit once per process; a launch with more than 64 KiB of LDS on a
    device other than the one that was current then must still run"""
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = {[here] + [p for p in sys.path if p]!r}; "
            "import test_gpu_text_front_edges as m; m._second_device_child()")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "on cuda:1: ok" in run.stdout and "on cuda:0: ok" in run.stdout
