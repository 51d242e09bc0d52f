"""CPU checks of tests/text_front_refs.py: every builder produces what tests/test_gpu_text_front_edges.py relies on (slots hit,
token counts, slice edges, truncation edges, the share of elements that pins the order of the embedding adds, the
separation of the eps references), and the reference of every document the GPU tests expect to come back encoded holds
no more than `cap` entries."""
import numpy as np
import pytest

import encoder_refs as R
import text_front_refs as F

torch = pytest.importorskip("torch")
from advanced_rag.encoders import HashTokenizer  # noqa: E402


# ----------------------------------------------------------------------------------------------------------- BM25
def test_fit_corpus_gives_an_average_length_that_is_no_round_number():
    enc = F.bm25_encoder(1000)
    assert enc.n_docs == 7 and enc.total_len == 22 and enc.avgdl == 22 / 7


def test_byte_class_batch_has_zero_one_and_two_token_documents_and_every_class_edge():
    docs = F.byte_class_docs()
    assert len(docs) == 512
    for c in range(128):
        word = c in F.WORD_BYTES
        a_c_b, alone, c_a, a_c = (len(F.bm25_tokens(d)) for d in docs[4 * c: 4 * c + 4])
        assert (a_c_b, alone, c_a, a_c) == ((1, 1, 1, 1) if word else (2, 0, 1, 1)), c
        # the tokenizer: a byte that is neither word nor space is a token of its own
        own = 0 if word or c in F.SPACE_BYTES else 1
        assert [len(F.tok_tokens(d)) for d in docs[4 * c: 4 * c + 4]] == ([1, 1, 1, 1] if word else [2 + own, own, 1 + own, 1 + own]), c
    counts = {len(F.bm25_tokens(d)) for d in docs}
    assert counts == {0, 1, 2}
    assert [c in F.WORD_BYTES for c in F.CLASS_EDGE_BYTES] == [False, True, True, False, False, True, True, False, True, False,
                                                                 True, True, False]
    assert all(chr(c) in docs for c in F.CLASS_EDGE_BYTES)
    assert {0x1c, 0x1d, 0x1e, 0x1f} <= F.SPACE_BYTES and all(F.tok_tokens(chr(c)) == [] for c in F.SPACE_BYTES)


@pytest.mark.parametrize("dim", F.LENGTH_EDGE_DIMS)
def test_length_edge_documents(dim):
    most, one, over, alt = F.length_edge_docs(dim)
    assert [len(d) for d in (most, one, over, alt)] == [65535, 65535, 65536, 65535]
    assert len(F.bm25_tokens(most)) == 32768 and set(F.bm25_tokens(most)) == {"a"}
    assert F.bm25_tokens(one) == ["x" * 65535]
    j, (lo, hi, nxt) = F.adjacent_triple(dim)
    assert (F.slot_of(lo, dim), F.slot_of(hi, dim), F.slot_of(nxt, dim)) == (2 * j, 2 * j + 1, 2 * j + 2)
    toks = F.bm25_tokens(alt)
    assert toks.count(lo) == toks.count(hi) > 4000 and toks.count(nxt) == 1 and set(toks) == {lo, hi, nxt}
    enc = F.bm25_encoder(dim)
    idx, _ = F.bm25_want(enc, alt)
    assert idx.tolist() == [2 * j, 2 * j + 1, 2 * j + 2]
    assert F.bm25_flag(over, 1, 8) == 2 and F.bm25_flag(most, 1, 8) == 0


@pytest.mark.parametrize("dim", F.VOCAB_DIMS)
def test_vocabulary_documents_hit_their_slots(dim):
    slots = F.corner_slots(dim)
    assert slots == sorted({0, 1, dim - 2, dim - 1} & set(range(dim)))
    words = F.words_for_slots(dim, slots)
    assert [F.slot_of(w, dim) for w in words] == slots
    assert F.candidates_searched(dim, slots) < (130000 if dim == 65536 else 200000)
    if dim == 2:
        assert words == ["w0", "w4"]
    enc = F.bm25_encoder(dim)
    docs = F.vocab_docs(dim)
    idx, _ = F.bm25_want(enc, docs[0])
    assert idx.tolist() == slots
    assert len(docs) == (2 if dim <= F.EVERY_SLOT_MAX_DIM else 1)
    if len(docs) == 2:
        idx, val = F.bm25_want(enc, docs[1])
        assert idx.tolist() == list(range(dim))
        assert dim < 3 or len(set(val.tolist())) == 3                  # three term frequencies
    assert all(len(F.bm25_want(enc, d)[0]) <= F.vocab_cap(dim) for d in docs)


@pytest.mark.parametrize("cap", F.CAPS)
def test_cap_edge_documents(cap):
    enc = F.bm25_encoder(F.CAP_DIM)
    nnz = [len(F.bm25_want(enc, d)[0]) for d in F.cap_docs(cap)]
    assert nnz == [cap, cap + 1, cap]
    assert [F.bm25_flag(d, n, cap) for d, n in zip(F.cap_docs(cap), nnz)] == [0, 2, 0]


def test_seam_batches_would_merge_if_a_token_ran_across_a_seam():
    first = F.SEAM_BATCHES[0]
    assert first == ["abc", "def", "", "9", "_x", "", "End"]
    assert F.bm25_tokens("".join(first)) == ["abcdef9_xend"] and sum(len(F.bm25_tokens(d)) for d in first) == 5
    assert F.SEAM_BATCHES[1][0] == "" and F.SEAM_BATCHES[1][-1] == "" and len(F.SEAM_BATCHES[2]) == 1
    for batch in F.SEAM_BATCHES:
        text, off = F.pack(batch)
        assert off[0] == 0 and off[-1] == len(text) and np.all(np.diff(off) == [len(d) for d in batch])
        assert len(F.tok_tokens("".join(batch))) < sum(len(F.tok_tokens(d)) for d in batch) or len(batch) == 1


def test_flag_and_parameter_documents():
    assert [F.bm25_flag(d, 0, 8) for d in F.FLAG_DOCS] == [0, 1, 0, 1, 0, 1, 0]
    assert F.as_bytes(F.FLAG_DOCS[1]) == b"\x80" and F.as_bytes(F.FLAG_DOCS[3]) == b"\xff"
    assert [len(F.as_bytes(d)) for d in F.flag_docs_blanked()] == [15, 0, 22, 0, 11, 0, 1]
    lo, hi = F.avgdl_encoders(1000)
    assert lo.avgdl == 1 / 1000 and hi.avgdl == 5000.0
    enc = F.bm25_encoder(1000)
    assert max(len(F.bm25_want(e, d)[0]) for e in (enc, lo, hi) for d in F.PARAM_DOCS) <= 16
    # the parameters matter: every (k1, b) and both avgdl give other weights for the same document
    bits = {tuple(F.bm25_want(F.bm25_encoder(1000, k1, b), F.PARAM_DOCS[1])[1].tolist()) for k1, b in F.PARAMS}
    bits |= {tuple(F.bm25_want(e, F.PARAM_DOCS[1])[1].tolist()) for e in (lo, hi)}
    assert len(bits) == len(F.PARAMS) + 2


def test_every_document_expected_back_encoded_fits_the_cap_of_its_gpu_test():
    """(documents, cap, dims) as tests/test_gpu_text_front_edges.py launches them: every ASCII document of at most 65 535
    bytes is expected with flag 0, so its reference must hold no more than cap entries"""
    cases = [(F.byte_class_docs(), 2, (1000, 65536, 37)), (list(F.PARAM_DOCS), 16, (1000,)), (F.flag_docs_blanked(), 8, (1000,)),
             ([d for d in F.FLAG_DOCS if isinstance(d, str)], 8, (1000,))]
    cases += [(list(b), 4, (1000, 2)) for b in F.SEAM_BATCHES]
    cases += [(F.length_edge_docs(dim)[:2] + F.length_edge_docs(dim)[3:], 4, (dim,)) for dim in F.LENGTH_EDGE_DIMS]
    cases += [(F.vocab_docs(65536) + F.length_edge_docs(65536)[:2], 4, (65536,))]          # the second-device batch
    for docs, cap, dims in cases:
        for dim in dims:
            enc = F.bm25_encoder(dim)
            assert all(F.bm25_flag(d, len(F.bm25_want(enc, d)[0]), cap) == 0 for d in docs), (cap, dim)


# ------------------------------------------------------------------------------------------------------ tokenizer
@pytest.mark.parametrize("length", F.SLICE_LENGTHS)
def test_slice_edge_texts_start_and_end_tokens_on_slice_edges(length):
    text = F.slice_edge_text(length)
    assert len(text) == length and all(ord(c) < 128 for c in text)
    sl = [s for s in F.slices_of(length) if s[1] > s[0]]
    assert sl[0][0] == 0 and sl[-1][1] == length and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
    is_word = lambda i: 0 <= i < length and ord(text[i]) in F.WORD_BYTES   # noqa: E731
    starts = sum(is_word(b0) and not is_word(b0 - 1) for b0, _ in sl)
    ends = sum(is_word(b1 - 1) and not is_word(b1) for _, b1 in sl)
    assert starts >= 20 and ends >= 20
    if length > 256:                                                       # a word that runs across a slice edge
        assert sum(is_word(b1 - 1) and is_word(b1) for _, b1 in sl) >= 20
    assert len(F.tok_tokens(text)) > 90


def test_long_word_is_the_last_token_kept():
    text, max_len = F.long_word_text()
    toks = F.tok_tokens(text)
    per = -(-len(text) // F.TOK_THREADS)
    assert len(text) == 1025 and len(toks[max_len - 3]) > 3 * per and len(toks) > max_len
    ids, _ = HashTokenizer(30522, max_len).encode(text)
    assert len(ids) == max_len and ids[-2] == HashTokenizer(30522, 64).encode(toks[max_len - 3])[0][1]


@pytest.mark.parametrize("max_len", F.TRUNC_MAX_LENS)
def test_truncation_texts_sit_on_both_sides_of_the_room(max_len):
    room = max_len - 2
    texts = F.truncation_texts(max_len)
    assert [len(F.tok_tokens(t)) for t in texts] == [room - 1, room, room + 1]
    rows, lens = F.tok_rows(HashTokenizer(30522, max_len), texts)
    for r, n_tok in zip(rows, (room - 1, room, room + 1)):
        sep = 1 + min(n_tok, room)
        assert r[0] == 101 and r[sep] == 102 and np.all(r[sep + 1:] == 0) and np.all(r[1:sep] >= 1000)
    assert lens.tolist() == [max_len - 1, max_len, max_len]


def test_fourteen_tokens_fill_a_row_of_sixteen():
    rows, lens = F.tok_rows(HashTokenizer(30522, 16), [F.token_run(14)])
    assert rows[0, 0] == 101 and rows[0, 15] == 102 and np.all(rows[0, 1:15] >= 1000) and lens[0] == 16


def test_vocabulary_of_1001_maps_every_token_to_1000():
    rows, _ = F.tok_rows(HashTokenizer(1001, 16), ["any words, at all!"])
    assert rows[0].tolist()[:8] == [101, 1000, 1000, 1000, 1000, 1000, 1000, 102]
    assert len({int(v) for v in F.tok_rows(HashTokenizer(1002, 64), [F.token_run(40)])[0][0]} - {0, 101, 102}) == 2


# ------------------------------------------------------------------------------------------------------ LayerNorm
def test_fp16_add_rounds_once_and_overflows_to_infinity():
    a = np.array([1.0, 2048.0, 2048.0, 60000.0, 1.0], dtype=np.float16)
    b = np.array([2.0 ** -11, 1.0, 3.0, 60000.0, 2.0 ** -11 + 2.0 ** -21], dtype=np.float16)
    assert F.fp16_add(a, b).tolist() == [1.0, 2048.0, 2052.0, np.inf, 1.0 + 2.0 ** -10]


@pytest.mark.parametrize("regime", F.LN_REGIMES)
def test_layernorm_regimes_and_the_yardstick_is_not_vacuous(regime):
    """torch's unfused fp16 path on the CPU stays within a few fp16 ulps of the fp64 reference in every regime: a kernel
    held to twice that is held to something"""
    x, res = F.ln_inputs(regime)
    assert x.shape == res.shape == (F.LN_ROWS, F.LN_HIDDEN) and x.dtype == np.float16
    g, b = F.ln_params(F.LN_HIDDEN)
    h = F.fp16_add(x, res)
    want = F.ln_ref(h, g, b, 1e-12)
    plain = torch.nn.functional.layer_norm(torch.from_numpy(h), (F.LN_HIDDEN,), torch.from_numpy(g), torch.from_numpy(b), 1e-12)
    e_u = np.abs(plain.double().numpy() - want)
    assert np.isfinite(want).all() and e_u.max() < 1e-2 and e_u.max() < 4 * R.fp16_ulp_at(np.abs(want).max())
    if regime == "offset_tight":
        # the one-pass variance E[x^2] - mean^2 in fp32 has lost the variance here: its relative error is far above what
        # the yardstick lets through
        h32 = h.astype(np.float32)
        mean = h32.mean(axis=1, dtype=np.float32)
        one_pass = (h32 * h32).mean(axis=1, dtype=np.float32) - mean * mean
        true = h.astype(np.float64).var(axis=1)
        big = np.abs(mean) > 20
        assert np.abs(one_pass[big] / true[big] - 1).max() > 0.02
        assert (true[big] < 1e-5 * mean[big].astype(np.float64) ** 2).all()


def test_eps_references_are_far_apart():
    x, res = F.ln_inputs("small_variance")
    g, b = F.ln_params(F.LN_HIDDEN)
    refs = [F.ln_ref(F.fp16_add(x, res), g, b, eps) for eps in F.EPS_VALUES]
    for i in range(3):
        for j in range(i + 1, 3):
            u = R.fp16_ulp_at(max(np.abs(refs[i]).max(), np.abs(refs[j]).max()))
            assert np.abs(refs[i] - refs[j]).max() > 10 * u, (i, j)


def test_constant_rows_have_an_exact_mean_in_the_kernels_arithmetic():
    """-> the kernels return beta bit for bit on a constant row: x - mean is exactly 0 for every constant and width of the
    GPU test (and for all the fp16 values k / 64 up to 32)"""
    for width in F.CONSTANT_WIDTHS + (64,):
        rows = F.constant_rows(width)
        assert rows.shape == (17, width) and {float(v) for v in rows[:, 0]} == {float(np.float16(c)) for c in F.CONSTANTS}
        for c in np.array(F.CONSTANTS, dtype=np.float16):
            assert F.emulated_mean(c, width) == np.float32(c), (width, c)
    for width in (8, 136, 384, 1024):
        for k in range(1, 2048, 37):
            c = np.float16(k / 64)
            assert F.emulated_mean(c, width) == np.float32(c), (width, c)


def test_poisoned_rows():
    x, res = F.ln_inputs("unit")
    px, pres = F.poisoned(x, res)
    h = F.fp16_add(px, pres)
    assert np.isnan(h[F.NAN_ROW]).all() and np.isposinf(h[F.OVERFLOW_ROW]).all()
    others = np.ones(F.LN_ROWS, dtype=bool)
    others[[F.NAN_ROW, F.OVERFLOW_ROW]] = False
    assert np.array_equal(h[others], F.fp16_add(x, res)[others])
    g, b = F.ln_params(F.LN_HIDDEN)
    want = F.ln_ref(h, g, b, 1e-12)
    assert not np.isfinite(want[~others]).any() and np.isfinite(want[others]).all()
    assert F.NAN_ROW // 4 != F.OVERFLOW_ROW // 4 and F.NAN_ROW // 16 != F.OVERFLOW_ROW // 16   # other waves, other blocks


def test_embedding_cases():
    for n_seq, T in F.EMBED_SHAPES:
        ids, types = F.embed_ids(n_seq, T)
        assert ids.min() == 0 and ids.max() == F.N_WORD - 1 and set(types.reshape(-1).tolist()) <= {0, 1}
        assert (n_seq * T) % 16 != 0 or T % 16 == 0
    word, pos, seg = F.embed_tables(384)
    assert len({p.tobytes() for p in pos}) == F.N_POS                       # position rows all distinct
    ids, types = F.embed_ids(5, 7)
    # `order`: the two orders of the adds differ in at least a tenth of the elements
    word, pos, seg = F.embed_tables(384, regime="order")
    a, b = F.embed_chain(word, pos, seg, ids, types), F.embed_other_order(word, pos, seg, ids, types)
    assert (a != b).mean() >= 0.10
    # `order_planted`: the chain returns the word rows exactly, the other order moves a good share of them by 2
    word, pos, seg = F.embed_tables(384, regime="order_planted")
    a, b = F.embed_chain(word, pos, seg, ids, types), F.embed_other_order(word, pos, seg, ids, types)
    assert np.array_equal(a, word[ids]) and (a != b).mean() > 0.3 and set(np.abs(a.astype(np.float64) - b).reshape(-1)) == {0.0, 2.0}
    g, be = F.ln_params(384)
    apart = np.abs(F.ln_ref(a, g, be, 1e-12) - F.ln_ref(b, g, be, 1e-12))
    assert apart.max() > 20 * R.fp16_ulp_at(np.abs(F.ln_ref(a, g, be, 1e-12)).max())
