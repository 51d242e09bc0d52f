"""The three hand-written launches of an encoder layer — linear_rows_kernel, attention_kernel, encoder_tail_kernel
(csrc/encoder_layer.h, csrc/attention.h) — at the edges and value ranges the tests that arrived with them never reach.
The cases, the references and the reasoning behind every bound are in tests/encoder_refs.py; tests/test_encoder_refs_host.py
shows on the CPU that the cases have the properties they are named after and that the attention bound is met by the
kernel's documented arithmetic.

A  attention with EXACT scores (scale = ln 2, integer Q and K): every valid output element within the derived bound
   2^-10 sum p |v| + 2^-11 |want| + L 2^-24 max|v| of fp64, in all three entry points, at the length edges, with planted
   keys that move the lazy reference maximum, with poisoned padding (bitwise), degenerate lengths, identical copies (bitwise).
B  hr_linear_rows_f16_dev: exact integer products, the 65 536-row variant boundary, NaN pad rows.
C  hr_encoder_tail_f16_dev against fp64, with the unfused fp16 path on the same inputs as the yardstick
   (max E_k <= 2 max E_u + u, mean E_k <= 2 mean E_u), over value regimes trained checkpoints have; row edges, NaN pads, a
   chain of launches over NaN-prefilled buffers, identical rows (all bitwise).
D  whole models with trained-like statistics against an fp64 copy, and re-packing after a weight changes in place.
E  load_local drops the captured graphs."""
import copy

import numpy as np
import pytest

import encoder_refs as R

torch = pytest.importorskip("torch")
from advanced_rag.encoders import CrossEncoderModel, EncoderConfig, SentenceEncoder, add_layer_norm  # noqa: E402

NAN = float("nan")
_REFS = {}


def _ref(case, nq):
    key = (case.name, nq)
    if key not in _REFS:
        _REFS[key] = R.attention_ref(case, nq)
    return _REFS[key]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run_attention(case, row_queries=(1, 33)):
    """All three entry points on one case, every output buffer prefilled with NaN -> numpy fp16 arrays: 'rm' and 'fr'
    [n_seq][T][H] (the fragment-order one read back), nq: [n_seq][nq][H] of hr_attention_rows_f16_dev."""
    from advanced_rag import _native as nat
    from advanced_rag.encoder_kernels import fr_rows, from_fragment_order
    n_seq, T, hd = case.n_seq, case.T, case.hd
    H = R.HEADS * hd
    qkv = torch.from_numpy(case.qkv).cuda()
    lengths = torch.from_numpy(case.lengths).cuda()
    out = torch.full((n_seq, T, H), NAN, dtype=torch.float16, device="cuda")
    nat.attention_f16_dev(qkv.data_ptr(), lengths.data_ptr(), out.data_ptr(), n_seq, T, R.HEADS, hd, R.LN2, _stream())
    M = n_seq * T
    ofr = torch.full((fr_rows(M), H), NAN, dtype=torch.float16, device="cuda")
    nat.attention_fr_f16_dev(qkv.data_ptr(), lengths.data_ptr(), ofr.data_ptr(), n_seq, T, R.HEADS, hd, R.LN2, _stream())
    res = {}
    kv = qkv[:, :, 1:].contiguous()
    for nq in row_queries:
        qrows = qkv[:, :nq, 0].contiguous()
        o2 = torch.full((n_seq, nq, H), NAN, dtype=torch.float16, device="cuda")
        nat.attention_rows_f16_dev(qrows.data_ptr(), nq * H, H, kv.data_ptr(), kv.data_ptr() + 2 * H, T * 2 * H, 2 * H,
                                   lengths.data_ptr(), o2.data_ptr(), n_seq, T, nq, R.HEADS, hd, R.LN2, _stream())
        res[nq] = o2
    torch.cuda.synchronize()
    back = from_fragment_order(ofr, fr_rows(M))
    assert torch.isnan(back[M:]).all()                   # the pad rows of a fragment-order buffer are never written
    res = {k: v.cpu().numpy() for k, v in res.items()}
    res["rm"] = out.cpu().numpy()
    res["fr"] = back[:M].reshape(n_seq, T, H).cpu().numpy()
    return res


def _hold_to_bound(case, res):
    """every entry point's valid query rows within the derived bound of fp64; sequences without a valid key: zeros"""
    for key, got in res.items():
        nq = None if key in ("rm", "fr") else key
        want, bound = _ref(case, nq)
        ok = R.valid_query_rows(case, nq)
        g = got.astype(np.float64)
        assert np.isfinite(g[ok]).all(), (case.name, key)
        err = np.abs(g - want)
        ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
        print(f"{case.name} [{key}]: max error / bound = {ratio:.3f}, max error = {float(err[ok].max()) if ok.any() else 0.0:.3e}")
        assert (err[ok] <= bound[ok]).all(), (case.name, key, ratio)
        dead = case.live() == 0
        assert (got[dead].view(np.uint16) << 1 == 0).all(), (case.name, key)      # +-0 in every query row


# ------------------------------------------------------------------------------------------------------ A. attention
@pytest.mark.gpu
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_exact_scores_at_the_length_edges(gpu, hd):
    """T = 129 with one sequence per length in {0, 1, 15 .. 17, 31 .. 33, 63 .. 65, 96, 127 .. 129}: hr_attention_f16_dev,
    hr_attention_fr_f16_dev WITH the same lengths (read back and held to fp64 itself) and hr_attention_rows_f16_dev with 1
    and 33 queries, NaN-prefilled outputs, against fp64 within the derived bound on the rows below each length."""
    case = R.length_edges_case(hd)
    _hold_to_bound(case, _run_attention(case))


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_valid_rows_do_not_depend_on_the_padding(gpu, hd):
    """Q, K and V at positions >= length overwritten with +-60 000 (finite, as padded tokens are in production): the rows
    below the length are BITWISE what they were."""
    clean = R.length_edges_case(hd)
    a, b = _run_attention(clean), _run_attention(R.poison_padding(clean))
    for key in a:
        ok = R.valid_query_rows(clean, None if key in ("rm", "fr") else key)
        assert np.array_equal(a[key][ok].view(np.uint16), b[key][ok].view(np.uint16)), key


@pytest.mark.gpu
@pytest.mark.parametrize("T,hd", R.LAZY_SHAPES)
def test_attention_lazy_reference_maximum(gpu, T, hd):
    """Planted keys move the reference maximum in the middle of sequences of lengths T and T - 63: (a) once in a middle
    chunk, (b) twice, the second time at the last valid key, (c) in chunk 0 with every later probability flushed, (d) at
    each of the 32 in-chunk key positions for one query column (the vote and the column maximum from every lane group),
    (e) by more than 128 log2 units (the first exp2 overflows), (step) by exactly 9 and 10 units over a flat past, where the
    rescaled sum still carries a fifth of the result; (equal) Q = 0 gives the mean of V.  Within the derived bound."""
    case = R.lazy_maximum_case(T, hd)
    _hold_to_bound(case, _run_attention(case, row_queries=(64,)))


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_degenerate_lengths(gpu, hd):
    """lengths 0 and negative: all-zero rows; above T: T (include/hbmrag.h)."""
    case = R.degenerate_lengths_case(hd)
    res = _run_attention(case, row_queries=(1,))
    _hold_to_bound(case, res)
    for key in ("rm", "fr"):
        assert (res[key][:5] == 0).all()
    # a length above T is the length T: the same bits as a launch that says T
    capped = R.AttnCase(case.name + "_capped", hd, case.qkv, np.minimum(case.lengths, case.T).astype(np.int32))
    res_t = _run_attention(capped, row_queries=(1,))
    for key in res:
        assert np.array_equal(res[key].view(np.uint16), res_t[key].view(np.uint16)), key


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_identical_sequences_give_identical_bits(gpu, hd):
    """11 copies of one sequence (11 x 2 head groups: a ragged last group of the XCD-aware block mapping): every copy's
    output is bitwise the first one's, in all three entry points, and within the bound."""
    case = R.copies_case(hd)
    res = _run_attention(case)
    _hold_to_bound(case, res)
    for key, got in res.items():
        bits = got.view(np.uint16)
        assert (bits == bits[:1]).all(), key


# ---------------------------------------------------------------------------------------------------- B. linear rows
def _fr_with_pad(x, pad_value):
    """fragment order of x with the pad rows of the last 16-row tile set to pad_value"""
    from advanced_rag.encoder_kernels import fr_rows, to_fragment_order
    M, H = x.shape
    full = torch.full((fr_rows(M), H), pad_value, dtype=x.dtype, device=x.device)
    full[:M] = x
    return to_fragment_order(full)


@pytest.mark.gpu
@pytest.mark.parametrize("n_out", R.LINEAR_NS)
def test_linear_rows_exact_integer_product(gpu, n_out):
    """One-hot rows give back W[:, k] + bias EXACTLY — every packed weight and bias element through the device — at N = 64,
    1152 and the documented limit 4096, in both input layouts; `pair` rows and dense integer rows (partial sums exact in
    fp32) equal the fp64 product rounded once to fp16."""
    from advanced_rag.encoder_kernels import linear_rows, pack_linear, to_fragment_order
    w, b, x = R.linear_weight(n_out), R.linear_bias(n_out), R.linear_exact_rows()
    want = torch.from_numpy((x @ w.T + b).astype(np.float16)).cuda()
    wd, bd, xd = torch.from_numpy(w).cuda().half(), torch.from_numpy(b).cuda().float(), torch.from_numpy(x).cuda().half()
    M = xd.shape[0]
    for fr in (False, True):
        out = torch.full((M, n_out), NAN, dtype=torch.float16, device="cuda")
        linear_rows(to_fragment_order(xd) if fr else xd, *pack_linear(wd, bd, fr), n_out, rows=M, x_fr=fr, out=out)
        torch.cuda.synchronize()
        wrong = (out != want)
        assert not wrong.any(), (fr, int(wrong.sum()), wrong.nonzero()[:5].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [65535, 65536, 65537, 65536 + 255])
def test_linear_rows_at_the_variant_boundary(gpu, rows):
    """Both sides of the 65 536 rows at which the launch switches to four token tiles per wave, and a ragged last block of
    that variant: 64 distinct rows tiled; the first 64 output rows against fp64, every copy bitwise its first copy."""
    from advanced_rag.encoder_kernels import linear_rows, pack_linear, to_fragment_order
    g = torch.Generator(device="cuda").manual_seed(5)
    N = 1152
    x64 = torch.randn((64, 384), device="cuda", generator=g).half()
    w = (torch.randn((N, 384), device="cuda", generator=g) * 0.05).half()
    b = torch.randn((N,), device="cuda", generator=g)
    want = (x64.double() @ w.double().t() + b.double()).float()
    x = x64.repeat(-(-rows // 64), 1)[:rows].contiguous()
    for fr in (False, True):
        out = linear_rows(to_fragment_order(x) if fr else x, *pack_linear(w, b, fr), N, rows=rows, x_fr=fr)
        torch.cuda.synchronize()
        assert out.shape == (rows, N)
        assert torch.allclose(out[:64].float(), want, atol=4e-3, rtol=4e-3), (fr, (out[:64].float() - want).abs().max())
        full = rows // 64
        first = _bits(out[:64])
        assert (_bits(out[:full * 64]).view(full, 64, N) == first[None]).all(), fr
        rem = rows - full * 64
        assert torch.equal(_bits(out[full * 64:]), first[:rem]), fr


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 17, 129 + 5])
def test_linear_rows_ignores_poisoned_pad_rows(gpu, M):
    """fragment-order input whose pad rows hold NaN: bitwise the result with zero pads"""
    from advanced_rag.encoder_kernels import linear_rows, pack_linear
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn((M, 384), device="cuda", generator=g).half()
    w = (torch.randn((1152, 384), device="cuda", generator=g) * 0.05).half()
    b = torch.randn((1152,), device="cuda", generator=g)
    wp, bp = pack_linear(w, b, True)
    clean = linear_rows(_fr_with_pad(x, 0.0), wp, bp, 1152, rows=M, x_fr=True)
    dirty = linear_rows(_fr_with_pad(x, NAN), wp, bp, 1152, rows=M, x_fr=True)
    torch.cuda.synchronize()
    assert torch.isfinite(dirty).all() and torch.equal(_bits(clean), _bits(dirty))
    want = (x.double() @ w.double().t() + b.double()).float()
    assert torch.allclose(dirty.float(), want, atol=4e-3, rtol=4e-3)


# ----------------------------------------------------------------------------------------------------- C. layer tail
def _gpu_layer(layer):
    return copy.deepcopy(layer).to("cuda", torch.float16)


def _tail(layer_gpu, a, x, eps, x_fr=False, out_fr=False, pad=0.0):
    """hr_encoder_tail_f16_dev on CPU fp16 tensors a, x -> row-major GPU result (a fragment-order output is read back)"""
    from advanced_rag.encoder_kernels import encoder_tail, from_fragment_order
    rows = a.shape[0]
    k = layer_gpu.kernels.ensure(layer_gpu)
    a_fr = _fr_with_pad(a.cuda(), pad)
    xin = _fr_with_pad(x.cuda(), pad) if x_fr else x.cuda()
    out = encoder_tail(a_fr, xin, k, 1536, eps, layer_gpu.gelu == "erf", rows=rows, x_fr=x_fr, out_fr=out_fr)
    torch.cuda.synchronize()
    return from_fragment_order(out, rows) if out_fr else out


def _tail_unfused(layer_gpu, a, x, eps):
    """the yardstick: the same inputs through the PyTorch fp16 GEMMs and the separate add + LayerNorm kernel"""
    layer_gpu.ln1.eps = layer_gpu.ln2.eps = eps
    a, x = a.cuda(), x.cuda()
    x1 = add_layer_norm(x, layer_gpu.out(a), layer_gpu.ln1)
    y = add_layer_norm(x1, layer_gpu.down(layer_gpu._ffn_up(x1[None])[0]), layer_gpu.ln2)
    torch.cuda.synchronize()
    return y


def _tail_errors(layer, layer_gpu, a, x, eps, label):
    """-> (kernel result, want): asserts the yardstick criterion and prints E_k / E_u"""
    with torch.inference_mode():
        got = _tail(layer_gpu, a, x, eps)
        plain = _tail_unfused(layer_gpu, a, x, eps)
    want = R.tail_ref(a, x, layer, eps=eps)
    assert torch.isfinite(got).all()
    e_k = (got.cpu().double() - want).abs().numpy()
    e_u = (plain.cpu().double() - want).abs().numpy()
    ok, (mk, mu, ak, au), u = R.yardstick_ok(e_k, e_u, float(want.abs().max()))
    print(f"tail {label}: max E_k {mk:.3e}  max E_u {mu:.3e}  mean E_k {ak:.3e}  mean E_u {au:.3e}  u {u:.2e}")
    assert ok, (label, mk, mu, ak, au, u)
    return got, want, 2 * mu + u


@pytest.mark.gpu
@pytest.mark.parametrize("gelu", ["tanh", "erf"])
@pytest.mark.parametrize("regime", R.TAIL_REGIMES)
def test_encoder_tail_value_regimes_against_fp64(gpu, regime, gelu):
    """200 rows per regime (unit; rows offset by +-8 / +-30 with a spread of 0.5; three hidden dimensions 30 x larger; FFN
    pre-activations beyond +-11.5, both saturated ends of the tanh form; variance 1e-6 with eps = 1e-12 and eps = 1e-5):
    the kernel's error against fp64 is at most twice the unfused fp16 path's plus one ulp, in the maximum and on average."""
    layer = R.tail_layer(gelu, regime)
    lg = _gpu_layer(layer)
    a, x = R.tail_inputs(regime, 200)
    if regime != "small_variance":
        _tail_errors(layer, lg, a, x, 1e-12, f"{regime}/{gelu}")
        return
    g12, w12, b12 = _tail_errors(layer, lg, a, x, 1e-12, f"{regime}/{gelu}/eps=1e-12")
    g5, w5, b5 = _tail_errors(layer, lg, a, x, 1e-5, f"{regime}/{gelu}/eps=1e-5")
    # eps is used: the two results differ by what the reference says they differ by
    assert float((w12 - w5).abs().max()) > 0.5
    d = ((g12.cpu().double() - g5.cpu().double()) - (w12 - w5)).abs().max()
    assert float(d) <= b12 + b5, (float(d), b12, b5)


@pytest.mark.gpu
@pytest.mark.parametrize("gelu", ["tanh", "erf"])
def test_encoder_tail_row_edges(gpu, gelu):
    """Row counts around a 16-row tile, a wave's 32 rows and a block's 128: the fragment-order output, read back, is
    bitwise the row-major output, and both meet the unit regime's criterion."""
    layer = R.tail_layer(gelu)
    lg = _gpu_layer(layer)
    for rows in R.TAIL_ROW_EDGES:
        a, x = R.tail_inputs("unit", rows)
        got, _, _ = _tail_errors(layer, lg, a, x, 1e-12, f"rows={rows}/{gelu}")
        with torch.inference_mode():
            got_fr = _tail(lg, a, x, 1e-12, x_fr=True, out_fr=True)
        assert got.shape == got_fr.shape == (rows, 384) and torch.equal(_bits(got), _bits(got_fr)), rows


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 17, 129 + 5])
def test_encoder_tail_ignores_poisoned_pad_rows(gpu, rows):
    """the pad rows of the fragment-order attention output and of a fragment-order x hold NaN: the valid rows are bitwise
    those of the zero-pad run, in both output layouts"""
    lg = _gpu_layer(R.tail_layer("tanh"))
    a, x = R.tail_inputs("unit", rows)
    with torch.inference_mode():
        for out_fr in (False, True):
            clean = _tail(lg, a, x, 1e-12, x_fr=True, out_fr=out_fr, pad=0.0)
            dirty = _tail(lg, a, x, 1e-12, x_fr=True, out_fr=out_fr, pad=NAN)
            assert torch.isfinite(dirty).all() and torch.equal(_bits(clean), _bits(dirty)), out_fr


@pytest.mark.gpu
def test_layer_chain_over_poisoned_buffers(gpu):
    """What forward_fused does between two layers, over buffers prefilled with NaN instead of fresh memory: QKV projection
    -> hr_attention_fr_f16_dev (real lengths) -> tail with a fragment-order output -> the next layer's projection from
    fragment order.  9 x 17 = 153 rows: the last 16-row tile is ragged, its pad rows are never written and are read by the
    next launch as whole tiles.  Bitwise the same chain over zero-prefilled buffers."""
    from advanced_rag import _native as nat
    from advanced_rag.encoder_kernels import fr_rows, linear_rows
    n_seq, T, H = 9, 17, 384
    M = n_seq * T
    la, lb = _gpu_layer(R.tail_layer("tanh", seed=1)), _gpu_layer(R.tail_layer("erf", seed=2))
    ka, kb = la.kernels.ensure(la), lb.kernels.ensure(lb)
    x = R.tail_inputs("unit", M)[1].cuda()
    lengths = torch.tensor([17, 1, 2, 16, 17, 5, 9, 17, 3], dtype=torch.int32, device="cuda")
    results = []
    with torch.inference_mode():
        for fill in (0.0, NAN):
            qkv = linear_rows(x, ka.qkv_w, ka.qkv_b, 3 * H)
            attn = torch.full((fr_rows(M), H), fill, dtype=torch.float16, device="cuda")
            nat.attention_fr_f16_dev(qkv.data_ptr(), lengths.data_ptr(), attn.data_ptr(), n_seq, T, la.heads, 32, 32 ** -0.5, _stream())
            y = torch.full((fr_rows(M), H), fill, dtype=torch.float16, device="cuda")
            nat.encoder_tail_f16_dev(attn.data_ptr(), x.data_ptr(), False, y.data_ptr(), True, ka.stream.data_ptr(),
                                     ka.tables.data_ptr(), M, H, 1536, 1e-12, False, _stream())
            nxt = linear_rows(y, kb.qkv_w_fr, kb.qkv_b, 3 * H, rows=M, x_fr=True)
            torch.cuda.synchronize()
            results.append((attn, y, nxt))
    (a0, y0, n0), (a1, y1, n1) = results
    assert torch.isfinite(n1).all() and torch.equal(_bits(n0), _bits(n1))
    from advanced_rag.encoder_kernels import from_fragment_order
    for clean, dirty in ((a0, a1), (y0, y1)):
        c, d = from_fragment_order(clean, fr_rows(M)), from_fragment_order(dirty, fr_rows(M))
        assert torch.equal(_bits(c[:M]), _bits(d[:M])) and torch.isnan(d[M:]).all() and (c[M:] == 0).all()


@pytest.mark.gpu
def test_encoder_tail_identical_rows_give_identical_bits(gpu):
    """16 distinct (a, x) rows tiled over 300 rows: every token-tile index, wave and block, and the ragged last block,
    computes the same bits for the same row, in both layouts"""
    lg = _gpu_layer(R.tail_layer("tanh"))
    a16, x16 = R.tail_inputs("unit", 16)
    a, x = a16.repeat(19, 1)[:300].contiguous(), x16.repeat(19, 1)[:300].contiguous()
    with torch.inference_mode():
        for fr in (False, True):
            out = _tail(lg, a, x, 1e-12, x_fr=fr, out_fr=fr)
            first = _bits(out[:16])
            assert (_bits(out[:288]).view(18, 16, 384) == first[None]).all() and torch.equal(_bits(out[288:]), first[:12]), fr


# ---------------------------------------------------------------------------------------------------- D. whole models
def _trained_like(module, seed):
    """in place: linear weights N(0, 0.05), biases N(0, 0.1), LayerNorm gamma U(0.5, 1.5), beta N(0, 0.2), three word-embedding
    dimensions 12 x larger — the statistics of a trained checkpoint instead of BERT's initialisation"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for mod in module.modules():
            if isinstance(mod, torch.nn.Linear):
                mod.weight.normal_(0, 0.05, generator=gen)
                mod.bias.normal_(0, 0.1, generator=gen)
            elif isinstance(mod, torch.nn.LayerNorm):
                mod.weight.uniform_(0.5, 1.5, generator=gen)
                mod.bias.normal_(0, 0.2, generator=gen)
        module.encoder.word.weight[:, [3, 100, 300]] *= 12


def _three_forwards(module, ref, batch):
    """-> (fused, unfused, fp64) results of one module on one batch"""
    ids, types, mask = batch
    layers = module.encoder.layers
    with torch.inference_mode():
        fused = module(ids, types, mask).double().cpu()
        for layer in layers:
            layer.use_layer_kernels = False
        try:
            plain = module(ids, types, mask).double().cpu()
        finally:
            for layer in layers:
                layer.use_layer_kernels = True
        want = ref(ids.cpu(), types.cpu(), mask.cpu()).double()
    torch.cuda.synchronize()
    return fused, plain, want


def _criterion(fused, plain, want, label):
    e_k, e_u = float((fused - want).abs().max()), float((plain - want).abs().max())
    u = R.fp16_ulp_at(float(want.abs().max()))
    print(f"{label}: max|fused - fp64| {e_k:.3e}  max|unfused - fp64| {e_u:.3e}  u {u:.2e}")
    assert torch.isfinite(fused).all() and e_k <= 2 * e_u + u, (label, e_k, e_u, u)
    return 2 * e_u + u


@pytest.mark.gpu
@pytest.mark.parametrize("gelu", ["tanh", "erf"])
@pytest.mark.parametrize("T", [17, 129])
def test_whole_models_with_trained_like_statistics(gpu, T, gelu):
    """A cross-encoder (logits: the last layer for token 0 only — the keys / values projection and the one-query attention)
    and a sentence encoder (embeddings) whose parameters have trained-like statistics, B = 9, lengths from 2 to T: the
    fused forward is no further from an fp64 copy of the module than twice the unfused fp16 forward plus one ulp.  Then one
    layer's output projection is negated IN PLACE: the fused forward follows (LayerKernels.ensure re-packed)."""
    B = 9
    g = torch.Generator(device="cuda").manual_seed(T)
    ids = torch.randint(1000, 30000, (B, T), device="cuda", generator=g)
    ids[:, 0] = 101
    types = (torch.arange(T, device="cuda")[None, :] >= T // 3).long().expand(B, T).contiguous()
    lens = torch.tensor([T, 2, 16, T - 1, 3, 15, 17, T // 2, 2], device="cuda").clamp(2, T)
    mask = torch.arange(T, device="cuda")[None, :] < lens[:, None]
    ids = ids.masked_fill(~mask, 0)
    batch = (ids, types, mask)
    for name, model in (("cross-encoder logits", CrossEncoderModel(EncoderConfig(gelu=gelu), device="cuda:0", seed=5)),
                        ("sentence embeddings", SentenceEncoder(EncoderConfig(gelu=gelu), device="cuda:0", seed=6))):
        module = model.module
        _trained_like(module, 11)
        ref = copy.deepcopy(module).to("cpu", torch.float64)
        fused, plain, want = _three_forwards(module, ref, batch)
        _criterion(fused, plain, want, f"{name} T={T} {gelu}")
        with torch.no_grad():
            module.encoder.layers[2].out.weight.neg_()
            ref.encoder.layers[2].out.weight.neg_()
        fused2, plain2, want2 = _three_forwards(module, ref, batch)
        crit = _criterion(fused2, plain2, want2, f"{name} T={T} {gelu}, layer 2 W_out negated")
        moved = float((fused2 - fused).abs().max())
        assert moved > crit and float((want2 - want).abs().max()) > crit, (name, moved, crit)   # the change is visible, and followed


# ------------------------------------------------------------------------------------------------- E. graph cache
def _hf_state(module):
    """our parameters under HuggingFace BERT names (what load_local reads)"""
    sd = module.state_dict()
    out = {"embeddings.word_embeddings.weight": sd["encoder.word.weight"],
           "embeddings.position_embeddings.weight": sd["encoder.pos.weight"],
           "embeddings.token_type_embeddings.weight": sd["encoder.seg.weight"],
           "embeddings.LayerNorm.weight": sd["encoder.ln.weight"], "embeddings.LayerNorm.bias": sd["encoder.ln.bias"]}
    i = 0
    while f"encoder.layers.{i}.qkv.weight" in sd:
        ours, L = f"encoder.layers.{i}.", f"encoder.layer.{i}."
        for p in ("weight", "bias"):
            for name, part in zip(("query", "key", "value"), sd[ours + f"qkv.{p}"].chunk(3)):
                out[L + f"attention.self.{name}.{p}"] = part
            for mine, theirs in (("out", "attention.output.dense"), ("ln1", "attention.output.LayerNorm"),
                                 ("up", "intermediate.dense"), ("down", "output.dense"), ("ln2", "output.LayerNorm")):
                out[L + f"{theirs}.{p}"] = sd[ours + f"{mine}.{p}"]
        i += 1
    return {k: v.detach().cpu().contiguous() for k, v in out.items()}


@pytest.mark.gpu
def test_load_local_drops_the_captured_graphs(gpu, tmp_path):
    """A graph captured before load_local replays the tanh-GELU kernels; load_local switches the layers to the erf form, so
    it must drop the captured graphs: the next encode captures anew and equals a fresh encoder that loaded the same file
    before its first encode."""
    from safetensors.torch import save_file

    def cfg():
        return EncoderConfig(vocab_size=5000, layers=2)

    text = ["what is retrieval augmented generation"]
    enc = SentenceEncoder(cfg(), device="cuda:0", max_len=64, seed=3)
    before = enc.encode_to_device(text).clone()
    old = {k: v[0] for k, v in enc._graphs.items()}
    assert old
    path = str(tmp_path / "donor.safetensors")
    save_file(_hf_state(SentenceEncoder(cfg(), device="cuda:0", max_len=64, seed=4).module), path)
    enc.load_local(path)
    assert not enc.__dict__.get("_graphs")                                   # the pre-load graph is gone
    assert all(layer.gelu == "erf" for layer in enc.module.encoder.layers)
    after = enc.encode_to_device(text).clone()
    assert enc._graphs and all(enc._graphs[k][0] is not old.get(k) for k in enc._graphs)
    fresh = SentenceEncoder(cfg(), device="cuda:0", max_len=64, seed=3).load_local(path)
    want = fresh.encode_to_device(text)
    torch.cuda.synchronize()
    assert torch.allclose(after, want, atol=2e-3), (after - want).abs().max()
    assert float((after - before).abs().max()) > 1e-2                        # the loaded weights are what ran
