"""Sentence encoder and cross-encoder forward passes in PyTorch-ROCm.

The reference leaves both as plugin hooks: `index_manager.embedding_generator.
encode_semantic / encode_domain` (reference indexing.py:120, :610-620, :665-673)
and `retriever.reranker.score(pairs)` via `CrossEncoderReranker.model.predict`
(retrieval.py:546-547, :675-678; default name cross-encoder/ms-marco-MiniLM-L-6-v2).
These classes fill the hooks with BERT/MiniLM-shaped transformers whose GEMMs run
on the MFMA units through PyTorch (this is the one place the north star wants
PyTorch-ROCm rather than hand-written HIP).  The one elementwise piece PyTorch
leaves badly unfused — residual add + LayerNorm, twice per layer — goes through
`hr_add_layernorm_f16_dev` (csrc/encoder_ops.h) when the activations are fp16 on
the GPU; on the CPU (fp32, tests) the same expression runs in PyTorch.

Offline there are no weights: models are RANDOM-INIT with a fixed seed, so
results are structurally valid (shapes, determinism, batching, dtype) but carry
no semantics.  `load_local(path)` reads a local safetensors file with
HuggingFace BERT parameter names when a caller has one; nothing is ever fetched
by model name.
"""
from __future__ import annotations

import math
import re
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native
from .encoder_kernels import LayerKernels, encoder_tail, fr_rows, linear_rows

_WORD = re.compile(r"\w+|[^\w\s]")
PAD, CLS, SEP = 0, 101, 102


@dataclass
class EncoderConfig:
    """MiniLM-L6-H384 shape by default (the class of model the reference names)."""
    vocab_size: int = 30522
    hidden: int = 384
    layers: int = 6
    heads: int = 12
    intermediate: int = 1536
    max_len: int = 512
    type_vocab: int = 2
    eps: float = 1e-12
    # FFN activation: "tanh" = GELU's tanh approximation, computed in the epilogue of the up-projection GEMM on the GPU
    # (hipBLASLt bias + GELU epilogue through torch._addmm_activation: the [tokens, 4H] intermediate is written once
    # instead of written, re-read and re-written); "erf" = the exact form BERT checkpoints were trained with, as a
    # separate elementwise pass.  Random-init models (all there is offline) default to the fused form; a caller that
    # loads real weights with load_local() passes EncoderConfig(gelu="erf") if the last 1e-3 of the logits matters.
    gelu: str = "tanh"


class HashTokenizer:
    """Dependency-free stand-in for WordPiece: lower-cased words/punctuation hashed
    (crc32) into the vocabulary.  Real vocabularies are not available offline."""

    _MEMO_MAX = 1 << 20

    def __init__(self, vocab_size: int = 30522, max_len: int = 512):
        self.vocab_size, self.max_len = vocab_size, max_len
        self._memo: Dict[str, int] = {}      # token -> id: a corpus repeats its vocabulary, the hash is paid once per token

    def _id(self, t: str) -> int:
        i = 1000 + zlib.crc32(t.encode("utf-8")) % (self.vocab_size - 1000)
        if len(self._memo) < self._MEMO_MAX:
            self._memo[t] = i
        return i

    def _ids(self, text: str, limit: Optional[int] = None) -> List[int]:
        memo, slow = self._memo, self._id
        toks = _WORD.findall(text.lower())
        if limit is not None:
            toks = toks[:limit]              # what lies beyond max_len is never encoded
        return [memo[t] if t in memo else slow(t) for t in toks]

    def encode(self, text: str, pair: Optional[str] = None) -> Tuple[List[int], List[int]]:
        if pair is None:
            ids = [CLS] + self._ids(text, self.max_len - 2) + [SEP]
            return ids, [0] * len(ids)
        a = self._ids(text)
        b = self._ids(pair)
        room = self.max_len - 3
        a = a[: max(1, min(len(a), room // 2))]
        b = b[: room - len(a)]
        ids = [CLS] + a + [SEP] + b + [SEP]
        return ids, [0] * (len(a) + 2) + [1] * (len(b) + 1)

    def _batch_on_device(self, texts: Sequence[str], dev):
        """Single texts tokenised by ONE launch on the GPU (hr_hash_tokenize_dev, csrc/text.h): the bytes go up once, the ids
        never come down.  None when a text is not ASCII (Unicode case mapping / categories are Python's): the host path."""
        from . import _native
        raw = [t.encode("utf-8") for t in texts]
        n = len(raw)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(r) for r in raw], out=off[1:])
        d_text = torch.frombuffer(bytearray(b"".join(raw) or b"\0"), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(off).to(dev)
        ids = torch.empty((n, self.max_len), dtype=torch.long, device=dev)
        lens = torch.empty(n, dtype=torch.int32, device=dev)
        flags = torch.empty(n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _native.hash_tokenize_dev(d_text.data_ptr(), d_off.data_ptr(), n, self.max_len, self.vocab_size, ids.data_ptr(),
                                      lens.data_ptr(), flags.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            stat = torch.stack([lens.max(), flags.max()]).cpu()
        if int(stat[1]):
            return None
        width = -(-int(stat[0]) // 8) * 8
        ids = ids[:, :width].contiguous() if width <= self.max_len else torch.nn.functional.pad(ids, (0, width - self.max_len))
        return ids, torch.zeros_like(ids), ids != PAD

    def batch(self, texts: Sequence[str], pairs: Optional[Sequence[str]] = None, device="cpu"):
        if pairs is None and len(texts) and torch.device(device).type == "cuda":
            on_dev = self._batch_on_device(texts, torch.device(device))
            if on_dev is not None:
                return on_dev
        enc = [self.encode(t, None if pairs is None else pairs[i]) for i, t in enumerate(texts)]
        width = max(len(i) for i, _ in enc)
        width = -(-width // 8) * 8  # friendlier GEMM shapes
        ids_h = np.full((len(enc), width), PAD, dtype=np.int64)      # one host array, one conversion (was a tensor per row)
        types_h = np.zeros((len(enc), width), dtype=np.int64)
        for r, (i, t) in enumerate(enc):
            ids_h[r, : len(i)] = i
            if pairs is not None:
                types_h[r, : len(t)] = t
        ids, types = torch.from_numpy(ids_h), torch.from_numpy(types_h)
        return ids.to(device), types.to(device), (ids != PAD).to(device)


def add_layer_norm(x: torch.Tensor, residual: Optional[torch.Tensor], ln: nn.LayerNorm) -> torch.Tensor:
    """LayerNorm(x + residual) (residual may be None).  fp16 CUDA activations take the fused HIP kernel — one pass
    instead of an add and a layer-norm launch; it raises if libhbmrag is missing rather than falling back."""
    if x.is_cuda and x.dtype == torch.float16 and ln.weight.dtype == torch.float16:
        H = x.shape[-1]
        xc = x.contiguous()
        rc = residual.contiguous() if residual is not None else None
        out = torch.empty_like(xc)
        _native.add_layernorm_f16_dev(xc.data_ptr(), rc.data_ptr() if rc is not None else 0, ln.weight.data_ptr(),
                                      ln.bias.data_ptr(), out.data_ptr(), xc.numel() // H, H, float(ln.eps),
                                      torch.cuda.current_stream(x.device).cuda_stream)
        return out
    return ln(x if residual is None else x + residual)


class _Layer(nn.Module):
    def __init__(self, c: EncoderConfig):
        super().__init__()
        self.heads = c.heads
        self.gelu = c.gelu
        self.qkv = nn.Linear(c.hidden, 3 * c.hidden)
        self.out = nn.Linear(c.hidden, c.hidden)
        self.ln1 = nn.LayerNorm(c.hidden, eps=c.eps)
        self.up = nn.Linear(c.hidden, c.intermediate)
        self.down = nn.Linear(c.intermediate, c.hidden)
        self.ln2 = nn.LayerNorm(c.hidden, eps=c.eps)
        self.kernels = LayerKernels()     # packed operands of the hand-written layer kernels (built on first GPU use)
        self.use_layer_kernels = True     # False: the PyTorch GEMMs + fused elementwise kernels of round 3 (A/B, tests)

    def _hip_attention_ok(self, x, lengths, hd, T) -> bool:
        return (lengths is not None and x.is_cuda and x.dtype == torch.float16 and
                ((hd == 32 and T <= 1024) or (hd == 64 and T <= 512)))

    def _fused_ok(self, x, lengths, hd, T) -> bool:
        return (self.use_layer_kernels and not getattr(_SMALL, "gemms", False) and self._hip_attention_ok(x, lengths, hd, T)
                and self.gelu in ("tanh", "erf") and LayerKernels.supports(self))

    def forward_fused(self, x2, B, T, lengths, x_fr: bool = False, out_fr: bool = False):
        """The layer as three hand-written launches (csrc/encoder_layer.h, attention.h): QKV projection -> attention ->
        output projection + residual + LayerNorm + FFN + residual + LayerNorm.  x2: [B * T, H] row-major, or the
        fragment-order buffer of the previous layer (x_fr); returns row-major [B * T, H] or fragment order (out_fr).
        Between the launches of a chain of layers the activations stay in fragment order."""
        H = x2.shape[1]
        hd = H // self.heads
        M = B * T
        k = self.kernels.ensure(self)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        qkv = linear_rows(x2, k.qkv_w_fr if x_fr else k.qkv_w, k.qkv_b, 3 * H, rows=M, x_fr=x_fr)
        a = torch.empty((fr_rows(M), H), dtype=x2.dtype, device=x2.device)
        _native.attention_fr_f16_dev(qkv.data_ptr(), lengths.data_ptr(), a.data_ptr(), B, T, self.heads, hd, hd ** -0.5,
                                     torch.cuda.current_stream(x2.device).cuda_stream)
        return encoder_tail(a, x2, k, self.up.weight.shape[0], float(self.ln1.eps), self.gelu == "erf", rows=M, x_fr=x_fr,
                            out_fr=out_fr)

    def forward(self, x, attn_bias, lengths=None):
        B, T, H = x.shape
        hd = H // self.heads
        if self._fused_ok(x, lengths, hd, T):
            return self.forward_fused(x.reshape(B * T, H), B, T, lengths).view(B, T, H)
        qkv = self.qkv(x)
        if self._hip_attention_ok(x, lengths, hd, T):
            # head dimension 32 on the GPU: the HIP attention kernel reads the fused projection as it stands and writes
            # the [tokens, hidden] layout the output projection wants — no permute / transpose copies, no SDPA
            qkv = qkv.contiguous()
            a = torch.empty((B, T, H), dtype=x.dtype, device=x.device)
            _native.attention_f16_dev(qkv.data_ptr(), lengths.data_ptr(), a.data_ptr(), B, T, self.heads, hd, hd ** -0.5,
                                      torch.cuda.current_stream(x.device).cuda_stream)
        else:
            q, k, v = qkv.view(B, T, 3, self.heads, hd).permute(2, 0, 3, 1, 4)
            a = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_bias).transpose(1, 2).reshape(B, T, H)
        x = add_layer_norm(x, self.out(a), self.ln1)  # post-LN, as BERT
        return add_layer_norm(x, self.down(self._ffn_up(x)), self.ln2)

    def forward_first_token(self, x, mask, lengths=None):
        """The LAST layer of a model whose head reads token 0 only (the cross-encoder's relevance head reads [CLS]:
        reference retrieval.py:651-685 hands the pairs to `CrossEncoder.predict`, whose classifier sits on the pooled
        first token): keys and values of every token, and everything else — the query projection, the attention row,
        the output projection, both LayerNorms, the FFN — for token 0 of each sequence alone.  The same arithmetic on
        the rows that reach the output; 10/12 of the layer's GEMM work is for rows nothing reads.  x: [B, T, H] ->
        [B, 1, H]."""
        B, T, H = x.shape
        hd = H // self.heads
        W, b = self.qkv.weight, self.qkv.bias
        if self._fused_ok(x, lengths, hd, T):   # keys and values of every token through the hand-written projection
            k = self.kernels.ensure(self)
            x2 = x.reshape(B * T, H)
            kv = linear_rows(x2 if x2.is_contiguous() else x2.contiguous(), k.kv_w, k.kv_b, 2 * H).view(B, T, 2 * H)
        else:
            kv = F.linear(x, W[H:], b[H:])                                              # [B, T, 2, heads, hd]
        q = F.linear(x[:, 0], W[:H], b[:H])                                             # [B, heads, hd]
        if self._hip_attention_ok(x, lengths, hd, T):
            # the HIP attention kernel with ONE query row per sequence against the K / V buffer (hr_attention_rows_f16_dev)
            kv, q = kv.contiguous(), q.contiguous()
            a = torch.empty((B, 1, H), dtype=x.dtype, device=x.device)
            _native.attention_rows_f16_dev(q.data_ptr(), H, 0, kv.data_ptr(), kv.data_ptr() + 2 * H, T * 2 * H, 2 * H,
                                           lengths.data_ptr(), a.data_ptr(), B, T, 1, self.heads, hd, hd ** -0.5,
                                           torch.cuda.current_stream(x.device).cuda_stream)
        else:
            kv = kv.view(B, T, 2, self.heads, hd)
            k, v = kv[:, :, 0].permute(0, 2, 1, 3), kv[:, :, 1].permute(0, 2, 1, 3)     # [B, heads, T, hd] views
            s = torch.matmul(q.view(B, self.heads, 1, hd), k.transpose(-1, -2)).float() * (hd ** -0.5)   # [B, heads, 1, T]
            s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
            a = torch.matmul(torch.softmax(s, dim=-1).to(x.dtype), v).reshape(B, 1, H)
        x0 = add_layer_norm(x[:, :1], self.out(a), self.ln1)
        return add_layer_norm(x0, self.down(self._ffn_up(x0)), self.ln2)

    def _ffn_up(self, x):
        if self.gelu != "tanh":
            return F.gelu(self.up(x))
        if x.is_cuda:   # bias + GELU in the GEMM epilogue
            B, T, H = x.shape
            return torch._addmm_activation(self.up.bias, x.reshape(B * T, H), self.up.weight.t(), use_gelu=True).view(B, T, -1)
        return F.gelu(self.up(x), approximate="tanh")


class BertEncoder(nn.Module):
    def __init__(self, config: Optional[EncoderConfig] = None):
        super().__init__()
        c = self.config = config or EncoderConfig()
        self.word = nn.Embedding(c.vocab_size, c.hidden, padding_idx=PAD)
        self.pos = nn.Embedding(c.max_len, c.hidden)
        self.seg = nn.Embedding(c.type_vocab, c.hidden)
        self.ln = nn.LayerNorm(c.hidden, eps=c.eps)
        self.layers = nn.ModuleList(_Layer(c) for _ in range(c.layers))

    def forward(self, ids, types, mask, first_token_only: bool = False):
        """-> hidden states [B, T, H]; with first_token_only, [B, 1, H]: the last layer computes token 0 alone
        (_Layer.forward_first_token) — for heads that read nothing else."""
        B, T = ids.shape
        if ids.is_cuda and self.word.weight.dtype == torch.float16 and T <= self.pos.weight.shape[0]:
            # the embedding layer in one HIP kernel: two gathers, the position rows, both adds and the LayerNorm (ids outside
            # the tables are clamped by the kernel: no check here that would synchronise the stream)
            ids_c, types_c = ids.contiguous().long(), types.contiguous().long()
            H = self.word.weight.shape[1]
            x = torch.empty((B, T, H), dtype=torch.float16, device=ids.device)
            _native.embed_layernorm_f16_dev(ids_c.data_ptr(), types_c.data_ptr(), self.word.weight.data_ptr(),
                                            self.pos.weight.data_ptr(), self.seg.weight.data_ptr(), self.ln.weight.data_ptr(),
                                            self.ln.bias.data_ptr(), x.data_ptr(), B, T, H, float(self.ln.eps),
                                            self.word.weight.shape[0], self.seg.weight.shape[0],
                                            torch.cuda.current_stream(ids.device).cuda_stream)
        else:
            x = add_layer_norm(self.word(ids) + self.pos(torch.arange(T, device=ids.device))[None], self.seg(types), self.ln)
        bias = torch.zeros(mask.shape, dtype=x.dtype, device=x.device).masked_fill(~mask, float("-inf"))[:, None, None, :]
        # valid tokens per sequence for the HIP attention kernel: padding sits at the tail (HashTokenizer.batch), so the
        # key mask is "position < length"
        lengths = mask.sum(dim=1).to(torch.int32) if x.is_cuda and x.dtype == torch.float16 else None
        n_full = len(self.layers) - (1 if first_token_only else 0)
        H = x.shape[-1]
        if n_full and all(layer._fused_ok(x, lengths, H // layer.heads, T) for layer in self.layers[:n_full]):
            # every layer through the hand-written kernels: the activations stay in fragment order between the layers
            x2 = x.reshape(B * T, H)
            for i, layer in enumerate(self.layers[:n_full]):
                x2 = layer.forward_fused(x2, B, T, lengths, x_fr=i > 0, out_fr=i + 1 < n_full)
            x = x2.view(B, T, H)
        else:
            for layer in self.layers[:n_full]:
                x = layer(x, bias, lengths)
        if first_token_only:
            x = self.layers[-1].forward_first_token(x, mask, lengths)
        return x


def _seeded(module_fn, seed: int):
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        m = module_fn()
        for mod in m.modules():  # BERT init: N(0, 0.02)
            if isinstance(mod, (nn.Linear, nn.Embedding)):
                nn.init.normal_(mod.weight, std=0.02)
            if isinstance(mod, nn.Linear) and mod.bias is not None:
                nn.init.zeros_(mod.bias)
        return m
    finally:
        torch.random.set_rng_state(gen_state)


_TUNED_GEMMS = None
_SMALL = __import__("threading").local()    # .gemms = True while a small batch is being captured (see _Base._forward_replayed)


def use_recorded_gemm_solutions() -> bool:
    """Let PyTorch's TunableOp pick the hipBLASLt solutions RECORDED for the encoder's GEMM shapes on gfx950
    (tunableop_gfx950_minilm.csv, written by `tests/perf_probe_ce.py` on an MI355X: QKV / output / FFN projections of
    MiniLM-L6-H384 at 2560 pairs x 128 and x 512 tokens — hipBLASLt's default heuristic is 12 % slower on these K = 384
    shapes).  Nothing is tuned online and the file is never rewritten; shapes or library versions the file does not cover
    fall back to the default heuristic.  Process-wide (it is a torch setting); returns whether it took effect."""
    global _TUNED_GEMMS
    if _TUNED_GEMMS is None:
        _TUNED_GEMMS = False
        try:
            import atexit
            import os
            import shutil
            import tempfile
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_gfx950_minilm.csv")
            if torch.cuda.is_available() and os.path.exists(path):
                # TunableOp may rewrite its results file when the process ends: it gets a private copy in a directory
                # only this user can enter (mkdtemp: mode 0700, unpredictable name), removed when the process exits
                private = tempfile.mkdtemp(prefix="hbmrag_tunableop_")
                atexit.register(shutil.rmtree, private, ignore_errors=True)
                work = os.path.join(private, "solutions.csv")
                shutil.copyfile(path, work)
                torch.cuda.tunable.enable(True)
                torch.cuda.tunable.tuning_enable(False)
                torch.cuda.tunable.set_filename(work)
                _TUNED_GEMMS = True
        except Exception:   # an older torch without the API: the default heuristic it is
            _TUNED_GEMMS = False
    return _TUNED_GEMMS


class _Base:
    def __init__(self, config, device, dtype, seed, max_len, batch_size):
        self.config = config or EncoderConfig()
        self.device = torch.device(device if device is not None else ("cuda:0" if torch.cuda.is_available() else "cpu"))
        self.dtype = dtype if dtype is not None else (torch.float16 if self.device.type == "cuda" else torch.float32)
        self.tokenizer = HashTokenizer(self.config.vocab_size, min(max_len, self.config.max_len))
        self.batch_size = batch_size
        self.seed = seed
        self.tuned_gemms = use_recorded_gemm_solutions() if self.device.type == "cuda" else False

    # A lone query (or the 20 pairs of one rerank) through a BERT-class model is ~100 launches of a few microseconds of
    # work each: the forward is bound by launching, not by the GPU.  Such batches are captured ONCE per shape as a HIP graph
    # (torch.cuda.CUDAGraph: the hand-written kernels launch on the capturing stream like any torch op) and replayed: one
    # launch per forward.  Shapes are quantised (GRAPH_BATCHES texts x GRAPH_WIDTHS tokens — up to a round of the batching front —, zero padded and masked) so that
    # a few graphs cover the request side; larger batches (ingest, a full round of the batching front, the throughput
    # bench) run eagerly.  Inside a replayed forward the layers use the library GEMMs, not the token-stationary layer
    # kernels: those stream a layer's weights through ONE compute unit per 128 rows (0.12 ms per layer whatever the batch),
    # which pays from ~4 000 rows on (tests/probes/fused_crossover.py: 2 560 rows 0.77 ms eager / fused, 0.36 ms replayed /
    # GEMMs; 16 rows 0.69 against 0.21 ms).
    GRAPH_BATCHES, GRAPH_WIDTHS, use_graphs, MAX_GRAPHS = (1, 2, 4, 8, 16, 32, 64), (16, 32, 64), True, 24

    def _forward_replayed(self, ids, types, mask):
        if not (self.use_graphs and ids.is_cuda) or ids.shape[0] > self.GRAPH_BATCHES[-1] or ids.shape[1] > self.GRAPH_WIDTHS[-1]:
            return None
        import threading
        n, w = ids.shape
        B = next(b for b in self.GRAPH_BATCHES if b >= n)
        W = next(x for x in self.GRAPH_WIDTHS if x >= w)
        lock = self.__dict__.setdefault("_graph_lock", threading.Lock())
        with lock:
            graphs = self.__dict__.setdefault("_graphs", {})
            g = graphs.get((B, W))
            if g is None:
                if len(graphs) >= self.MAX_GRAPHS:
                    return None
                s_ids = torch.zeros((B, W), dtype=ids.dtype, device=ids.device)
                s_types, s_mask = torch.zeros_like(s_ids), torch.zeros((B, W), dtype=torch.bool, device=ids.device)
                s_ids[:, 0], s_ids[:, 1], s_mask[:, :2] = CLS, SEP, True           # rows beyond n: an empty text
                _SMALL.gemms = True
                try:
                    side = torch.cuda.Stream(ids.device)
                    side.wait_stream(torch.cuda.current_stream(ids.device))
                    with torch.cuda.stream(side):                                    # warm-up off the capturing stream
                        for _ in range(2):
                            self.module(s_ids, s_types, s_mask)
                    torch.cuda.current_stream(ids.device).wait_stream(side)
                    graph = torch.cuda.CUDAGraph()
                    # thread_local: other threads of the process (the batching front's searches, an ingest) may allocate
                    # device memory while this one captures
                    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                        s_out = self.module(s_ids, s_types, s_mask)
                finally:
                    _SMALL.gemms = False
                g = graphs[(B, W)] = (graph, s_ids, s_types, s_mask, s_out)
            graph, s_ids, s_types, s_mask, s_out = g
            s_ids.zero_(); s_types.zero_(); s_mask.zero_()
            s_ids[:, 0], s_ids[:, 1], s_mask[:, :2] = CLS, SEP, True
            s_ids[:n, :w], s_types[:n, :w], s_mask[:n, :w] = ids, types, mask
            graph.replay()
            return s_out[:n].clone()

    def load_local(self, path: str, keep_gelu: bool = False) -> "._Base":
        """Load weights from a LOCAL safetensors file with HuggingFace BERT names (never by model name).  BERT / MiniLM
        checkpoints were trained with the exact (erf) GELU — what the reference's `CrossEncoder.predict` computes
        (retrieval.py:675-678) — so loading real weights switches the model to `gelu="erf"`; keep_gelu=True keeps
        whatever the config says (the faster tanh form, ~1e-3 of a logit away)."""
        from safetensors.torch import load_file
        sd = load_file(path)
        if not keep_gelu:
            self.config.gelu = "erf"
            for layer in self.module.encoder.layers:
                layer.gelu = "erf"
        own = self.module.state_dict()
        mapped = {}
        pre = "bert." if any(k.startswith("bert.") for k in sd) else ""
        emb = pre + "embeddings."
        for ours, theirs in (("encoder.word.weight", emb + "word_embeddings.weight"),
                             ("encoder.pos.weight", emb + "position_embeddings.weight"),
                             ("encoder.seg.weight", emb + "token_type_embeddings.weight"),
                             ("encoder.ln.weight", emb + "LayerNorm.weight"), ("encoder.ln.bias", emb + "LayerNorm.bias")):
            if theirs in sd:
                mapped[ours] = sd[theirs]
        for i in range(self.config.layers):
            L = f"{pre}encoder.layer.{i}."
            try:
                mapped[f"encoder.layers.{i}.qkv.weight"] = torch.cat([sd[L + f"attention.self.{n}.weight"] for n in ("query", "key", "value")])
                mapped[f"encoder.layers.{i}.qkv.bias"] = torch.cat([sd[L + f"attention.self.{n}.bias"] for n in ("query", "key", "value")])
            except KeyError:
                continue
            for ours, theirs in (("out", "attention.output.dense"), ("ln1", "attention.output.LayerNorm"),
                                 ("up", "intermediate.dense"), ("down", "output.dense"), ("ln2", "output.LayerNorm")):
                for p in ("weight", "bias"):
                    if L + f"{theirs}.{p}" in sd:
                        mapped[f"encoder.layers.{i}.{ours}.{p}"] = sd[L + f"{theirs}.{p}"]
        for ours, theirs in (("head.weight", "classifier.weight"), ("head.bias", "classifier.bias")):
            if ours in own and theirs in sd:
                mapped[ours] = sd[theirs]
        own.update({k: v.to(own[k].dtype) for k, v in mapped.items() if k in own and own[k].shape == v.shape})
        self.module.load_state_dict(own)
        # graphs captured before the load replay the kernels of the model as it was (the tanh-GELU epilogue): drop them,
        # the next small batch captures anew
        import threading
        with self.__dict__.setdefault("_graph_lock", threading.Lock()):
            self.__dict__.pop("_graphs", None)
        return self


class _SentenceModule(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.encoder = BertEncoder(c)

    def forward(self, ids, types, mask):
        h = self.encoder(ids, types, mask)
        m = mask[..., None].to(h.dtype)
        pooled = (h * m).sum(1) / m.sum(1).clamp_min(1.0)  # mean pooling over real tokens
        return F.normalize(pooled.float(), dim=-1)


class SentenceEncoder(_Base):
    """`embedding_generator` plugin: encode_semantic / encode_semantic_batch / encode_domain (+ optional BM25
    for encode_sparse).  Output dim = config.hidden (384 MiniLM, 768 with EncoderConfig(hidden=768, layers=12,
    intermediate=3072) = bge-base shape)."""

    def __init__(self, config: Optional[EncoderConfig] = None, device=None, dtype=None, seed: int = 0, max_len: int = 256,
                 batch_size: int = 64, sparse_encoder=None, domain_dim: Optional[int] = None):
        super().__init__(config, device, dtype, seed, max_len, batch_size)
        self.module = _seeded(lambda: _SentenceModule(self.config), seed).to(self.device, self.dtype).eval()
        self.dim = self.config.hidden
        self.sparse_encoder = sparse_encoder
        self.domain_dim = domain_dim or self.dim

    @torch.inference_mode()
    def encode_to_device(self, texts: Sequence[str], batch_size: Optional[int] = None) -> torch.Tensor:
        """float32 [n, dim] tensor on the encoder's device (feeds hr_add_dense_raw_dev / search without a host hop).
        batch_size overrides the encoder's own (the batching front encodes the queries of a round in ONE forward)."""
        out = []
        step = batch_size or self.batch_size
        self.forwards = getattr(self, "forwards", 0)
        for i in range(0, len(texts), step):
            ids, types, mask = self.tokenizer.batch(texts[i: i + step], device=self.device)
            small = self._forward_replayed(ids, types, mask)
            out.append(small if small is not None else self.module(ids, types, mask))
            self.forwards += 1
        return torch.cat(out) if out else torch.zeros((0, self.dim), device=self.device)

    @torch.inference_mode()
    def encode_domain_to_device(self, texts: Sequence[str], domain: Optional[str] = None) -> torch.Tensor:
        """Device counterpart of encode_domain for a batch: float32 [n, domain_dim] on the encoder's device."""
        v = self.encode_to_device([f"{domain}: {t}" if domain else t for t in texts])
        if self.domain_dim == self.dim:
            return v
        reps = -(-self.domain_dim // self.dim)
        return v.repeat(1, reps)[:, : self.domain_dim].contiguous()

    def encode_semantic_batch(self, texts: Sequence[str]) -> List[np.ndarray]:
        return list(self.encode_to_device(list(texts)).cpu().numpy())

    def encode_semantic(self, text: str) -> np.ndarray:
        return self.encode_semantic_batch([text])[0]

    def encode_domain(self, text: str, domain: Optional[str] = None) -> np.ndarray:
        v = self.encode_semantic(f"{domain}: {text}" if domain else text)
        if self.domain_dim == self.dim:
            return v
        reps = -(-self.domain_dim // self.dim)
        return np.tile(v, reps)[: self.domain_dim].astype(np.float32)

    def encode_sparse(self, text: str):
        if self.sparse_encoder is None:
            raise RuntimeError("no sparse encoder configured (pass sparse_encoder=BM25SparseEncoder(...))")
        return self.sparse_encoder.encode_document(text)

    def encode_sparse_csr(self, texts: Sequence[str]):
        """Batch form of encode_sparse for the ingest path: (indptr int64, indices int32, values float32) of all the texts —
        one launch on the encoder's GPU (hr_bm25_encode_dev) instead of a Python call per chunk."""
        if self.sparse_encoder is None:
            raise RuntimeError("no sparse encoder configured (pass sparse_encoder=BM25SparseEncoder(...))")
        dev = torch.device(self.device)
        return self.sparse_encoder.encode_documents_csr(texts, device=dev if dev.type == "cuda" else None)

    def encode_sparse_query(self, text: str):
        if self.sparse_encoder is None:
            raise RuntimeError("no sparse encoder configured")
        return self.sparse_encoder.encode_query(text)


class _CrossModule(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.encoder = BertEncoder(c)
        self.head = nn.Linear(c.hidden, 1)

    def forward(self, ids, types, mask, all_tokens_last_layer: bool = False):
        """Relevance logit per pair from token 0.  The last layer is computed for token 0 only (what the head reads);
        all_tokens_last_layer=True runs it over every token, as a generic encoder would — the same logits (tests)."""
        return self.head(self.encoder(ids, types, mask, first_token_only=not all_tokens_last_layer)[:, 0]).squeeze(-1).float()


class CrossEncoderModel(_Base):
    """`CrossEncoderReranker.model`: predict([(query, document), ...]) -> float32 array of relevance logits."""
    GRAPH_BATCHES, GRAPH_WIDTHS = (1, 4, 8, 12, 16, 20, 24, 32), (64, 128, 256, 512)   # the 20 pairs of one rerank, mostly

    def __init__(self, config: Optional[EncoderConfig] = None, device=None, dtype=None, seed: int = 1, max_len: int = 512,
                 batch_size: int = 64):
        super().__init__(config, device, dtype, seed, max_len, batch_size)
        self.module = _seeded(lambda: _CrossModule(self.config), seed).to(self.device, self.dtype).eval()

    @torch.inference_mode()
    def predict_to_device(self, pairs: Sequence[Tuple[str, str]]) -> torch.Tensor:
        out = []
        for i in range(0, len(pairs), self.batch_size):
            chunk = pairs[i: i + self.batch_size]
            ids, types, mask = self.tokenizer.batch([q for q, _ in chunk], [d for _, d in chunk], device=self.device)
            small = self._forward_replayed(ids, types, mask)
            out.append(small if small is not None else self.module(ids, types, mask))
        return torch.cat(out) if out else torch.zeros(0, device=self.device)

    def predict(self, pairs: Sequence[Tuple[str, str]]) -> np.ndarray:
        return self.predict_to_device(list(pairs)).cpu().numpy()

    def flops_per_pair(self, seq_len: int, executed: bool = True) -> float:
        """Arithmetic of one pair's forward: per token and layer 8 H^2 + 4 H I for the projections and the FFN, plus
        4 T H per token for the attention products.  executed=True (what `predict` runs): the last layer computes keys
        and values for every token and the rest for token 0 only; executed=False: every layer over every token."""
        c = self.config
        H, I, T = c.hidden, c.intermediate, seq_len
        per_layer = 2 * T * (4 * H * H + 2 * H * I) + 4 * T * T * H
        if not executed:
            return float(c.layers * per_layer)
        last = 2 * T * (2 * H * H) + 2 * (2 * H * H + 2 * H * I) + 4 * T * H
        return float((c.layers - 1) * per_layer + last)
