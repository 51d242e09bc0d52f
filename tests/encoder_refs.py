"""References and input builders for the encoder layer kernels (tests/test_gpu_encoder_edges.py on the GPU,
tests/test_encoder_refs_host.py for the builders and the bound themselves).

The three hand-written launches of a layer — linear_rows_kernel, attention_kernel, encoder_tail_kernel (csrc/encoder_layer.h,
csrc/attention.h) — are held to fp64 arithmetic on the same fp16-rounded operands.  Everything here is deterministic, numpy
or CPU PyTorch, and needs no device.

ATTENTION WITH EXACT SCORES.  The entry points take `scale`; with scale = ln 2 the kernel's pre-scale factor
scale * log2(e) rounds to exactly 1.0 in fp16, so integer Q and K give integer scores in log2 units: the pre-scaling is
exact, the fp32 scores are exact, and the fp64 reference 2^s / sum 2^s is well conditioned at any score magnitude.  What
remains of the kernel's error is
  * the round-toward-zero packing of a probability to fp16: at most 2^-10 relative per probability;
  * the fp16 flush of probabilities below 2^-24 of the reference maximum (which is at most the true maximum);
  * fp32 accumulation and the final fp16 rounding (2^-11 relative);
hence, per output element, with p the true probabilities, v the fp16 V and L the sequence's length,

    |got - want| <= 2^-10 sum_j p_ij |v_j| + 2^-11 |want| + L 2^-24 max|v|          (attention_bound)

— derived, not measured.  `attention_emulate` is the kernel's arithmetic in numpy (fp32 scores, the lazy reference maximum
per 32-key chunk with the wave-wide vote, rtz fp16 P, an fp32 sum over the unrounded exponentials, fp32 output
accumulators); the host tests show that it meets the bound on every case the GPU tests use.
"""
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

LN2 = math.log(2.0)            # the softmax scale of every exact-score case: scale * log2(e) == 1.0 in fp16
HEADS = 3                      # odd: the head-pair tail of head dimension 32
V_SCALE = 1.5
LENGTH_EDGES = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129)
PAD_VALUE = 60000.0            # finite in fp16, like the activations of padded tokens in production


# --------------------------------------------------------------------------------------------------- attention cases
@dataclass
class AttnCase:
    name: str
    hd: int
    qkv: np.ndarray                        # [n_seq][T][3][HEADS][hd] fp16
    lengths: np.ndarray                    # [n_seq] int32 (as handed to the kernel: may be <= 0 or > T)
    # (family, sequence, query, {"at": planted key positions, "min_gap": log2 units the planted score must clear})
    planted: List[Tuple[str, int, int, Dict]] = field(default_factory=list)

    @property
    def n_seq(self):
        return self.qkv.shape[0]

    @property
    def T(self):
        return self.qkv.shape[1]

    def live(self) -> np.ndarray:
        """valid keys per sequence as the kernel takes them: min(length, T), nothing below 0"""
        return np.clip(self.lengths, 0, self.T).astype(np.int64)


def _random_qkv(rng, n_seq, T, hd, lo=-2, hi=2):
    qkv = np.empty((n_seq, T, 3, HEADS, hd), dtype=np.float16)
    qkv[:, :, :2] = rng.integers(lo, hi + 1, size=(n_seq, T, 2, HEADS, hd))
    qkv[:, :, 2] = (V_SCALE * rng.standard_normal((n_seq, T, HEADS, hd))).astype(np.float16)
    return qkv


def length_edges_case(hd: int) -> AttnCase:
    """T = 129, one sequence per length in LENGTH_EDGES (0, 1 and both sides of the 16-key tile, the 32-key chunk and the
    128-query block), integer Q and K in [-2, 2]."""
    rng = np.random.default_rng(1000 + hd)
    return AttnCase(f"length_edges_hd{hd}", hd, _random_qkv(rng, len(LENGTH_EDGES), 129, hd),
                    np.array(LENGTH_EDGES, dtype=np.int32))


def poison_padding(case: AttnCase) -> AttnCase:
    """The same case with Q, K and V of every token at or beyond its sequence's length set to +-PAD_VALUE."""
    qkv = case.qkv.copy()
    rng = np.random.default_rng(7)
    for s, n in enumerate(case.live()):
        tail = qkv[s, n:]
        tail[...] = np.where(rng.integers(0, 2, size=tail.shape) == 1, PAD_VALUE, -PAD_VALUE).astype(np.float16)
    return AttnCase(case.name + "_poisoned", case.hd, qkv, case.lengths.copy(), list(case.planted))


def degenerate_lengths_case(hd: int) -> AttnCase:
    """lengths 0 and negative (all-zero rows), above T (= T), and ordinary ones beside them."""
    rng = np.random.default_rng(2000 + hd)
    lengths = np.array([0, -1, -5, -64, -1000, 40 + 100, 40 + 1, 2 ** 31 - 1, 7, 40], dtype=np.int32)
    return AttnCase(f"degenerate_hd{hd}", hd, _random_qkv(rng, len(lengths), 40, hd), lengths)


def copies_case(hd: int, copies: int = 11, T: int = 77, length: int = 70) -> AttnCase:
    """`copies` identical sequences of one length: 11 x 2 head groups is no multiple of 8 (a ragged last XCD group)."""
    rng = np.random.default_rng(3000 + hd)
    one = _random_qkv(rng, 1, T, hd)
    return AttnCase(f"copies_hd{hd}", hd, np.repeat(one, copies, axis=0).copy(), np.full(copies, length, dtype=np.int32))


def lazy_maximum_case(T: int, hd: int) -> AttnCase:
    """Planted keys on top of random integer K, so that for a chosen query of each sequence the score jumps far above
    everything before it in the middle of the sequence (families in the module's test docstrings: a .. e, `equal`, `step`).
    Every family comes at lengths T and T - 63."""
    rng = np.random.default_rng(4000 + 10 * T + hd)
    lens_of = (T, T - 63)
    seqs, lengths, planted = [], [], []

    def new_seq(length):
        seqs.append(_random_qkv(rng, 1, T, hd)[0])
        lengths.append(length)
        return len(seqs) - 1

    def plant(s, query, pos, factor):
        q = seqs[s][query, 0].astype(np.float32)                      # [HEADS][hd]
        seqs[s][pos, 1] = (factor * np.sign(q)).astype(np.float16)

    for length in lens_of:
        mid = 32 * (((length + 31) // 32) // 2) + 6
        # a) one planted key in a middle chunk
        s = new_seq(length)
        plant(s, 17, mid, 8)
        planted.append(("a", s, 17, {"at": [mid], "min_gap": 8}))
        # b) two moves: 8 sign(q) early, 16 sign(q) at the last valid key (the last live chunk)
        s = new_seq(length)
        plant(s, 40, 40, 8)
        plant(s, 40, length - 1, 16)
        planted.append(("b", s, 40, {"at": [40, length - 1], "min_gap": 8}))
        # c) the planted key in chunk 0, nothing above it afterwards: every later probability underflows
        s = new_seq(length)
        plant(s, 3, 7, 8)
        planted.append(("c", s, 3, {"at": [7], "min_gap": 8, "underflow_after": True}))
        # e) a jump of more than 128 log2 units: the first exp2 overflows to +inf before the branch recomputes it
        s = new_seq(length)
        plant(s, 33, mid + 32 if mid + 32 < length else mid, 32)
        planted.append(("e", s, 33, {"at": [mid + 32 if mid + 32 < length else mid], "min_gap": 128}))
        # equal) Q = 0: all scores equal, the output is the mean of V over the valid keys
        s = new_seq(length)
        seqs[s][:, 0] = 0
        planted.append(("equal", s, 0, {"at": [], "min_gap": 0}))
        # step) K = 0 but two keys that lift queries with q[0] = 1 / q[1] = 1 by exactly 9 and 10 log2 units above a flat
        # past: the rescale factor alpha = 2^-9 / 2^-10 multiplies a sum that still carries a fifth of the result
        s = new_seq(length)
        seqs[s][:, 1] = 0
        seqs[s][100, 1, :, 0] = 9
        seqs[s][130, 1, :, 1] = 10
        seqs[s][50, 0, :, :2] = [[1, 0]] * HEADS
        seqs[s][51, 0, :, :2] = [[0, 1]] * HEADS
        seqs[s][52, 0, :, :2] = [[1, 1]] * HEADS
        seqs[s][50:53, 0, :, 2:] = 0
        planted.append(("step", s, 50, {"at": [100], "min_gap": 8, "exact_gap": 9}))
        planted.append(("step", s, 51, {"at": [130], "min_gap": 8, "exact_gap": 10}))
    # d) the planted key at each of the 32 in-chunk positions (4 g + r of both key tiles: every lane group's 8 keys) for
    # ONE query column, so the wave vote and the column maximum are taken from every lane group
    for pos in range(32):
        length = lens_of[pos % 2]
        s = new_seq(length)
        plant(s, 5, 64 + pos, 8)
        planted.append(("d", s, 5, {"at": [64 + pos], "min_gap": 8}))
    return AttnCase(f"lazy_T{T}_hd{hd}", hd, np.stack(seqs), np.array(lengths, dtype=np.int32), planted)


LAZY_SHAPES = ((200, 32), (200, 64), (512, 64))


# ----------------------------------------------------------------------------------------- attention reference / bound
def attention_scores(case: AttnCase, seq: int, head: int, n_queries: Optional[int] = None) -> np.ndarray:
    """exact integer scores (log2 units at scale = ln 2) of the first n_queries tokens against every key, fp64"""
    nq = case.T if n_queries is None else n_queries
    q = case.qkv[seq, :nq, 0, head].astype(np.float64)
    k = case.qkv[seq, :, 1, head].astype(np.float64)
    return q @ k.T


def attention_ref(case: AttnCase, n_queries: Optional[int] = None):
    """-> (want, bound): fp64 softmax(scores in log2 units) V over the valid keys as [n_seq][n_queries][HEADS * hd], and the
    bound of the module docstring per element.  Sequences without valid keys: zeros (the kernel's rule), bound 0."""
    nq = case.T if n_queries is None else n_queries
    hd = case.hd
    want = np.zeros((case.n_seq, nq, HEADS * hd))
    bound = np.zeros_like(want)
    for s, L in enumerate(case.live()):
        if L == 0:
            continue
        for h in range(HEADS):
            sc = attention_scores(case, s, h, nq)[:, :L]
            v = case.qkv[s, :L, 2, h].astype(np.float64)
            p = np.exp2(sc - sc.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            w = p @ v
            want[s, :, h * hd:(h + 1) * hd] = w
            bound[s, :, h * hd:(h + 1) * hd] = (2.0 ** -10 * (p @ np.abs(v)) + 2.0 ** -11 * np.abs(w)
                                                + L * 2.0 ** -24 * np.abs(v).max())
    return want, bound


def rtz_fp16(e: np.ndarray) -> np.ndarray:
    """float32 >= 0 -> fp16, rounded toward zero (v_cvt_pkrtz_f16_f32)"""
    with np.errstate(over="ignore"):
        h = e.astype(np.float16)
    h = np.where(np.isinf(h) & np.isfinite(e), np.float16(65504.0), h)
    over = h.astype(np.float32) > e
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def attention_emulate(case: AttnCase, n_queries: Optional[int] = None) -> np.ndarray:
    """The kernel's arithmetic (csrc/attention.h) in numpy -> fp16 [n_seq][n_queries][HEADS * hd].

    A wave owns 32 queries (rows past n_queries repeat the last one); lane group g of a query column holds keys 4 g .. 4 g + 3
    of both 16-key tiles of a chunk.  Per chunk: fp32 scores minus the reference maximum m, masked keys -inf, e = exp2;
    the lane's sum of its eight e.  When any lane of the WAVE has a sum above 256 (and always in chunk 0) every query of
    the wave moves m to the maximum seen so far and rescales its sum and its output by alpha = exp2(-(move)).  P = rtz
    fp16(e); the sum takes the unrounded e; the output accumulates P V in fp32.  At the end out = fp16(o / sum)."""
    f32 = np.float32
    nq = case.T if n_queries is None else n_queries
    hd, T = case.hd, case.T
    nq_pad = -(-nq // 32) * 32
    qi = np.minimum(np.arange(nq_pad), nq - 1)
    grp = np.concatenate([np.arange(16) // 4, np.arange(16) // 4])          # lane group of an in-chunk key position
    out = np.zeros((case.n_seq, nq, HEADS * hd), dtype=np.float16)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        for s, L in enumerate(case.live()):
            live_chunks = (L + 31) // 32
            for h in range(HEADS):
                S = attention_scores(case, s, h, nq)[qi].astype(f32)         # integers: exact in fp32
                S = np.pad(S, ((0, 0), (0, 32 * (-(-T // 32)) - T)))
                V = np.pad(case.qkv[s, :, 2, h].astype(f32), ((0, S.shape[1] - T), (0, 0)))
                m = np.zeros(nq_pad, dtype=f32)
                l = np.zeros((nq_pad, 4), dtype=f32)
                o = np.zeros((nq_pad, hd), dtype=f32)
                for c in range(live_chunks):
                    keys = np.arange(32 * c, 32 * c + 32)
                    sc = S[:, keys] - (m[:, None] if c else f32(0))
                    sc[:, keys >= L] = -np.inf

                    def exps(sc):
                        e = np.exp2(sc).astype(f32)
                        eg = np.stack([e[:, grp == g] for g in range(4)], axis=1)          # [query][g][8]: tile 0's 4, tile 1's 4
                        sum8 = ((eg[..., 0] + eg[..., 1]) + (eg[..., 2] + eg[..., 3])) + ((eg[..., 4] + eg[..., 5]) + (eg[..., 6] + eg[..., 7]))
                        return e, sum8.astype(f32)

                    e, sum8 = exps(sc)
                    vote = np.repeat((sum8.reshape(-1, 32 * 4) > 256).any(axis=1), 32) | (c == 0)
                    if vote.any():
                        mx = sc.max(axis=1)
                        up = np.where(vote, mx if c == 0 else np.maximum(mx, f32(0)), f32(0)).astype(f32)
                        alpha = np.zeros_like(up) if c == 0 else np.exp2(-up).astype(f32)
                        m = up.copy() if c == 0 else (m + up).astype(f32)
                        l = (l * alpha[:, None]).astype(f32)
                        o = (o * alpha[:, None]).astype(f32)
                        sc = (sc - up[:, None]).astype(f32)
                        e, sum8 = exps(sc)
                    p = rtz_fp16(e)
                    l = (l + sum8).astype(f32)
                    o = (o.astype(np.float64) + p.astype(np.float64) @ V[keys].astype(np.float64)).astype(f32)
                lt = ((l[:, 0] + l[:, 1]) + (l[:, 2] + l[:, 3])).astype(f32)
                inv = np.where(lt > 0, f32(1) / lt, f32(0)).astype(f32)
                out[s, :, h * hd:(h + 1) * hd] = (o * inv[:, None]).astype(np.float16)[:nq]
    return out


def valid_query_rows(case: AttnCase, n_queries: Optional[int] = None) -> np.ndarray:
    """[n_seq][n_queries] bool: the query rows below their sequence's length (the rows a caller reads)"""
    nq = case.T if n_queries is None else n_queries
    return np.arange(nq)[None, :] < case.live()[:, None]


def planted_gaps(case: AttnCase):
    """For every planted (family, sequence, query): per head the score at each planted key minus the maximum score over
    the keys before it, in log2 units — what moves the reference maximum — and the largest valid score after it."""
    res = []
    L = case.live()
    for family, s, query, info in case.planted:
        for h in range(HEADS):
            sc = attention_scores(case, s, h)[query, :L[s]]
            gaps = [sc[p] - sc[:p].max() for p in info["at"] if p > 0]
            after = [sc[p] - (sc[p + 1:].max() if p + 1 < L[s] else -np.inf) for p in info["at"]]
            res.append((family, s, query, h, info, gaps, after))
    return res


# --------------------------------------------------------------------------------------------------------- linear rows
LINEAR_K = 384
LINEAR_NS = (1152, 4096, 64)
N_PAIR_ROWS, N_DENSE_ROWS = 32, 32


def linear_weight(n_out: int) -> np.ndarray:
    """W[n][k] = ((7 n + 13 k) mod 2039) - 1019: integers exact in fp16; every column is distinct, and every row together
    with its bias (rows repeat after 2039, linear_bias after 19)"""
    n, k = np.arange(n_out)[:, None], np.arange(LINEAR_K)[None, :]
    return ((7 * n + 13 * k) % 2039 - 1019).astype(np.float64)


def linear_bias(n_out: int) -> np.ndarray:
    """integers in [-9, 9]: |W + bias| and |W[:, k1] - W[:, k2] + bias| stay below 2048, where every integer is an fp16"""
    return ((np.arange(n_out) * 5) % 19 - 9).astype(np.float64)


def linear_exact_rows() -> np.ndarray:
    """[384 + 64][384]: the 384 one-hot rows (output = a column of W + bias: every packed weight element, through the
    device); 32 `pair` rows (+1 at k1, -1 at k2: |result| < 2048, exactly representable); 32 `dense` rows of integers in
    [-3, 3] on 96 of the 384 inputs (every partial sum is an integer below 2^24, exact in the fp32 accumulator, so the
    device result is the ONE fp16 rounding of the exact sum)."""
    rng = np.random.default_rng(11)
    x = np.zeros((LINEAR_K + N_PAIR_ROWS + N_DENSE_ROWS, LINEAR_K))
    x[:LINEAR_K] = np.eye(LINEAR_K)
    for i in range(N_PAIR_ROWS):
        k1, k2 = rng.choice(LINEAR_K, 2, replace=False)
        sign = 1 if i % 2 == 0 else -1
        x[LINEAR_K + i, k1], x[LINEAR_K + i, k2] = sign, -sign
    for i in range(N_DENSE_ROWS):
        cols = rng.choice(LINEAR_K, 96, replace=False)
        x[LINEAR_K + N_PAIR_ROWS + i, cols] = rng.integers(-3, 4, size=96)
    return x


def fp16_exact(a: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return a.astype(np.float16).astype(np.float64) == a


# ---------------------------------------------------------------------------------------------------------- layer tail
TAIL_REGIMES = ("unit", "offset_rows", "outlier_dims", "wide_gelu", "small_variance")
TAIL_ROW_EDGES = (15, 16, 17, 31, 33, 63, 65, 127, 129, 255, 257)


def tail_layer(gelu: str, regime: str = "unit", seed: int = 0):
    """An encoders._Layer (fp32, CPU) with non-trivial LayerNorm parameters and biases, its parameters rounded to fp16
    values: linear weights N(0, 0.05), biases N(0, 0.1), gamma U(0.5, 1.5), beta N(0, 0.2); `wide_gelu`: W_up N(0, 0.3), b_up
    N(0, 2); `small_variance`: b_out = 0."""
    import torch
    from advanced_rag.encoders import EncoderConfig, _Layer
    gen = torch.Generator().manual_seed(100 + seed)
    layer = _Layer(EncoderConfig(gelu=gelu))
    with torch.no_grad():
        for lin in (layer.qkv, layer.out, layer.up, layer.down):
            lin.weight.normal_(0, 0.05, generator=gen)
            lin.bias.normal_(0, 0.1, generator=gen)
        for ln in (layer.ln1, layer.ln2):
            ln.weight.uniform_(0.5, 1.5, generator=gen)
            ln.bias.normal_(0, 0.2, generator=gen)
        if regime == "wide_gelu":
            layer.up.weight.normal_(0, 0.3, generator=gen)
            layer.up.bias.normal_(0, 2.0, generator=gen)
        if regime == "small_variance":
            layer.out.bias.zero_()
        for p in layer.parameters():
            p.copy_(p.half().float())
    return layer.eval()


def tail_inputs(regime: str, rows: int, seed: int = 0):
    """-> (a, x) fp16 CPU tensors [rows][384]: the attention output and the layer input of a regime."""
    import torch
    gen = torch.Generator().manual_seed(200 + seed + 7 * rows)
    a = torch.randn((rows, 384), generator=gen)
    x = torch.randn((rows, 384), generator=gen)
    if regime == "offset_rows":
        c = torch.tensor([8.0, -8.0, 30.0, -30.0])[torch.arange(rows) % 4]
        x = c[:, None] + 0.5 * x
    elif regime == "outlier_dims":
        for d in (5, 190, 383):
            a[:, d] *= 30
            x[:, d] *= 30
    elif regime == "small_variance":
        a = torch.zeros_like(a)
        x = 1e-3 * x
    return a.half(), x.half()


def tail_ref(a, x, layer, eps: Optional[float] = None, return_preact: bool = False):
    """fp64 arithmetic of everything after the attention on the fp16-rounded operands (no intermediate rounding):
    LN2(x1 + W_down gelu(W_up x1 + b_up) + b_down), x1 = LN1(x + W_out a + b_out)."""
    import torch
    F = torch.nn.functional
    d = lambda t: t.detach().cpu().double()   # noqa: E731
    eps = float(layer.ln1.eps) if eps is None else eps
    H = x.shape[-1]
    x1 = F.layer_norm(d(x) + d(a) @ d(layer.out.weight).t() + d(layer.out.bias), (H,), d(layer.ln1.weight), d(layer.ln1.bias), eps)
    pre = x1 @ d(layer.up.weight).t() + d(layer.up.bias)
    h = F.gelu(pre, approximate="tanh" if layer.gelu == "tanh" else "none")
    y = F.layer_norm(x1 + h @ d(layer.down.weight).t() + d(layer.down.bias), (H,), d(layer.ln2.weight), d(layer.ln2.bias), eps)
    return (y, pre) if return_preact else y


def fp16_ulp_at(value: float) -> float:
    """one fp16 ulp at |value| (normal range)"""
    return 2.0 ** (math.floor(math.log2(max(abs(value), 2.0 ** -14))) - 10)


def yardstick_ok(e_k, e_u, want_absmax: float):
    """The project's criterion for a fused path against the unfused fp16 path, both measured against fp64:
    max E_k <= 2 max E_u + u and mean E_k <= 2 mean E_u (u = one fp16 ulp at max|want|).  -> (ok, the four numbers, u)"""
    nums = (float(e_k.max()), float(e_u.max()), float(e_k.mean()), float(e_u.mean()))
    u = fp16_ulp_at(want_absmax)
    return nums[0] <= 2 * nums[1] + u and nums[2] <= 2 * nums[3], nums, u
