"""Case builders and references for the kernels in FRONT of the scan: bm25_encode_kernel and hash_tokenize_kernel
(csrc/text.h), add_layernorm_f16_kernel and embed_layernorm_f16_kernel (csrc/encoder_ops.h).  tests/test_gpu_text_front_edges.py
runs them on the GPU; tests/test_text_front_refs_host.py shows on the CPU that every builder produces what it claims.
Nothing here needs a device: numpy, zlib and the package's own host encoders (the references the kernels restate).

TEXT.  A document is `bytes` (a str is its ASCII / UTF-8 encoding); a batch is packed back to back with NO separator, as the
entry points take it.  The references are BM25SparseEncoder.encode_document and HashTokenizer.encode / .batch on the host,
bit for bit.  Words for chosen slots are found by a crc32 search over the candidates w0, w1, ...

LAYERNORM.  The reference is fp64 LayerNorm of the fp16-ROUNDED sum (one rounding per fp16 add, done in numpy from the exact
fp64 sum); the embedding kernel's sum is the chain fp16(fp16(word + pos) + seg).  Accuracy is judged by
encoder_refs.yardstick_ok against the unfused fp16 path on the same GPU — no tolerance is fixed here."""
import functools
import re
import zlib
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

INT_SENTINEL = -7
WORD_BYTES = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_")
SPACE_BYTES = frozenset(b"\t\n\x0b\x0c\r \x1c\x1d\x1e\x1f")
# both neighbours of every edge of the byte classes: '/' 0..9 ':'   '@' A..Z '['   '_' '`' a..z '{'
CLASS_EDGE_BYTES = tuple(b"/09:@AZ[_`az{")
_BM25_WORD = re.compile(r"\b\w+\b")
_TOK = re.compile(r"\w+|[^\w\s]")

# 7 documents, 22 tokens: avgdl = 22 / 7 is no round number
FIT_CORPUS = ("alpha beta gamma", "Beta delta", "gamma gamma gamma epsilon", "one two three four five six",
              "under_score 42", "a b c d", "END.")


def as_bytes(doc) -> bytes:
    return doc if isinstance(doc, bytes) else doc.encode("utf-8")


def pack(docs: Sequence) -> Tuple[bytes, np.ndarray]:
    """-> (the documents' bytes back to back, offsets int64 [n + 1])"""
    raw = [as_bytes(d) for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return b"".join(raw), off


def bm25_tokens(text: str) -> List[str]:
    return _BM25_WORD.findall(text.lower())


def tok_tokens(text: str) -> List[str]:
    return _TOK.findall(text.lower())


def bm25_encoder(sparse_dim: int, k1: float = 1.2, b: float = 0.75):
    from advanced_rag.bm25 import BM25SparseEncoder
    return BM25SparseEncoder(sparse_dim=sparse_dim, k1=k1, b=b).fit(FIT_CORPUS)


def bm25_want(enc, doc) -> Tuple[np.ndarray, np.ndarray]:
    """the host payload of an ASCII document -> (indices int32, weight bits uint32)"""
    p = enc.encode_document(as_bytes(doc).decode("ascii"))
    return np.asarray(p["indices"], dtype=np.int32), np.asarray(p["values"], dtype=np.float32).view(np.uint32)


def bm25_flag(doc, nnz: int, cap: int) -> int:
    """the flag the header documents: 2 = longer than 65 535 bytes or more than cap slots, 1 = a byte >= 0x80"""
    raw = as_bytes(doc)
    if len(raw) > 65535:
        return 2
    if any(c >= 0x80 for c in raw):
        return 1
    return 2 if nnz > cap else 0


# ------------------------------------------------------------------------------------------------- words for slots
def slot_of(word: str, dim: int) -> int:
    return zlib.crc32(word.encode("ascii")) % dim


SEARCH_LIMIT = 2_000_000


@functools.lru_cache(maxsize=None)
def _find(dim: int, slots: Tuple[int, ...]) -> Tuple[Tuple[str, ...], int]:
    wanted = set(slots)
    found: Dict[int, str] = {}
    i = 0
    while len(found) < len(wanted):
        assert i < SEARCH_LIMIT, (dim, slots)
        w = f"w{i}"
        s = zlib.crc32(w.encode("ascii")) % dim
        if s in wanted and s not in found:
            found[s] = w
        i += 1
    return tuple(found[s] for s in slots), i


def words_for_slots(dim: int, slots: Iterable[int]) -> List[str]:
    """the first candidate w<i> of every wanted slot, in the order of `slots`"""
    return list(_find(dim, tuple(slots))[0])


def candidates_searched(dim: int, slots: Iterable[int]) -> int:
    return _find(dim, tuple(slots))[1]


@functools.lru_cache(maxsize=None)
def adjacent_triple(dim: int) -> Tuple[int, Tuple[str, str, str]]:
    """-> (j, words for the slots 2j, 2j + 1 — the two halves of ONE histogram word — and 2j + 2, the next word's low half):
    the first such j among the candidates w0 .. w199999"""
    first: Dict[int, str] = {}
    for i in range(200000):
        w = f"w{i}"
        first.setdefault(zlib.crc32(w.encode("ascii")) % dim, w)
    for j in range((dim - 2) // 2):
        if 2 * j in first and 2 * j + 1 in first and 2 * j + 2 in first:
            return j, (first[2 * j], first[2 * j + 1], first[2 * j + 2])
    raise AssertionError(f"no adjacent slots at {dim}")


# ---------------------------------------------------------------------------------------------------- shared batches
def byte_class_docs() -> List[str]:
    """A1 / B1: for every byte c below 0x80 the documents a<c>b, <c>, <c>a and a<c> (512 documents, in that order)"""
    out = []
    for c in range(128):
        ch = chr(c)
        out += ["a" + ch + "b", ch, ch + "a", "a" + ch]
    return out


SEAM_BATCHES = (
    ["abc", "def", "", "9", "_x", "", "End"],      # no separator anywhere: abcdef9_xEnd would be ONE token
    ["", "abc", "def", ""],                        # an empty first and an empty last document
    ["abc"],                                       # n_docs = 1
    ["x", "y"],
    ["a!", "?b", "", "c"],
)


# ----------------------------------------------------------------------------------------------------------- BM25
LENGTH_EDGE_DIMS = (1000, 65536)
VOCAB_DIMS = (1, 2, 3, 100, 255, 256, 257, 511, 512, 513, 65535, 65536)
EVERY_SLOT_MAX_DIM = 513
CAPS = (1, 4, 64)
CAP_DIM = 1000
PARAMS = ((1.2, 0.75), (0.0, 0.75), (2.0, 0.0), (1.2, 1.0))


def length_edge_docs(dim: int) -> List[str]:
    """A2: 65 535 bytes with 32 768 tokens in one slot (the largest count); 65 535 bytes in one token; 65 536 bytes (handed
    back); 65 535 bytes alternating the words of slots 2j and 2j + 1 with one word of slot 2j + 2."""
    _, (lo, hi, nxt) = adjacent_triple(dim)
    unit = f"{lo} {hi} "
    k = (65535 - len(nxt)) // len(unit)
    alt = unit * k + nxt
    alt += " " * (65535 - len(alt))
    return ["a " * 32767 + "a", "x" * 65535, "a " * 32768, alt]


def corner_slots(dim: int) -> List[int]:
    return sorted({s for s in (0, 1, dim - 2, dim - 1) if 0 <= s < dim})


def vocab_docs(dim: int) -> List[str]:
    """A3: a document on the slots 0, 1, dim - 2, dim - 1 (the k-th of them k + 1 times) and, at dim <= 513, one on EVERY
    slot (slot s 1 + s mod 3 times, words in a scattered order)."""
    corner = words_for_slots(dim, corner_slots(dim))
    docs = [" ".join(" ".join([w] * (k + 1)) for k, w in enumerate(corner))]
    if dim <= EVERY_SLOT_MAX_DIM:
        words = words_for_slots(dim, range(dim))
        order = np.random.default_rng(dim).permutation(dim)
        docs.append(" ".join(" ".join([words[s]] * (1 + s % 3)) for s in order))
    return docs


def vocab_cap(dim: int) -> int:
    return min(dim, EVERY_SLOT_MAX_DIM)


def cap_docs(cap: int) -> List[str]:
    """A4: exactly cap distinct slots, cap + 1, and cap again (the row behind the refused one)"""
    words = words_for_slots(CAP_DIM, range(3, 3 + cap + 1))
    fits = " ".join(words[:cap]) + " " + words[0]
    return [fits, " ".join(words), ", ".join(reversed(words[1:]))]


FLAG_DOCS = ("plain text here", b"\x80", "more words, more Words", b"\xff", "tail_doc 42", b"caf\xc3\xa9 au lait", "z")
PARAM_DOCS = ("alpha", "alpha alpha alpha beta", "one two three four five six seven eight nine ten " * 20, "", "x_1 X_1 x_1!",
              "gamma " * 300)


def flag_docs_blanked() -> List:
    return [d if isinstance(d, str) else "" for d in FLAG_DOCS]


def avgdl_encoders(dim: int):
    """A7: encoders whose avgdl is 1 / 1000 and 5 000 (merge_stats of another rank's counts)"""
    lo, hi = bm25_encoder(dim), bm25_encoder(dim)
    lo.merge_stats(1000, 1, lo.df)
    hi.merge_stats(1, 5000, hi.df)
    return lo, hi


# ------------------------------------------------------------------------------------------------------ tokenizer
TOK_THREADS = 256
EVERY_BYTE_NS = (1, 63, 64, 65, 255, 256, 257, 1000)
SLICE_LENGTHS = (255, 256, 257, 511, 512, 513, 1025)
TRUNC_MAX_LENS = (3, 4, 16, 257, 512)
VOCABS = (1001, 1002, 30522)


def slices_of(length: int) -> List[Tuple[int, int]]:
    """the byte range [b0, b1) of every thread of hash_tokenize_kernel for a text of `length` bytes"""
    per = -(-length // TOK_THREADS)
    return [(min(t * per, length), min(min(t * per, length) + per, length)) for t in range(TOK_THREADS)]


def slice_edge_text(length: int) -> str:
    """B3: slices in groups of four — t = 0 mod 4: letters (a word STARTS on the slice's first byte, the slice before it
    ends in '-'), 1: letters (the same word goes on and ENDS on this slice's last byte), 2: blanks, with '!' inside when
    the slice has three bytes or more, 3: '-' on every byte.  Letters vary with the position so that tokens hash apart."""
    out = []
    for t, (b0, b1) in enumerate(slices_of(length)):
        for i in range(b0, b1):
            kind = t % 4
            if kind < 2:
                out.append(chr(ord("a") + (i * 7 + t) % 26))
            elif kind == 2:
                out.append("!" if b0 < i < b1 - 1 else " ")
            else:
                out.append("-")
    return "".join(out)


def long_word_text(length: int = 1025) -> Tuple[str, int]:
    """-> (text, max_len): four short tokens, then a word longer than three slices that is the LAST token kept at max_len,
    then tokens that are cut off"""
    per = -(-length // TOK_THREADS)
    head = "a! b? "
    word = "q" * (3 * per + 5)
    text = head + word
    text += (" x" * length)[: length - len(text)]
    return text, len(tok_tokens(head)) + 1 + 2


def token_run(n: int) -> str:
    """a text of exactly n tokens: words, with every third token a punctuation mark"""
    return " ".join("#" if i % 3 == 2 else f"t{i}" for i in range(n))


def truncation_texts(max_len: int) -> List[str]:
    room = max_len - 2
    return [token_run(room - 1), token_run(room), token_run(room + 1)]


def tok_rows(tok, texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """-> ([n][max_len] int64: CLS ids SEP then zeros, lens [n]) from HashTokenizer.encode"""
    rows = np.zeros((len(texts), tok.max_len), dtype=np.int64)
    lens = np.zeros(len(texts), dtype=np.int32)
    for i, t in enumerate(texts):
        ids, _ = tok.encode(t)
        rows[i, : len(ids)] = ids
        lens[i] = len(ids)
    return rows, lens


# ------------------------------------------------------------------------------------------------------ LayerNorm
LN_REGIMES = ("unit", "offset_rows", "outlier_dims", "small_variance", "offset_tight")
LN_ROWS, LN_HIDDEN = 37, 384
DISPATCH_CHUNKS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128)
ROW_EDGES = (1, 15, 16, 17, 33)
CONSTANTS = (0.0, 2.0, -0.5, 0.1, 3.3, 30.0, -30.0)
CONSTANT_WIDTHS = (8, 136, 384, 768, 1024)
EPS_VALUES = (1e-12, 1e-5, 1.0)
NAN_ROW, OVERFLOW_ROW = 5, 22
OVERFLOW_VALUE = 60000.0


def fp16_add(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """ONE round-to-nearest-even fp16 add (the fp64 sum of two fp16 values is exact)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (a.astype(np.float64) + b.astype(np.float64)).astype(np.float16)


def ln_params(hidden: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """gamma U(0.5, 1.5), beta N(0, 0.2), fp16"""
    rng = np.random.default_rng(300 + seed + hidden)
    return rng.uniform(0.5, 1.5, hidden).astype(np.float16), (0.2 * rng.standard_normal(hidden)).astype(np.float16)


def ln_ref(h16: np.ndarray, gamma: np.ndarray, beta: np.ndarray, eps: float) -> np.ndarray:
    """fp64 LayerNorm over the last axis of the fp16-rounded sum (a row with a non-finite value comes out non-finite)"""
    h = h16.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = h.mean(axis=-1, keepdims=True)
        var = ((h - mean) ** 2).mean(axis=-1, keepdims=True)
        return (h - mean) / np.sqrt(var + eps) * gamma.astype(np.float64) + beta.astype(np.float64)


def ln_inputs(regime: str, rows: int = LN_ROWS) -> Tuple[np.ndarray, np.ndarray]:
    """-> (x, res) fp16 [rows][384].  The first four regimes are encoder_refs.tail_inputs with (a, x) as (residual, input).
    `offset_tight`: every row is one of 8, -8, 30, -30 plus -3 .. 3 fp16 ulps of it, no residual signal (res = 0): the variance
    (about 4 ulp^2, 1e-3 at 30) is a 1e-6 of the squared mean, where E[x^2] - mean^2 in fp32 has no digit left."""
    import encoder_refs as R
    if regime != "offset_tight":
        a, x = R.tail_inputs(regime, rows)
        return x.numpy().copy(), a.numpy().copy()
    rng = np.random.default_rng(17 + rows)
    c = np.array([8.0, -8.0, 30.0, -30.0])[np.arange(rows) % 4][:, None]
    ulp = 2.0 ** (np.floor(np.log2(np.abs(c))) - 10)
    x = (c + ulp * rng.integers(-3, 4, size=(rows, LN_HIDDEN))).astype(np.float16)
    return x, np.zeros_like(x)


def unit_inputs(rows: int, hidden: int) -> Tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(1000 * rows + hidden)
    return (2 * rng.standard_normal((rows, hidden))).astype(np.float16), rng.standard_normal((rows, hidden)).astype(np.float16)


def constant_rows(hidden: int, rows: int = 17) -> np.ndarray:
    """[rows][hidden] fp16: row r holds CONSTANTS[r mod 7] in every element"""
    c = np.array(CONSTANTS, dtype=np.float16)[np.arange(rows) % len(CONSTANTS)]
    return np.repeat(c[:, None], hidden, axis=1)


def emulated_mean(value: np.float16, hidden: int) -> np.float32:
    """the kernels' mean of a constant row in fp32: lane j sums its elements one by one (chunks j, j + 16, ...), row16_sum
    adds the 16 lanes (rotate by 8, 4, 2, 1), and the total is MULTIPLIED by the rounded 1 / hidden"""
    f32 = np.float32
    chunks = hidden // 8
    lanes = np.zeros(16, dtype=f32)
    for j in range(16):
        s = f32(0)
        for _ in range(len(range(j, chunks, 16)) * 8):
            s = f32(s + f32(value))
        lanes[j] = s
    for r in (8, 4, 2, 1):
        lanes = (lanes + np.roll(lanes, r)).astype(f32)
    return f32(lanes[0] * (f32(1.0) / f32(hidden)))


def poisoned(x: np.ndarray, res: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """C5: row NAN_ROW of x all NaN; row OVERFLOW_ROW 60 000 + 60 000, which is +inf in fp16"""
    x, res = x.copy(), res.copy()
    x[NAN_ROW] = np.nan
    x[OVERFLOW_ROW] = OVERFLOW_VALUE
    res[OVERFLOW_ROW] = OVERFLOW_VALUE
    return x, res


# ------------------------------------------------------------------------------------------------------ embedding
EMBED_SHAPES = ((37, 1), (5, 7), (3, 17), (3, 512))     # (n_seq, T): rows 37, 35, 51 — and 1 536: T = 512 is a multiple of 16
N_WORD, N_POS = 300, 512


def embed_tables(hidden: int, n_seg: int = 2, regime: str = "unit"):
    """-> word [N_WORD][hidden], pos [512][hidden] (all rows distinct), seg [n_seg][hidden], fp16.
    `order`: word N(0, 8), pos and seg N(0, 0.01) — the two orders of the adds round apart in a good share of the elements.
    `order_planted`: word = even integers in [2052, 2116) (fp16 ulp 2), |pos| and |seg| in [0.6, 0.9]: each add alone is below
    half an ulp, so the kernel's chain returns the word row EXACTLY, while word + (pos + seg) moves it by 2 wherever pos and
    seg agree in sign — a hundredth of the row's spread, a tenth of an output unit."""
    rng = np.random.default_rng(500 + hidden + n_seg)
    if regime == "unit":
        scale = (0.5, 0.5, 0.5)
    elif regime == "order":
        scale = (8.0, 0.01, 0.01)
    else:
        word = (2052 + 2 * rng.integers(0, 32, size=(N_WORD, hidden))).astype(np.float16)
        small = lambda n: (rng.uniform(0.6, 0.9, size=(n, hidden)) * rng.choice([-1.0, 1.0], size=(n, hidden))).astype(np.float16)  # noqa: E731
        return word, small(N_POS), small(n_seg)
    return ((scale[0] * rng.standard_normal((N_WORD, hidden))).astype(np.float16),
            (scale[1] * rng.standard_normal((N_POS, hidden))).astype(np.float16),
            (scale[2] * rng.standard_normal((n_seg, hidden))).astype(np.float16))


def embed_ids(n_seq: int, T: int, n_seg: int = 2) -> Tuple[np.ndarray, np.ndarray]:
    """ids over the whole table with 0 and N_WORD - 1 planted, types over every segment"""
    rng = np.random.default_rng(n_seq * 1000 + T)
    ids = rng.integers(0, N_WORD, size=(n_seq, T)).astype(np.int64)
    ids.reshape(-1)[0] = 0
    ids.reshape(-1)[-1] = N_WORD - 1
    return ids, rng.integers(0, n_seg, size=(n_seq, T)).astype(np.int64)


def embed_chain(word, pos, seg, ids, types) -> np.ndarray:
    """fp16(fp16(word + pos) + seg) — the order of the unfused fp16 module and of the kernel"""
    T = ids.shape[1]
    return fp16_add(fp16_add(word[ids], pos[:T][None]), seg[types])


def embed_other_order(word, pos, seg, ids, types) -> np.ndarray:
    """fp16(word + fp16(pos + seg)) — what the kernel must NOT compute"""
    T = ids.shape[1]
    return fp16_add(word[ids], fp16_add(np.broadcast_to(pos[:T][None], word[ids].shape), seg[types]))
