"""MMR on the device: hr_mmr_select_dev (csrc/mmr.h) against oracle.mmr / HybridRetriever._mmr_diversify — positions
and counts exactly — and the one-round path of a manager created with mmr_on_device=True against the general path of one
created without, hit dict for hit dict."""
import asyncio
import json
import os

import numpy as np
import pytest

import g5_data
import oracle
from advanced_rag import _native as nat
from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag.columns import TokenSetColumn
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ("semantic", "sparse", "domain")


def gold(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def method_names(mask):
    return sorted(n for bit, n in enumerate(NAMES) if (int(mask) >> bit) & 1)


@pytest.fixture()
def long_timeout():
    old = RetrievalConstants.TIMEOUT_SECONDS
    RetrievalConstants.TIMEOUT_SECONDS = 60.0
    yield
    RetrievalConstants.TIMEOUT_SECONDS = old


# --------------------------------------------------------------------------- the kernel alone
def mmr_dev(lists, column, lambdas, k_out, k_in=None, first_row=0):
    """lists: per query (ids, float64 scores).  column: TokenSetColumn over rows first_row .. (or None: no rows).
    -> (positions per query as lists, cut to d_out_n; d_out_n; the raw [B][k_out] positions)."""
    dev = torch.device("cuda", 0)
    B = len(lists)
    k_in = k_in or max(1, max(len(i) for i, _ in lists))
    ids = np.full((B, k_in), -1, dtype=np.int64)
    sc = np.zeros((B, k_in), dtype=np.float64)
    n = np.zeros(B, dtype=np.int32)
    for q, (i, s) in enumerate(lists):
        ids[q, :len(i)], sc[q, :len(i)], n[q] = i, s, len(i)
    d_ids, d_sc, d_n = (torch.from_numpy(a).to(dev) for a in (ids, sc, n))
    d_lam = torch.from_numpy(np.asarray(lambdas, dtype=np.float64)).to(dev)
    rows = len(column) if column is not None else 0
    d_ptr = torch.from_numpy(column.indptr().copy()).to(dev) if rows else None
    d_tok = torch.from_numpy(np.concatenate([column.tokens(), np.zeros(1, np.int32)])).to(dev) if rows else None
    pos = torch.full((B, k_out), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    nat.mmr_select_dev(d_ids.data_ptr(), d_sc.data_ptr(), d_n.data_ptr(), B, k_in, d_ptr.data_ptr() if rows else 0,
                       d_tok.data_ptr() if rows else 0, rows, first_row, d_lam.data_ptr(), k_out, pos.data_ptr(),
                       cnt.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    pos, cnt = pos.cpu().numpy(), cnt.cpu().numpy()
    for q in range(B):
        assert (pos[q, cnt[q]:] == -1).all(), q          # -1 padded behind the selection
    return [pos[q, :cnt[q]].tolist() for q in range(B)], cnt.tolist(), pos


def _column(contents):
    col = TokenSetColumn()
    col.extend(contents)
    return col


def _intern(*lists):
    table = {}
    out = [[table.setdefault(x, len(table)) for x in lst] for lst in lists]
    return out, {v: k for k, v in table.items()}


def test_g11_fuse_cases_through_the_kernel(gpu):
    """The 15 `_fuse_results` + MMR cases the reference produced: oracle.rrf -> upload -> kernel; positions equal
    oracle.mmr, and what they select equals the fixture (ids, float64 scores bit for bit, methods).  One launch per case:
    k_in is the case's own fused length."""
    cases = gold("g11_mmr.json")["fuse"]
    assert len(cases) == 15
    for c in cases:
        (a, b, d), back = _intern(c["semantic"], c["sparse"], c["domain"])
        ids, scores, methods = oracle.rrf(a, b, d, c["dense_weight"], c["sparse_weight"], 0.2, 60)
        contents = [c["content"][back[r]] for r in range(len(back))]       # row r of the column = interned id r
        want = oracle.mmr(ids, [float(s) for s in scores], [contents[int(r)] for r in ids], c["top_k"], c["mmr_lambda"])
        k_out = min(c["top_k"], len(ids))
        got, cnt, _ = mmr_dev([(ids, scores)], _column(contents), [c["mmr_lambda"]], k_out)
        assert got[0] == want and cnt[0] == len(want), c["label"]
        assert [back[int(ids[i])] for i in got[0]] == c["ids"], c["label"]
        assert [float(scores[i]).hex() for i in got[0]] == c["scores"], c["label"]
        assert [method_names(methods[i]) for i in got[0]] == c["methods"], c["label"]


def test_one_launch_mixed_lengths_lambdas_and_set_sizes(gpu):
    """B = 7 in one launch: n = 0 .. 160 (k_in = 160: three strides of the block's 64-lane waves and a partial one),
    lambda 0 .. 1.5, k_out = 40.  Ordinary rows draw up to 12 tokens from a 40-token vocabulary (heavy overlaps, equal
    similarities); the rows with the set sizes at the wave edges (63, 64, 65, 129, 130) are prefixes of that vocabulary
    extended to 130 words, so they nest; sizes 0 and 1, two rows with identical contents, exact duplicates among the
    scores, and two ids outside the column (before first_row and behind its last row: the empty set)."""
    rng = np.random.default_rng(11)
    vocab = [f"w{i}" for i in range(130)]
    special = [0, 1, 63, 64, 65, 129, 130]
    contents = [" ".join(vocab[:s]) for s in special]
    for _ in range(200 - len(special)):
        contents.append(" ".join(rng.choice(vocab[:40], size=int(rng.integers(0, 13))).tolist()))
    contents[50] = contents[51] = "w3 w1 w4 w1 w5 W9"             # identical contents: similarity 1
    col = _column(contents)
    assert sorted({len(col.row(r)) for r in range(len(special))}) == special
    first_row = 1000
    outside = [first_row - 1, first_row + len(contents)]
    ns = [0, 1, 2, 63, 64, 65, 160]
    lams = [0.0, 0.3, 0.5, 0.7, 0.8, 1.0, 1.5]
    levels = np.array([1.0 / (60 + r) * w for r in range(1, 9) for w in (0.7, 0.3)])     # few values: exact duplicates
    lists, want = [], []
    for n, lam in zip(ns, lams):
        if n >= 63:        # the special rows, the twins and the two strangers are in every long list
            must = list(range(len(special))) + [50, 51]
            rest = [r for r in rng.permutation(len(contents)).tolist() if r not in must][:n - len(must) - 2]
            ids = rng.permutation(np.array([first_row + r for r in must + rest] + outside, dtype=np.int64))
        else:
            ids = rng.permutation(len(contents))[:n].astype(np.int64) + first_row
        assert len(ids) == n == len(set(ids.tolist()))
        scores = np.sort(rng.choice(levels, size=n))[::-1].copy()
        assert n < 3 or len(set(scores.tolist())) < n
        text = [contents[i - first_row] if 0 <= i - first_row < len(contents) else "" for i in ids.tolist()]
        lists.append((ids, scores))
        want.append(oracle.mmr(ids.tolist(), scores.tolist(), text, 40, lam))
    got, cnt, _ = mmr_dev(lists, col, lams, 40, k_in=160, first_row=first_row)
    assert cnt == [min(40, n) for n in ns]
    for q in range(len(ns)):
        assert got[q] == want[q], (ns[q], lams[q])


@pytest.mark.parametrize("n,k_out,max_tokens", [(768, 32, 8), (256, 256, 4)])
def test_widest_list_and_longest_selection(gpu, n, k_out, max_tokens):
    """k_in = n = 3 * HR_MAX_TOPK (every LDS entry in use, three candidates per thread) and a selection as long as the
    list (every candidate selected, the last steps with a handful of live entries)."""
    rng = np.random.default_rng(n)
    vocab = [f"t{i}" for i in range(24)]
    contents = [" ".join(rng.choice(vocab, size=int(rng.integers(0, max_tokens + 1))).tolist()) for _ in range(n)]
    ids = rng.permutation(n).astype(np.int64)
    scores = np.sort(rng.choice(np.array([1.0 / (60 + r) for r in range(1, 200)]), size=n))[::-1].copy()
    want = oracle.mmr(ids.tolist(), scores.tolist(), [contents[i] for i in ids.tolist()], k_out, 0.5)
    got, cnt, _ = mmr_dev([(ids, scores)], _column(contents), [0.5], k_out)
    assert cnt == [k_out] and got[0] == want


def _diversify_positions(scores, contents, k, lam):
    ranked = [{"pos": i, "score": float(s), "content": c} for i, (s, c) in enumerate(zip(scores, contents))]
    return [r["pos"] for r in HybridRetriever._mmr_diversify(ranked, k, lam)]


def test_corners_against_the_packages_own_diversify(gpu):
    """Where the reference's loop would append None (no candidate above -1e9) this package stops; the kernel does too."""
    contents = ["a b c", "a b", "c d", "", "a b c", "e"]
    col = _column(contents)
    ids = np.arange(6, dtype=np.int64)
    # all scores <= -1e9: nothing is selected
    low = np.array([-1e9, -2e9, -1e9, -1e12, -np.inf, -1e9])
    got, cnt, _ = mmr_dev([(ids, low)], col, [0.5], 4)
    assert cnt == [0] and got[0] == _diversify_positions(low, contents, 4, 0.5) == []
    # lambda = NaN: the first pick is by score alone, then every value is NaN and the selection stops
    sc = np.array([0.3, 0.9, 0.9, 0.1, 0.2, 0.05])
    got, cnt, _ = mmr_dev([(ids, sc)], col, [float("nan")], 4)
    assert cnt == [1] and got[0] == _diversify_positions(sc, contents, 4, float("nan")) == [1]
    # k_out > n: the selection ends with the list
    got, cnt, raw = mmr_dev([(ids[:3], sc[:3])], col, [0.7], 6, k_in=6)
    assert cnt == [3] and got[0] == _diversify_positions(sc[:3], contents[:3], 6, 0.7) and raw[0, 3:].tolist() == [-1] * 3
    # a column without rows (a payload-free collection): every set is empty, every similarity 0
    got, cnt, _ = mmr_dev([(ids, sc)], None, [0.5], 6)
    assert got[0] == _diversify_positions(sc, [""] * 6, 6, 0.5) == [1, 2, 0, 4, 3, 5]
    # one candidate below the bar among good ones is never taken, the rest is
    mixed = np.array([0.5, -1e9, 0.4, -3e9, 0.3, 0.2])
    got, cnt, _ = mmr_dev([(ids, mixed)], col, [1.0], 6)
    assert got[0] == _diversify_positions(mixed, contents, 6, 1.0) == [0, 2, 4, 5] and cnt == [4]


def test_argument_errors_launch_nothing(gpu):
    dev = torch.device("cuda", 0)
    B, k = 2, 769
    ids = torch.zeros((B, k), dtype=torch.int64, device=dev)
    sc = torch.zeros((B, k), dtype=torch.float64, device=dev)
    n = torch.full((B,), 4, dtype=torch.int32, device=dev)
    lam = torch.full((B,), 0.5, dtype=torch.float64, device=dev)
    ptr = torch.zeros(2, dtype=torch.int64, device=dev)
    tok = torch.zeros(1, dtype=torch.int32, device=dev)
    pos = torch.full((B, k), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)

    def call(B=B, k_in=8, k_out=4, ptr=ptr.data_ptr(), tok=tok.data_ptr(), rows=1, pos=pos.data_ptr(), cnt=cnt.data_ptr(),
             ids=ids.data_ptr()):
        nat.mmr_select_dev(ids, sc.data_ptr(), n.data_ptr(), B, k_in, ptr, tok, rows, 0, lam.data_ptr(), k_out, pos, cnt, 0)

    with pytest.raises(nat.HbmRagError) as ei:
        call(k_in=769, k_out=4)
    assert ei.value.status == 5                     # HR_ELIMIT
    for bad in (dict(k_out=0), dict(k_out=9), dict(B=0), dict(pos=0), dict(cnt=0), dict(ids=0), dict(k_in=0),
                dict(ptr=0), dict(tok=0), dict(rows=0), dict(rows=-1)):
        with pytest.raises(ValueError):             # HR_EINVAL
            call(**bad)
    torch.cuda.synchronize(dev)
    assert (pos == -7).all().item() and (cnt == -7).all().item()       # nothing ran
    call(k_in=768, k_out=4)                          # the largest list is served (n = 4 of them valid)
    call(ptr=0, tok=0, rows=0)                       # no column: NULL arrays
    torch.cuda.synchronize(dev)
    assert cnt.tolist() == [4, 4]


# --------------------------------------------------------------------------- end to end
def _payload(rows):
    cols = {k: [row[k] for row in rows] for k in ("doc_id", "chunk_index", "token_count", "entropy", "redundancy",
                                                   "domain_density", "timestamp", "metadata_json")}
    return dict(ids=[row["chunk_id"] for row in rows], contents=[row["content"] for row in rows], **cols)


def _manager(dtype, X, csr, with_sparse, mmr_on_device):
    mgr = MilvusIndexManager(semantic_dim=X.shape[1], sparse_dim=g5_data.SPARSE_DIM, dtype=dtype, enable_domain=False,
                             mmr_on_device=mmr_on_device)
    if not with_sparse:
        del mgr.collections["sparse_index"]
    mgr.add_rows(X, csr if with_sparse else None, **_payload([g5_data.payload_row(r) for r in range(X.shape[0])]))
    mgr.finalize()
    return mgr


class _KeyedGen:
    """Embeddings keyed by the trailing query number of the text ("... q<i>"), or one fixed query."""

    def __init__(self, Q, SQ, fixed=None):
        self.Q, self.SQ, self.fixed = Q, SQ, fixed

    def _i(self, text):
        return self.fixed if self.fixed is not None else int(text.rsplit("q", 1)[1])

    def encode_semantic(self, text):
        return self.Q[self._i(text)]

    def encode_sparse(self, text):
        qi, qv = self.SQ[self._i(text)]
        return {"indices": qi.tolist(), "values": qv.astype(float).tolist()}

    def encode_domain(self, text, domain=None):
        return np.zeros(8, np.float32)


def _timeless(hits):
    """The hit dicts without metadata["recency"]: it is 1 / (1 + age in days) at the moment of the call (retrieval.py
    `_finish_fused_hit`), so two calls never give the same float.  Everything else must be equal."""
    out = []
    for h in hits:
        h = dict(h, metadata=dict(h["metadata"]))
        assert 0.0 < h["metadata"].pop("recency") < 1.0
        out.append(h)
    return out


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_g11_retrieve_one_round_equals_general_path_and_reference(gpu, long_timeout, dtype):
    """The 30 retrieve() runs of G11 on a manager that diversifies on the device and on one that does not: the same hit
    dicts (both managers hold the same rows, so the fp16 near-tie caveat against the fp32 reference does not arise between
    them); at float32 also the reference's ids, float64 scores bit for bit, methods and profile."""
    g, X, csr, Q, SQ = g5_data.inputs()
    runs = gold("g11_mmr.json")["retrieve"]
    assert len(runs) == 30
    for with_sparse in (True, False):
        mine = [r for r in runs if r["with_sparse"] == with_sparse]
        pair = {flag: _manager(dtype, X, csr, with_sparse, flag) for flag in (True, False)}
        try:
            outs = {}
            for flag, mgr in pair.items():
                outs[flag] = []
                for run in mine:
                    initialize_caches()
                    mgr.embedding_generator = _KeyedGen(Q, SQ, fixed=run["query"])
                    retr = HybridRetriever(mgr, RetrievalConfig(top_k=20))
                    outs[flag].append(asyncio.run(retr.retrieve("plain statement", profile_hint=run["profile_hint"])))
                    assert (retr.config.enable_mmr, retr.config.mmr_lambda, retr.config.top_k) == (run["enable_mmr"], run["mmr_lambda"], run["top_k"])
            for run, on, off in zip(mine, outs[True], outs[False]):
                assert _timeless(on) == _timeless(off), (with_sparse, run["profile_hint"], run["query"])
                assert len(on) == run["top_k"] and on[0]["metadata"]["retrieval_profile"] == run["profile"]
                if dtype == "float32":
                    assert [o["id"] for o in on] == run["ids"], (with_sparse, run["profile_hint"], run["query"])
                    assert [float(o["score"]).hex() for o in on] == run["scores"]
                    assert [sorted(o["retrieval_methods"]) for o in on] == run["methods"]
            n_mmr = sum(1 for r in mine if r["enable_mmr"])
            if with_sparse:
                on, off = pair[True]._front.stats, pair[False]._front.stats
                assert on["mmr_launches"] == n_mmr > 0 and on["hybrid_launches"] == len(mine)     # MMR rounds are hybrid rounds
                assert off["mmr_launches"] == 0 and off["hybrid_launches"] == len(mine) - n_mmr
                assert pair[True]._dev_tokens is not None and pair[False]._dev_tokens is None
            else:      # no sparse collection: nothing to fuse in one round, both take the general path
                assert pair[True]._front.stats["mmr_launches"] == 0
        finally:
            for mgr in pair.values():
                asyncio.run(mgr.close())


def _more_queries(D, n, seed):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, D)).astype(np.float32)
    SQ = [((np.arange(100) * 100 + rng.integers(0, 100, size=100)).astype(np.int32),
           np.abs(rng.standard_normal(100)).astype(np.float32)) for _ in range(n)]
    return Q, SQ


def test_concurrent_mmr_requests_share_rounds(gpu, long_timeout):
    """24 retrieve() calls of one profile in flight at once, each with its own query: the answers of the sequential run,
    from fewer than 24 launches."""
    g, X, csr, _, _ = g5_data.inputs()
    Q, SQ = _more_queries(X.shape[1], 24, seed=2024)
    mgr = _manager("float32", X, csr, True, True)
    try:
        mgr.embedding_generator = _KeyedGen(Q, SQ)
        initialize_caches()
        retr = HybridRetriever(mgr, RetrievalConfig(top_k=20))
        one_by_one = [asyncio.run(retr.retrieve(f"plain statement q{i}", profile_hint="troubleshooting")) for i in range(24)]
        assert mgr._front.stats["mmr_launches"] == 24
        before = mgr._front.stats["mmr_launches"]

        async def burst():
            return await asyncio.gather(*(retr.retrieve(f"plain statement q{i}", profile_hint="troubleshooting") for i in range(24)))

        together = asyncio.run(burst())
        assert [_timeless(o) for o in together] == [_timeless(o) for o in one_by_one]
        assert all(len(o) == 30 for o in together) and len({o[0]["id"] for o in together}) > 1
        assert 0 < mgr._front.stats["mmr_launches"] - before < 24
    finally:
        asyncio.run(mgr.close())


def test_mmr_follows_appends_deletes_and_filters(gpu, long_timeout):
    """The row space moves under the mirror: after a first MMR request 20 rows are appended (ten of them with identical
    contents) that a new query ranks on top, one of them is deleted, and the query runs under a chunk_index filter; every
    answer equals the general path's of a manager that went through the same steps."""
    g, X, csr, Q, SQ = g5_data.inputs()
    N, D = X.shape
    rng = np.random.default_rng(5)
    target = rng.standard_normal(D).astype(np.float32)
    newX = (target[None, :] + 0.05 * rng.standard_normal((20, D))).astype(np.float32)
    t_idx = (np.arange(100) * 100 + 7).astype(np.int32)
    new_csr = (np.arange(21, dtype=np.int64) * 100, np.tile(t_idx, 20), (1.0 + rng.random(2000)).astype(np.float32))
    new_rows = []
    for j in range(20):
        row = g5_data.payload_row(N + j)
        row["content"] = "the same words in ten rows" if j < 10 else f"fresh row {j} with words of its own topic{j % 3}"
        new_rows.append(row)
    Q2 = np.concatenate([Q, target[None, :]])
    SQ2 = SQ + [(t_idx, np.ones(100, np.float32))]
    answers = {}
    for flag in (True, False):
        mgr = _manager("float32", X, csr, True, flag)
        try:
            mgr.embedding_generator = _KeyedGen(Q2, SQ2)
            initialize_caches()
            retr = HybridRetriever(mgr, RetrievalConfig(top_k=20))
            got = [asyncio.run(retr.retrieve("plain statement q0", profile_hint="troubleshooting"))]
            if flag:
                assert mgr._dev_tokens.tensors()[2] == N
            mgr.add_rows(newX, new_csr, **_payload(new_rows))
            mgr.finalize()
            got.append(asyncio.run(retr.retrieve("plain statement q8", profile_hint="troubleshooting")))
            new_ids = {r["chunk_id"] for r in new_rows}
            # the new rows head both lists, so the first pick (by fused score alone) is one of them; behind it the ten
            # twins are worth lambda * score - (1 - lambda) * 1 at best once one of them is in
            victim = got[1][0]["id"]
            assert victim in new_ids
            assert sum(1 for h in got[1] if h["content"] == "the same words in ten rows") <= 1
            asyncio.run(mgr.delete_by_filter("semantic_index", f'chunk_id == "{victim}"'))
            got.append(asyncio.run(retr.retrieve("plain statement q8", profile_hint="analysis", filters={"chunk_index": {"$gte": 3}})))
            assert victim not in {h["id"] for h in got[2]} and all(h["metadata"]["chunk_index"] >= 3 for h in got[2])
            assert any(h["id"] in new_ids for h in got[2])
            if flag:
                assert mgr._front.stats["mmr_launches"] == 3 and mgr._dev_tokens.tensors()[2] == N + 20
                col = mgr._cols.token_sets()
                assert len(col) == N + 20 and col.row(N).tolist() == col.row(N + 9).tolist() != col.row(N + 10).tolist()
                # every row went up once (the seam entry of indptr is written by both uploads)
                assert mgr._dev_tokens.stats["uploaded_bytes"] == col.tokens().nbytes + col.indptr().nbytes + 8
            else:
                assert mgr._front.stats["mmr_launches"] == 0
            answers[flag] = got
        finally:
            asyncio.run(mgr.close())
    for step, (on, off) in enumerate(zip(answers[True], answers[False])):
        assert _timeless(on) == _timeless(off), step
        assert len(on) == 30
