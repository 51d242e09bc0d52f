"""The layer that keeps several query batches on the chip at once, off the good-luck schedule.

A. The two-phase C entry points (hr_hybrid_prep_dev / hr_hybrid_scan_dev / hr_hybrid_finish_dev) at all HR_MAX_SLOTS
   workspace slots: several scans before the first finish, finishes in any order on another stream, prep on a third
   stream, one slot reused with other shapes, refused slots, one modality empty, two callers of the one-call form at
   once.  The contract is "bit-identical to one batch at a time": the reference is the one-shot device forms
   (hr_search_dense_dev, hr_search_sparse_dev), each run alone with the device synchronised before and after; ids,
   score bits and flags are compared exactly, and every list with flag 1 is held to the oracle as well.

B. PipelinedSearchEngine against HybridSearchEngine.search (one batch at a time, synchronised), with the finishing
   stream HELD BACK by a device-side delay, so that a native slot comes round again — with a smaller batch, which
   reallocates nothing — while the batch that used it last still has to be finished.  Only the engine's events can
   make that schedule right; the tests assert the ordering itself and the values.
"""
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag.engine import EngineConfig, HybridSearchEngine, PipelinedSearchEngine, pack_sparse_queries
from test_gpu_engine import corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hbmrag.h")
with open(_HEADER) as _f:
    HR_MAX_SLOTS = int(re.search(r"#define\s+HR_MAX_SLOTS\s+(\d+)", _f.read()).group(1))

D, V, NNZ, Q_NNZ, DROP = 64, 500, 8, 24, 0.2
SENTINEL = -7
# the four batches of A1: (B, k, masked).  B = 3: below the fused finish's threshold; 70: above it; k = 200: C = 304
# candidate groups, the finishing chain; 130: more than one dense scan pass.
A1 = [(3, 10, False), (70, 40, True), (16, 200, False), (130, 40, False)]
ENGINE_KEYS = ("ids", "scores", "flags", "fused_ids", "fused_scores", "fused_methods", "rr_ids", "rr_scores")
CFG = EngineConfig(top_k=20)      # k' = 40 per modality


class Batch:
    """One query batch: host copies for the oracle, device copies for the entry points."""

    def __init__(self, n_rows, B, k, masked, seed):
        rng = np.random.default_rng(seed)
        self.B, self.k = B, k
        self.Q = rng.standard_normal((B, D)).astype(np.float32)
        self.SQ = [(np.sort(rng.choice(V, Q_NNZ, replace=False)).astype(np.int32),
                    np.abs(rng.standard_normal(Q_NNZ)).astype(np.float32)) for _ in range(B)]
        self.mask = np.packbits(rng.random(n_rows) < 0.6, bitorder="little") if masked else None
        p, i, v, self.mx = pack_sparse_queries(self.SQ, DROP)
        self.nnz = len(i)
        self.q = torch.from_numpy(self.Q).cuda()
        self.ptr, self.idx, self.val = torch.from_numpy(p).cuda(), torch.from_numpy(i).cuda(), torch.from_numpy(v).cuda()
        self.dmask = torch.from_numpy(self.mask).cuda() if masked else None
        self.mp = self.dmask.data_ptr() if masked else 0
        self.qargs = (self.q.data_ptr(), self.ptr.data_ptr(), self.idx.data_ptr(), self.val.data_ptr())
        self.sparse = (self.ptr, self.idx, self.val, self.mx)      # what the engines take


class Out:
    """Sentinel-filled [2][B][k] lists and [2][B] flags of one call."""

    def __init__(self, bt):
        self.ids = torch.full((2, bt.B, bt.k), SENTINEL, dtype=torch.int64, device="cuda")
        self.scores = torch.full((2, bt.B, bt.k), float(SENTINEL), dtype=torch.float32, device="cuda")
        self.flags = torch.full((2, bt.B), SENTINEL, dtype=torch.int32, device="cuda")
        self.ptrs = (self.ids.data_ptr(), self.scores.data_ptr(), self.flags.data_ptr())

    def numpy(self):
        return self.ids.cpu().numpy(), self.scores.cpu().numpy(), self.flags.cpu().numpy()

    def untouched(self):
        i, s, f = self.numpy()
        return (i == SENTINEL).all() and (s == float(SENTINEL)).all() and (f == SENTINEL).all()


def prep(h, bt, slot, stream):
    h.hybrid_prep_dev(*bt.qargs, bt.B, bt.nnz, bt.mx, bt.k, slot, stream.cuda_stream)


def scan(h, bt, slot, stream):
    h.hybrid_scan_dev(*bt.qargs, bt.B, bt.nnz, bt.mx, bt.k, slot, stream.cuda_stream, bt.mp)


def finish(h, bt, slot, stream, out):
    h.hybrid_finish_dev(*bt.qargs, bt.B, bt.mx, bt.k, slot, *out.ptrs, stream.cuda_stream, bt.mp)


def one_call(h, bt, stream, out):
    h.search_hybrid_dev(*bt.qargs, bt.B, bt.nnz, bt.mx, bt.k, *out.ptrs, bt.mp, stream.cuda_stream if stream else 0)


def order(after, before):
    """Stream `after` waits for what stream `before` holds now."""
    ev = torch.cuda.Event()
    ev.record(before)
    after.wait_event(ev)


def same_lists(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            and np.array_equal(got[2], want[2]))


class Shard:
    """A finalized hybrid shard with its batches, their one-shot references and their oracle lists, each made once."""

    def __init__(self, n, seed):
        self.n = n
        self.X, self.ptr, self.idx, self.val, _, _ = corpus(n, D, V, NNZ, 1, seed=seed)
        self.X[11] = self.X[n - 3]                      # a tie that straddles candidate groups
        self.h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, V)
        self.h.add_dense(self.X)
        self.h.add_sparse(self.ptr, self.idx, self.val)
        self.h.finalize()
        self._batches, self._refs, self._oracle, self._engine_refs = {}, {}, {}, {}
        self._seq = None

    def batch(self, B, k, masked=False, variant=0):
        key = (B, k, masked, variant)
        if key not in self._batches:
            self._batches[key] = Batch(self.n, B, k, masked, seed=((B * 256 + k) * 2 + masked) * 16 + variant + self.n)
        return self._batches[key]

    def ref(self, bt):
        """The one-shot device forms, each alone between two device synchronisations."""
        if bt not in self._refs:
            out = Out(bt)
            torch.cuda.synchronize()
            self.h.search_dense_dev(bt.q.data_ptr(), bt.B, bt.k, out.ids[0].data_ptr(), out.scores[0].data_ptr(),
                                    out.flags[0].data_ptr(), bt.mp, 0)
            torch.cuda.synchronize()
            self.h.search_sparse_dev(bt.ptr.data_ptr(), bt.idx.data_ptr(), bt.val.data_ptr(), bt.B, bt.nnz, bt.mx, bt.k,
                                     out.ids[1].data_ptr(), out.scores[1].data_ptr(), out.flags[1].data_ptr(), bt.mp, 0)
            torch.cuda.synchronize()
            self._refs[bt] = out.numpy()
            assert np.isin(self._refs[bt][2], (0, 1)).all()
        return self._refs[bt]

    def oracle_lists(self, bt):
        """Oracle lists of the batch, [2][B][k] ids and scores; one query per task (the C oracle runs without the GIL)."""
        if bt not in self._oracle:
            oracle.lib()

            def one(b):
                di, ds = oracle.dense_search(self.X, bt.Q[b], bt.k, oracle.COSINE, bt.mask)
                si, ss = oracle.sparse_search(self.ptr, self.idx, self.val, bt.SQ[b:b + 1], bt.k, DROP, bt.mask)
                return di[0], si[0], ds[0], ss[0]

            with ThreadPoolExecutor(8) as pool:
                rows = list(pool.map(one, range(bt.B)))
            di, si, ds, ss = (np.stack(col) for col in zip(*rows))
            self._oracle[bt] = (np.stack([di, si]), np.stack([ds, ss]))
        return self._oracle[bt]

    def check(self, bt, out, what):
        """`out` equals the one-shot reference exactly; its proven lists equal the oracle, ids and score bits."""
        got, want = out.numpy(), self.ref(bt)
        assert same_lists(got, want), f"{what}: B={bt.B} k={bt.k} differs from the one-shot forms"
        oi, os_ = self.oracle_lists(bt)
        proven = got[2] == 1
        assert proven[0].any() and proven[1].any(), f"{what}: no proven list, the oracle check would be empty"
        assert np.array_equal(got[0][proven], oi[proven]), f"{what}: proven lists differ from the oracle (ids)"
        assert np.array_equal(got[1][proven].view(np.uint32), os_[proven].view(np.uint32)), \
            f"{what}: proven lists differ from the oracle (scores)"

    # ---- engine side
    def engine_ref(self, bt):
        """HybridSearchEngine.search of the batch alone, synchronised: clones of the compared tensors."""
        if bt not in self._engine_refs:
            if self._seq is None:
                self._seq = HybridSearchEngine(self.h, CFG)
            torch.cuda.synchronize()
            o = self._seq.search(bt.q, bt.sparse)
            torch.cuda.synchronize()
            self._engine_refs[bt] = {k: o[k].clone() for k in ENGINE_KEYS}
            torch.cuda.synchronize()
        return self._engine_refs[bt]


@pytest.fixture(scope="module")
def shards(gpu):
    """main: 20 000 rows (more than one 16 384-doc sparse range, 16-row groups, two-level group selection);
    tiny: 700 rows (fewer groups than candidates: every group is a candidate)."""
    s = {"main": Shard(20000, seed=61), "tiny": Shard(700, seed=62)}
    yield s
    torch.cuda.synchronize()
    for sh in s.values():
        sh.h.close()


# ====================================================================================================== A. native slots
@pytest.mark.parametrize("finish_order", [(3, 1, 0, 2), (0, 1, 2, 3)])
@pytest.mark.parametrize("which", ["main", "tiny"])
def test_four_batches_in_four_slots(shards, which, finish_order):
    """A1: four different batches scanned into slots 0..3 back to back on one stream, finished on another in any order.
    State that should be per slot but lives on the handle, or is shared between slots, shows as another batch's lists."""
    sh = shards[which]
    batches = [sh.batch(*spec) for spec in A1]
    assert len(batches) == HR_MAX_SLOTS
    for bt in batches:
        sh.ref(bt)
    outs = [Out(bt) for bt in batches]
    X, Y = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for slot, bt in enumerate(batches):
        scan(sh.h, bt, slot, X)
    order(Y, X)
    for slot in finish_order:
        finish(sh.h, batches[slot], slot, Y, outs[slot])
    torch.cuda.synchronize()
    for slot, bt in enumerate(batches):
        sh.check(bt, outs[slot], f"slot {slot}")


def test_prep_on_a_third_stream_is_consumed_once(shards):
    """A2: hr_hybrid_prep_dev on its own stream, the scan behind it on another, the finish on a third; the next scan of
    the slot, with no prep call, prepares its own queries (the mark was consumed) instead of scanning with the old ones."""
    sh = shards["main"]
    U, W = sh.batch(70, 40, True), sh.batch(3, 10)
    sh.ref(U), sh.ref(W)
    out_u, out_w = Out(U), Out(W)
    P, X, Y = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    prep(sh.h, U, 2, P)
    order(X, P)
    scan(sh.h, U, 2, X)
    order(Y, X)
    finish(sh.h, U, 2, Y, out_u)
    order(X, Y)                      # the slot is free again once U is finished
    scan(sh.h, W, 2, X)              # no prep call for W
    order(Y, X)
    finish(sh.h, W, 2, Y, out_w)
    torch.cuda.synchronize()
    sh.check(U, out_u, "prepared batch")
    sh.check(W, out_w, "unprepared batch after a prepared one")


def test_prep_mark_is_per_slot(shards):
    """A2: a prep of slot 1 must not make the scan of slot 3 skip its own query preparation."""
    sh = shards["main"]
    U, W = sh.batch(70, 40, True), sh.batch(16, 200)
    sh.ref(U), sh.ref(W)
    out_u, out_w = Out(U), Out(W)
    P, X, Y = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    prep(sh.h, U, 1, P)
    scan(sh.h, W, 3, X)              # unprepared, another slot
    order(X, P)
    scan(sh.h, U, 1, X)
    order(Y, X)
    finish(sh.h, W, 3, Y, out_w)
    finish(sh.h, U, 1, Y, out_u)
    torch.cuda.synchronize()
    sh.check(W, out_w, "unprepared slot 3")
    sh.check(U, out_u, "prepared slot 1")


@pytest.mark.parametrize("which", ["main", "tiny"])
def test_one_slot_changing_shapes(shards, which):
    """A3: slot 0 with B = 16, 130, 3, 16 and k = 40, 10, 200, 40, each scan behind the previous finish: the workspace
    grows, a smaller batch follows a larger one, C changes with k, one batch takes two scan passes.  Rows of an earlier,
    larger batch must never show."""
    sh = shards[which]
    batches = [sh.batch(16, 40), sh.batch(130, 10), sh.batch(3, 200), sh.batch(16, 40, variant=1)]
    for bt in batches:
        sh.ref(bt)
    outs = [Out(bt) for bt in batches]
    X, Y = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for bt, out in zip(batches, outs):
        order(X, Y)
        scan(sh.h, bt, 0, X)
        order(Y, X)
        finish(sh.h, bt, 0, Y, out)
    torch.cuda.synchronize()
    for step, (bt, out) in enumerate(zip(batches, outs)):
        sh.check(bt, out, f"step {step}")


def test_refused_slots_touch_nothing(shards):
    """A4: slots -1 and HR_MAX_SLOTS are refused by prep, scan and finish alike, the outputs keep their sentinels, and
    the slots next to the refused numbers still give the right lists."""
    sh = shards["main"]
    bt = sh.batch(16, 200)
    sh.ref(bt)
    s = torch.cuda.Stream()
    bad_out = Out(bt)
    good = {0: Out(bt), HR_MAX_SLOTS - 1: Out(bt)}
    torch.cuda.synchronize()
    for slot in (-1, HR_MAX_SLOTS):
        with pytest.raises(ValueError):
            prep(sh.h, bt, slot, s)
        with pytest.raises(ValueError):
            scan(sh.h, bt, slot, s)
        with pytest.raises(ValueError):
            finish(sh.h, bt, slot, s, bad_out)
    torch.cuda.synchronize()
    assert bad_out.untouched()
    for slot, out in good.items():
        scan(sh.h, bt, slot, s)
        finish(sh.h, bt, slot, s, out)
    torch.cuda.synchronize()
    for slot, out in good.items():
        sh.check(bt, out, f"slot {slot} after the refused calls")


@pytest.mark.parametrize("empty", ["sparse", "dense"])
def test_one_modality_empty(shards, empty):
    """A5: a handle with a sparse dimension but no sparse rows, and one with no dense rows: the two-phase forms give,
    bit for bit, what hr_search_hybrid_dev gives on the same handle; the empty half is all padding."""
    sh = shards["main"]
    n = 5000
    h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, V)
    if empty == "sparse":
        h.add_dense(sh.X[:n])
    else:
        h.add_sparse(sh.ptr[:n + 1], sh.idx[:sh.ptr[n]], sh.val[:sh.ptr[n]])
    h.finalize()
    assert (h.num_rows, h.num_sparse_rows) == ((n, 0) if empty == "sparse" else (0, n))
    s = torch.cuda.Stream()
    half = 1 if empty == "sparse" else 0
    for slot, (B, k) in ((1, (16, 40)), (3, (70, 40))):    # one batch for the finishing chain, one for the fused kernel
        bt = Batch(n, B, k, False, seed=500 + B)
        want, got = Out(bt), Out(bt)
        torch.cuda.synchronize()
        one_call(h, bt, None, want)
        torch.cuda.synchronize()
        scan(h, bt, slot, s)
        finish(h, bt, slot, s, got)
        torch.cuda.synchronize()
        w, g = want.numpy(), got.numpy()
        assert same_lists(g, w)
        assert (g[0][half] == -1).all() and (g[1][half].view(np.uint32) == 0).all()
        assert np.array_equal(g[2][half], w[2][half])            # the flag value is the one-call form's
        assert (g[0][1 - half][:, 0] >= 0).all()                  # the other half found rows
    h.close()


def test_two_callers_of_the_one_call_form(shards):
    """A6: two streams run hr_search_hybrid_dev on the same handle, enqueued alternately from the host, three rounds,
    each with its own batch and outputs: every result equals the serial one."""
    sh = shards["main"]
    U, W = sh.batch(70, 40, True), sh.batch(130, 40)
    sh.ref(U), sh.ref(W)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [(Out(U), Out(W)) for _ in range(3)]
    torch.cuda.synchronize()
    for out_u, out_w in outs:
        one_call(sh.h, U, s1, out_u)
        one_call(sh.h, W, s2, out_w)
    torch.cuda.synchronize()
    for r, (out_u, out_w) in enumerate(outs):
        sh.check(U, out_u, f"round {r}, first caller")
        sh.check(W, out_w, f"round {r}, second caller")


# ============================================================================================================ B. engine
DELAY_MS = 50.0


@pytest.fixture(scope="module")
def delay_cycles(gpu):
    """torch.cuda._sleep cycles for about DELAY_MS, calibrated once with events."""
    s = torch.cuda.Stream()

    def timed(cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
        b.synchronize()
        return max(a.elapsed_time(b), 1e-3)

    timed(1000)                                   # first launch
    n = 1_000_000
    ms = timed(n)
    if ms < 5.0:                                  # too short to scale from: aim at 10 ms and measure again
        n = int(n * 10.0 / ms)
        ms = timed(n)
    cycles = int(n * DELAY_MS / ms)
    print(f"\n[batches in flight] delay calibration: {n} cycles took {ms:.3f} ms -> {cycles} cycles for {DELAY_MS} ms")
    return cycles


def _held_back(sh, cycles, depth, prep_stream, hook_mode=None):
    """The ordering schedule: `depth` batches of 64 fill the slots, then a batch of 16 lands in the first batch's slot
    (no reallocation anywhere: every buffer has been sized by an undelayed pass of the same schedule), all submitted
    while the light stream sits behind a delay.  Returns nothing; asserts premise, ordering and values."""
    pipe = PipelinedSearchEngine(sh.h, CFG, depth=depth, prep_stream=prep_stream)
    calls, seen = [], []
    if hook_mode is not None:
        def hook(b):
            calls.append(b)
            seen.append(b["fused_ids"].clone())
        pipe.post_hook = hook
        pipe.post_hook_exclusive = hook_mode == "exclusive"
    batches = [sh.batch(64, 40, variant=i) for i in range(depth)] + [sh.batch(16, 40)]
    want = [sh.engine_ref(bt) for bt in batches]
    try:
        # undelayed pass: sizes every native workspace and creates every buffer set; 2 * depth submits, so that the
        # delayed pass starts at slot 0 again
        for bt in batches + batches[1:depth]:
            pipe.submit(bt.q, bt.sparse)
        pipe.synchronize()
        torch.cuda.synchronize()
        del calls[:], seen[:]
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(pipe.light):
            t0.record()
            torch.cuda._sleep(cycles)
            t1.record()
        outs, got = [], []
        for bt in batches:                       # no synchronisation from here to the premise
            o = pipe.submit(bt.q, bt.sparse)
            outs.append(o)
            with torch.cuda.stream(pipe.light):
                got.append({k: o[k].clone() for k in ENGINE_KEYS})
        first, last = outs[0], outs[-1]
        assert first is not last
        # (a) premise: the first batch is still unfinished when its slot has been handed to the last one
        premise = not first["done"].query()
        assert premise, "the delay did not hold the first batch's finish back: the schedule under test did not happen"
        # (b) ordering: when the scan of the slot's next batch has completed, the first batch is done
        deadline = time.monotonic() + 5.0
        while not last["scan_done"].query():
            assert time.monotonic() < deadline, "the last batch's scan did not complete"
        ordered = first["done"].query()
        pipe.synchronize()
        wrong = [(i, k) for i, (w, g) in enumerate(zip(want, got)) for k in ENGINE_KEYS if not torch.equal(w[k], g[k])]
        print(f"\n[batches in flight] depth={depth} prep={prep_stream} hook={hook_mode}: premise held, "
              f"delay {t0.elapsed_time(t1):.1f} ms, ordered={ordered}, wrong (batch, tensor)={wrong}")
        assert ordered, "slot reused: the scan of the next batch completed before the previous batch was done"
        # (c) values
        assert not wrong, f"(batch, tensor) that differ from the sequential engine: {wrong}"
        if hook_mode is not None:
            assert len(calls) == len(outs) and all(c is o for c, o in zip(calls, outs)), "one hook per batch, in order"
            for i, (w, s) in enumerate(zip(want, seen)):
                assert torch.equal(w["fused_ids"], s), f"hook of batch {i} saw other fused ids"
    finally:
        pipe.close()                             # synchronises: a failed schedule leaves nothing in flight


@pytest.mark.parametrize("prep_stream", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_slot_reused_by_a_smaller_batch_while_its_finish_is_held_back(shards, delay_cycles, depth, prep_stream):
    """B1.  On the engine that waited for the (slot, B) buffer set's own event only, the B = 16 batch scanned into the
    slot while the B = 64 batch before it was still to be finished: run once against that engine, all eight cases
    failed the ordering assertion, and every compared tensor of the first batch differed from the sequential engine."""
    _held_back(shards["main"], delay_cycles, depth, prep_stream)


@pytest.mark.parametrize("hook_mode", ["inline", "exclusive"])
@pytest.mark.parametrize("depth", [2, 3])
def test_held_back_schedule_with_a_post_hook(shards, delay_cycles, depth, hook_mode):
    """B2.  In exclusive mode `done` is recorded behind the deferred hook; the slot rule has to hold with that event."""
    _held_back(shards["main"], delay_cycles, depth, False, hook_mode)


@pytest.mark.parametrize("depth", [1, 4])
def test_mixed_sizes_at_depth_1_and_4(shards, depth):
    """B3: mixed batch sizes with the prep stream and no delay, at the two depths no other test uses; one batch is held
    to the oracle itself."""
    sh = shards["main"]
    sizes = (16, 64, 16, 130, 3, 64, 16)
    count = {}
    batches = []
    for B in sizes:
        batches.append(sh.batch(B, 40, variant=count.get(B, 0)))
        count[B] = count.get(B, 0) + 1
    assert len(set(batches)) == len(sizes)
    want = [sh.engine_ref(bt) for bt in batches]
    pipe = PipelinedSearchEngine(sh.h, CFG, depth=depth, prep_stream=True)
    got = []
    for bt in batches:
        o = pipe.submit(bt.q, bt.sparse)
        with torch.cuda.stream(pipe.light):
            got.append({k: o[k].clone() for k in ENGINE_KEYS})
    pipe.synchronize()
    for i, (w, g) in enumerate(zip(want, got)):
        for k in ENGINE_KEYS:
            assert torch.equal(w[k], g[k]), f"batch {i} (B={sizes[i]}): {k}"
    bt, g = batches[3], got[3]                  # the two-pass batch against the oracle
    oi, os_ = sh.oracle_lists(bt)               # k' = 2 * top_k lists of both modalities, unmasked
    assert g["flags"].min().item() == 1
    assert np.array_equal(g["ids"].cpu().numpy(), oi)
    assert np.array_equal(g["scores"].cpu().numpy().view(np.uint32), os_.view(np.uint32))
    pipe.close()
