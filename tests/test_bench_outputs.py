"""bench.py's plain run and --dump-outputs: the result line of a run without --full, and the last timed step's results
written as .npy files (float32 / float64, at most 64 MB, the same inputs from run to run).  The bench runs in a CHILD
process, as the driver starts it."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float_arrays_and_caps_the_size(tmp_path):
    mod = _bench_module()
    B, top_k, kp = 64, 20, 40
    rng = np.random.default_rng(3)
    b = {"fused_ids": rng.integers(-1, 1 << 40, (B, top_k)), "fused_scores": rng.random((B, top_k)),
         "fused_methods": rng.integers(0, 4, (B, top_k)).astype(np.int32), "fused_n": np.full(B, top_k, np.int32),
         "rr_ids": rng.integers(0, 1 << 40, (B, 5)), "rr_scores": rng.random((B, 5)), "rr_orig": rng.random((B, 5)),
         "list_ids": rng.integers(-1, 1 << 30, (2, B, kp)), "list_scores": rng.random((2, B, kp)).astype(np.float32),
         "agg_flags": np.ones((2, B), np.int32), "ce_scores": rng.random((B, 5)).astype(np.float16),
         "pack": np.zeros(7, np.uint8)}                                   # not a result: not written
    shapes = mod.dump_outputs(str(tmp_path / "all"), b)
    assert set(shapes) == {k for k in b if k != "pack"}
    for name in shapes:
        a = np.load(tmp_path / "all" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and a.shape == b[name].shape
        if np.issubdtype(b[name].dtype, np.integer) or b[name].dtype == np.float64:
            assert a.dtype == np.float64 and np.array_equal(a, b[name])   # ids up to 2^40 survive exactly
        else:
            assert a.dtype == np.float32 and np.array_equal(a, b[name].astype(np.float32))

    # above the cap: a fixed, seeded sample of the queries, the same for every call, under the cap with its row list
    cap = 20_000
    s1 = mod.dump_outputs(str(tmp_path / "s1"), b, max_bytes=cap)
    mod.dump_outputs(str(tmp_path / "s2"), b, max_bytes=cap)
    rows = np.load(tmp_path / "s1" / "query_rows.npy").astype(np.int64)
    assert 0 < len(rows) < B and np.all(np.diff(rows) > 0)
    assert s1["fused_ids"] == (len(rows), top_k) and s1["list_ids"] == (2, len(rows), kp)
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= cap + 128 * len(s1)
    for f in os.listdir(tmp_path / "s1"):
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f))
    assert np.array_equal(np.load(tmp_path / "s1" / "fused_ids.npy"), b["fused_ids"][rows].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "s1" / "list_scores.npy"), b["list_scores"][:, rows])


def _run_bench(args, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_bench_dumps_the_same_last_step_whatever_the_split_of_steps(gpu, tmp_path):
    """Two plain runs whose last timed step is the same batch (warmup 1 + 3 steps, warmup 0 + 4 steps): each line counts
    its own steps and carries none of the --full blocks, and both write the same results, bit for bit."""
    common = ["--gpus", "1", "--rows", "200000", "--batch", "128"]
    a = _run_bench(common + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")])
    b = _run_bench(common + ["--steps", "4", "--warmup", "0", "--dump-outputs", str(tmp_path / "b")])
    for out, steps in ((a, 3), (b, 4)):
        assert out["steps"] == steps and out["full"] is False and out["all_lists_proven_exact"] is True
        assert out["metric"] == "queries_per_sec_hybrid_retrieve" and out["unit"] == "queries/s" and out["dtype"] == "f16"
        assert out["higher_is_better"] is True and out["ms_per_step"] > 0
        assert abs(out["value"] - 128 * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
        for moved in ("parity_gate", "p50_retrieve_ms", "api_concurrent", "config4_full", "finishing_alone"):
            assert moved not in out
        assert out["cpu_baseline"] is None and out["roofline_sparse"] is None
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(da) == set(db) >= {"fused_ids", "fused_scores", "rr_ids", "rr_scores", "list_ids", "list_scores", "agg_flags"}
    for k in da:
        assert da[k].dtype in (np.float32, np.float64) and np.array_equal(da[k], db[k]), k
    assert da["fused_ids"].shape == (128, 20) and da["rr_ids"].shape == (128, 5) and da["list_ids"].shape == (2, 128, 40)
    assert np.all(da["agg_flags"] == 1) and np.all((da["fused_ids"] >= 0) & (da["fused_ids"] < 200000))
    assert np.all(np.diff(da["fused_scores"], axis=1) <= 0)


@pytest.mark.gpu
def test_plain_bench_dump_with_the_deferred_cross_encoder_hook(gpu, tmp_path):
    """With --rerank cross-encoder the hook of the last batch is deferred (engine.post_hook_exclusive): the dump enqueues
    it, so ce_ids / ce_scores are written, while the line still reports the forwards of the timed region only."""
    out = _run_bench(["--gpus", "1", "--rows", "200000", "--batch", "16", "--steps", "2", "--warmup", "1",
                      "--rerank", "cross-encoder", "--ce-seq-len", "32", "--dump-outputs", str(tmp_path / "ce")])
    assert out["cross_encoder"]["forwards_timed"] == 2 and out["cross_encoder"]["pairs_per_step"] == 16 * 20
    d = _load(tmp_path / "ce")
    assert d["ce_ids"].shape == (16, 5) and d["ce_scores"].shape == (16, 5) and d["ce_scores"].dtype == np.float32
    assert np.all(np.isfinite(d["ce_scores"])) and np.all(np.diff(d["ce_scores"], axis=1) <= 0)
    for q in range(16):   # the cross-encoder keeps 5 of the query's fused candidates
        assert set(d["ce_ids"][q].tolist()) <= set(d["fused_ids"][q].tolist())
