"""The references, bounds and case builders of tests/encoder_refs.py, shown on the CPU to have teeth before they go to a
GPU (tests/test_gpu_encoder_edges.py): the numpy emulation of the attention kernel's arithmetic meets the derived bound on
every case the GPU test uses, the planted keys really move the reference maximum the way each family says, the exact
linear-map inputs really are exact, and the layer-tail regimes really reach the value ranges they are named after."""
import numpy as np
import pytest

import encoder_refs as R

torch = pytest.importorskip("torch")


def _attention_cases():
    for hd in (32, 64):
        yield R.length_edges_case(hd), (None, 1, 33)
        yield R.poison_padding(R.length_edges_case(hd)), (None, 1, 33)
        yield R.degenerate_lengths_case(hd), (None, 1)
        yield R.copies_case(hd), (None, 1, 33)
    for T, hd in R.LAZY_SHAPES:
        yield R.lazy_maximum_case(T, hd), (None, 64)


def test_scale_ln2_makes_the_prescale_factor_exactly_one_in_fp16():
    """the kernel multiplies Q by fp16(scale * log2 e) (float arithmetic on the host, csrc/hbmrag.hip): exactly 1 at ln 2"""
    factor = np.float32(np.float32(R.LN2) * np.float32(1.4426950408889634))
    assert np.float16(factor) == np.float16(1.0)
    assert abs(float(factor) - 1.0) < 2.0 ** -12          # not a tie: any fp32 rounding of the product lands on 1.0


def test_rtz_fp16_rounds_toward_zero():
    e = np.array([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 - 2.0 ** -20, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 255.9999, 3e-5],
                 dtype=np.float32)
    got = R.rtz_fp16(e).astype(np.float64)
    assert (got <= e).all() and got[1] == 1.0 and got[2] == 1.0 and got[3] == 1.0 and got[4] == 2.0 ** -24
    assert got[5] == 0.0 and got[6] == 2.0 ** -24 and got[7] == 255.875
    assert ((e - got) <= np.maximum(2.0 ** -10 * e, 2.0 ** -24)).all()


@pytest.mark.parametrize("case,nqs", list(_attention_cases()), ids=lambda v: v.name if isinstance(v, R.AttnCase) else None)
def test_the_emulated_kernel_arithmetic_meets_the_attention_bound(case, nqs):
    """attention_emulate (fp32 scores, lazy reference maximum with the wave vote, rtz fp16 P, fp32 sums) against the fp64
    reference: within the DERIVED bound on every valid query row of every case the GPU test runs — so a GPU failure of the
    same bound is a difference between the kernel and its documented arithmetic, not a bound that was too tight."""
    worst = 0.0
    for nq in nqs:
        want, bound = R.attention_ref(case, nq)
        got = R.attention_emulate(case, nq).astype(np.float64)
        ok = R.valid_query_rows(case, nq)
        assert np.isfinite(got[ok]).all()
        err = np.abs(got - want)[ok]
        assert (err <= bound[ok]).all(), (case.name, nq, float((err / bound[ok]).max()))
        if err.size:
            worst = max(worst, float((err / bound[ok]).max()))
        # sequences without a valid key: zeros
        dead = case.live() == 0
        assert (got[dead] == 0).all() and (want[dead] == 0).all()
    print(f"{case.name}: emulation / bound <= {worst:.3f}")


@pytest.mark.parametrize("T,hd", R.LAZY_SHAPES)
def test_planted_keys_move_the_reference_maximum_as_each_family_says(T, hd):
    case = R.lazy_maximum_case(T, hd)
    assert sorted(set(case.lengths.tolist())) == [T - 63, T]
    seen = set()
    for family, s, query, h, info, gaps, after in R.planted_gaps(case):
        seen.add(family)
        L = int(case.live()[s])
        assert query < L and all(0 <= p < L for p in info["at"])
        if family == "equal":
            sc = R.attention_scores(case, s, h)
            assert (sc == 0).all()
            continue
        # the planted score clears everything before it by more than the family's gap (2^8 in probability = 8 log2 units)
        assert gaps and all(g > info["min_gap"] for g in gaps) or (family == "c" and not gaps), (family, s, h, gaps)
        if "exact_gap" in info:
            assert gaps == [info["exact_gap"]]
        if family == "b":
            assert len(gaps) == 2 and info["at"][1] // 32 == (L - 1) // 32 and info["at"][0] // 32 < info["at"][1] // 32
        if family == "c":
            assert info["at"][0] < 32 and after[0] > 24       # later probabilities are below 2^-24 of the maximum: flushed
            sc = R.attention_scores(case, s, h)[query, :L]
            assert sc[info["at"][0]] - sc[:32].max() == 0     # it is chunk 0's maximum
        if family == "e":
            assert all(g > 128 for g in gaps)                 # exp2 of the first pass overflows fp32
        if family in ("a", "e"):
            assert 0 < info["at"][0] // 32 < (L - 1) // 32 or T - 63 == L   # a middle chunk
    assert seen == {"a", "b", "c", "d", "e", "equal", "step"}
    d_pos = sorted(info["at"][0] % 32 for f, s, q, h, info, *_ in R.planted_gaps(case) if f == "d" and h == 0)
    assert d_pos == list(range(32))                            # 4 g + r of both key tiles, every lane group
    assert len({q for f, s, q, *_ in R.planted_gaps(case) if f == "d"}) == 1   # one query column


def test_equal_scores_give_the_mean_of_v():
    case = R.lazy_maximum_case(200, 32)
    want, _ = R.attention_ref(case)
    for family, s, *_ in case.planted:
        if family == "equal":
            L = int(case.live()[s])
            mean = case.qkv[s, :L, 2].astype(np.float64).mean(axis=0).reshape(-1)
            assert np.allclose(want[s, :L], mean[None], rtol=0, atol=1e-12)


def test_poisoned_padding_changes_nothing_the_reference_reads():
    for hd in (32, 64):
        clean = R.length_edges_case(hd)
        dirty = R.poison_padding(clean)
        ok = R.valid_query_rows(clean)
        for s, L in enumerate(clean.live()):
            assert np.array_equal(clean.qkv[s, :L], dirty.qkv[s, :L])
            assert (np.abs(dirty.qkv[s, L:].astype(np.float64)) == R.PAD_VALUE).all()
        assert np.array_equal(R.attention_ref(clean)[0][ok], R.attention_ref(dirty)[0][ok])
        # and nothing the kernel's arithmetic reads either: the emulation's valid rows are bitwise the same
        a, b = R.attention_emulate(clean), R.attention_emulate(dirty)
        assert np.array_equal(a[ok].view(np.uint16), b[ok].view(np.uint16))


def test_degenerate_lengths_and_copies_cases():
    case = R.degenerate_lengths_case(32)
    assert (case.lengths[:5] <= 0).all() and (case.lengths[5:8] > case.T).all()
    assert case.live().tolist() == [0, 0, 0, 0, 0, 40, 40, 40, 7, 40]
    c = R.copies_case(64)
    assert c.n_seq == 11 and all(np.array_equal(c.qkv[0], c.qkv[i]) for i in range(11))
    assert (c.n_seq * ((R.HEADS + 1) // 2)) % 8 != 0 and (c.n_seq * R.HEADS) % 8 != 0   # a ragged last XCD group at both head dims


@pytest.mark.parametrize("n_out", R.LINEAR_NS)
def test_linear_exact_inputs_are_exact(n_out):
    w, b, x = R.linear_weight(n_out), R.linear_bias(n_out), R.linear_exact_rows()
    assert R.fp16_exact(w).all() and R.fp16_exact(b).all() and R.fp16_exact(x).all()
    assert len({tuple(r) + (bb,) for r, bb in zip(w.tolist(), b.tolist())}) == n_out and len({tuple(c) for c in w.T.tolist()}) == R.LINEAR_K
    y = x @ w.T + b
    K, P = R.LINEAR_K, R.N_PAIR_ROWS
    assert np.array_equal(y[:K], w.T + b)                                   # one-hot rows: a column of W + bias
    assert R.fp16_exact(y[:K + P]).all() and np.abs(y[:K + P]).max() < 2048   # one-hot and pair rows: every element an fp16
    assert (np.abs(x[K:K + P]).sum(axis=1) == 2).all() and (x[K:K + P].sum(axis=1) == 0).all()
    dense = x[K + P:]
    assert np.abs(dense).max() == 3 and ((dense != 0).sum(axis=1) > 64).all()
    # dense rows: every partial sum in ANY order is bounded by sum |x| |w| + |b| < 2^24 (exact in fp32), the result is finite in fp16
    assert (np.abs(dense) @ np.abs(w).T + np.abs(b)).max() < 2 ** 24 and np.abs(y[K + P:]).max() < 65504
    assert not R.fp16_exact(y[K + P:]).all()                                # ... and they do exercise the final rounding


def test_packed_linear_operands_reproduce_the_product_on_the_cpu():
    """pack_linear's store-order rows and both k orders, unpacked by the documented index formulas, give back W and bias"""
    from advanced_rag.encoder_kernels import pack_linear, store_order_rows
    w, b = torch.from_numpy(R.linear_weight(64)), torch.from_numpy(R.linear_bias(64))
    perm = store_order_rows(64)
    for fr in (False, True):
        wp, bp = pack_linear(w, b, fr)
        v = wp.reshape(4, 12, 4, 16, 8).double()                            # [t][s][g][r][j]
        back = torch.empty(64, 384, dtype=torch.float64)
        for g in range(4):
            for j in range(8):
                kk = (16 * (j >> 2) + 4 * g + (j & 3)) if fr else 8 * g + j
                back[:, kk::32] = v[:, :, g, :, j].permute(0, 2, 1).reshape(64, 12)
        assert torch.equal(back, w[perm]) and torch.equal(bp.double(), b[perm])


@pytest.mark.parametrize("gelu", ["tanh", "erf"])
def test_tail_regimes_reach_the_ranges_they_are_named_after(gelu):
    rows = 200
    stats = {}
    for regime in R.TAIL_REGIMES:
        layer = R.tail_layer(gelu, regime)
        a, x = R.tail_inputs(regime, rows)
        want, pre = R.tail_ref(a, x, layer, return_preact=True)
        assert torch.isfinite(want).all()
        stats[regime] = (float(pre.min()), float(pre.max()))
        if regime == "unit":
            assert pre.abs().max() < 8                       # the range the older tests stay in
        if regime == "wide_gelu":
            assert pre.min() < -11.5 and pre.max() > 11.5     # both saturated ends of the tanh form
            hist = torch.histc(pre.float(), bins=12, min=-6, max=6)
            assert (hist > 0).all()                           # every unit interval of [-6, 6]
        if regime == "offset_rows":
            xf = x.double()
            assert set(xf.mean(dim=1).round().tolist()) == {8.0, -8.0, 30.0, -30.0}
            assert (xf.mean(dim=1).abs() > 10 * xf.std(dim=1)).all()
        if regime == "outlier_dims":
            xf = x.double()
            big = xf.abs().mean(dim=0) > 10
            assert int(big.sum()) == 3
        if regime == "small_variance":
            assert float(a.abs().max()) == 0 and float(layer.out.bias.detach().abs().max()) == 0
            w12, w5 = R.tail_ref(a, x, layer, eps=1e-12), R.tail_ref(a, x, layer, eps=1e-5)
            assert float((w12 - w5).abs().max()) > 0.5        # eps = 1e-5 is visible next to a variance of 1e-6
            w0 = R.tail_ref(a, x, layer, eps=0.0)
            assert float((w12 - w0).abs().max()) < 1e-4       # ... and 1e-12 is not
    print(gelu, stats)


def test_yardstick_criterion_and_ulp():
    assert R.fp16_ulp_at(1.0) == 2.0 ** -10 and R.fp16_ulp_at(1.999) == 2.0 ** -10 and R.fp16_ulp_at(2.0) == 2.0 ** -9
    assert R.fp16_ulp_at(0.3) == 2.0 ** -12
    e_u = np.array([1e-3, 2e-3])
    assert R.yardstick_ok(np.array([4e-3, 1e-4]), e_u, 1.0)[0]
    assert not R.yardstick_ok(np.array([6e-3, 1e-4]), e_u, 1.0)[0]             # max above 2 max + u
    assert not R.yardstick_ok(np.array([3.5e-3, 3.5e-3]), e_u, 1.0)[0]         # mean above 2 mean
