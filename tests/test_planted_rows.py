"""The planted corpora of tests/planted_rows.py, held to their own claims in fp64 (no GPU): the planted row is the strict
best allowed row of its query by at least 100 x the scans' error bound (range_yardstick.scan_eps, in the scans' domain:
COSINE the cosine, IP S / |q|, L2 (|q|^2 - D) / (2 |q|)), the positions cover what the docstring of positions() says,
masks and decoys are what the variants promise.  tests/test_gpu_scan_walk.py leans on the margin: with it, a device list
that is not proven exact at k = 1 means a wrong group maximum or a wrong cut, never bad luck."""
import numpy as np
import pytest

import planted_rows as pr
import range_yardstick as ry

MARGIN = 100.0            # planted row over the best other allowed row, in units of scan_eps
BOUND_MARGIN = 10.0       # range variant: every row's distance from the ceiling, in units of scan_eps

assert (pr.IP, pr.COSINE, pr.L2) == (ry.IP, ry.COSINE, ry.L2)
CASES = [(name, np_dtype, metric, B, variant)
         for name, s in pr.SHARDS.items() for np_dtype in s.np_dtypes for metric in s.metrics for B in s.batches
         for variant in s.variants]


def _scan_domain(X, Q, metric):
    """-> (T [B, n] the scans' exact value of every row, S [B, n] the score the result semantics rank by, |q|^2 [B])."""
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    dot = Q64 @ X64.T
    xn2 = (X64 * X64).sum(axis=1)[None, :]
    qn2 = (Q64 * Q64).sum(axis=1)[:, None]
    qn = np.sqrt(qn2)
    if metric == pr.COSINE:
        T = dot / (qn * np.sqrt(xn2))
        return T, T, qn2[:, 0]
    if metric == pr.IP:
        return dot / qn, dot, qn2[:, 0]
    return (2.0 * dot - xn2) / (2.0 * qn), qn2 + xn2 - 2.0 * dot, qn2[:, 0]


def _case_id(c):
    return "%s-%s-%s-B%d-%s" % (c[0], np.dtype(c[1]).name, ("IP", "COSINE", "L2")[c[2]], c[3], c[4])


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_the_planted_row_wins_by_a_hundred_error_bounds(case):
    name, np_dtype, metric, B, variant = case
    s = pr.SHARDS[name]
    p = pr.planted(s.n, s.d, np_dtype, metric, B, variant)
    assert p.X.shape == (s.n, s.d) and p.X.dtype == np_dtype and p.Q.shape == (B, s.d) and p.Q.dtype == np.float32
    assert len(set(p.pos.tolist())) == B and p.pos.min() >= 0 and p.pos.max() < s.n
    T, S, qn2 = _scan_domain(p.X, p.Q, metric)
    M = ry.max_row_norm(p.X)
    f16 = np_dtype == np.float16
    eps = np.array([ry.scan_eps(metric, f16, s.d, M, qn2[b]) for b in range(B)])
    allowed = np.ones((B, s.n), bool)
    if variant == "mask":
        allowed &= p.keep[None, :]
    if variant == "range":
        allowed &= np.stack([ry.in_range(S[b], metric, p.radius[b], p.range_filter[b]) for b in range(B)])
        # nothing sits near the ceiling: what is above it is above it for the scan as well
        if metric == pr.L2:
            ceil_t = (qn2 - p.range_filter) / (2.0 * np.sqrt(qn2))
        else:
            ceil_t = p.range_filter / (np.sqrt(qn2) if metric == pr.IP else 1.0)
        off = np.abs(T - ceil_t[:, None]).min(axis=1) / eps
        assert off.min() >= BOUND_MARGIN, f"a row within {off.min():.1f} eps of the ceiling"
        floor_ok = np.stack([ry.in_range(S[b], metric, p.radius[b], None) for b in range(B)])
        assert floor_ok.all()                                  # the floor lies beyond every row
    own = T[np.arange(B), p.pos]
    assert allowed[np.arange(B), p.pos].all()
    others = np.where(allowed, T, -np.inf)
    others[np.arange(B), p.pos] = -np.inf
    gap = (own - others.max(axis=1)) / eps
    print(f"{_case_id(case)}: smallest gap {gap.min():.0f} eps (query {gap.argmin()}), eps {eps.min():.3g} .. {eps.max():.3g}")
    assert gap.min() >= MARGIN, f"query {gap.argmin()}: planted row only {gap.min():.1f} eps above the best other row"
    # the scales keep IP and L2 from reducing to COSINE: norms spread over the whole scale range
    lo, hi = p.scales
    if B >= 20:
        qn = np.sqrt(qn2)
        assert qn.min() < 1.05 * lo and qn.max() > hi / 1.05
        if metric != pr.L2 and variant != "range":
            rn = np.linalg.norm(p.X[p.pos].astype(np.float64), axis=1)
            assert rn.min() < 1.05 * lo and rn.max() > hi / 1.05


@pytest.mark.parametrize("n,B", sorted({(s.n, B) for s in pr.SHARDS.values() for B in s.batches}))
def test_positions_cover_groups_offsets_and_edges(n, B):
    pos = pr.positions(n, B)
    ns = pr.n_super(n)
    last0 = (ns - 1) * pr.SUPER
    assert len(set(pos.tolist())) == B
    assert (n - 1) in pos                                      # last row of the shard = last row of the ragged last group
    if B >= 2:
        assert 0 in pos
    if B >= 3:
        assert last0 in pos                                    # first row of the ragged last group
    groups, offsets = set((pos // pr.SUPER).tolist()), set((pos % pr.SUPER).tolist())
    # rows 0 and last0 share offset 0, rows n - 1 and last0 share the last group: one query each is spent twice
    assert len(groups) == min(ns, B - 1 if B >= 3 else B)
    assert len(offsets) >= min(pr.SUPER, B - 1 if B >= 3 else B)
    if B >= ns + 1:
        assert groups == set(range(ns))
    if B >= pr.SUPER + 1:
        assert offsets == set(range(pr.SUPER))


def test_the_small_batches_of_the_lds_scan_cover_every_offset_between_them():
    s = pr.SHARDS["d128"]
    seen = set()
    for B in (1, 33, 64):
        seen |= set((pr.positions(s.n, B) % pr.SUPER).tolist())
    assert seen == set(range(pr.SUPER))


@pytest.mark.parametrize("name", ["d128", "d768"])
def test_mask_variant_decoys_and_mask(name):
    s = pr.SHARDS[name]
    for metric in s.metrics:
        for B in s.batches:
            p = pr.planted(s.n, s.d, s.np_dtypes[0], metric, B, "mask")
            planted_rows = set(p.pos.tolist())
            assert p.keep[p.pos].all() and not p.keep[p.decoys].any()
            assert np.array_equal(np.unpackbits(p.mask, bitorder="little")[:s.n].astype(bool), p.keep)
            want = set()
            for q in p.pos:
                for step in pr.DECOY_STEPS:
                    t = int(q) + step
                    if 0 <= t < s.n and t not in planted_rows:
                        want.add(t)
            assert want == set(p.decoys.tolist())
            rows = {p.X[q].tobytes() for q in p.pos}
            assert all(p.X[t].tobytes() in rows for t in p.decoys)          # exact copies of a planted row
            filler = np.ones(s.n, bool)
            filler[p.pos] = False
            filler[p.decoys] = False
            assert 0.45 < p.keep[filler].mean() < 0.55
            if B >= 64:
                steps_seen = {int(t - q) for q in p.pos for t in p.decoys if int(t - q) in pr.DECOY_STEPS
                              and p.X[t].tobytes() == p.X[q].tobytes()}
                assert steps_seen == set(pr.DECOY_STEPS)


def test_range_variant_decoys_lie_above_the_ceiling_next_to_the_planted_row():
    s = pr.SHARDS["d128_range"]
    for np_dtype in s.np_dtypes:
        for metric in s.metrics:
            for B in s.batches:
                p = pr.planted(s.n, s.d, np_dtype, metric, B, "range")
                assert p.mask is None and len(p.decoys) > B
                _, S, _ = _scan_domain(p.X, p.Q, metric)
                near_block, near_next = 0, 0
                for b in range(B):
                    above = ~ry.in_range(S[b], metric, None, p.range_filter[b])
                    assert np.all(p.decoy_of[above] == b)           # nothing but this query's decoys lies above its ceiling
                    q = int(p.pos[b])
                    near_block += bool(above[(q // 16) * 16:(q // 16) * 16 + 16].any())
                    near_next += bool(q + 16 < s.n and above[q + 16])
                    # the expectation the GPU test uses: the planted row heads the in-range list
                    ids, _ = ry.topk_in_range(S[b].astype(np.float32), metric, 1, p.radius[b], p.range_filter[b])
                    assert ids[0] == q
                assert near_block >= 0.9 * B and near_next >= 0.9 * B
