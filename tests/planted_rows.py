"""Planted corpora for the dense scans (no GPU): small shards in which the best row of every query sits at a position
that is CHOSEN, not drawn, so that a defect tied to a position (one lane quad, the last row block of a super-group, a
trip after the first of a persistent wave, a row next to a masked row, the last row of the shard) cannot hide behind the
luck of a Gaussian draw.  tests/test_planted_rows.py holds the construction itself to its claims in fp64;
tests/test_gpu_scan_walk.py searches it.

The corpus.  X is a filler of N(0, 1/d) rows rounded to the store dtype.  The queries are Gaussian directions g_b (drawn
until no two of them have a cosine above QQ_MAX: with B > d they cannot be orthogonal, and a row planted for one query
must stay far below the planted row of every other) with norms u_b spread over the scale range.  Query b's unique best
row is row pos[b]:
  COSINE, IP   r_b g_b / |g_b|, the row norms r_b spread over the scale range (another order than the u_b), so that
               the inner product r_b u_b and the cosine 1 rank the planted rows differently;
  L2           Q[b] + 0.02 u_b e_b, e_b a unit direction: squared distance 4e-4 u_b^2, every other row ~ u_b^2 away.
The scale range is 0.5 .. 2 from d = 512 up and 0.75 .. 2 below: at d = 128 the largest cosine between a filler row and
one of 130 queries is ~0.45, and in the scans' domain (IP: S / |q| = r_b for the planted row) a planted row of norm 0.5
would clear it by less than 100 x the scans' error bound, which is the margin test_planted_rows.py asserts.

variant = "mask": exact copies of the planted row ("decoys") at p + 1, p - 1, p + 8, p + 16 and p + 64 — the neighbouring
mask bit on either side, the next mask byte, the next row block, the next super-group — where those lie inside the
shard and on no planted row; the packed row mask clears the decoys, clears about half of the filler at random and keeps
every planted row.  A scan that reads the wrong mask bit either finds a decoy or loses the planted row.

variant = "range": the planted row lies IN the range (cosine RANGE_COS to the query; L2: |x - q| = RANGE_L2_OFFSET u_b)
and unmasked decoys that score ABOVE the ceiling (copies of the query direction; L2: the near copy above) sit in the
same 16-row block (the row beside p) and at p + 16.  Only the ceiling (range_filter) bites: the floor (radius) lies
beyond every row.  To every OTHER query such a decoy is an ordinary in-range row.  Scales 0.8 .. 1.6: a row planted in
range for another query reaches 0.28 r in the scans' domain."""
import collections
import functools
import math

import numpy as np

IP, COSINE, L2 = 0, 1, 2          # HR_METRIC_*
SUPER = 64                        # rows of a super-group: what one trip of a scan wave or block covers
QQ_MAX = 0.2                      # largest |cosine| between two query directions (and a range row's noise and a query)
L2_OFFSET = 0.02                  # planted L2 row: |x - q| / |q|
RANGE_COS = 0.85                  # range variant, COSINE / IP: cosine of the planted row
RANGE_COS_CEIL = 0.925            # ... and the ceiling, as a cosine (IP: times r_b u_b)
RANGE_L2_OFFSET = 0.45            # range variant, L2: |x - q| / |q| of the planted row: D = 0.2025 u^2
RANGE_L2_FLOOR_D = 0.05           # ... and range_filter = 0.05 u^2 (the decoys' D = 4e-4 u^2 lies below it)
DECOY_STEPS = (1, -1, 8, 16, 64)

Planted = collections.namedtuple("Planted", "X Q pos mask keep decoys decoy_of radius range_filter scales")
# X [n, d] store dtype; Q [B, d] float32; pos [B] int64; mask = packed uint8 row mask or None; keep = the same as bool [n]
# (None: every row); decoys = sorted int64 row numbers; decoy_of [n] = the query a decoy row was written for (-1: not a
# decoy; a range decoy is an ordinary in-range row to every OTHER query); radius / range_filter = float64 [B] or None;
# scales = (lo, hi)


def n_super(n):
    return -(-n // SUPER)


@functools.lru_cache(maxsize=None)
def positions(n, B):
    """B distinct rows.  Rows n - 1 (last row of the shard and of the ragged last super-group), 0 and the first row of
    the last super-group come first; every further row goes to the super-group that holds the fewest planted rows so far
    and, there, to the in-group offset used least so far (ties: a fixed stride order, rotated by B so that small batches
    do not all test the same offsets).  Hence every super-group is hit where B >= n_super + 1, every offset 0..63 where
    B >= 65, and a batch smaller than that hits as many distinct groups and offsets as it has queries to spend.  (Not from
    B = n_super and B = 64: the three rows above are required and lie in two groups and on two offsets — n - 1 and the
    first row of the last group share a group, that row and row 0 share offset 0 — so one query is spent twice.)"""
    ns = n_super(n)
    assert 1 <= B <= n
    pos = []
    for p in (n - 1, 0, (ns - 1) * SUPER):
        if len(pos) < B and p not in pos:
            pos.append(p)
    taken = set(pos)
    in_group = collections.Counter(p // SUPER for p in pos)
    at_offset = collections.Counter(p % SUPER for p in pos)
    g_stride = next(s for s in range(max(1, int(0.37 * ns)), 2 * ns + 2) if math.gcd(s, ns) == 1)
    g_rank = {(i * g_stride) % ns: i for i in range(ns)}                 # hop across the shard, not along it
    o_rank = {(37 * i + 11 + 7 * (B % 61)) % SUPER: i for i in range(SUPER)}
    rows_of = lambda g: min(SUPER, n - g * SUPER)                        # noqa: E731
    while len(pos) < B:
        g = min((g for g in range(ns) if in_group[g] < rows_of(g)), key=lambda g: (in_group[g], g_rank[g]))
        o = min((o for o in range(rows_of(g)) if g * SUPER + o not in taken), key=lambda o: (at_offset[o], o_rank[o]))
        p = g * SUPER + o
        pos.append(p)
        taken.add(p)
        in_group[g] += 1
        at_offset[o] += 1
    pos = np.array(pos, np.int64)
    pos.setflags(write=False)
    return pos


def default_scales(d, variant):
    if variant == "range":
        return (0.8, 1.6)
    return (0.5, 2.0) if d >= 512 else (0.75, 2.0)


def _spread(lo, hi, B, rng):
    """B values spread geometrically over [lo, hi], both ends included, in a random order."""
    v = lo * (hi / lo) ** (np.arange(B) / max(B - 1, 1)) if B > 1 else np.array([math.sqrt(lo * hi)])
    return v[rng.permutation(B)]


def _unit(v):
    return v / np.linalg.norm(v)


def _directions(B, d, rng, against=None, limit=QQ_MAX):
    """B unit Gaussian directions, each redrawn until its |cosine| to every earlier one (and to every row of `against`,
    orthogonalised against against[b] first when given) is below `limit`.  Falls back to the limit rising by 10 % after
    2 000 draws for one vector, so the loop ends at any (B, d); test_planted_rows.py asserts the margin that results."""
    out = np.empty((B, d))
    for b in range(B):
        lim, tries = limit, 0
        while True:
            v = rng.standard_normal(d)
            if against is not None:
                v -= (v @ against[b]) * against[b]
            v = _unit(v)
            others = out[:b] if against is None else against
            if others.shape[0] == 0 or np.abs(others @ v).max() < lim:
                break
            tries += 1
            if tries % 2000 == 0:
                lim *= 1.1
        out[b] = v
    return out


@functools.lru_cache(maxsize=12)
def _query_directions(B, d, seed):
    """(query directions [B, d], range noise [B, d]): the same for every dtype, metric and variant of a (B, d)."""
    rng = np.random.default_rng([seed, B, d])
    G = _directions(B, d, rng)
    return G, _directions(B, d, rng, against=G)


@functools.lru_cache(maxsize=12)     # what one family of GPU cases goes round (d = 768: 12 corpora of ~10 MB)
def planted(n, d, np_dtype, metric, B, variant="plain", seed=0):
    """-> Planted.  variant: "plain", "mask" or "range" (module docstring).  Deterministic in its arguments; cached, and
    the arrays are shared between tests: treat them as read-only."""
    assert variant in ("plain", "mask", "range")
    rng = np.random.default_rng([seed, n, d, B, metric, ("plain", "mask", "range").index(variant)])
    lo, hi = default_scales(d, variant)
    X = (rng.standard_normal((n, d)) / math.sqrt(d)).astype(np.float32).astype(np_dtype)
    G, noise = _query_directions(B, d, seed)
    u = _spread(lo, hi, B, rng)                           # query norms
    r = _spread(lo, hi, B, rng)                           # row norms (COSINE, IP)
    Q = (G * u[:, None]).astype(np.float32)
    pos = positions(n, B)
    on_planted = np.zeros(n, bool)
    on_planted[pos] = True

    if variant == "range":
        if metric == L2:
            rows = Q.astype(np.float64) + (RANGE_L2_OFFSET * u)[:, None] * noise
            above = Q.astype(np.float64) + (L2_OFFSET * u)[:, None] * noise
        else:
            rows = r[:, None] * (RANGE_COS * G + math.sqrt(1.0 - RANGE_COS ** 2) * noise)
            above = r[:, None] * G
    elif metric == L2:
        rows = Q.astype(np.float64) + (L2_OFFSET * u)[:, None] * _directions(B, d, rng, limit=2.0)
        above = None
    else:
        rows = r[:, None] * G
        above = None
    X[pos] = rows.astype(np.float32).astype(np_dtype)

    decoys = []
    decoy_of = np.full(n, -1, np.int64)
    if variant != "plain":
        steps = DECOY_STEPS if variant == "mask" else None
        for b, p in enumerate(pos):
            beside = p + 1 if (p % 16 < 15 and p + 1 < n) else p - 1          # the same 16-row block
            targets = [p + s for s in steps] if steps else [beside, p + 16]
            for t in targets:
                if 0 <= t < n and not on_planted[t]:
                    X[t] = X[p] if variant == "mask" else above[b].astype(np.float32).astype(np_dtype)
                    decoys.append(t)
                    decoy_of[t] = b
    decoys = np.unique(np.array(decoys, np.int64))

    keep = mask = radius = rfilter = None
    if variant == "mask":
        keep = rng.random(n) < 0.5
        keep[decoys] = False
        keep[pos] = True
        mask = np.packbits(keep, bitorder="little")
    if variant == "range":
        qn2 = (Q.astype(np.float64) ** 2).sum(axis=1)
        if metric == L2:                                  # range_filter <= D < radius
            rfilter = RANGE_L2_FLOOR_D * qn2
            radius = np.full(B, 1.0e6)
        else:                                             # radius < s <= range_filter
            full = np.ones(B) if metric == COSINE else r * np.sqrt(qn2)     # the score of a decoy
            rfilter = RANGE_COS_CEIL * full
            radius = -2.0 * full
    for a in (X, Q, mask, keep, decoys, decoy_of, radius, rfilter):
        if a is not None:
            a.setflags(write=False)
    return Planted(X, Q, pos, mask, keep, decoys, decoy_of, radius, rfilter, (lo, hi))


# ---- the shards tests/test_gpu_scan_walk.py searches; tests/test_planted_rows.py checks the construction of each -------
WALK_N = 101 * 64 - 27            # 101 super-groups, the last one ragged (37 rows)
LONG_N = 27 * 64 - 5              # the long-row shard: 27 super-groups, 59 rows in the last
Shard = collections.namedtuple("Shard", "n d np_dtypes metrics batches variants")
SHARDS = {
    "d128": Shard(WALK_N, 128, (np.float16, np.float32), (COSINE, IP, L2), (1, 33, 64, 130), ("plain", "mask")),
    "d128_range": Shard(WALK_N, 128, (np.float16, np.float32), (COSINE, IP, L2), (64, 130), ("range",)),
    "d768": Shard(WALK_N, 768, (np.float16,), (COSINE, IP), (64, 256, 300), ("plain", "mask")),
    "d1024": Shard(WALK_N, 1024, (np.float16,), (COSINE,), (256,), ("plain",)),
    "d3000": Shard(LONG_N, 3000, (np.float32,), (IP, L2), (1, 20), ("plain",)),
}


def device_mask(mask, n):
    """The packed mask padded to whole 64-row words, as the device entry points take it."""
    out = np.zeros(8 * -(-n // 64), np.uint8)
    out[:mask.shape[0]] = mask
    return out
