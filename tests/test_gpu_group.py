"""The two kernels of grouping search (csrc/group.h) alone: hr_group_select_dev against the ten-line restatement "the
first k rows whose key differs from the key of every row before them", and hr_mask_drop_groups_dev against numpy.  Every
comparison is exact equality."""
import numpy as np
import pytest

from advanced_rag import _native as nat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
ROWS_PER_QUERY = 800          # query b of a launch draws its ids from rows [b * 800, b * 800 + k_in) of the key column


def first_k_distinct(ranked_rows, keys, k):
    """The first k rows of a ranking whose key differs from the key of every row before them."""
    seen, out = set(), []
    for r in ranked_rows:
        if keys[r] not in seen:
            seen.add(keys[r])
            out.append(r)
            if len(out) == k:
                break
    return out


def restate(ids, n, keys, first_row, k_out):
    """-> (positions, keys of the selected, flag) of one list.  An id outside the key column is a group of its own."""
    k_in = len(ids)
    if n is None:
        neg = np.nonzero(ids < 0)[0]
        n = int(neg[0]) if len(neg) else k_in
    n = max(0, min(int(n), k_in))
    label, value = [], []
    for i, r in enumerate(ids[:n].tolist()):
        inside = first_row <= r < first_row + len(keys)
        label.append(("key", int(keys[r - first_row])) if inside else ("none", i))
        value.append(int(keys[r - first_row]) if inside else r)
    pos = first_k_distinct(list(range(n)), label, k_out)
    return pos, [value[i] for i in pos], int(len(pos) == k_out or n < k_in)


def select_dev(ids, n, keys, first_row, k_out, with_keys=True, with_flags=True):
    dev = torch.device("cuda", 0)
    B, k_in = ids.shape
    d_ids = torch.from_numpy(ids).to(dev)
    d_n = torch.from_numpy(np.asarray(n, dtype=np.int32)).to(dev) if n is not None else None
    d_keys = torch.from_numpy(keys).to(dev) if len(keys) else None
    pos = torch.full((B, k_out), -7, dtype=torch.int32, device=dev)
    okeys = torch.full((B, k_out), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    fl = torch.full((B,), -7, dtype=torch.int32, device=dev)
    nat.group_select_dev(d_ids.data_ptr(), d_n.data_ptr() if d_n is not None else 0, B, k_in,
                         d_keys.data_ptr() if d_keys is not None else 0, len(keys), first_row, k_out, pos.data_ptr(),
                         okeys.data_ptr() if with_keys else 0, cnt.data_ptr(), fl.data_ptr() if with_flags else 0,
                         torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return pos.cpu().numpy(), okeys.cpu().numpy(), cnt.cpu().numpy(), fl.cpu().numpy()


def _patterns(k_in, rng):
    """name -> (key per position, {position: id override}, n or None).  The keys are written into the key column at the
    rows the list names, so a pattern says exactly which positions share a group."""
    distinct = rng.permutation(k_in).astype(np.int64) * 3 + 5
    out = {"all_distinct": (distinct.copy(), {}, None), "all_equal": (np.full(k_in, 42, np.int64), {}, None)}
    pk = distinct.copy()
    for a in (63, 255):          # a duplicate pair across a wave edge and across the edge of a 256-position trip
        if a + 1 < k_in:
            pk[a + 1] = pk[a]
    out["pairs_across_edges"] = (pk, {}, None)
    pk = distinct.copy()
    pk[-1] = pk[0]
    out["first_again_at_the_end"] = (pk, {}, None)
    pk = np.where(np.arange(k_in) % 2 == 0, np.int64(7), np.int64(7) + (np.int64(1) << 32))      # differ in the high word only
    pk[k_in // 2:] += np.arange(k_in - k_in // 2) % 2                                             # ... and in the low word only
    out["high_or_low_word_only"] = (pk.astype(np.int64), {}, None)
    pk = distinct.copy()
    pk[::3] = I64_MIN
    pk[1::3] = I64_MAX
    out["extremes"] = (pk, {}, None)
    pk = rng.integers(0, max(2, k_in // 3), k_in).astype(np.int64)                                 # many repeats
    out["minus_one_mid_list"] = (pk.copy(), {k_in // 2: -1}, None)
    out["n_shorter_than_the_list"] = (pk.copy(), {}, max(0, k_in - 3))
    out["n_zero"] = (pk.copy(), {}, 0)
    out["n_beyond_the_list"] = (pk.copy(), {}, k_in + 9)                                           # clamped to k_in
    # two EQUAL ids far outside, one just behind the column, one just below first_row: each a group of its own
    outside = dict(zip(sorted({0, k_in // 3, k_in // 2, k_in - 1}), ["far", "far", "behind", "below"]))
    out["ids_outside_the_column"] = (pk.copy(), outside, None)
    return out


SHAPES = sorted({(k_in, k_out) for k_in in (1, 40, 63, 64, 65, 255, 256, 257, 768) for k_out in (1, 20, k_in) if k_out <= k_in})


@pytest.mark.parametrize("first_row", [0, 1000])
@pytest.mark.parametrize("k_in,k_out", SHAPES)
def test_group_select_equals_the_restatement(gpu, k_in, k_out, first_row):
    rng = np.random.default_rng(k_in * 1000 + k_out)
    pats = _patterns(k_in, rng)
    names = list(pats)
    B = 3
    for with_n in (True, False):
        use = [p for p in names if with_n or pats[p][2] is None]
        for c0 in range(0, len(use), B):
            chunk = (use[c0:c0 + B] + use[:B])[:B]
            keys = rng.integers(-50, 50, B * ROWS_PER_QUERY).astype(np.int64)
            ids = np.empty((B, k_in), np.int64)
            n = []
            for b, name in enumerate(chunk):
                pk, override, n_b = pats[name]
                rows = b * ROWS_PER_QUERY + rng.permutation(k_in)
                keys[rows] = pk
                ids[b] = rows + first_row
                for p, v in override.items():
                    ids[b, p] = {-1: -1, "far": 10**12, "behind": first_row + len(keys),
                                 "below": first_row - 1 if first_row else I64_MAX}[v]
                n.append(k_in if n_b is None else n_b)
            pos, okeys, cnt, fl = select_dev(ids, n if with_n else None, keys, first_row, k_out)
            for b, name in enumerate(chunk):
                want_pos, want_keys, want_flag = restate(ids[b], n[b] if with_n else None, keys, first_row, k_out)
                m = len(want_pos)
                what = (name, with_n, b)
                assert cnt[b] == m, what
                assert pos[b, :m].tolist() == want_pos and (pos[b, m:] == -1).all(), what
                assert okeys[b, :m].tolist() == want_keys and (okeys[b, m:] == 0).all(), what
                assert fl[b] == want_flag, what


def test_group_select_flags_for_each_reason_and_optional_outputs(gpu):
    keys = np.array([1, 1, 1, 2, 2, 3, 3, 3], np.int64)
    ids = np.array([[0, 1, 2, 3, 4, 5, 6, 7],         # three groups in a full window
                    [0, 1, 2, 3, 4, -1, -1, -1],      # two groups, then the search ran out of rows
                    [0, 1, 2, 1, 0, 2, 1, 0]], np.int64)   # one group in a full window
    pos, okeys, cnt, fl = select_dev(ids, None, keys, 0, 3)
    assert cnt.tolist() == [3, 2, 1]
    assert fl.tolist() == [1, 1, 0]                   # k_out reached | fewer than k_in valid entries | the window ended early
    assert pos.tolist() == [[0, 3, 5], [0, 3, -1], [0, -1, -1]] and okeys.tolist() == [[1, 2, 3], [1, 2, 0], [1, 0, 0]]
    pos2, okeys2, cnt2, fl2 = select_dev(ids, None, keys, 0, 3, with_keys=False, with_flags=False)
    assert np.array_equal(pos2, pos) and np.array_equal(cnt2, cnt)
    assert (okeys2 == -7).all() and (fl2 == -7).all()  # NULL outputs are not written
    # no key column at all: every entry is a group of its own
    pos3, okeys3, cnt3, fl3 = select_dev(ids, [8, 5, 8], np.zeros(0, np.int64), 0, 8)
    assert cnt3.tolist() == [8, 5, 8] and fl3.tolist() == [1, 1, 1] and okeys3[1, :5].tolist() == [0, 1, 2, 3, 4]


def test_group_select_limits_and_bad_arguments(gpu):
    dev = torch.device("cuda", 0)
    ids = torch.zeros((2, 769), dtype=torch.int64, device=dev)
    keys = torch.zeros(16, dtype=torch.int64, device=dev)
    pos = torch.full((2, 769), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((2,), -7, dtype=torch.int32, device=dev)

    def call(B=2, k_in=8, k_out=4, ids=ids.data_ptr(), keys=keys.data_ptr(), rows=16, first_row=0, pos=pos.data_ptr(),
             cnt=cnt.data_ptr()):
        nat.group_select_dev(ids, 0, B, k_in, keys, rows, first_row, k_out, pos, 0, cnt, 0, 0)

    with pytest.raises(nat.HbmRagError) as ei:
        call(k_in=769, k_out=4)
    assert ei.value.status == 5                       # HR_ELIMIT
    for bad in (dict(k_out=0), dict(k_out=9), dict(B=-1), dict(k_in=0), dict(ids=0), dict(pos=0), dict(cnt=0), dict(keys=0),
                dict(rows=-1), dict(first_row=-1)):
        with pytest.raises(ValueError):               # HR_EINVAL
            call(**bad)
    call(B=0)                                         # nothing to do: HR_OK, nothing launched
    call(B=0, ids=0, pos=0, cnt=0)
    torch.cuda.synchronize(dev)
    assert (pos == -7).all().item() and (cnt == -7).all().item()
    call(rows=0)                                      # an empty key column: its buffer is not read, every entry its own group
    torch.cuda.synchronize(dev)
    assert cnt.tolist() == [4, 4] and pos.view(-1)[:8].tolist() == [0, 1, 2, 3] * 2      # written as [B][k_out]
    call(k_in=768, k_out=768)                         # the largest list is served
    torch.cuda.synchronize(dev)
    assert cnt.tolist() == [1, 1]                     # 768 times row 0: one group


# --------------------------------------------------------------------------- hr_mask_drop_groups_dev
def _words(n_rows):
    return (n_rows + 63) // 64


def drop_dev(mask_in, n_rows, keys, drop, alias=False):
    """mask_in: uint8 [8 * words] or None.  -> uint8 [8 * words] written by the kernel (prefilled with 0xFF)."""
    dev = torch.device("cuda", 0)
    d_keys = torch.from_numpy(keys).to(dev)
    d_drop = torch.from_numpy(np.concatenate([drop, np.zeros(1, np.int64)])).to(dev)
    d_in = torch.from_numpy(mask_in.copy()).to(dev) if mask_in is not None else None
    d_out = d_in if alias else torch.full((8 * _words(n_rows),), 0xFF, dtype=torch.uint8, device=dev)
    nat.mask_drop_groups_dev(d_in.data_ptr() if d_in is not None else 0, d_out.data_ptr(), n_rows, d_keys.data_ptr(),
                             d_drop.data_ptr() if len(drop) else 0, len(drop), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    if d_in is not None and not alias:
        assert np.array_equal(d_in.cpu().numpy(), mask_in)       # the input is only read
    return d_out.cpu().numpy()


def _key_pool(rng):
    pool = rng.integers(-2000, 2000, 1500).astype(np.int64)
    special = np.array([I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, 0, -1, 1 << 32, (1 << 32) + 1, 1, -(1 << 32), 1 << 62], np.int64)
    return np.concatenate([pool, special]), special


@pytest.mark.parametrize("n_drop", [0, 1, 768])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 1000, 4097])
def test_mask_drop_groups_equals_numpy(gpu, n_rows, n_drop):
    rng = np.random.default_rng(n_rows * 7 + n_drop)
    pool, special = _key_pool(rng)
    keys = rng.choice(pool, n_rows)
    keys[rng.integers(0, n_rows, min(n_rows, 8))] = rng.choice(special, min(n_rows, 8))
    if n_drop == 1:
        drops = [np.array([k], np.int64) for k in (keys[0], I64_MIN, I64_MAX, 1 << 32)]
    elif n_drop:
        d = np.concatenate([special[:6], rng.choice(keys, 300), rng.choice(pool, 400)])     # unsorted, with duplicates
        d = np.concatenate([d, rng.choice(d, n_drop - len(d))])
        drops = [rng.permutation(d)]
        assert len(drops[0]) == 768 and len(np.unique(drops[0])) < 768
    else:
        drops = [np.zeros(0, np.int64)]
    nbytes = 8 * _words(n_rows)
    random_mask = rng.integers(0, 256, nbytes).astype(np.uint8)    # bits at and beyond n_rows are garbage on purpose
    tail = np.arange(nbytes * 8) >= n_rows
    for drop in drops:
        gone = np.isin(keys, drop)
        for mask_in, alias in ((None, False), (random_mask, False), (random_mask, True)):
            got = drop_dev(mask_in, n_rows, keys, drop, alias)
            bits = np.unpackbits(got, bitorder="little")
            before = np.ones(n_rows, bool) if mask_in is None else np.unpackbits(mask_in, bitorder="little")[:n_rows].astype(bool)
            assert np.array_equal(bits[:n_rows].astype(bool), before & ~gone), (len(drop), mask_in is None, alias)
            assert not bits[tail].any()                             # the tail of the last word is written 0


def test_mask_drop_groups_limits_and_bad_arguments(gpu):
    dev = torch.device("cuda", 0)
    keys = torch.zeros(128, dtype=torch.int64, device=dev)
    drop = torch.zeros(769, dtype=torch.int64, device=dev)
    out = torch.full((24,), 0xFF, dtype=torch.uint8, device=dev)

    def call(mask_in=0, out=out.data_ptr(), n_rows=100, keys=keys.data_ptr(), drop=drop.data_ptr(), n_drop=4):
        nat.mask_drop_groups_dev(mask_in, out, n_rows, keys, drop, n_drop, 0)

    with pytest.raises(nat.HbmRagError) as ei:
        call(n_drop=769)
    assert ei.value.status == 5                       # HR_ELIMIT
    for bad in (dict(n_rows=-1), dict(n_drop=-1), dict(out=0), dict(keys=0), dict(drop=0), dict(out=out.data_ptr() + 4),
                dict(mask_in=out.data_ptr() + 1)):
        with pytest.raises(ValueError):               # HR_EINVAL
            call(**bad)
    call(n_rows=0)                                    # nothing to do: HR_OK, nothing launched
    call(n_rows=0, out=0, keys=0)
    torch.cuda.synchronize(dev)
    assert (out == 0xFF).all().item()
    call(n_drop=768)                                  # the largest drop set is served: every row has key 0, and 0 is dropped
    torch.cuda.synchronize(dev)
    assert not out[:16].any().item() and (out[16:] == 0xFF).all().item()
