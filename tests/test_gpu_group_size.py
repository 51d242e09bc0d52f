"""The kernels of grouping search with group_size > 1 (csrc/group.h) alone: hr_group_select_n_dev against the plain
restatement "walk the list, count the members of every key, keep the first k_out groups and the first group_size of each",
and hr_mask_keep_groups_dev against numpy.  Every comparison is exact equality."""
import numpy as np
import pytest

from advanced_rag import _native as nat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
ROWS_PER_QUERY = 800          # query b of a launch draws its ids from rows [b * 800, b * 800 + k_in) of the key column
LIMIT = 3 * nat.HR_MAX_TOPK


def restate(ids, n, keys, first_row, k_out, g):
    """-> (positions per selected group, keys of the groups, flags) of one list.  An id outside the key column is a
    group of its own with one member."""
    k_in = len(ids)
    if n is None:
        neg = np.nonzero(ids < 0)[0]
        n = int(neg[0]) if len(neg) else k_in
    n = max(0, min(int(n), k_in))
    groups, value = {}, {}
    for i, r in enumerate(ids[:n].tolist()):
        inside = first_row <= r < first_row + len(keys)
        label = ("key", int(keys[r - first_row])) if inside else ("none", i)
        if label not in groups:
            if len(groups) == k_out:
                continue
            groups[label] = []
            value[label] = int(keys[r - first_row]) if inside else r
        if len(groups[label]) < g:
            groups[label].append(i)
    # how many groups the list holds in all (for bit 0) needs no second walk: fewer than k_out selected = all of them
    members = list(groups.values())
    ran_out = n < k_in
    flags = int(len(members) == k_out or ran_out) | (2 if (all(len(m) == g for m in members) or ran_out) else 0)
    return members, [value[label] for label in groups], flags


def select_n_dev(ids, n, keys, first_row, k_out, g, with_keys=True, with_flags=True):
    dev = torch.device("cuda", 0)
    B, k_in = ids.shape
    d_ids = torch.from_numpy(ids).to(dev)
    d_n = torch.from_numpy(np.asarray(n, dtype=np.int32)).to(dev) if n is not None else None
    d_keys = torch.from_numpy(keys).to(dev) if len(keys) else None
    pos = torch.full((B, k_out * g), -7, dtype=torch.int32, device=dev)
    okeys = torch.full((B, k_out), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((B, k_out), -7, dtype=torch.int32, device=dev)
    n_sel = torch.full((B,), -7, dtype=torch.int32, device=dev)
    fl = torch.full((B,), -7, dtype=torch.int32, device=dev)
    nat.group_select_n_dev(d_ids.data_ptr(), d_n.data_ptr() if d_n is not None else 0, B, k_in,
                           d_keys.data_ptr() if d_keys is not None else 0, len(keys), first_row, k_out, g, pos.data_ptr(),
                           okeys.data_ptr() if with_keys else 0, cnt.data_ptr(), n_sel.data_ptr(),
                           fl.data_ptr() if with_flags else 0, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return pos.cpu().numpy(), okeys.cpu().numpy(), cnt.cpu().numpy(), n_sel.cpu().numpy(), fl.cpu().numpy()


def select_1_dev(ids, n, keys, first_row, k_out):
    """hr_group_select_dev on the same inputs -> positions, keys, groups, flag"""
    dev = torch.device("cuda", 0)
    B, k_in = ids.shape
    d_ids = torch.from_numpy(ids).to(dev)
    d_n = torch.from_numpy(np.asarray(n, dtype=np.int32)).to(dev) if n is not None else None
    d_keys = torch.from_numpy(keys).to(dev)
    pos = torch.full((B, k_out), -7, dtype=torch.int32, device=dev)
    okeys = torch.full((B, k_out), -7, dtype=torch.int64, device=dev)
    n_sel = torch.full((B,), -7, dtype=torch.int32, device=dev)
    fl = torch.full((B,), -7, dtype=torch.int32, device=dev)
    nat.group_select_dev(d_ids.data_ptr(), d_n.data_ptr() if d_n is not None else 0, B, k_in, d_keys.data_ptr(), len(keys),
                         first_row, k_out, pos.data_ptr(), okeys.data_ptr(), n_sel.data_ptr(), fl.data_ptr(),
                         torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return pos.cpu().numpy(), okeys.cpu().numpy(), n_sel.cpu().numpy(), fl.cpu().numpy()


def _patterns(k_in, g, rng):
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
    outside = dict(zip(sorted({0, k_in // 3, k_in // 2, k_in - 1}), ["far", "far", "behind", "below"]))
    out["ids_outside_the_column"] = (pk.copy(), outside, None)
    # groups of exactly group_size and of group_size + 1 members, scattered over the list, the rest distinct
    for extra, name in ((0, "a_group_of_exactly_group_size"), (1, "a_group_of_group_size_plus_one")):
        pk = distinct.copy()
        m = min(k_in, g + extra)
        pk[rng.permutation(k_in)[:m]] = -9
        out[name] = (pk, {}, None)
    # a group whose members straddle positions 255 / 256 (and the wave edge 63 / 64 in shorter lists)
    pk = distinct.copy()
    for a in (62, 63, 64, 65, 254, 255, 256, 257):
        if a < k_in:
            pk[a] = -11 if a < 128 else -12
    out["members_straddle_an_edge"] = (pk, {}, None)
    return out


def _k_outs(k_in, g):
    largest = min(k_in, LIMIT // g)
    return sorted({k for k in (1, 5, largest) if 1 <= k <= largest})


SHAPES = sorted({(k_in, g, k_out) for k_in in (1, 63, 64, 65, 255, 256, 257, 768) for g in (1, 2, 3, k_in)
                 for k_out in _k_outs(k_in, g)})


@pytest.mark.parametrize("k_in,g,k_out", SHAPES)
def test_group_select_n_equals_the_restatement(gpu, k_in, g, k_out):
    rng = np.random.default_rng(k_in * 100000 + g * 1000 + k_out)
    pats = _patterns(k_in, g, rng)
    names = list(pats)
    B = 3
    first_row = 1000 if (k_in + g + k_out) % 2 else 0
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
            if with_n:                                      # B = 3 lists with different d_n: the last one is cut short as well
                n[2] = min(n[2], max(0, k_in - 1 - c0 % 5))
            pos, okeys, cnt, n_sel, fl = select_n_dev(ids, n if with_n else None, keys, first_row, k_out, g)
            if g == 1:
                pos1, okeys1, n_sel1, fl1 = select_1_dev(ids, n if with_n else None, keys, first_row, k_out)
                assert np.array_equal(pos, pos1) and np.array_equal(okeys, okeys1) and np.array_equal(n_sel, n_sel1)
                assert np.array_equal(fl & 1, fl1) and (fl & 2).all()
            for b, name in enumerate(chunk):
                members, want_keys, want_flags = restate(ids[b], n[b] if with_n else None, keys, first_row, k_out, g)
                m = len(members)
                what = (name, with_n, b)
                want_pos = np.full((k_out, g), -1, np.int64)
                for o, at in enumerate(members):
                    want_pos[o, :len(at)] = at
                assert n_sel[b] == m, what
                assert np.array_equal(pos[b].reshape(k_out, g), want_pos), what
                assert cnt[b].tolist() == [len(at) for at in members] + [0] * (k_out - m), what
                assert okeys[b, :m].tolist() == want_keys and (okeys[b, m:] == 0).all(), what
                assert fl[b] == want_flags, what


def test_group_select_n_flags_and_optional_outputs(gpu):
    keys = np.array([1, 1, 1, 2, 2, 3, 3, 3], np.int64)
    ids = np.array([[0, 1, 2, 3, 4, 5, 6, 7],         # three groups in a full window, the second one short
                    [0, 1, 2, 3, 4, -1, -1, -1],      # two groups, then the search ran out of rows
                    [0, 1, 2, 1, 0, 2, 1, 0],         # one group in a full window, complete
                    [0, 3, 1, 5, 6, 2, 7, 4]], np.int64)   # three groups in a full window, all complete at group_size 2
    pos, okeys, cnt, n_sel, fl = select_n_dev(ids, None, keys, 0, 3, 3)
    assert n_sel.tolist() == [3, 2, 1, 3]
    assert fl.tolist() == [1, 3, 2, 1]                # bit 0: the groups are final; bit 1: so are their members
    assert pos.tolist() == [[0, 1, 2, 3, 4, -1, 5, 6, 7], [0, 1, 2, 3, 4, -1, -1, -1, -1], [0, 1, 2, -1, -1, -1, -1, -1, -1],
                            [0, 2, 5, 1, 7, -1, 3, 4, 6]]
    assert cnt.tolist() == [[3, 2, 3], [3, 2, 0], [3, 0, 0], [3, 2, 3]] and okeys.tolist() == [[1, 2, 3], [1, 2, 0], [1, 0, 0], [1, 2, 3]]
    assert select_n_dev(ids, None, keys, 0, 3, 2)[4].tolist() == [3, 3, 2, 3]
    pos2, okeys2, cnt2, n_sel2, fl2 = select_n_dev(ids, None, keys, 0, 3, 3, with_keys=False, with_flags=False)
    assert np.array_equal(pos2, pos) and np.array_equal(cnt2, cnt) and np.array_equal(n_sel2, n_sel)
    assert (okeys2 == -7).all() and (fl2 == -7).all()  # NULL outputs are not written
    # no key column at all: every entry is a group of its own with one member
    pos3, okeys3, cnt3, n_sel3, fl3 = select_n_dev(ids, [8, 5, 8, 0], np.zeros(0, np.int64), 0, 4, 2)
    assert n_sel3.tolist() == [4, 4, 4, 0] and fl3.tolist() == [1, 3, 1, 3]
    assert pos3[0].tolist() == [0, -1, 1, -1, 2, -1, 3, -1] and cnt3[1].tolist() == [1, 1, 1, 1] and okeys3[3].tolist() == [0] * 4


def test_group_select_n_limits_and_bad_arguments(gpu):
    dev = torch.device("cuda", 0)
    ids = torch.zeros((2, 769), dtype=torch.int64, device=dev)
    keys = torch.zeros(16, dtype=torch.int64, device=dev)
    pos = torch.full((2, 769), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((2, 769), -7, dtype=torch.int32, device=dev)
    n_sel = torch.full((2,), -7, dtype=torch.int32, device=dev)

    def call(B=2, k_in=8, k_out=4, g=2, ids=ids.data_ptr(), keys=keys.data_ptr(), rows=16, first_row=0, pos=pos.data_ptr(),
             cnt=cnt.data_ptr(), n_sel=n_sel.data_ptr()):
        nat.group_select_n_dev(ids, 0, B, k_in, keys, rows, first_row, k_out, g, pos, 0, cnt, n_sel, 0, 0)

    for beyond in (dict(k_in=769, k_out=4), dict(k_in=768, k_out=385, g=2), dict(k_in=768, k_out=1, g=769),
                   dict(k_in=768, k_out=768, g=2)):
        with pytest.raises(nat.HbmRagError) as ei:
            call(**beyond)
        assert ei.value.status == 5                   # HR_ELIMIT
    for bad in (dict(k_out=0), dict(k_out=9), dict(B=-1), dict(k_in=0), dict(g=0), dict(g=-1), dict(ids=0), dict(pos=0),
                dict(cnt=0), dict(n_sel=0), dict(keys=0), dict(rows=-1), dict(first_row=-1)):
        with pytest.raises(ValueError):               # HR_EINVAL
            call(**bad)
    call(B=0)                                         # nothing to do: HR_OK, nothing launched
    call(B=0, ids=0, pos=0, cnt=0, n_sel=0)
    torch.cuda.synchronize(dev)
    assert (pos == -7).all().item() and (cnt == -7).all().item() and (n_sel == -7).all().item()      # refused calls wrote nothing
    call(rows=0)                                      # an empty key column: its buffer is not read, every entry its own group
    torch.cuda.synchronize(dev)
    assert n_sel.tolist() == [4, 4] and pos.view(-1)[:16].tolist() == [0, -1, 1, -1, 2, -1, 3, -1] * 2   # written as [B][k_out * g]
    call(k_in=768, k_out=1, g=768)                    # the largest list, all of it one group (768 times row 0)
    torch.cuda.synchronize(dev)
    assert n_sel.tolist() == [1, 1] and cnt.view(-1)[:2].tolist() == [768, 768]
    assert pos.view(-1)[:1536].tolist() == list(range(768)) * 2


# --------------------------------------------------------------------------- hr_mask_keep_groups_dev
def _words(n_rows):
    return (n_rows + 63) // 64


def mask_dev(op, mask_in, n_rows, keys, key_set, alias=False):
    """mask_in: uint8 [8 * words] or None.  -> uint8 [8 * words] written by the kernel (prefilled with 0xFF)."""
    dev = torch.device("cuda", 0)
    d_keys = torch.from_numpy(keys).to(dev)
    d_set = torch.from_numpy(np.concatenate([key_set, np.zeros(1, np.int64)])).to(dev)
    d_in = torch.from_numpy(mask_in.copy()).to(dev) if mask_in is not None else None
    d_out = d_in if alias else torch.full((8 * _words(n_rows),), 0xFF, dtype=torch.uint8, device=dev)
    op(d_in.data_ptr() if d_in is not None else 0, d_out.data_ptr(), n_rows, d_keys.data_ptr(),
       d_set.data_ptr() if len(key_set) else 0, len(key_set), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    if d_in is not None and not alias:
        assert np.array_equal(d_in.cpu().numpy(), mask_in)       # the input is only read
    return d_out.cpu().numpy()


@pytest.mark.parametrize("n_keep", [0, 1, 768])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 20011])
def test_mask_keep_groups_equals_numpy(gpu, n_rows, n_keep):
    rng = np.random.default_rng(n_rows * 7 + n_keep)
    pool = rng.integers(-2000, 2000, 1500).astype(np.int64)
    special = np.array([I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, 0, -1, 1 << 32, (1 << 32) + 1, 1, -(1 << 32), 1 << 62], np.int64)
    pool = np.concatenate([pool, special])
    keys = rng.choice(pool, n_rows)
    keys[rng.integers(0, n_rows, min(n_rows, 8))] = rng.choice(special, min(n_rows, 8))
    if n_keep == 1:
        sets = [np.array([k], np.int64) for k in (keys[0], I64_MIN, I64_MAX, 1 << 32)]
    elif n_keep:
        d = np.concatenate([special[:6], rng.choice(keys, 300), rng.choice(pool, 400)])     # unsorted, with duplicates
        d = np.concatenate([d, rng.choice(d, n_keep - len(d))])
        sets = [rng.permutation(d)]
        assert len(sets[0]) == 768 and len(np.unique(sets[0])) < 768
    else:
        sets = [np.zeros(0, np.int64)]
    nbytes = 8 * _words(n_rows)
    random_mask = rng.integers(0, 256, nbytes).astype(np.uint8)    # bits at and beyond n_rows are garbage on purpose
    tail = np.arange(nbytes * 8) >= n_rows
    for key_set in sets:
        among = np.isin(keys, key_set)
        for mask_in, alias in ((None, False), (random_mask, False), (random_mask, True)):
            what = (len(key_set), mask_in is None, alias)
            kept = np.unpackbits(mask_dev(nat.mask_keep_groups_dev, mask_in, n_rows, keys, key_set, alias), bitorder="little")
            dropped = np.unpackbits(mask_dev(nat.mask_drop_groups_dev, mask_in, n_rows, keys, key_set, alias), bitorder="little")
            before = np.ones(n_rows, bool) if mask_in is None else np.unpackbits(mask_in, bitorder="little")[:n_rows].astype(bool)
            assert np.array_equal(kept[:n_rows].astype(bool), before & among), what
            assert not kept[tail].any() and not dropped[tail].any(), what        # the tail of the last word is written 0
            # the two senses split the input: keep | drop = input, keep & drop = nothing
            assert np.array_equal((kept | dropped)[:n_rows].astype(bool), before) and not (kept & dropped).any(), what
            if not len(key_set):
                assert not kept.any()                                            # n_keep == 0: an all-zero mask


def test_mask_keep_groups_limits_and_bad_arguments(gpu):
    dev = torch.device("cuda", 0)
    keys = torch.zeros(128, dtype=torch.int64, device=dev)
    keep = torch.zeros(769, dtype=torch.int64, device=dev)
    out = torch.full((24,), 0xFF, dtype=torch.uint8, device=dev)

    def call(mask_in=0, out=out.data_ptr(), n_rows=100, keys=keys.data_ptr(), keep=keep.data_ptr(), n_keep=4):
        nat.mask_keep_groups_dev(mask_in, out, n_rows, keys, keep, n_keep, 0)

    with pytest.raises(nat.HbmRagError) as ei:
        call(n_keep=769)
    assert ei.value.status == 5                       # HR_ELIMIT
    for bad in (dict(n_rows=-1), dict(n_keep=-1), dict(out=0), dict(keys=0), dict(keep=0), dict(out=out.data_ptr() + 4),
                dict(mask_in=out.data_ptr() + 1)):
        with pytest.raises(ValueError):               # HR_EINVAL
            call(**bad)
    call(n_rows=0)                                    # nothing to do: HR_OK, nothing launched
    call(n_rows=0, out=0, keys=0)
    torch.cuda.synchronize(dev)
    assert (out == 0xFF).all().item()                 # refused calls wrote nothing
    call(n_keep=768)                                  # the largest set is served: every row has key 0, and 0 is kept
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    assert (got[:12] == 0xFF).all() and got[12] == 0x0F and not got[13:16].any() and (got[16:] == 0xFF).all()
    call(n_keep=0, keep=0)                            # nothing kept
    torch.cuda.synchronize(dev)
    assert not out[:16].any().item() and (out[16:] == 0xFF).all().item()
