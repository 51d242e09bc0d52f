"""hr_mask_rows_dev alone (include/hbmrag.h, csrc/query.h): a packed row mask -> the count of its set bits and one page
of row ids, against np.flatnonzero(bits[:n])[offset:offset + limit] + first_row.  Sizes sit on both sides of a word, of a
wave's 64 words, of a scan block's 1024 words, and span four blocks so that the block sums matter."""
import numpy as np
import pytest

from advanced_rag import _native as nat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -0x0123456789ABCDEF
N_ROWS = [1, 63, 64, 65, 4095, 4097, 65536, 65537, 200003]
FIRST_ROWS = [0, 10 ** 10]


def _masks(rng, n):
    last = np.zeros(n, bool)
    last[-1] = True
    first = np.zeros(n, bool)
    first[0] = True
    return {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool), "last": last, "first": first,
            "half": rng.random(n) < 0.5, "sparse": rng.random(n) < 0.001}


def _device_mask(bits, garbage):
    """8 * ceil(n / 64) bytes in HBM; garbage = the bits beyond n in the last word set to ones."""
    n = len(bits)
    padded = np.zeros(64 * ((n + 63) // 64), bool)
    padded[:n] = bits
    if garbage:
        padded[n:] = True
    return torch.from_numpy(np.packbits(padded, bitorder="little")).cuda()


def _launch(d_mask, n, first_row, offset, limit, scratch):
    """One call -> (counts [2], the whole sentinel-prefilled output buffer of limit + 8 entries)."""
    rows = torch.full((limit + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda")
    nat.mask_rows_dev(d_mask.data_ptr() if d_mask is not None else 0, n, first_row, offset, limit, rows.data_ptr(),
                      counts.data_ptr(), scratch.data_ptr(), 0)
    return counts.cpu().numpy(), rows.cpu().numpy()


def _windows(count):
    offsets = sorted({o for o in (0, 1, 63, 64, count - 1, count, count + 5) if o >= 0})
    limits = sorted({0, 1, 64, 1000, count + 10})
    return [(o, lim) for o in offsets for lim in limits]


@pytest.mark.parametrize("n", N_ROWS)
def test_pages_equal_flatnonzero(gpu, n):
    rng = np.random.default_rng(n)
    scratch = torch.empty(nat.mask_rows_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    cases = [(name, bits, g) for name, bits in _masks(rng, n).items() for g in (False, True)]
    cases.append(("null", None, False))
    for name, bits, garbage in cases:
        d_mask = _device_mask(bits, garbage) if bits is not None else None
        want_all = np.flatnonzero(bits) if bits is not None else np.arange(n)
        count = len(want_all)
        for offset, limit in _windows(count):
            for first_row in FIRST_ROWS:
                counts, rows = _launch(d_mask, n, first_row, offset, limit, scratch)
                want = want_all[offset:offset + limit] + first_row
                tag = (name, garbage, offset, limit, first_row)
                assert counts.tolist() == [count, len(want)], tag
                assert np.array_equal(rows[:len(want)], want), tag
                assert (rows[len(want):] == SENTINEL).all(), tag
        # the result is a function of the inputs alone: two identical launches, identical buffers
        for offset, limit in ((0, count + 10), (1, 1000)):
            a, b = _launch(d_mask, n, 7, offset, limit, scratch), _launch(d_mask, n, 7, offset, limit, scratch)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, garbage, offset, limit)


def test_empty_mask_and_zero_limit_still_write_the_counts(gpu):
    scratch = torch.empty(nat.mask_rows_scratch_bytes(0), dtype=torch.uint8, device="cuda")
    empty = torch.zeros(8, dtype=torch.uint8, device="cuda")
    for d_mask in (None, empty):
        counts, rows = _launch(d_mask, 0, 5, 0, 10, scratch)
        assert counts.tolist() == [0, 0] and (rows == SENTINEL).all()
    d_mask = _device_mask(np.ones(100, bool), True)
    scratch = torch.empty(nat.mask_rows_scratch_bytes(100), dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda")
    nat.mask_rows_dev(d_mask.data_ptr(), 100, 0, 3, 0, 0, counts.data_ptr(), scratch.data_ptr(), 0)   # no id buffer at limit 0
    assert counts.cpu().tolist() == [100, 0]


def test_scratch_size_covers_the_block_sums():
    assert nat.mask_rows_scratch_bytes(0) >= 16
    assert nat.mask_rows_scratch_bytes(65536) >= 16 and nat.mask_rows_scratch_bytes(65537) >= 24
    assert nat.mask_rows_scratch_bytes(200003) >= 8 * 5
    assert nat.mask_rows_scratch_bytes(10_000_000) <= 4096          # 10M rows: 153 blocks


def test_bad_arguments_are_refused(gpu):
    d_mask = _device_mask(np.ones(100, bool), False)
    scratch = torch.empty(nat.mask_rows_scratch_bytes(100), dtype=torch.uint8, device="cuda")
    rows = torch.full((16,), SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda")
    m, r, c, s = d_mask.data_ptr(), rows.data_ptr(), counts.data_ptr(), scratch.data_ptr()
    for args in ((m, -1, 0, 0, 8, r, c, s), (m, 100, 0, -1, 8, r, c, s), (m, 100, 0, 0, -1, r, c, s),
                 (m, 100, 0, 0, 8, 0, c, s), (m, 100, 0, 0, 8, r, 0, s), (0, 100, 0, 0, 8, r, 0, s)):
        with pytest.raises(ValueError):
            nat.mask_rows_dev(*args, 0)
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == SENTINEL).all() and (counts.cpu().numpy() == SENTINEL).all()   # a refused call launches nothing
