"""The slot function of the sector-packed gather table (csrc/common.h gh_cg_slot, gh_cg_bytes) through its host copy in
the library (gh_compact_slot, gh_compact_bytes): 12-byte rows, five to a 64-byte sector.  No GPU."""
import numpy as np
import pytest

SPARE = 1024   # GH_POS_PAD_ROWS: the table covers the spare rows behind the n positions


@pytest.fixture(scope="module")
def lib():
    from graphem_rapids_amd import _native
    return _native.load()


def _slots(lib, count, v0=0):
    """The library's host copy of the device function over [v0, v0 + count)."""
    out = np.empty(count, dtype=np.int64)
    assert lib.gh_compact_slots(v0, count, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("n", [1, 4, 5, 6, 4099, 10**6])
def test_rows_are_disjoint_inside_one_sector_and_inside_the_table(lib, n):
    count = n + SPARE
    slot = _slots(lib, count)
    assert slot[0] == lib.gh_compact_slot(0) and slot[-1] == lib.gh_compact_slot(count - 1)
    assert np.array_equal(slot, (np.arange(count) // 5) * 16 + (np.arange(count) % 5) * 3)   # the layout as the issue states it
    # injective, and more: rows of three dwords do not overlap
    assert np.all(np.diff(slot) >= 3)
    # no row crosses a 64-byte boundary
    first, last = slot * 4, slot * 4 + 11
    assert np.array_equal(first // 64, last // 64)
    # the pad dword of a sector (dword 15) belongs to no row
    assert np.all(slot % 16 + 2 <= 14)
    # the last row lies inside the allocation, which is whole sectors
    total = lib.gh_compact_bytes(n)
    assert total == -(-(n + SPARE) // 5) * 64 and total % 64 == 0
    assert last[-1] < total


def test_multiply_high_division_is_exact_at_the_edges(lib):
    for v in [0, 1, 4, 5, 6, 2**16 - 1, 2**16, 5 * 2**20 - 1, 5 * 2**20, 2**27, 2**31 - 1, 2**31, 2**32 - 6, 2**32 - 1]:
        assert lib.gh_compact_slot(v) == (3 * v + v // 5) % 2**32, v   # (a 32-bit dword offset: the plan stops at 2^27 vertices)
    top = _slots(lib, 1 << 20, 2**32 - (1 << 20))   # the last million 32-bit vertex numbers: the division stays exact
    v = np.arange(2**32 - (1 << 20), 2**32, dtype=np.int64)
    assert np.array_equal(top, (3 * v + v // 5) % 2**32)
    assert lib.gh_compact_slot(-1) == -1 and lib.gh_compact_slot(2**32) == -1 and lib.gh_compact_bytes(-1) == -1
