"""CPU: the guard-band helper (tests/guarded.py) catches what tests/test_gpu_abi_contract.py relies on it to catch -- one stray
element anywhere outside the logical region, one unwritten element inside it -- for every dtype the kernels write."""
import pytest
import torch

from guarded import guarded, sentinel_bits, strided_input

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.uint8]
ROWS, COLS, LD, GUARD = 5, 7, 11, 64


def _filled(dtype):
    g = guarded((ROWS, COLS), dtype, "cpu", ld=LD, guard=GUARD)
    vals = (torch.arange(ROWS * COLS).reshape(ROWS, COLS) % 100 + 1).to(dtype)       # (never the sentinel pattern)
    g.view.copy_(vals)
    return g, vals


@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_buffer_passes(dtype):
    g, vals = _filled(dtype)
    assert g.view.shape == (ROWS, COLS) and g.view.stride() == (LD, 1) and g.ld == LD
    assert g.view.data_ptr() % 16 == 0
    assert g.flat.numel() == 2 * GUARD + ROWS * LD
    g.assert_untouched()
    g.assert_fully_written()
    assert torch.equal(g.view, vals)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fresh_buffer_is_all_sentinel_and_counts_as_unwritten(dtype):
    g = guarded((ROWS, COLS), dtype, "cpu", ld=LD, guard=GUARD)
    idt, bits = sentinel_bits(dtype)
    assert bool((g.flat.view(idt) == bits).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(g.flat.float()).all())                               # the sentinel is a NaN: padding poisons sums
    g.assert_untouched()
    with pytest.raises(AssertionError, match=r"row 0, column 0"):
        g.assert_fully_written()
    assert not bool(g.written_mask().any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_stray_store_in_the_row_padding_is_caught(dtype):
    g, _ = _filled(dtype)
    g.flat[GUARD + 3 * LD + COLS] = 1                                                # row 3, first padding column
    with pytest.raises(AssertionError, match=rf"row padding written at \(row 3, column {COLS}\)"):
        g.assert_untouched()
    g.assert_fully_written()
    g2, _ = _filled(dtype)
    g2.flat[GUARD + 4 * LD + LD - 1] = 0                                             # last padding element of the last row
    with pytest.raises(AssertionError, match=rf"row 4, column {LD - 1}"):
        g2.assert_untouched()


@pytest.mark.parametrize("dtype", DTYPES)
def test_stray_store_in_the_front_guard_is_caught(dtype):
    g, _ = _filled(dtype)
    g.flat[GUARD - 1] = 1                                                            # the element just before row 0
    with pytest.raises(AssertionError, match=r"front guard written at offset -1 "):
        g.assert_untouched()
    g2, _ = _filled(dtype)
    g2.flat[0] = 1
    with pytest.raises(AssertionError, match=rf"front guard written at offset -{GUARD} "):
        g2.assert_untouched()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [0, GUARD - 1])
def test_stray_store_in_the_rear_guard_is_caught(dtype, offset):
    g, _ = _filled(dtype)
    g.flat[GUARD + ROWS * LD + offset] = 1
    with pytest.raises(AssertionError, match=rf"rear guard written at offset {offset} "):
        g.assert_untouched()
    g.assert_fully_written()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_unwritten_logical_element_is_caught(dtype):
    g = guarded((ROWS, COLS), dtype, "cpu", ld=LD, guard=GUARD)
    vals = torch.ones(ROWS, COLS, dtype=dtype)
    g.view[:2].copy_(vals[:2])
    g.view[3:].copy_(vals[3:])
    g.view[2, :4].copy_(vals[2, :4])
    g.view[2, 5:].copy_(vals[2, 5:])                                                 # everything but (2, 4)
    g.assert_untouched()
    with pytest.raises(AssertionError, match=r"row 2, column 4.*\(1 unwritten"):
        g.assert_fully_written()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_store_counts_as_a_store(dtype):
    """The comparison is on bits: writing 0 (or any value but the sentinel itself) is seen, in the guards and in the body."""
    g = guarded((ROWS, COLS), dtype, "cpu", ld=LD, guard=GUARD)
    g.view.zero_()
    g.assert_fully_written()
    g.assert_untouched()
    g.flat[GUARD + ROWS * LD] = 0
    with pytest.raises(AssertionError):
        g.assert_untouched()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tight_and_flat_shapes(dtype):
    g = guarded((3, 4, 6), dtype, "cpu", guard=32)                                   # leading dimensions flatten into rows, ld = cols
    assert g.view.shape == (12, 6) and g.ld == 6 and g.view.is_contiguous()
    g.view.fill_(1)
    g.assert_untouched()
    g.assert_fully_written()
    v = guarded(9, dtype, "cpu", guard=32)                                           # a vector: one row
    assert v.view.shape == (1, 9)
    v.flat[32 + 9] = 1
    with pytest.raises(AssertionError, match="rear guard written at offset 0 "):
        v.assert_untouched()


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_input_copies_and_poisons_the_padding(dtype):
    t = (torch.arange(ROWS * COLS).reshape(ROWS, COLS) % 50 + 1).to(dtype)
    s = strided_input(t, LD)
    assert s.shape == t.shape and s.stride() == (LD, 1) and s.data_ptr() % 16 == 0 and torch.equal(s, t)
    idt, bits = sentinel_bits(dtype)
    wide = s.as_strided((ROWS, LD), (LD, 1))                                         # the rows with their padding
    assert bool((wide.view(idt)[:, COLS:] == bits).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(wide.float().sum(1)).all())                          # a kernel that sums the padding yields NaN
