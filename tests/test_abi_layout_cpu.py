"""tests/abi_views.py on CPU tensors: the helper the layout tests of the C ABI stand on has to be right itself -- where the
window lies, what the pads hold, that ONE changed pad word is noticed wherever it sits, and which base alignment an
element offset gives."""
import numpy as np
import pytest
import torch

import abi_views as V


def _mat(rows, cols, dtype):
    return (np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) + 1.0).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rows,cols,ld,off", [(5, 7, 7, 0), (5, 7, 10, 1), (3, 4, 8, 2), (1, 1, 1, 4), (4, 300, 301, 1), (0, 5, 6, 3)])
def test_window_placement_and_fill(dtype, rows, cols, ld, off):
    m = _mat(rows, cols, dtype)
    buf, ptr = V.strided(m, ld, off, device="cpu")
    assert buf.dim() == 1 and buf.numel() == off + rows * ld + 8
    assert ptr == buf.data_ptr() + m.dtype.itemsize * off
    raw = buf.numpy()
    for i in range(rows):
        assert np.array_equal(raw[off + i * ld: off + i * ld + cols], m[i])
    assert np.array_equal(V.body(buf, rows, cols, ld, off), m)
    # every word outside the window holds the fill's bits: a quiet NaN with the payload
    words = raw.view(np.uint32 if dtype == np.float32 else np.uint64)
    inside = np.zeros(raw.size, dtype=bool)
    for i in range(rows):
        inside[off + i * ld: off + i * ld + cols] = True
    want = 0x7FC0DEAD if dtype == np.float32 else V.NAN64_BITS
    assert np.all(words[~inside] == want) and np.isnan(raw[~inside]).all()
    assert (~inside).sum() == raw.size - rows * cols
    assert V.pads_untouched(buf, rows, cols, ld, off)


def test_the_default_fill_is_a_quiet_nan_with_the_payload():
    assert V.fill_bits(np.float32) == 0x7FC0DEAD
    v = np.array([0x7FC0DEAD], dtype=np.uint32).view(np.float32)[0]
    assert np.isnan(v) and (0x7FC0DEAD >> 22) & 1 == 1          # quiet bit set
    assert np.isnan(np.array([V.NAN64_BITS], dtype=np.uint64).view(np.float64)[0])
    assert V.fill_bits(np.float32, -7.0) == 0xC0E00000 and V.fill_bits(np.float64, 0.0) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("fill", [None, -7.0])
def test_one_changed_pad_word_is_noticed(dtype, fill):
    rows, cols, ld, off = 4, 5, 9, 3
    m = _mat(rows, cols, dtype)
    pad_positions = {"lead-in first": 0, "lead-in last": off - 1, "between rows": off + cols, "before next row": off + ld - 1,
                     "behind the last row": off + (rows - 1) * ld + cols, "tail first": off + rows * ld, "tail last": off + rows * ld + 7}
    for where, idx in pad_positions.items():
        buf, _ = V.strided(m, ld, off, fill, device="cpu")
        assert V.pads_untouched(buf, rows, cols, ld, off, fill), where
        buf[idx] = 1.5
        assert not V.pads_untouched(buf, rows, cols, ld, off, fill), where
        assert V.touched_pads(buf, rows, cols, ld, off, fill).tolist() == [idx], where
    # another NaN is a change too (bit patterns are compared, not values), and so is the fill's own VALUE with other bits
    buf, _ = V.strided(m, ld, off, fill, device="cpu")
    buf[off + cols] = float("nan")
    assert not V.pads_untouched(buf, rows, cols, ld, off, fill)
    # a changed element of the window is not a pad
    buf, _ = V.strided(m, ld, off, fill, device="cpu")
    buf[off] = -1.0
    buf[off + (rows - 1) * ld + cols - 1] = -1.0
    assert V.pads_untouched(buf, rows, cols, ld, off, fill)


def test_signed_zero_is_a_changed_pad():
    m = _mat(2, 2, np.float32)
    buf, _ = V.strided(m, 3, 1, 0.0, device="cpu")
    buf[0] = -0.0
    assert not V.pads_untouched(buf, 2, 2, 3, 1, 0.0)


@pytest.mark.parametrize("off,want32,want64", [(0, 0, 0), (1, 4, 8), (2, 8, 0), (4, 0, 0), (3, 12, 8)])
def test_base_alignment_of_an_offset(off, want32, want64):
    for dtype, want in ((np.float32, want32), (np.float64, want64)):
        buf, ptr = V.strided(_mat(3, 5, dtype), 6, off, device="cpu")
        assert buf.data_ptr() % V.BASE_ALIGN == 0
        assert ptr % 16 == want == V.expected_align16(off, np.dtype(dtype).itemsize)
    v = V.View(_mat(3, 5, np.float32), 6, off, device="cpu")
    assert v.assert_aligned() % 16 == want32 and (v.rows, v.cols, v.ld, v.off) == (3, 5, 6, off)
    assert np.array_equal(v.body(), _mat(3, 5, np.float32)) and v.pads_untouched()


def test_view_notices_a_moved_pointer():
    v = V.View(_mat(2, 4, np.float32), 5, 1, device="cpu")
    v.ptr += 4
    with pytest.raises(AssertionError):
        v.assert_aligned()


def test_output_views_hold_the_sentinel_everywhere():
    o = V.View.output(3, 4, ld=7, off=1, device="cpu")
    assert np.all(o.buf.numpy() == -7.0) and o.pads_untouched()
    o.buf[1 + 7 + 2] = 3.0                      # the window: not a pad
    assert o.pads_untouched() and o.body()[1, 2] == 3.0
    o.buf[1 + 4] = 3.0                          # column 4 of row 0: a pad
    assert o.touched_pads().tolist() == [5]
    d = V.View.output(2, 3, ld=4, off=1, dtype=np.float64, device="cpu")
    assert d.buf.dtype == torch.float64 and d.assert_aligned() % 16 == 8
