"""CPU: tests/carve.py puts a tensor where it says and notices a byte written outside it."""
import numpy as np
import pytest

from carve import FILL, carve, carve_out, untouched


@pytest.mark.parametrize("dtype,offset", [(np.uint8, 0), (np.uint8, 1), (np.uint8, 13),
                                          (np.float32, 4), (np.float32, 12), (np.float64, 8)])
def test_carve_places_the_array(dtype, offset):
    arr = (np.arange(2 * 3 * 5) % 251).astype(dtype).reshape(2, 3, 5)
    arr.setflags(write=False)
    buf, view = carve(arr, offset, device="cpu")
    assert view.shape == arr.shape and view.is_contiguous()
    assert view.data_ptr() == buf.data_ptr() + 4096 + offset and buf.data_ptr() % 16 == 0
    assert np.array_equal(view.numpy(), arr)
    assert buf.numel() == 4096 + 64 + arr.nbytes + 4096
    untouched(buf, offset, arr.nbytes)
    out_buf, out = carve_out(arr.shape, dtype, offset, device="cpu")
    assert np.all(out.numpy().view(np.uint8) == FILL)
    untouched(out_buf, offset, arr.nbytes)


def test_carve_refuses_an_offset_off_the_item_size():
    with pytest.raises(AssertionError):
        carve_out((4,), np.float32, 2, device="cpu")
    with pytest.raises(AssertionError):
        carve_out((4,), np.float64, 4, device="cpu")


@pytest.mark.parametrize("where", [-1, -4096 - 5, 24, 24 + 58, 24 + 59 + 4095])
def test_untouched_sees_one_stray_byte(where):
    """one byte changed just before, far before, just past, in the slack and at the very end"""
    buf, view = carve_out((24,), np.uint8, 5, device="cpu")
    view.fill_(0)           # the tensor's own bytes may be anything
    untouched(buf, 5, 24)
    buf[4096 + 5 + where] = 0
    with pytest.raises(AssertionError, match="bytes written"):
        untouched(buf, 5, 24)
