"""Device tensors at a chosen byte offset inside a guarded allocation (tests/test_alignment_gpu.py).

A fresh torch allocation is at least 256-byte aligned, so a test that wants a buffer at 8, 4 or 1
mod 16 has to carve it out of a larger one.  The larger one is filled with 0xA5 first: what a
kernel writes outside the carved tensor -- a vector store that overruns a misaligned head or
tail -- shows up as a changed guard byte.

  buf, x = carve(img, 3)                 # img's bytes at base + 4096 + 3, x a tensor over them
  buf, y = carve_out(shape, dtype, 5)    # the same, nothing copied: an output
  untouched(buf, 5, y.nbytes)            # asserts every byte of buf outside y is still 0xA5
"""
import numpy as np

FILL = 0xA5
SLACK = 64  # room for the offset behind the array


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32,
            np.dtype(np.float64): torch.float64, np.dtype(np.int64): torch.int64,
            np.dtype(np.int32): torch.int32}[np.dtype(dtype)]


def carve_out(shape, dtype, offset, guard=4096, device="cuda"):
    """(buf, view): one uint8 device buffer of guard + 64 + nbytes + guard bytes of 0xA5, and a
    contiguous tensor of `dtype` and `shape` over its bytes [guard + offset, + nbytes).  offset
    must be a multiple of the itemsize (a float tensor keeps its natural alignment) and < 64."""
    import torch
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    assert 0 <= offset < SLACK and offset % dt.itemsize == 0 and guard % 256 == 0
    buf = torch.full((guard + SLACK + nbytes + guard,), FILL, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0  # the offsets are what they say only from an aligned base
    view = buf[guard + offset:guard + offset + nbytes].view(_torch_dtype(dt)).view(tuple(shape))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + guard + offset
    return buf, view


def carve(arr, offset, guard=4096, device="cuda"):
    """carve_out for arr's shape and dtype, with arr (a numpy array) copied in"""
    import torch
    arr = np.array(arr, order="C")  # a private copy: the caller's array may be read-only
    buf, view = carve_out(arr.shape, arr.dtype, offset, guard, device)
    view.copy_(torch.from_numpy(arr).to(device))
    return buf, view


def untouched(buf, offset, nbytes, guard=4096):
    """assert that both guards and the slack of a carved buffer still read 0xA5"""
    import torch
    if buf.is_cuda:
        torch.cuda.synchronize()
    lo, hi = guard + offset, guard + offset + nbytes
    assert buf.numel() == guard + SLACK + nbytes + guard
    head, tail = buf[:lo], buf[hi:]
    bad_h = torch.nonzero(head != FILL).reshape(-1)
    bad_t = torch.nonzero(tail != FILL).reshape(-1)
    assert bad_h.numel() == 0, f"bytes written before the tensor: at {(bad_h[:8] - lo).tolist()}"
    assert bad_t.numel() == 0, f"bytes written past the tensor: at +{bad_t[:8].tolist()}"
