"""The guard-band arena of the bounds tests (tests/arena.py) on a CPU tensor: layout, and that a byte written just outside
a buffer is reported with the buffer's name, the side and the offset.  No library needed."""
import numpy as np
import pytest
import torch

from tests import arena as A

SIZES = (1, 20, 255, 256, 257, 85 * 5 * 4, 4097)


def make(fill):
    ar = A.Arena("cpu", fill, A.capacity_for(SIZES))
    views = [ar.take(f"buf{k}", n) for k, n in enumerate(SIZES)]
    return ar, views


@pytest.mark.parametrize("fill", A.FILLS)
def test_layout(fill):
    ar, views = make(fill)
    assert A.BAND == 4096 and A.TAIL == 1 << 20 and A.BAND == 4 * 64 * 16
    prev_end = 0
    for (name, start, end), v, n in zip(ar.regions, views, SIZES):
        assert v.data_ptr() % 256 == 0 and v.data_ptr() == ar.base + start
        assert v.numel() == n == end - start and v.is_contiguous()        # exact, not rounded up
        assert start - A.BAND >= prev_end + (A.BAND if prev_end else 0)    # a whole band on either side, no overlap
        assert start - A.BAND - (prev_end + A.BAND) < A.ALIGN or prev_end == 0   # only alignment padding between bands
        assert (ar.mem[start - A.BAND:start] == fill).all() and (ar.mem[end:end + A.BAND] == fill).all()
        assert (v == fill).all()                                          # handed out uninitialised = the fill
        prev_end = end
    assert ar.mem.numel() - (prev_end + A.BAND) >= A.TAIL                  # the 1 MiB tail behind the last band
    assert ar.check() == []


def test_shapes_dtypes_and_uploads():
    ar = A.Arena("cpu", 0xFF, A.capacity_for([60, 15, 40, 3]))
    f = ar.take("f", (5, 3), torch.float32)
    assert f.shape == (5, 3) and f.dtype == torch.float32 and torch.isnan(f).all()
    b = ar.take("b", (3, 5), torch.int8)
    assert b.numel() == 15 and (b == -1).all()
    host = np.arange(10, dtype=np.int32)
    i = ar.take("i", host)
    assert i.dtype == torch.int32 and i.tolist() == host.tolist()
    h = ar.take("h", np.asarray([1, 2, 65535], np.uint16).view(np.int16))
    assert h.dtype == torch.int16 and h.numel() == 3
    assert ar.check() == []
    z = A.Arena("cpu", 0x00, A.capacity_for([16])).take("z", (4,), torch.float32)
    assert (z == 0).all()


def test_device_and_fill_alone_suffice():
    ar = A.Arena("cpu", 0xFF)                                              # the capacity is an optional hint
    v = ar.take("a", (1000,), torch.float32)
    assert v.data_ptr() % 256 == 0 and v.numel() == 1000 and ar.mem.numel() - ar.regions[-1][2] >= A.BAND + A.TAIL
    assert ar.check() == []


def test_only_the_two_fills():
    with pytest.raises(ValueError):
        A.Arena("cpu", 0xAB, 1 << 21)


def test_a_full_arena_refuses():
    ar = A.Arena("cpu", 0, A.capacity_for([100]))
    ar.take("a", 100)
    with pytest.raises(MemoryError):
        ar.take("b", 1 << 20)


@pytest.mark.parametrize("fill", A.FILLS)
@pytest.mark.parametrize("k", (0, 3, len(SIZES) - 1))
def test_one_byte_outside_is_reported(fill, k):
    ar, views = make(fill)
    name, start, end = ar.regions[k]
    other = 0x5A
    ar.mem[end] = other                                                    # one byte behind the last
    assert ar.check() == [(name, "after", end - start, 1)]
    ar.mem[end] = fill
    ar.mem[start - 1] = other                                              # one byte in front of the first
    assert ar.check() == [(name, "before", -1, 1)]
    ar.mem[start - 1] = fill
    views[k].fill_(other)                                                  # writes inside a buffer are no finding
    assert ar.check() == []


def test_far_writes_and_counts():
    ar, views = make(0xFF)
    name, start, end = ar.regions[2]
    ar.mem[end + 10:end + 26] = 0                                          # a 16-byte store ten bytes behind the end
    ar.mem[start - A.BAND] = 0                                             # the first byte of the leading band
    assert ar.check() == [(name, "before", -A.BAND, 1), (name, "after", end - start + 10, 16)]
    ar2, _ = make(0x00)
    last, ls, le = ar2.regions[-1]
    ar2.mem[-1] = 1                                                        # the last byte of the tail
    assert ar2.check() == [(last, "after", ar2.mem.numel() - 1 - ls, 1)]
