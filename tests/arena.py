"""A guard-band arena for the bounds tests: one allocation, buffers of exactly the documented size, bands between.

The library allocates nothing (include/gcnmaxcut.h): every array and workspace is the caller's, of the size the header
states.  A tensor from ``torch.empty`` cannot check that - the caching allocator rounds it up to 512 bytes and puts it
beside other live tensors - so the bounds tests (tests/test_gpu_bounds_*.py) take every piece of device memory from an
``Arena`` instead.

Layout of the one ``torch.uint8`` tensor an arena owns (``BAND`` = 4096 bytes, ``ALIGN`` = 256)::

    | pad | BAND | data 0 | BAND | pad to ALIGN | BAND | data 1 | BAND | pad | ... | BAND | data k | BAND | pad | TAIL |

- the first byte of every data region is 256-byte aligned (as an address, not only as an offset);
- a data region is exactly as long as was asked, never rounded up;
- a band of ``BAND`` bytes lies directly before the first and directly behind the last byte of every region: the
  alignment padding goes behind the trailing band, never between data and band.  4096 bytes is four times the widest
  store a wave can issue (64 lanes x 16 bytes);
- the arena ends with ``TAIL`` = 1 MiB more of band, so a stray access behind the last buffer still lands in memory the
  test owns.

``fill`` is 0xFF or 0x00 and nothing else: every band byte, every padding byte and every byte of a buffer handed out
uninitialised (outputs, workspace) holds it.  The reason for these two values: a band word that a kernel wrongly READS
and then uses as an index is -1 or 0 - both stay inside the arena (one element before a buffer's start is its leading
band, element 0 is the buffer itself), so such a bug is found by comparing results, without a wild access.  As floats
the two fills are NaN and 0.0, as class bytes 255 and 0: a read beyond a buffer that reaches a result makes the 0xFF
run and the 0x00 run differ.
"""
import numpy as np
import torch

BAND = 4096
ALIGN = 256
TAIL = 1 << 20
FILLS = (0xFF, 0x00)


def footprint(nbytes):
    """Bytes of arena one ``take`` of ``nbytes`` uses at most (bands, padding), for sizing an arena beforehand."""
    return 2 * BAND + (int(nbytes) + ALIGN - 1) // ALIGN * ALIGN + ALIGN


def capacity_for(sizes):
    """An arena capacity that holds one ``take`` for each of ``sizes`` (bytes), the tail included."""
    return sum(footprint(n) for n in sizes) + ALIGN + TAIL


DEFAULT_CAPACITY = 8 << 20


class Arena:
    """``Arena(device, fill)``; ``capacity`` (bytes, the tail included) is an optional hint for a caller that knows what
    it will take - `capacity_for` - so that the one tensor, which `check` copies whole, is no larger than needed."""

    def __init__(self, device, fill, capacity=DEFAULT_CAPACITY):
        if fill not in FILLS:
            raise ValueError(f"fill must be 0xFF or 0x00 (see the module docstring), got {fill!r}")
        self.fill = int(fill)
        self.device = torch.device(device)
        self.mem = torch.full((int(capacity),), self.fill, dtype=torch.uint8, device=self.device)
        self.base = self.mem.data_ptr()
        self.regions = []     # (name, start, end) offsets of the data regions, ascending
        self._next = 0        # offset of the next leading band

    def take(self, name, what, dtype=None):
        """A contiguous view of exactly the size asked, between two bands.  ``what``: a number of BYTES (the view is
        left holding the fill; ``dtype`` - a torch dtype - views it, default uint8), a shape tuple (of ``dtype``), or a
        host numpy array, which is uploaded (``dtype`` then defaults to the array's)."""
        host = None
        if isinstance(what, np.ndarray):
            host = np.ascontiguousarray(what)
            shape, nbytes = host.shape, host.nbytes
            t_dtype = dtype or torch.from_numpy(host[:0].reshape(-1)).dtype
        elif isinstance(what, (tuple, list)):
            t_dtype = dtype or torch.uint8
            shape = tuple(int(s) for s in what)
            nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=t_dtype).element_size()
        else:
            t_dtype = dtype or torch.uint8
            nbytes = int(what)
            item = torch.empty(0, dtype=t_dtype).element_size()
            if nbytes % item:
                raise ValueError(f"{name}: {nbytes} bytes are no whole number of {t_dtype}")
            shape = (nbytes // item,)
        start = self._next + BAND
        start += -(self.base + start) % ALIGN          # padding in front of the leading band only
        end = start + nbytes
        if end + BAND + TAIL > self.mem.numel():
            raise MemoryError(f"{name}: arena of {self.mem.numel()} bytes is full")
        self.regions.append((name, start, end))
        self._next = end + BAND                        # (the next take pads from here: behind this trailing band)
        view = self.mem[start:end]
        if host is not None:
            view.copy_(torch.from_numpy(host.reshape(-1).view(np.uint8)))
        return view.view(t_dtype).reshape(shape)

    def check(self):
        """Copies the arena to the host once; for every band that is not all ``fill`` returns
        ``(buffer name, "before" | "after", first offending offset, count)``.  Offsets count bytes from the buffer's
        first byte for "before" (so they are negative: -1 is the byte in front of it) and from its first byte for
        "after" as well (so the byte behind the last one has offset = the buffer's length).  The bytes between two
        buffers are split at the next buffer's leading band; the tail belongs to the last buffer's "after"."""
        host = self.mem.cpu().numpy()
        found = []
        prev_end, prev = 0, None
        for k, (name, start, end) in enumerate(self.regions):
            lead = start - BAND
            if prev is not None:
                bad = np.flatnonzero(host[prev_end:lead] != self.fill)
                if bad.size:
                    found.append((prev[0], "after", int(prev_end + bad[0] - prev[1]), int(bad.size)))
            lo = lead if prev is not None else 0
            bad = np.flatnonzero(host[lo:start] != self.fill)
            if bad.size:
                found.append((name, "before", int(lo + bad[0] - start), int(bad.size)))
            prev_end, prev = end, (name, start, end)
        if prev is not None:
            bad = np.flatnonzero(host[prev_end:] != self.fill)
            if bad.size:
                found.append((prev[0], "after", int(prev_end + bad[0] - prev[1]), int(bad.size)))
        elif (host != self.fill).any():
            bad = np.flatnonzero(host != self.fill)
            found.append(("<empty arena>", "after", int(bad[0]), int(bad.size)))
        return found
