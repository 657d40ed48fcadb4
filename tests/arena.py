"""Arrays at chosen byte offsets inside one 16-byte-aligned allocation, for the tests that call the library
on raw pointers and compare EVERY byte: the arrays, the guard bytes between them and around them.

The host side is one numpy uint8 buffer with (possibly unaligned) typed views into it; the device side is one
uint8 tensor of the same bytes, from which the pointers are taken.  A test fills the host buffer, copies it,
applies the numpy restatement of the kernel's index rule to the copy's views, runs the kernel on the device
bytes and compares the two buffers whole."""
import numpy as np
import torch

GUARD = 16
# byte offsets past a 16-byte boundary that the tests give (source doubles, destination doubles, source
# int32s, destination int32s): between them the unit rule picks 16-, 8- and 4-byte units
OFFSETS = ((0, 0, 0, 0), (8, 8, 4, 4), (0, 8, 8, 8), (8, 0, 12, 0), (0, 0, 0, 8), (8, 8, 8, 4))


class Arena:
    def __init__(self):
        self.at, self.size = {}, GUARD

    def add(self, name, dtype, shape, offset=0):
        """`name`: an array of `dtype` and `shape` that begins `offset` bytes past a 16-byte boundary, with at
        least GUARD bytes that belong to no array on either side."""
        start = -(-self.size // 16) * 16 + offset
        self.at[name] = (start, np.dtype(dtype), tuple(shape))
        self.size = start + int(np.prod(shape)) * np.dtype(dtype).itemsize + GUARD

    def random(self, rng):
        """The host buffer filled with random bits; of every float64 array a quarter are NaNs with random
        payloads (quiet and signalling, either sign): those whose two lowest bits are 0."""
        words = rng.integers(0, 2 ** 64, self.size // 8 + 1, dtype=np.uint64, endpoint=False)
        buf = words.view(np.uint8)[:self.size]
        for name, (_, dtype, _) in self.at.items():
            if dtype == np.float64:
                bits = self.view(buf, name).view(np.uint64)
                np.bitwise_or(bits, np.uint64(0x7FF0000000000004), out=bits, where=(bits & np.uint64(3)) == 0)
        return buf

    def view(self, buf, name):
        start, dtype, shape = self.at[name]
        n = int(np.prod(shape)) * dtype.itemsize
        return buf[start:start + n].view(dtype).reshape(shape)

    def views(self, buf, names):
        return {k: self.view(buf, k) for k in names}

    def upload(self, buf, device):
        dev = torch.from_numpy(buf).to(device)
        assert dev.data_ptr() % 16 == 0
        return dev

    def ptr(self, dev, name):
        return dev.data_ptr() + self.at[name][0]


def same_bytes(got, want, arena):
    """Every byte equal; on a difference, the arrays (or 'guard') that hold the differing bytes."""
    if np.array_equal(got, want):
        return True
    bad = np.flatnonzero(got != want)
    where = set()
    for i in bad[:64]:
        where.add(next((k for k, (s, d, sh) in arena.at.items() if s <= i < s + int(np.prod(sh)) * d.itemsize), "guard"))
    print("bytes differ in:", sorted(where), "first at", int(bad[0]), "of", len(bad))
    return False
