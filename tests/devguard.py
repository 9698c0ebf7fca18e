"""Guard bands around caller-owned device buffers (tests/test_dev_bounds.py).

The `_dev` entries of include/legkilo_hip.h write into HBM the caller owns.  A store one piece too far, a gather that runs to the launch
size instead of `n`, a kernel that scribbles on its input: all of that lands in a neighbouring allocation, faults nothing and changes no
value a parity test looks at.  A `Guarded` buffer is one device allocation

    | leading band | payload | trailing band |

whose bands hold a position-dependent pattern (bytes of a seeded generator: a stray store of zeros, of 0x5a or of a copy of real data is
seen whatever its value - a written byte escapes only where it happens to equal the pattern byte at its position, one chance in 256 per
byte).  An OUTPUT payload is pre-filled with 0xFF bytes (NaN as f64 / f32, 255 as a `valid` byte, -1 as a count: never a legal result),
so "written" can be told from "left alone"; an INPUT payload keeps a host copy.  check() reads the whole allocation back once.

`GuardLayout` is the host side of it (pattern, image, verdict) and needs no device: the CPU self-test drives it on a host mirror.
"""
import zlib

import numpy as np

PAD = 256   # room for the payload offset: the allocation is band + PAD + nbytes + band bytes


class GuardError(AssertionError):
    """A band or an input payload came back changed.  side: "leading" | "trailing" | "input"; first / last: the first and last changed
    byte as offsets RELATIVE TO THE PAYLOAD's first byte (leading band: negative; trailing band: >= nbytes); count: changed bytes."""

    def __init__(self, name, side, first, last, count, nbytes):
        self.name, self.side, self.first, self.last, self.count, self.nbytes = name, side, int(first), int(last), int(count), int(nbytes)
        what = "input payload modified" if side == "input" else f"{side} guard band written"
        super().__init__(f"{name}: {what}: {self.count} byte(s) changed, first at payload offset {self.first:+d}, last at {self.last:+d} "
                         f"(payload = [0, {self.nbytes}) bytes)")


class GuardLayout:
    """Where the payload lies inside the allocation, what the bands hold, and the verdict on a read-back image."""

    def __init__(self, nbytes, offset=0, band=4096, seed=0, name="buffer"):
        assert nbytes >= 0 and 0 <= offset <= PAD and band >= 1
        self.nbytes, self.offset, self.band, self.name = int(nbytes), int(offset), int(band), name
        self.total = self.band + PAD + self.nbytes + self.band
        self.lo = self.band + self.offset          # payload = image[lo:hi]
        self.hi = self.lo + self.nbytes
        self.pattern = np.random.default_rng([0x6A12D, int(seed), self.nbytes, self.offset]).integers(0, 256, size=self.total, dtype=np.uint8)
        self.host_copy = None                      # an input's bytes

    def image(self, data=None):
        """The allocation's initial bytes: pattern | payload | pattern.  data = None: an output (0xFF); else the input's bytes."""
        img = self.pattern.copy()
        if data is None:
            img[self.lo:self.hi] = 0xFF
            self.host_copy = None
        else:
            b = np.frombuffer(np.ascontiguousarray(data).tobytes(), dtype=np.uint8)
            assert b.size == self.nbytes, (b.size, self.nbytes)
            img[self.lo:self.hi] = b
            self.host_copy = b.copy()
        return img

    def _diff(self, side, got, want, base):
        bad = np.flatnonzero(got != want)
        if bad.size:
            raise GuardError(self.name, side, base + bad[0], base + bad[-1], bad.size, self.nbytes)

    def verify(self, img):
        """Bands bit-identical to the pattern, an input bit-identical to its host copy -> the payload bytes (a copy)."""
        img = np.asarray(img, dtype=np.uint8)
        assert img.size == self.total
        self._diff("leading", img[:self.lo], self.pattern[:self.lo], -self.lo)
        self._diff("trailing", img[self.hi:], self.pattern[self.hi:], self.nbytes)
        if self.host_copy is not None:
            self._diff("input", img[self.lo:self.hi], self.host_copy, 0)
        return img[self.lo:self.hi].copy()


class Guarded:
    """One device_malloc(band + 256 + nbytes + band) of the handle `g`; the payload starts at base + band + offset.  `offset` is the
    smallest alignment the header grants the caller for the argument (16 for d_rows8 and lk_point arrays, 8 for doubles and lk_kin_imu,
    1 for bytes) - deliberately not 256.  data = None: an output payload (0xFF); else an input (host copy kept, checked by check())."""

    def __init__(self, g, nbytes, offset=0, band=4096, data=None, name=None):
        self.g = g
        name = name or "guarded"
        # the pattern depends on the buffer's name, size and offset only: a test's bytes do not depend on the tests that ran before it
        self.lay = GuardLayout(nbytes, offset, band, seed=zlib.crc32(name.encode()), name=name)
        self.base = g.device_malloc(self.lay.total)
        self.ptr = self.base + self.lay.lo
        self.nbytes = self.lay.nbytes
        g.h2d(self.base, self.lay.image(data))

    @classmethod
    def input(cls, g, arr, offset=0, band=4096, name=None):
        arr = np.ascontiguousarray(arr)
        return cls(g, arr.nbytes, offset, band, data=arr, name=name)

    def reset(self, data=None):
        """Bands and payload back to their initial bytes (an output: 0xFF again; or a new input of the same size)."""
        self.g.h2d(self.base, self.lay.image(data))

    def check(self):
        """Reads the allocation back once.  Raises GuardError naming the side, the first and last changed byte offset relative to the
        payload and the number of changed bytes; returns the payload bytes (uint8)."""
        img = np.zeros(self.lay.total, dtype=np.uint8)
        self.g.synchronize()
        self.g.d2h(img, self.base)
        return self.lay.verify(img)

    def read(self, dtype, count=None):
        """check(), then the payload (or its first `count` records) as `dtype`."""
        b = self.check()
        dt = np.dtype(dtype)
        n = b.size // dt.itemsize if count is None else int(count)
        return np.frombuffer(b[: n * dt.itemsize].tobytes(), dtype=dt)

    def free(self):
        if self.base:
            self.g.device_free(self.base)
            self.base = 0


def sentinel_free(arr):
    """No 0xFF-filled word in `arr`: every field of every record was written.  Words are the fields' own items (f64 / f32 / i32 / u8),
    so a legal value can only look like the sentinel if it IS the all-ones pattern - NaN with an all-ones payload, -1, 255 - which none of
    the checked outputs can hold."""
    arr = np.ascontiguousarray(arr)

    def words(a):
        if a.dtype.names:
            for f in a.dtype.names:
                yield from words(np.ascontiguousarray(a[f]))
        else:
            u = a.reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
            yield u, np.iinfo(u.dtype).max

    for u, ones in words(arr):
        bad = np.flatnonzero(u == ones)
        assert bad.size == 0, f"{bad.size} word(s) of the documented extent still hold the 0xFF sentinel, first at word {int(bad[0])} of {u.size}"
    return True


def untouched(payload_bytes):
    """The whole payload still holds its 0xFF fill (an output the call was told not to write)."""
    b = np.asarray(payload_bytes, dtype=np.uint8)
    bad = np.flatnonzero(b != 0xFF)
    assert bad.size == 0, f"{bad.size} byte(s) of an output that must stay untouched were written, first at offset {int(bad[0])}"
    return True
