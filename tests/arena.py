"""Arenas for the layer tests: a tensor handed to a kernel sits inside ONE larger allocation the test owns,

    [band][front][t][behind][band]

so that whatever the kernel reads in front of or behind the tensor is a value the test chose, and whatever it writes there is seen.
`front` / `behind` are the bytes the C header lets a kernel read around the tensor (none for most arguments); a band is at least
BAND bytes and at least one frame of t (t.shape[0] frames), so a fetch that runs a whole row, plane or frame past the tensor still
lands in memory of the test.  The tensor starts 256 bytes past a 512-byte boundary (OFFSET past ALIGN): the alignment
Engine.debug_layer's staging gives an fp16 input -- the smallest the kernels are ever handed.

Everything outside t holds one of the fills, as 16-bit words around a 2-byte element type and as 32-bit words otherwise, word i
counted from the start of the allocation (t starts at an even word):
  "zeros"  0: what the staging buffers of Engine.debug_layer hold -- equal to the padding value of a convolution, so a broken
           mask that reads them goes unseen
  "nan"    a quiet NaN with a payload (fp32 0x7FC00BAD, fp16 0x7E01)
  "poison" +-2^40 (fp16 +-2^14), word i positive when i is even: finite, so no max / med3 drops it the way it drops a NaN, and of
           both signs, so one of two neighbouring words survives relu(x * scale + shift) whatever the sign of scale
  "a5"     the byte 0xA5, for outputs: the tensor region holds it too (place_out), so an element the kernel never stored shows.
  "5a"     the byte 0x5A, a second pre-fill for outputs: two runs whose outputs start as 0xA5 and as 0x5A can only end with equal bits
           in the elements the kernel stored, so comparing them finds an element it never stored without naming a pattern.
untouched(arena): every byte outside t still holds the fill (integer comparison of the bytes, no float semantics).

`offset` (default OFFSET) moves the tensor's start within its 512-byte block: 260 gives a 4-byte element type an address that is
4-byte aligned only (% 16 == 4), 264 an 8-byte one that is 8-byte aligned only, 272 one that is 16-byte aligned and no more.  An input
whose tensor the kernel updates in place is place(..., inplace=True): it keeps its contents, and untouched() then compares the
surroundings alone, as for an output."""
import numpy as np
import torch

BAND = 64 * 1024
ALIGN, OFFSET = 512, 256
FILLS = ("zeros", "nan", "poison")
OUT_FILLS = {"a5": 0xA5, "5a": 0x5A}  # pre-fill bytes of an output arena
_WORDS = {("nan", 4): (0x7FC00BAD, 0x7FC00BAD), ("nan", 2): (0x7E01, 0x7E01),
          ("poison", 4): (0x53800000, 0xD3800000), ("poison", 2): (0x7400, 0xF400),  # +-2^40, +-2^14
          ("zeros", 4): (0, 0), ("zeros", 2): (0, 0), ("a5", 4): (0xA5A5A5A5, 0xA5A5A5A5), ("a5", 2): (0xA5A5, 0xA5A5)}


_PAIRS = {}


def fill_words(fill, esize, nbytes, device):
    """nbytes (a multiple of 4) of fill `fill` as a uint8 tensor: 16-bit words for esize 2, 32-bit words otherwise"""
    ws = 2 if esize == 2 else 4
    key = (fill, ws, str(device))
    if key not in _PAIRS:  # the two words as bytes, on the device
        _PAIRS[key] = torch.from_numpy(np.array(_WORDS[(fill, ws)], dtype=np.uint16 if ws == 2 else np.uint32).view(np.uint8).copy()).to(device)
    assert nbytes % (2 * ws) == 0
    return _PAIRS[key].repeat(nbytes // (2 * ws))


class Arena:
    """buf: the whole allocation (uint8); t: the tensor view inside it; lo, hi: t's byte range in buf; snap: a copy of buf taken by
    seal() once t holds its contents; out: an output arena (the kernel is expected to write t)"""

    def __init__(self, shape, dtype, device, front_bytes, behind_bytes, fill, offset=OFFSET):
        esize = torch.empty((), dtype=dtype).element_size()
        assert 0 <= offset < ALIGN and offset % esize == 0, (offset, esize)
        nbytes = int(np.prod(shape)) * esize
        band = max(BAND, -(-nbytes // max(1, int(shape[0]))))
        raw = torch.empty(2 * band + front_bytes + nbytes + behind_bytes + 3 * ALIGN, dtype=torch.uint8, device=device)
        skip = (-raw.data_ptr()) % ALIGN                   # the allocator aligns to 512 already; not relied on
        lo = band + front_bytes
        lo += (offset - (raw.data_ptr() + skip + lo)) % ALIGN
        total = (lo + nbytes + behind_bytes + band + 7) & ~7
        self.buf = raw[skip:skip + total]
        assert total <= raw.numel() - skip and lo >= band + front_bytes and total - (lo + nbytes) >= behind_bytes + band
        if fill in OUT_FILLS:
            self.buf.fill_(OUT_FILLS[fill])
        else:
            self.buf.copy_(fill_words(fill, esize, total, device))
        self.lo, self.hi, self.fill, self.esize, self.out, self.snap = lo, lo + nbytes, fill, esize, fill in OUT_FILLS, None
        self.t = self.buf[lo:lo + nbytes].view(dtype).view(shape)
        assert self.t.data_ptr() % ALIGN == offset and self.t.data_ptr() == self.buf.data_ptr() + lo

    def seal(self):
        self.snap = self.buf.clone()
        return self

    @property
    def ptr(self):
        return self.t.data_ptr()

    def words(self):
        """t as integers of its element size"""
        return self.t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.esize])

    def stale(self):
        """number of elements of t that still hold the byte pattern 0xA5 (place_out arenas)"""
        pattern = int.from_bytes(b"\xa5" * self.esize, "little", signed=self.esize > 1)
        return int((self.words() == pattern).sum())


def place(t, front_bytes=0, behind_bytes=0, fill="zeros", offset=OFFSET, inplace=False):
    """Arena whose .t has t's shape, type and contents; `front_bytes` / `behind_bytes` of contractual slack, then the bands, all `fill`.
    inplace: the kernel may rewrite the tensor, so untouched() judges the surroundings alone."""
    a = Arena(tuple(t.shape), t.dtype, t.device, front_bytes, behind_bytes, fill, offset)
    a.t.copy_(t)
    a.out = bool(inplace)
    return a.seal()


def place_out(shape, dtype, device="cuda", fill="a5", offset=OFFSET):
    """Arena for an output: tensor region and surroundings pre-filled with the byte 0xA5 (fill "5a": 0x5A)"""
    assert fill in OUT_FILLS
    return Arena(tuple(shape), dtype, torch.device(device), 0, 0, fill, offset).seal()


def untouched(arena):
    """True when every byte outside the tensor still holds the fill -- and, for an input arena (place), the tensor its contents: one
    integer comparison of the whole allocation with its snapshot, which for an output arena first takes over what the tensor holds now"""
    if arena.out:
        arena.snap[arena.lo:arena.hi] = arena.buf[arena.lo:arena.hi]
    return bool(torch.equal(arena.buf, arena.snap))


def pattern_free(a, esize):
    """CPU side: no element of the numpy array `a` (viewed as integers of `esize` bytes) equals the 0xA5 pattern"""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == esize
    return not (a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[esize]) == int.from_bytes(b"\xa5" * esize, "little")).any()
