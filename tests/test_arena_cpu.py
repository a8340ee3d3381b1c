"""tests/arena.py on the CPU: layout, alignment, the three fills bit by bit, and that `untouched` / `stale` see a single byte."""
import numpy as np
import pytest
import torch

import arena as A


@pytest.mark.parametrize("fill,word,half", [("zeros", (0, 0), (0, 0)), ("nan", (0x7FC00BAD,) * 2, (0x7E01,) * 2),
                                            ("poison", (0x53800000, 0xD3800000), (0x7400, 0xF400))])
def test_layout_alignment_and_fill_words(fill, word, half):
    x = torch.arange(3 * 5 * 8, dtype=torch.float32).reshape(3, 5, 8)
    a, b = A.place(x, 256, 512, fill), A.place(x.half(), 0, 0, fill)
    for ar, src, front, behind in ((a, x, 256, 512), (b, x.half(), 0, 0)):
        assert ar.t.data_ptr() % A.ALIGN == A.OFFSET and torch.equal(ar.t, src) and ar.hi - ar.lo == src.numel() * src.element_size()
        assert ar.lo >= A.BAND + front and ar.buf.numel() - ar.hi >= A.BAND + behind and A.untouched(ar)
    w = a.buf.numpy().view(np.uint32)
    outside = np.r_[w[:a.lo // 4], w[a.hi // 4:]]  # t starts and ends at an even word
    assert (outside[0::2] == word[0]).all() and (outside[1::2] == word[1]).all()
    hw = b.buf.numpy().view(np.uint16)
    outside = np.r_[hw[:b.lo // 2], hw[b.hi // 2:]]
    assert (outside[0::2] == half[0]).all() and (outside[1::2] == half[1]).all()
    if fill == "poison":  # element i positive when i is even, +-2^40 / +-2^14
        assert a.buf[:8].view(torch.float32).tolist() == [2.0 ** 40, -2.0 ** 40] and b.buf[:4].view(torch.float16).tolist() == [2.0 ** 14, -2.0 ** 14]
    if fill == "nan":
        assert bool(torch.isnan(a.buf[:a.lo].view(torch.float32)).all()) and bool(torch.isnan(b.buf[b.hi:].view(torch.float16)).all())


def test_a_band_holds_a_frame():
    big = A.place(torch.zeros((3, 64, 32, 48)), 0, 0, "zeros")
    assert big.lo >= 64 * 32 * 48 * 4 and big.buf.numel() - big.hi >= 64 * 32 * 48 * 4


@pytest.mark.parametrize("where", ["front", "behind", "first byte", "last byte", "inside"])
def test_untouched_sees_one_byte(where):
    a = A.place(torch.ones((2, 3, 4)), 256, 256, "poison")
    o = A.place_out((2, 3, 4), torch.float16, "cpu")
    at = dict(front=lambda r: r.lo - 1, behind=lambda r: r.hi, inside=lambda r: r.lo + 5)
    at["first byte"], at["last byte"] = (lambda r: 0), (lambda r: r.buf.numel() - 1)
    for ar in (a, o):
        assert A.untouched(ar)
        ar.buf[at[where](ar)] += 1
    assert not A.untouched(a)                      # an input arena: its tensor must keep its contents too
    assert A.untouched(o) == (where == "inside")   # an output arena: the tensor is the kernel's to write


def test_stale_counts_elements_left_at_the_pattern():
    for dt, n in ((torch.float16, 2), (torch.float32, 4), (torch.float64, 8)):
        o = A.place_out((3, 4, 2), dt, "cpu")
        assert o.esize == n and o.stale() == 24 and bool((o.buf == 0xA5).all())
        o.t[1:] = 0.0
        assert o.stale() == 8 and A.untouched(o)
    assert A.pattern_free(np.zeros(4, np.float32), 4) and not A.pattern_free(np.array([0xA5A5A5A5], np.uint32).view(np.float32), 4)
    assert not A.pattern_free(np.array([1.0, 0.0], np.float16).view(np.uint16).__or__(np.array([0, 0xA5A5], np.uint16)).view(np.float16), 2)
