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


@pytest.mark.parametrize("dtype,offset,mod16", [(torch.float32, 260, 4), (torch.int32, 260, 4), (torch.uint8, 260, 4), (torch.float64, 264, 8),
                                                (torch.float32, 264, 8), (torch.float32, 272, 0), (torch.float32, A.OFFSET, 0)])
def test_offset_places_the_tensor_at_that_alignment(dtype, offset, mod16):
    x = torch.arange(3 * 5 * 7).reshape(3, 5, 7).to(dtype)
    for fill in A.FILLS:
        a = A.place(x, 0, 0, fill, offset=offset)
        assert a.ptr % A.ALIGN == offset and a.ptr % 16 == mod16 and torch.equal(a.t, x) and A.untouched(a)
        assert a.lo >= A.BAND and a.buf.numel() - a.hi >= A.BAND
        if offset == 272:
            assert a.ptr % 32 == 16  # 16-byte aligned and no more
        a.buf[a.lo - 1] += 1
        assert not A.untouched(a)
    o = A.place_out((3, 5, 7), dtype, "cpu", offset=offset)
    assert o.ptr % A.ALIGN == offset and o.out and bool((o.buf == 0xA5).all())
    with pytest.raises(AssertionError):
        A.place(x, offset=A.ALIGN)
    if x.element_size() == 8:
        with pytest.raises(AssertionError):
            A.place(x, offset=260)


def test_default_offset_is_unchanged():
    x = torch.ones((2, 3), dtype=torch.float16)
    a, b = A.place(x, 0, 0, "poison"), A.place(x, 0, 0, "poison", offset=A.OFFSET)
    assert a.lo == b.lo and a.hi == b.hi and torch.equal(a.buf, b.buf) and not a.out and not b.out
    o, p = A.place_out((2, 3), torch.float16, "cpu"), A.place_out((2, 3), torch.float16, "cpu", fill="a5")
    assert o.lo == p.lo and torch.equal(o.buf, p.buf) and o.fill == p.fill == "a5"


def test_second_output_prefill():
    o, p = A.place_out((4, 3), torch.float32, "cpu"), A.place_out((4, 3), torch.float32, "cpu", fill="5a")
    assert p.out and p.fill == "5a" and bool((p.buf == 0x5A).all()) and bool((o.buf == 0xA5).all())
    assert not torch.equal(o.words(), p.words())  # an element neither run stores differs between the two
    o.t[:] = 1.5
    p.t[:] = 1.5
    assert torch.equal(o.words(), p.words()) and A.untouched(o) and A.untouched(p)
    p.t[1, 1] = torch.tensor([0x5A5A5A5A], dtype=torch.int32).view(torch.float32)[0]  # left as it was
    assert not torch.equal(o.words(), p.words())
    p.buf[p.hi] ^= 0xFF
    assert not A.untouched(p)
    with pytest.raises(AssertionError):
        A.place_out((2,), torch.float32, "cpu", fill="nan")


def test_inplace_arena_compares_the_surroundings_alone():
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    a = A.place(x, 0, 0, "nan", inplace=True)
    assert a.out and torch.equal(a.t, x) and A.untouched(a)
    a.t.mul_(2.0)
    assert A.untouched(a) and torch.equal(a.t, 2 * x)
    a.buf[a.hi + 3] += 1
    assert not A.untouched(a)


def test_helpers_of_the_training_arena_module():
    """The comparison helpers of tests/test_train_arena_gpu.py: a poison tensor is arena's fill, and bit equality sees one bit and
    takes equal NaNs as equal."""
    import test_train_arena_gpu as T
    p = T.poison_like((3, 5))
    a = A.place(torch.zeros((2, 2)), 0, 0, "poison")
    assert np.array_equal(p.reshape(-1)[:8].view(np.uint32), a.buf[:32].numpy().view(np.uint32)) and p.dtype == np.float32
    x = torch.tensor([1.0, float("nan"), -0.0, 2.0 ** 40])
    T.assert_same({"t": x.clone()}, {"t": x.clone()}, "equal")
    for i in range(4):
        y = x.clone()
        T.bits(y)[i] ^= 1
        with pytest.raises(AssertionError, match="t differs in 1 of 4"):
            T.assert_same({"t": y}, {"t": x}, "one bit")
    with pytest.raises(AssertionError):
        T.assert_same({"t": x, "u": x}, {"t": x}, "another set of outputs")
    for align, off in T.ODD_OFFSET.items():  # exactly that alignment and no more
        assert off % align == 0 and off % (2 * align) != 0 and 0 < off < A.ALIGN


def test_argument_order_is_the_tabulated_one():
    """call_of of tests/test_train_arena_gpu.py lays its arguments out as tests/test_trainargs_gpu.py tabulates the ABI."""
    import test_train_arena_gpu as T
    from test_trainargs_gpu import SPEC
    scalars = {"mode", "C", "h", "w", "cin", "cout", "hin", "win", "branch", "nb", "chunk_frames", "stream"}
    shapes = {"unit": T.UNIT_SHAPES[0], "down": T.DOWN_SHAPES[0], "neck": T.NECK_MAPS[0]}
    seen = set()
    for fam in shapes:
        for form in T.FORMS:
            for mode in ((0, 1) if form == "in" else (0,)):  # the table has the _mp twins of the InstanceNorm entries
                entry, ints, args = T.call_of(fam, shapes[fam], form, mode, branch=1 if fam == "neck" else None)
                spec = SPEC[entry].split()
                assert len(args) == len(spec), entry
                for a, name in zip(args, spec):
                    assert isinstance(a, T.Arg) == (name not in scalars), (entry, name)
                    if isinstance(a, T.Arg):
                        assert a.name == {"wgt": "w"}.get(name, name), (entry, name, a.name)
                        assert a.align == (16 if name == "wgt" else 8 if name in ("dscale", "dshift") else 4)
                        assert (a.role == "out") == (name in ("dw", "du", "dx", "dscale", "dshift"))
                seen.add(entry)
    assert seen == {e for e in SPEC if not e.endswith("_path")}
