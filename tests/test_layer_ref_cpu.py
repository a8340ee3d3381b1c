"""CPU (-m "not gpu"): the plain single-layer reference of tests/layer_ref.py is itself pinned -- its rounding helpers bit for bit
against torch's conversions, its three operations against torch.nn.functional in float64, and its exact-arithmetic data against the
exactness condition the bit-exact GPU tests (test_layer_exact_gpu.py) rest on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rounding_inputs():
    rng = np.random.default_rng(7)
    parts = [rng.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rng.integers(-9, 6, 20000).astype(np.float32)]
    # ties: exactly half way between two neighbours of the 8-bit (bf16) and 11-bit (fp16) significands, both parities
    m8 = (128 + rng.integers(0, 128, 2000)).astype(np.float64)
    parts.append(((m8 + 0.5) * 2.0 ** rng.integers(-20, 20, 2000)).astype(np.float32))
    m11 = (1024 + rng.integers(0, 1024, 2000)).astype(np.float64)
    parts.append(((m11 + 0.5) * 2.0 ** rng.integers(-24, 5, 2000)).astype(np.float32))
    # fp16 subnormals and their ties (spacing 2^-24), underflow to zero
    parts.append((rng.integers(0, 2050, 2000) * 0.5 * 2.0 ** -24).astype(np.float32))
    # the largest finite values of the three formats and the values around their overflow thresholds
    f32max = np.finfo(np.float32).max
    parts.append(np.array([0.0, -0.0, 65504.0, 65519.0, 65519.996, 65520.0, 65536.0, 1e5, 3.3895314e38, 3.396e38, f32max,
                           np.nextafter(np.float32(3.3961775e38), np.float32(0)), 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25,
                           np.finfo(np.float32).tiny, np.inf], dtype=np.float32))
    x = np.concatenate(parts)
    return np.concatenate([x, -x])


def test_round_bf16_matches_torch_bit_for_bit():
    x = rounding_inputs()
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(bits(R.round_bf16(x)), bits(want))


def test_round_fp16_matches_torch_bit_for_bit():
    x = rounding_inputs()
    want = torch.from_numpy(x).to(torch.float16).to(torch.float32).numpy()
    got = R.round_fp16(x)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    # float64 input (the exact sums of the reference): ONE rounding.  Just above a tie the result is the upper neighbour; a conversion
    # by way of float32 (torch's for float64 tensors) lands on the tie first and then on the even one.  numpy converts directly.
    d = x.astype(np.float64) * (1.0 + 2.0 ** -30)
    with np.errstate(over="ignore"):
        want64 = d.astype(np.float16).astype(np.float64)
    assert np.array_equal(R.round_fp16(d).view(np.uint64), want64.view(np.uint64))
    assert R.round_fp16(np.float64(100.65625 * (1.0 + 2.0 ** -30))) == 100.6875


def test_split_bf16_terms():
    x = np.random.default_rng(3).standard_normal(5000).astype(np.float32)
    hi, lo = R.split_bf16(x)
    t = torch.from_numpy(x)
    thi = t.to(torch.bfloat16).to(torch.float32)
    assert np.array_equal(bits(hi), bits(thi.numpy())) and np.array_equal(bits(lo), bits((t - thi).to(torch.bfloat16).to(torch.float32).numpy()))
    assert np.abs(x.astype(np.float64) - hi - lo).max() <= 2.0 ** -16 * np.abs(x).max()  # two 8-bit pieces leave 2^-17 relative
    pairs = R.operand_pairs(x, x, "bf16x3")
    assert len(pairs) == 3 and np.array_equal(pairs[0][0], hi) and np.array_equal(pairs[1][1], lo) and np.array_equal(pairs[2][0], lo)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_matches_torch(stride):
    rng = np.random.default_rng(stride)
    x, w = rng.standard_normal((3, 24, 14, 20)), rng.standard_normal((40, 24, 3, 3))
    want = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), stride=stride, padding=1).numpy()
    got = R.conv3x3(x, w, stride)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("s", [1, 2, 4])
def test_deconv_matches_torch(s):
    rng = np.random.default_rng(10 + s)
    x, w = rng.standard_normal((3, 32, 6, 10)), rng.standard_normal((32, 24, s, s))
    want = F.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(w), stride=s).numpy()
    got = R.deconv(x, w)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_head_matches_torch():
    rng = np.random.default_rng(5)
    na, C, H, W, nb = 9, 32, 6, 8, 3
    x = rng.standard_normal((nb, C, H, W))
    ws = [rng.standard_normal((na * k, C)) for k in (1, 7, 2)]
    bs = [rng.standard_normal(na * k) for k in (1, 7, 2)]
    got = R.head(x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])
    for g, w, b, k in zip(got, ws, bs, (1, 7, 2)):
        y = F.conv2d(torch.from_numpy(x), torch.from_numpy(w).reshape(na * k, C, 1, 1), torch.from_numpy(b))
        # SharedHead.forward: [nb, na k, H, W] -> [nb, na, k, H, W] -> (anchor type, x, y, code) rows
        want = y.view(nb, na, k, H, W).permute(0, 1, 3, 4, 2).contiguous().view(nb, -1, k).numpy()
        np.testing.assert_allclose(g, want, rtol=0, atol=1e-12)


def test_prologue_residual_and_statistics():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((3, 16, 8, 12)).astype(np.float32)
    w = rng.standard_normal((16, 16, 3, 3)).astype(np.float32)
    res = rng.standard_normal((3, 16, 8, 12)).astype(np.float32)
    sc, sh = rng.standard_normal((3, 16)).astype(np.float32), rng.standard_normal((3, 16)).astype(np.float32)
    tx = torch.relu(torch.from_numpy(x).double() * torch.from_numpy(sc).double()[:, :, None, None] + torch.from_numpy(sh).double()[:, :, None, None])
    tx = tx.float().double()  # the kernels normalise in fp32 (one fma): the activation that is multiplied is an fp32 value
    want = (F.conv2d(tx, torch.from_numpy(w).double(), padding=1) + torch.from_numpy(res).double()).numpy()
    got = R.layer(0, x, w, "fp32", res=res, scale=sc, shift=sh)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    shared = R.layer(0, x, w, "fp32", scale=sc[0], shift=sh[0])
    np.testing.assert_allclose(shared[1], R.layer(0, x[1:2], w, "fp32", scale=sc[:1], shift=sh[:1])[0], rtol=0, atol=1e-12)
    st = R.channel_stats(want)
    np.testing.assert_allclose(st[..., 0], want.sum(axis=(2, 3)), rtol=1e-13)
    np.testing.assert_allclose(st[..., 1], (want ** 2).sum(axis=(2, 3)), rtol=1e-13)
    # operand rounding: the fp16 mode multiplies the rounded operands, in float64
    want16 = (F.conv2d(torch.from_numpy(R.round_fp16(tx.numpy().astype(np.float32))).double(), torch.from_numpy(R.round_fp16(w)).double(), padding=1)
              + torch.from_numpy(res).double()).numpy()
    np.testing.assert_allclose(R.layer(0, x, w, "fp16", res=res, scale=sc, shift=sh), want16, rtol=0, atol=1e-12)
    # fp16s stores fp16, behind the statistics; the head stays fp32
    assert np.array_equal(R.store(want, "fp16s", 0), R.round_fp16(want).astype(np.float32)) and np.array_equal(R.store(want, "fp16s", 2), want.astype(np.float32))


def test_plan_shapes_and_keys(synth):
    sd = synth.seeded_state_dict(0)
    shapes = R.plan_shapes(64, 96)
    assert len(shapes) == len(R.LAYER_KEYS) == 20 and [s["kind"] for s in shapes].count(0) == 16
    for s, key in zip(shapes[:-1], R.LAYER_KEYS[:-1]):
        w = np.asarray(sd[key])
        assert w.shape == ((s["cout"], s["cin"], 3, 3) if s["kind"] == 0 else (s["cin"], s["cout"], s["up"], s["up"])), key
    assert all(k in sd for k in R.HEAD_KEYS)


@pytest.fixture(scope="module")
def exact_sd(synth):
    return R.exact_state_dict(synth.seeded_state_dict(0))


@pytest.mark.parametrize("grid", sorted(R.ALL_GRIDS))
def test_exact_data_meets_its_exactness_condition(grid, exact_sd):
    """Every case the GPU tests run: sum |x||w| + |res| + |bias| < 2^20 unit at every output (the largest K is 9 * 256), every value a
    multiple of the unit, the operands unchanged by bf16 / fp16 rounding with zero `lo` parts, and the statistics condition."""
    worst = 0.0
    for index, L in enumerate(R.plan_shapes(*R.ALL_GRIDS[grid])):
        for pre in R.PROLOGUES:
            for with_res in ((False, True) if L["kind"] == 0 else (False,)):
                c = R.exact_case(exact_sd, index, grid, pre, with_res)
                margin = R.exactness_margin(c["mag"])
                worst = max(worst, margin)
                assert margin < 1.0, (index, pre, with_res, margin)
                outs = c["ref"] if isinstance(c["ref"], tuple) else (c["ref"],)
                for o in outs:
                    q = o / R.UNIT
                    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() < 2 ** R.EXACT_BITS
                    assert np.array_equal(o, o.astype(np.float32).astype(np.float64))
                xa = R.prologue(c["x"], c["scale"], c["shift"]).astype(np.float32)
                assert np.array_equal(xa / R.X_UNIT, np.rint(xa / R.X_UNIT)) and xa.max() <= 36 * R.X_UNIT
                if pre != "raw":
                    pre_relu = c["x"].astype(np.float64) * (c["scale"][None, :, None, None] if pre == "shared" else c["scale"][:, :, None, None]) \
                        + (c["shift"][None, :, None, None] if pre == "shared" else c["shift"][:, :, None, None])
                    assert 0.2 < (pre_relu < 0).mean() < 0.8  # the ReLU matters
                assert np.array_equal(R.round_bf16(xa), xa) and np.array_equal(R.round_fp16(xa), xa) and not R.split_bf16(xa)[1].any()
                assert np.array_equal(R.round_fp16(c["x"]), c["x"]) and xa[xa > 0].min() >= 2.0 ** -14  # clear of fp16 subnormals
                if c["res"] is not None:
                    assert np.array_equal(R.round_fp16(c["res"]), c["res"])
                if L["kind"] != 2:
                    # per-channel sums are exact in any grouping of fp32 partials; fp16s outputs stay finite
                    assert R.stats_exact_margin(c["ref"]) < 1.0 and np.abs(c["ref"]).max() < 65504
                    assert np.array_equal(c["stats"], R.channel_stats(c["ref"]))
                    assert (c["ref"] != 0).mean() > 0.25  # zero rows and columns, but not a degenerate map
    ws = [R.layer_weights(exact_sd, i) for i in range(19)]
    for w in ws:
        assert np.array_equal(R.round_bf16(w), w) and np.array_equal(R.round_fp16(w), w) and np.abs(w).max() <= 3 * R.W_UNIT
        assert np.array_equal(w / R.W_UNIT, np.rint(w / R.W_UNIT)) and 0.1 < (w == 0).mean() < 0.4
    # Winograd F(2x2,3x3) on the stride-1 convs: transformed weights on a grid of W_UNIT / 4, sums below 2^24 of the finer unit
    assert 9 * 256 * (4 * 36 * R.X_UNIT) * (2.25 * 3 * R.W_UNIT) < 2.0 ** 24 * R.WINO_UNIT
    print(f"[exact data] grid {grid}: largest sum |x||w| + |res| + |bias| = {worst:.4f} x 2^{R.EXACT_BITS} unit")


def test_exact_reference_is_the_same_in_every_mode(exact_sd):
    """The operands are exact in bf16 and fp16, so every mode's reference -- the three-term bf16x3 sum included -- is the fp32 one."""
    for index in (0, 3, 4, 11, 14, 18, 19):
        L = R.plan_shapes(*R.GRIDS["64x96"])[index]
        c = R.exact_case(exact_sd, index, "64x96", "frame", L["kind"] == 0)
        w = R.layer_weights(exact_sd, index)
        for mode in R.MODES[1:]:
            got = R.layer(L["kind"], c["x"], w, mode, stride=L["stride"], res=c["res"], scale=c["scale"], shift=c["shift"])
            for a, b in zip(got if isinstance(got, tuple) else (got,), c["ref"] if isinstance(c["ref"], tuple) else (c["ref"],)):
                assert np.array_equal(a, b), (index, mode)


def test_exact_cases_are_shared_and_read_only(exact_sd):
    a = R.exact_case(exact_sd, 1, "64x96", "shared", True)
    assert a is R.exact_case(exact_sd, 1, "64x96", "shared", True)
    with pytest.raises(ValueError):
        a["ref"][0, 0, 0, 0] = 1.0
