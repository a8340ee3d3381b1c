"""Plain numpy reference of ONE layer of the launch plan (3x3 convolution stride 1 / 2, ConvTranspose with kernel = stride,
the head's three 1x1 contractions) in int64 / float64, with the operand rounding of the reduced-precision modes, and the
exact-arithmetic data the single-layer GPU tests (test_layer_exact_gpu.py) feed the kernels.

Exactness.  Activations (after the prologue), weights, residual and bias are small integers times a power of two.  With
`unit` = (activation granularity) x (weight granularity), every product is an integer multiple of `unit`, and as long as
sum |x| |w| + |res| + |bias| < 2^24 unit every partial sum -- in ANY order, tile shape or MFMA shape -- is an integer below 2^24
times `unit`, hence exactly representable in fp32: the kernel has nothing to round and must reproduce the reference bit for bit.
EXACT_BITS = 20 leaves four bits to spare.  The operands have at most 8 significant bits, so rounding them to bf16 or fp16 changes
nothing either (and the `lo` parts of bf16x3 are exactly zero)."""
import numpy as np

MODES = ("fp32", "bf16x3", "bf16", "fp16", "fp16s")
EXACT_BITS = 20           # sum |x||w| + |res| + |bias| < 2^EXACT_BITS * unit
X_UNIT = 2.0 ** -3        # granularity of the activations after the prologue (raw inputs: 2^-2, a multiple of it)
W_UNIT = 2.0 ** -4        # granularity of the weights
UNIT = X_UNIT * W_UNIT    # granularity of every product, residual and bias
# Winograd F(2x2,3x3): G g G^T halves twice (granularity W_UNIT / 4: two more bits), B^T d B adds four inputs (x 4), |G g G^T| <=
# (3/2)^2 max|g|, and A^T (.) A adds nine positions: 9 * Cin * (4 max|x|) * (9/4 max|w|) must stay below 2^24 * UNIT / 4.
WINO_UNIT = UNIT / 4
STAT_N = 1024             # fp32 partial sums of the statistics span at most this many values (conv16: 640 per wave, rounded up)


# ------------------------------------------------------------------ rounding (round to nearest even)
def round_bf16(x):
    """float32 -> nearest bfloat16 (ties to even), returned as float32.  Finite values beyond the largest bf16 round to inf."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    out = r.astype(np.uint32).view(np.float32).reshape(x.shape)
    nan = np.isnan(x)
    return np.where(nan, x, out) if nan.any() else out


def round_fp16(x):
    """float32 / float64 -> nearest float16 (ties to even, subnormals kept, overflow to inf), returned in the input's type.
    Integer arithmetic on the float64 image (every float32 is one), so there is no double rounding and no library conversion."""
    x = np.asarray(x)
    dt = x.dtype if x.dtype in (np.float32, np.float64) else np.float64
    v = np.ascontiguousarray(x, dtype=np.float64)
    m, e = np.frexp(np.abs(v))                      # |v| = m 2^e, m in [0.5, 1)
    e = np.maximum(e, -13)                           # below 2^-14 the spacing stays 2^-24 (subnormals)
    q = np.ldexp(1.0, (e - 11).astype(np.int64))     # spacing of float16 around |v|: 11 significant bits
    r = np.rint(np.abs(v) / q) * q                   # np.rint rounds halves to even; |v| / q is exact (power of two)
    r = np.where(r >= 65520.0, np.inf, r)            # 65520 = the midpoint above the largest finite value rounds (even) to inf
    out = np.copysign(r, v)
    out = np.where(np.isfinite(v), out, v)
    return out.astype(dt)


def split_bf16(x):
    """bf16x3 operands as the kernels define them: hi = bf16(x), lo = bf16(x - hi), the difference taken in float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = round_bf16(x)
    lo = round_bf16((x - hi).astype(np.float32))
    return hi, lo


def operand_pairs(x, w, mode):
    """The (activation, weight) products a mode sums, as float64 arrays: one pair, or the three terms of bf16x3."""
    x32, w32 = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    if mode == "fp32":
        pairs = [(x32, w32)]
    elif mode == "bf16":
        pairs = [(round_bf16(x32), round_bf16(w32))]
    elif mode in ("fp16", "fp16s"):
        pairs = [(round_fp16(x32), round_fp16(w32))]
    elif mode == "bf16x3":
        xh, xl = split_bf16(x32)
        wh, wl = split_bf16(w32)
        pairs = [(xh, wh), (xh, wl), (xl, wh)]
    else:
        raise ValueError(mode)
    return [(a.astype(np.float64), b.astype(np.float64)) for a, b in pairs]


# ------------------------------------------------------------------ the three operations (float64)
def prologue(x, scale=None, shift=None):
    """relu(x * scale + shift); scale / shift [C] (shared) or [nb, C] (per frame); None: x as it is."""
    x = np.asarray(x, dtype=np.float64)
    if scale is None:
        return x
    s, t = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    if s.ndim == 1:
        s, t = s[None], t[None]
    return np.maximum(x * s[:, :, None, None] + t[:, :, None, None], 0.0)


def conv3x3(x, w, stride=1):
    """x [nb,C,H,W], w [Co,C,3,3] -> [nb,Co,H/stride,W/stride]; zero padding 1 (torch.nn.functional.conv2d(padding=1))."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    nb, C, H, W = x.shape
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    xp = np.zeros((C, nb, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x.transpose(1, 0, 2, 3)
    cols = np.empty((3, 3, C, nb * Ho * Wo))         # one GEMM over (tap, channel)
    for ky in range(3):
        for kx in range(3):
            cols[ky, kx] = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride].reshape(C, -1)
    out = np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(w.shape[0], 9 * C) @ cols.reshape(9 * C, -1)
    return np.ascontiguousarray(out.reshape(-1, nb, Ho, Wo).transpose(1, 0, 2, 3))


def deconv(x, w):
    """ConvTranspose2d with kernel = stride = s: x [nb,Ci,h,w], w [Ci,Co,s,s] -> [nb,Co,h s,w s]."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    nb, Ci, h, ww = x.shape
    Co, s = w.shape[1], w.shape[2]
    y = np.ascontiguousarray(w.reshape(Ci, Co * s * s).T) @ np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(Ci, -1)  # [Co s s, nb h w]
    y = y.reshape(Co, s, s, nb, h, ww).transpose(3, 0, 4, 1, 5, 2)                        # [nb, Co, h, dy, w, dx]
    return np.ascontiguousarray(y).reshape(nb, Co, h * s, ww * s)


def head(x, w_cls, b_cls, w_box, b_box, w_dir, b_dir):
    """x [nb,C,H,W]; w_* [rows,C]; -> cls [nb,A,1], box [nb,A,7], dir [nb,A,2] with A = na H W ordered (anchor type, x, y)."""
    x = np.asarray(x, dtype=np.float64)
    nb, C, H, W = x.shape
    xf = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(C, nb * H * W)
    na = np.asarray(w_cls).shape[0]
    outs = []
    for w, b, k in ((w_cls, b_cls, 1), (w_box, b_box, 7), (w_dir, b_dir, 2)):
        w = np.asarray(w, dtype=np.float64).reshape(na * k, C)
        y = w @ xf + np.asarray(b, dtype=np.float64)[:, None]                            # [na k, nb HW]
        outs.append(np.ascontiguousarray(y.reshape(na, k, nb, H * W).transpose(2, 0, 3, 1)).reshape(nb, na * H * W, k))
    return tuple(outs)


def channel_stats(y):
    """[nb,C,H,W] -> [nb,C,2] = (sum, sum of squares) per frame and channel."""
    y = np.asarray(y, dtype=np.float64)
    return np.stack([y.sum(axis=(2, 3)), (y * y).sum(axis=(2, 3))], axis=-1)


def layer(kind, x, weights, mode="fp32", stride=1, res=None, scale=None, shift=None, magnitude=False):
    """One layer as the kernels compute it: prologue in fp32-exact arithmetic, operands rounded to the mode's type, products summed
    in float64, then residual (conv) or bias (head).  kind 0 conv3x3 (weights = w [Co,C,3,3]), 1 upsampler (w [Ci,Co,s,s]), 2 head
    (weights = the six head tensors in state_dict order: w_cls, b_cls, w_box, b_box, w_dir, b_dir).  Returns the float64 result BEFORE
    any 16-bit rounding of the output (`store` applies that); the head returns the (cls, box, dir) tuple.
    magnitude=True: the same contraction over absolute values, sum |x||w| + |res| + |bias| -- what the exactness condition and the
    error bounds are stated in."""
    xa = prologue(x, scale, shift)
    if kind == 2:
        ws = [np.asarray(w, dtype=np.float32).reshape(np.asarray(w).shape[0], -1) for w in weights[0::2]]
        bs = [np.asarray(b, dtype=np.float64).reshape(-1) for b in weights[1::2]]
        dummy = np.zeros(1, dtype=np.float32)
        x_terms = [p[0] for p in operand_pairs(xa, dummy, mode)]
        w_terms = [[p[1] for p in operand_pairs(dummy, w, mode)] for w in ws]  # [tensor][term]
        zero = [np.zeros_like(b) for b in bs]
        acc = None
        for i, xs in enumerate(x_terms):
            wi = [w_terms[t][i] for t in range(3)]
            if magnitude:
                xs, wi = np.abs(xs), [np.abs(w) for w in wi]
            term = head(xs, wi[0], zero[0], wi[1], zero[1], wi[2], zero[2])
            acc = list(term) if acc is None else [p + q for p, q in zip(acc, term)]
        for k, b in enumerate(bs):
            nb, A, kk = acc[k].shape
            na = b.shape[0] // kk
            acc[k] = (acc[k].reshape(nb, na, A // na, kk) + (np.abs(b) if magnitude else b).reshape(1, na, 1, kk)).reshape(nb, A, kk)
        return tuple(acc)
    out = None
    for xs, ws in operand_pairs(xa, weights, mode):
        if magnitude:
            xs, ws = np.abs(xs), np.abs(ws)
        y = conv3x3(xs, ws, stride) if kind == 0 else deconv(xs, ws)
        out = y if out is None else out + y
    if res is not None:
        r = np.asarray(res, dtype=np.float64)
        out = out + (np.abs(r) if magnitude else r)
    return out


def store(y, mode, kind):
    """The stored tensor: fp16s rounds conv / upsampler outputs to fp16 behind the statistics; everything else is fp32."""
    if mode == "fp16s" and kind != 2:
        return round_fp16(y).astype(np.float32)
    return np.asarray(y).astype(np.float32)


# ------------------------------------------------------------------ exact-arithmetic data
def _sprinkle_zeros(a, rng):
    """zero rows, columns and a few whole channels of a [nb,C,H,W] tensor"""
    H, W = a.shape[2], a.shape[3]
    a[:, :, rng.integers(0, H, max(1, H // 8)), :] = 0
    a[:, :, :, rng.integers(0, W, max(1, W // 8))] = 0
    a[:, rng.integers(0, a.shape[1], 2)] = 0
    return a


def exact_activations(rng, shape):
    """raw inputs: integers in [-7, 7] times 2^-2 (fp16- and bf16-exact), with zero rows / columns / channels"""
    return _sprinkle_zeros(rng.integers(-7, 8, shape).astype(np.float64), rng) * 0.25


def exact_affine(rng, shape):
    """scale: a power of two (1/2, 1, 2) per channel; shift: integers in [-16, 8] times 2^-3.  relu(x * scale + shift) is then an
    integer in [0, 36] times X_UNIT, and negative before the ReLU for a good share of the values."""
    scale = 2.0 ** rng.integers(-1, 2, shape).astype(np.float64)
    shift = rng.integers(-16, 9, shape).astype(np.float64) * X_UNIT
    return scale.astype(np.float32), shift.astype(np.float32)


def exact_weights(rng, shape):
    """integers in [-3, 3] times W_UNIT, a fifth of them zero"""
    w = rng.integers(-3, 4, shape).astype(np.float64)
    w[rng.random(shape) < 0.2] = 0
    return (w * W_UNIT).astype(np.float32)


def exact_residual(rng, shape):
    """integers in [-15, 15] times 2^-2 (a multiple of UNIT; exact in fp16)"""
    return _sprinkle_zeros(rng.integers(-15, 16, shape).astype(np.float64), rng) * 0.25


def exact_bias(rng, n):
    return (rng.integers(-31, 32, n).astype(np.float64) * 2.0 ** -4).astype(np.float32)


LAYER_KEYS = []  # state_dict key of each plan layer in execution order (the head: its six tensors)
for _b, _units in ((1, (2, 1)), (2, (2, 2, 1)), (3, (2, 2, 1))):
    LAYER_KEYS.append(f"rpn.block{_b}.0.weight")
    for _u, _n in enumerate(_units):
        LAYER_KEYS.append(f"rpn.block{_b}.{3 + _u}.conv_block.2.weight")
        if _n == 2:
            LAYER_KEYS.append(f"rpn.block{_b}.{3 + _u}.conv_block.5.weight")
    LAYER_KEYS.append(f"rpn.deconv{_b}.0.weight")
HEAD_KEYS = ("heads.conv_cls.weight", "heads.conv_cls.bias", "heads.conv_box.weight", "heads.conv_box.bias",
             "heads.conv_dir.weight", "heads.conv_dir.bias")
LAYER_KEYS.append(HEAD_KEYS)


def exact_state_dict(sd, seed=0):
    """A copy of state_dict `sd` (numpy or torch values) whose 16 convolution, 3 upsampler and 6 head tensors are exact data."""
    rng = np.random.default_rng(seed)
    out = dict(sd)
    for key in LAYER_KEYS[:-1]:
        out[key] = exact_weights(rng, tuple(np.asarray(sd[key]).shape))
    for key in HEAD_KEYS:
        shape = tuple(np.asarray(sd[key]).shape)
        out[key] = exact_bias(rng, shape[0]) if key.endswith("bias") else exact_weights(rng, shape)
    return out


def layer_weights(sd, index):
    """numpy weights of plan layer `index` as `layer` takes them"""
    key = LAYER_KEYS[index]
    if isinstance(key, tuple):
        return tuple(np.asarray(sd[k], dtype=np.float32).reshape(np.asarray(sd[k]).shape[0], -1).squeeze(-1) if k.endswith("bias")
                     else np.asarray(sd[k], dtype=np.float32).reshape(np.asarray(sd[k]).shape[0], -1) for k in key)
    return np.asarray(sd[key], dtype=np.float32)


def exactness_margin(mag, limit_bits=EXACT_BITS, unit=UNIT):
    """largest sum |x||w| + |res| + |bias| of a layer, as a fraction of 2^limit_bits * unit (must be < 1)"""
    m = max(float(np.max(a)) for a in (mag if isinstance(mag, tuple) else (mag,)))
    return m / (2.0 ** limit_bits * unit)


def stats_exact_margin(y):
    """The per-channel sum is exact when every fp32 partial the kernels form is: a partial spans a subset of one channel's values,
    so sum |y| over the whole channel below 2^24 UNIT covers every grouping.  Returns the largest such sum / (2^24 UNIT)."""
    return float(np.abs(np.asarray(y, dtype=np.float64)).sum(axis=(2, 3)).max()) / (2.0 ** 24 * UNIT)


# ------------------------------------------------------------------ the plan's shapes and the shared exact cases
GRIDS = {"64x96": (64, 96), "16x160": (16, 160)}  # BEV cells -> maps 32x48 / 16x24 / 8x12 (every tile overhangs) and 8x80 / 4x40 / 2x20
# The strip grid (test_menu_exact_gpu.py): maps 36x44 / 18x22 / 9x11.  Level 0 is 2 x 2 main tiles of 16 x 16 px, a right strip 12 px wide and a
# bottom strip 4 px tall -- what the strip tilings of wino4 / wino6 cover.  Not in GRIDS: the tests that iterate GRIDS assert on the full set.
STRIP_GRID = {"72x88": (72, 88)}
ALL_GRIDS = {**GRIDS, **STRIP_GRID}
PROLOGUES = ("raw", "shared", "frame")
NB = 3


def plan_shapes(gx, gy, na=9):
    """[{kind, cin, cout, stride, up, level, hin, win, h, w}] of the 20 layers in execution order, as pp_layer_tilings lists them"""
    H, W = gx // 2, gy // 2
    out, cin = [], 64
    for b, n_convs in enumerate((3, 5, 5)):
        c, h, w = 64 << b, H >> b, W >> b
        out.append(dict(kind=0, cin=cin, cout=c, stride=2, up=1, level=b, hin=2 * h, win=2 * w, h=h, w=w))
        out += [dict(kind=0, cin=c, cout=c, stride=1, up=1, level=b, hin=h, win=w, h=h, w=w) for _ in range(n_convs)]
        out.append(dict(kind=1, cin=c, cout=128 if b else 64, stride=1, up=1 << b, level=b, hin=h, win=w, h=h, w=w))
        cin = c
    out.append(dict(kind=2, cin=320, cout=10 * na, stride=1, up=1, level=0, hin=H, win=W, h=H, w=W))
    return out


_CASES = {}


def exact_case(sd, index, grid, pre="raw", with_res=False):
    """The exact-arithmetic case of plan layer `index` on grid `grid`: inputs (x, res, scale, shift as float32 / None), the float64
    reference `ref` (before a 16-bit store; the head: a tuple), `mag` = sum |x||w| + |res| + |bias| and, for convs and upsamplers,
    `stats` [nb,C,2].  Computed once per key and shared read-only; the operands are exact in every mode, so one reference serves all
    of them.  sd must be the one exact_state_dict all callers share."""
    key = (index, grid, pre, with_res)
    if key in _CASES:
        return _CASES[key]
    L = plan_shapes(*ALL_GRIDS[grid])[index]
    rng = np.random.default_rng([index, ALL_GRIDS[grid][0], PROLOGUES.index(pre), int(with_res)])
    x = exact_activations(rng, (NB, L["cin"], L["hin"], L["win"])).astype(np.float32)
    scale = shift = None
    if pre != "raw":
        scale, shift = exact_affine(rng, (L["cin"],) if pre == "shared" else (NB, L["cin"]))
    res = exact_residual(rng, (NB, L["cout"], L["h"], L["w"])).astype(np.float32) if with_res else None
    w = layer_weights(sd, index)
    kw = dict(stride=L["stride"], res=res, scale=scale, shift=shift)
    case = dict(L, x=x, res=res, scale=scale, shift=shift, ref=layer(L["kind"], x, w, "fp32", **kw),
                mag=layer(L["kind"], x, w, "fp32", magnitude=True, **kw))
    if L["kind"] != 2:
        case["stats"] = channel_stats(case["ref"])
    for v in case.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _CASES[key] = case
    return case


# ------------------------------------------------------------------ Winograd F(4x4,3x3): not exact, a componentwise bound
_F4 = (np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64),
       np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64),
       np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64))


def winograd4_bound(xa, w):
    """F(4x4,3x3) divides by 6 and 24: its transformed weights are no dyadic numbers, so a kernel of that family cannot be bit-exact
    on any data.  Forward error bound of Y = A^T [sum_c (G g G^T) (.) (B^T d B)] A evaluated in fp32, per output element and from
    the data itself: every U = G g G^T is rounded once, the contraction over C channels adds C roundings, the two passes of each
    transform at most 6 each -- |Y - Y_exact| <= (C + 16) 2^-24 |A^T| (sum_c |U| (.) |V|) |A|.  xa [nb,C,H,W] is the activation
    after the prologue (4x4 tiles from the map's origin, zero padded), w [K,C,3,3]."""
    Bt, G, At = _F4
    xa, w = np.asarray(xa, dtype=np.float64), np.asarray(w, dtype=np.float64)
    nb, C, H, W = xa.shape
    nh, nw = -(-H // 4), -(-W // 4)
    xp = np.zeros((nb, C, nh * 4 + 2, nw * 4 + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = xa
    t = np.lib.stride_tricks.sliding_window_view(xp, (6, 6), axis=(2, 3))[:, :, ::4, ::4]
    V = np.abs(np.einsum("ai,ncxyij,bj->ncxyab", Bt, t, Bt, optimize=True))
    U = np.abs(np.einsum("ai,kcij,bj->kcab", G, w, G, optimize=True))
    S = np.einsum("kcab,ncxyab->nkxyab", U, V, optimize=True)
    Y = np.einsum("ia,nkxyab,jb->nkxiyj", np.abs(At), S, np.abs(At), optimize=True).reshape(nb, -1, nh * 4, nw * 4)
    return (C + 16) * 2.0 ** -24 * Y[:, :, :H, :W]
