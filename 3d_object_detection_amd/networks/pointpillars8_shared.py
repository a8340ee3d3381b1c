"""networks.pointpillars8_shared.PointPillars (reference pointpillars8_shared.py:346-382): the eager
network with the InstanceNorm backbone, running PFN / scatter / RPN / head as HIP kernels.

Training is one path with a depth.  train(scope=...) names how far back from the outputs the network trains; SCOPES lists the
depths from the head to the front, and each scope trains what the one before it trains and one group of tensors more (_GROUPS):

    "head"    the six tensors of the anchor head (HEAD_KEYS)
    "neck"    + the three upsampler weights (NECK_KEYS)
    "block3"  + the five unit convolutions of the deepest Resnet block (BLOCK3_KEYS, unit order)
    "stage3"  + that block's stride-2 convolution (STAGE3_KEY)
    "rpn"     + the ten convolutions of blocks 1 and 2: the whole RPN (RPN_KEYS, the reference's state_dict order, 25 tensors)
    "all"     + the pillar feature net (PFN_KEYS; ALL_KEYS = the 28 tensors net.parameters() yields in the reference)

Every shipped configuration trains (eight_20cm, ntusl_10cm, nuscene and nuscene_10class), and so does any class_table with at
most 24 anchors per location: the head backward takes 1 .. 24 (pp_head_backward raises above that), everything behind
dL/d(rpn_out) does not depend on the count.

Everything in front of the trained groups is frozen.  A training forward records up to three autograd Functions, each a thin
wrapper of engine calls: _HeadFunction (pp_head / pp_head_backward, csrc/train.hip); _RpnFunction, whose forward runs the backbone
with the taps its depth needs and whose backward (_rpn_backward) walks RPN_TABLE from the upsamplers (pp_neck_backward, csrc/neck_train.hip)
through each block's unit chain (pp_unit_backward, csrc/block_train.hip) and strided stage (pp_down_backward, csrc/down_train.hip),
stopping where nothing in front needs a gradient; and, under "all", _PfnFunction in front of it (csrc/pfn_train.hip), which consumes
the gradient of the canvases that _RpnFunction returns at full depth.  rpn_train() returns that gradient to any canvas that
requires grad.

The forward always reads the engine's packed images of the weights.  After an optimizer step each group whose tensors moved is
written into its committed image in place before it is next used (_sync_head, _sync_neck, _sync_pfn); when a convolution of
blocks 1 and 2 moved, all sixteen convolutions go up in one pp_update_rpn_weights, which also rewrites the sparse first
convolution's image.  state_dict() returns the current values of the groups that were stepped.

The pillar feature net under "all" follows the reference's train.py, whose net.train() makes BatchNorm1d normalise with batch
statistics: every training-mode forward runs pp_pfn_train_forward over the pillars of all frames of the batch, moves running_mean /
running_var (momentum 0.1, unbiased variance) and counts num_batches_tracked, whether or not grad is enabled.  The eval-mode PFN of
the engine (running statistics folded into scale / shift) is rewritten by pp_update_pfn_weights before it is next used.

The BatchNorm networks (pointpillars8_export / _trt, _norm = "batch") fine-tune with frozen statistics, train(scope=...,
bn_stats="frozen"): every BatchNorm2d of the RPN stays the per-channel affine of its running statistics, its weight / bias sit in the
group of the convolution whose backward primitive yields their gradient (with_bn: 63 tensors under "rpn", 66 under "all"), the
training forward is the same tapped inference pass, _RpnBnFunction runs the same walk with pp_*_backward_affine, and after a step
_sync_neck also folds the nineteen layers again in place (pp_update_bn_fold).  train(scope=..., bn_stats="moving") trains them as the
reference's net.train() does: every BatchNorm2d normalises with the statistics of the batch and moves its running statistics.  The
training forward is then one lock-step pass over all frames (pp_backbone_train_taps_bn) and _RpnBnBatchFunction runs the walk with
pp_*_backward_bn; the moved running statistics are folded again before the next eval-mode pass.

Mixed precision (grad_stages="rpn" extends it to the strided stages and the upsamplers, pp_down_backward_mp / pp_neck_backward_mp):
train(..., grad_precision="bf16x3" | "bf16") runs the two gradient products of every Resnet unit backward with split
or plain bf16 operands on the bf16 MFMA (pp_unit_backward_mp); the forward, the weights, every tensor handed around and the other
backwards stay fp32, and "fp32", the default, is the fp32 path bit for bit.  On a BatchNorm network train(..., bn_stats=...,
bn_grad_precision="bf16x3" | "bf16") does the same for the BatchNorm backwards (pp_*_backward_affine_mp / pp_*_backward_bn_mp), again
for the units alone or, under grad_stages="rpn", the stages and upsamplers too.

train(..., forward_precision="bf16x3" | "bf16" | "fp16") (InstanceNorm network) runs the training forward in that precision mode of
the engine: the plan committed for inference in that mode, tapped by pp_backbone_train_taps_mp, so a network is fine-tuned in the
arithmetic it is deployed in.  The taps are the fp32 activations of that forward, the backward is untouched (fp32 master weights,
straight through the operand rounding) and combines freely with grad_precision, and after a step the 16-bit images are rewritten in
place (pp_update_*_weights_mp).  The uploads pick their entry by the engine's effective precision in eval mode too, so weights stepped
in fp32 reach a network switched with half() / precision() without a reload; only "fp16s" cannot take them.  The PFN is fp32 in
every mode."""
import time
import types
import typing

import numpy as np
import torch

from ..engine import BackwardNorm, Engine, engine_for
from .init import init_state_dict

HEAD_KEYS = ("heads.conv_cls.weight", "heads.conv_cls.bias", "heads.conv_box.weight", "heads.conv_box.bias",
             "heads.conv_dir.weight", "heads.conv_dir.bias")
NECK_KEYS = ("rpn.deconv1.0.weight", "rpn.deconv2.0.weight", "rpn.deconv3.0.weight")
# block 3 behind its stride-2 head, h -> r3 = h + U_b(U_a(h)), r4 = r3 + U_d(U_c(r3)), x3 = r4 + U_e(r4): the weights of units a..e
BLOCK3_KEYS = Engine.BLOCK3_KEYS
STAGE3_KEY = Engine.DOWN_KEYS[2]  # block 3's stride-2 convolution, in front of unit a
RPN_CONV_KEYS = Engine.RPN_CONV_KEYS
# the backward of the whole RPN as a table, one row per level: (level, convolutions per Resnet module in forward order).  A module of
# two convolutions is r -> r + U_b(U_a(r)), one of a single convolution r -> r + U_a(r); the level's units count the convolutions.
RPN_TABLE = ((0, (2, 1)), (1, (2, 2, 1)), (2, (2, 2, 1)))
# the reference's state_dict order of everything behind the canvas: per block its convolutions, then its upsampler; then the head
PFN_KEYS = Engine.PFN_KEYS
PFN_STAT_KEYS = Engine.PFN_STAT_KEYS
PFN_NBT_KEY = "pillar_point_net.pfn_layers.1.num_batches_tracked"
BN_MOMENTUM = 0.1  # torch's BatchNorm1d default, which the reference keeps
RPN_KEYS = tuple(k for b in range(3) for k in RPN_CONV_KEYS[(0, 4, 10)[b]:(4, 10, 16)[b]] + (NECK_KEYS[b],)) + HEAD_KEYS
_RPN_EXTRA_KEYS = tuple(k for k in RPN_CONV_KEYS if k != STAGE3_KEY and k not in BLOCK3_KEYS)  # what the narrower scopes never train
ALL_KEYS = PFN_KEYS + RPN_KEYS  # everything net.parameters() yields in the reference, in its state_dict order
SCOPES = ("head", "neck", "block3", "stage3", "rpn", "all")
GRAD_PRECISIONS = ("fp32", "bf16x3", "bf16")  # train(grad_precision=...): the operands of the unit backwards' gradient products
FORWARD_PRECISIONS = Engine.FORWARD_PRECISIONS  # train(forward_precision=...): the precision mode the training forward runs in
GRAD_STAGES = ("units", "rpn")  # train(grad_stages=...): the backwards that take grad_precision: the units alone, or the strided stages
                                # and the upsamplers as well
BN_STATS = ("frozen", "moving", "batch")  # train(bn_stats=...) on a BatchNorm network; "batch" is refused: "moving" is its name here
BN2D_MOMENTUM = 0.01  # the reference's BatchNorm2d(eps=1e-3, momentum=0.01) of the RPN


def bn_affine_keys(conv_key):
    """(weight, bias) of the BatchNorm2d layer whose gradient the backward primitive of this RPN convolution or upsampler yields."""
    p = Engine.bn_prefix(conv_key)
    return p + ".weight", p + ".bias"


def with_bn(keys):
    """`keys` with, for every RPN convolution and upsampler among them, the weight and bias of its BatchNorm2d layer, in the reference's
    named_parameters() order: a unit's leading norm in front of its convolution, the norm of a strided convolution or of an upsampler
    behind it."""
    out = []
    for k in keys:
        if not k.startswith("rpn."):
            out.append(k)
        elif k in Engine.DOWN_KEYS or k in NECK_KEYS:
            out += [k, *bn_affine_keys(k)]
        else:
            out += [*bn_affine_keys(k), k]
    return tuple(out)


BN_RPN_KEYS = with_bn(RPN_KEYS)        # the 63 tensors train(scope="rpn", bn_stats="frozen") trains on a BatchNorm network
BN_ALL_KEYS = PFN_KEYS + BN_RPN_KEYS   # the 66 tensors net.parameters() yields in the reference's BatchNorm network


class _Group(typing.NamedTuple):
    """One group of trainable tensors of PointPillars, kept as a dict of device Parameters."""
    attr: str     # the dict's attribute
    keys: tuple   # its state_dict names
    scope: str    # the first of SCOPES that trains it; every later scope trains it too
    upload: typing.Callable  # net -> None: the engine call that rewrites the committed image of its current values
    covers: tuple = ()       # groups whose tensors that call carries as well
    stats: str = None        # a dict of tensors that are no parameters but go up with the group


# from the front of the network to the head
_GROUPS = {g.attr: g for g in (
    _Group("_pfn", PFN_KEYS, "all", lambda net: net._eng.update_pfn_weights(*[net._pfn[k] for k in PFN_KEYS],
                                                                           *[net._pfn_stats[k] for k in PFN_STAT_KEYS]), stats="_pfn_stats"),
    _Group("_rpn", _RPN_EXTRA_KEYS, "rpn", lambda net: net._eng.update_rpn_weights({**net._rpn, **net._down, **net._block}),
           covers=("_down", "_block")),  # a convolution of blocks 1 and 2 moved: all sixteen go up in one call
    _Group("_down", (STAGE3_KEY,), "stage3", lambda net: net._eng.update_down_weight(2, net._down[STAGE3_KEY])),
    _Group("_block", BLOCK3_KEYS, "block3", lambda net: net._eng.update_block_weights(net._block)),
    _Group("_neck", NECK_KEYS, "neck", lambda net: net._eng.update_neck_weights(net._neck)),
    _Group("_params", HEAD_KEYS, "head", lambda net: net._eng.update_head_weights(net._params)),
)}
_BACKBONE = ("_neck", "_rpn", "_block", "_down")  # the groups _sync_neck() uploads, in its order: what _RpnFunction differentiates


class _HeadFunction(torch.autograd.Function):
    """SharedHead.forward as pp_head, its backward as pp_head_backward.  The six parameters are inputs only so that autograd
    routes their gradients; the forward reads the engine's packed copy of them (PointPillars uploads it beforehand)."""

    @staticmethod
    def forward(ctx, eng, x, *params):
        ctx.eng = eng
        ctx.save_for_backward(x)
        return eng.head(x)

    @staticmethod
    def backward(ctx, gcls, gbox, gdir):
        (x,) = ctx.saved_tensors
        eng = ctx.eng
        nb = x.shape[0]
        zeros = lambda g, n: torch.zeros((nb, eng.A, n), dtype=torch.float32, device=x.device) if g is None else g.contiguous()  # noqa: E731
        g, dx = eng.head_backward(x, zeros(gcls, 1), zeros(gbox, 7), zeros(gdir, 2), need_dx=ctx.needs_input_grad[1])
        return (None, dx) + tuple(g[k] if ctx.needs_input_grad[2 + i] else None for i, k in enumerate(HEAD_KEYS))


class _Layer(typing.NamedTuple):
    """One trained convolution or upsampler of the RPN as its backward sees it, with its BatchNorm2d on a BatchNorm backbone."""
    w: torch.Tensor
    need_w: bool
    norm: BackwardNorm = None        # BatchNorm: the fold the forward used (and the batch statistics), need_affine = the norm trains
    stats: tuple = ()                # what bn_affine_grad reads: the running statistics when frozen, the batch's when they move
    need_gb: tuple = (False, False)  # the norm's weight / bias require grad

    def trains(self):
        return self.need_w or any(self.need_gb)


def _layer_backward(eng, primitive, layer, *args, prec=None, **kw):
    """One backward primitive of the engine (neck_backward, unit_backward, down_backward) for `layer` -> ((dw, dgamma, dbeta), dx),
    each gradient None unless its tensor requires grad.  prec, when given, goes in as grad_precision (InstanceNorm) or as
    bn_grad_precision (BatchNorm).  BatchNorm: the layer's norm goes in, and its dgamma / dbeta come from the primitive's two fp64 sums
    (pp_bn_affine_grad)."""
    if layer.norm is None:
        dw, dx = primitive(*args, **kw, **({} if prec is None else {"grad_precision": prec}))
        return (dw if layer.need_w else None, None, None), dx
    dw, dx, dscale, dshift = primitive(*args, **kw, norm=layer.norm, **({} if prec is None else {"bn_grad_precision": prec}))
    dg, db = eng.bn_affine_grad(dscale, dshift, *layer.stats) if layer.norm.need_affine else (None, None)
    return (dw if layer.need_w else None, dg if layer.need_gb[0] else None, db if layer.need_gb[1] else None), dx


def rpn_block_backward(eng, modules, units, weights, g, grad_precision="fp32", need_dh=True, layers=None):
    """The backward of one block's Resnet modules (a row of RPN_TABLE): units and weights in unit order, g = dL/d(block output) ->
    (dw per unit, dL/d(block input h)).  grad_precision: the operand precision of every unit backward (Engine.unit_backward).
    need_dh=False: nothing in front of the block trains, so its first unit computes its weight gradient only and h gets None.
    layers: the units' _Layer entries in place of weights=None (any norm form); a unit's result is then its (dw, dgamma, dbeta).
    The first unit runs its dgrad when something in front needs the gradient or its own norm trains: a unit's affine sums are sums
    over its dgrad product."""
    layers = layers or [_Layer(w, True) for w in weights]
    # a unit with a norm gets the keyword only in a 16-bit mode: fp32 runs make the calls they always made
    prec = lambda layer: None if layer.norm is not None and grad_precision == "fp32" else grad_precision  # noqa: E731
    unit = lambda i, g, **kw: _layer_backward(eng, eng.unit_backward, layers[i], units[i], layers[i].w, g, prec=prec(layers[i]), **kw)  # noqa: E731
    grads = [None] * len(units)
    i = len(units)
    for n in reversed(modules):
        i -= n
        skip = g  # the gradient of the module's output is also that of its residual path
        if n == 2:
            grads[i + 1], g = unit(i + 1, g)
        if i or need_dh or any(layers[i].need_gb):
            grads[i], g = unit(i, g, dskip=skip)
        else:
            grads[i], g = unit(i, g, need_du=False)
    return (grads if weights is None else [dw for dw, _, _ in grads]), g


_W0 = (0, 4, 10)  # each level's strided convolution in RPN_CONV_KEYS; its unit convolutions follow it


def _frame_taps(eng, first, canvas, forward_precision="fp32"):
    """One frame's forward with the taps a backward from convolution `first` of RPN_CONV_KEYS on needs ->
    (y, (x1, x2, x3), {level: unit inputs}, {level: z}).  A 16-bit forward_precision has the one tapped pass of every level
    (backbone_train_taps with the keyword) and keeps what `first` needs of it."""
    if forward_precision != "fp32":
        y, xs, units, zs = eng.backbone_train_taps(canvas, forward_precision=forward_precision)
        levels = [b for b, _ in RPN_TABLE if first <= _W0[b] + 1]
        return y, xs, {b: units[b] for b in levels}, {b: zs[b] for b in levels if first <= _W0[b]}
    if first == 0:
        y, xs, units, zs = eng.backbone_train_taps(canvas)
        return y, xs, dict(enumerate(units)), dict(enumerate(zs))
    if first == len(RPN_CONV_KEYS):
        y, *xs = eng.backbone_taps(canvas)
        return y, xs, {}, {}
    if first == _W0[2]:
        y, x1, x2, x3, units, z3 = eng.backbone_stage_taps(canvas)
        return y, (x1, x2, x3), {2: units}, {2: z3}
    y, x1, x2, x3, units = eng.backbone_block_taps(canvas)
    return y, (x1, x2, x3), {2: units}, {}


def _stacked_taps(eng, first, x, forward_precision="fp32"):
    """_frame_taps of every canvas of x, stacked over the frames -> [y, x1, x2, x3, the unit inputs of the levels `first` reaches, their
    z]: what a backward from `first` keeps, in the order _rpn_backward reads."""
    outs = [_frame_taps(eng, first, c, forward_precision) for c in x]
    y = torch.cat([o[0] for o in outs])
    taps = [torch.cat([o[1][b] for o in outs]) for b in range(3)]
    units = [torch.stack([o[2][b][k] for o in outs]) for b in sorted(outs[0][2]) for k in range(sum(RPN_TABLE[b][1]))]
    zs = [torch.cat([o[3][b] for o in outs]) for b in sorted(outs[0][3])]
    return [y, *taps, *units, *zs]


def _rpn_backward(eng, first, saved, layers, gy, need_x, prec=("fp32", "fp32")):
    """The backward of the RPN from its output back to convolution `first` of RPN_CONV_KEYS, for every norm form: pp_neck_backward
    for the three branches and then, from level 2 down along RPN_TABLE, the block's unit chain (rpn_block_backward) and its strided
    stage (pp_down_backward); the upsampler's dx plus the dx of the stage above (in this order) is the gradient of a level's block
    output.  saved: what the forward kept, the canvases when first = 0 and then the list of _stacked_taps; layers: the _Layer of
    RPN_CONV_KEYS[first:], then of the three upsamplers; prec as in _RpnFunction.  It stops where nothing in front needs a gradient:
    a dx is computed only when a layer in front of it trains or the canvases need one (need_x), and a layer whose tensors need no
    gradient runs only for the dx it hands on.
    -> (dL/d(canvases) or None, per layer its (dw, dgamma, dbeta), None for a tensor that does not require grad)."""
    saved = list(saved)
    x = saved.pop(0) if first == 0 else None
    y, taps, saved = saved[0], saved[1:4], saved[4:]
    levels = [(b, sum(mods)) for b, mods in RPN_TABLE if first <= _W0[b] + 1]  # the levels with taps
    units = {b: [saved.pop(0) for _ in range(n)] for b, n in levels}
    zs = {b: saved.pop(0) for b, _ in levels if first <= _W0[b]}
    nconv = len(RPN_CONV_KEYS)
    conv = lambda k: layers[k - first]  # noqa: E731
    # front[b]: the canvases or a convolution in front of level b's block needs a gradient, so the block's input does;
    # front[b + 1]: the same for the block's output
    front = [need_x]
    for b, mods in RPN_TABLE:
        front.append(front[b] or any(conv(k).trains() for k in range(max(first, _W0[b]), _W0[b] + 1 + sum(mods))))
    gy = gy.contiguous()
    stage_prec = None if prec[1] == "fp32" else prec[1]  # the keyword goes to the stages and upsamplers only in a 16-bit mode
    grads = [(None, None, None)] * len(layers)
    dxn = [None] * 3
    for b in range(3):
        i = nconv - first + b
        if layers[i].trains() or front[b + 1]:
            grads[i], dxn[b] = _layer_backward(eng, eng.neck_backward, layers[i], b, taps[b], layers[i].w, y, gy, prec=stage_prec, need_dx=front[b + 1])
    g = None
    for b, n in reversed(levels):
        w0, mods = _W0[b], RPN_TABLE[b][1]
        if not front[b + 1]:
            break
        g = dxn[b] if g is None else dxn[b] + g
        need_dh = first <= w0 and (conv(w0).trains() or front[b])
        grads[w0 + 1 - first:w0 + 1 + n - first], g = rpn_block_backward(eng, mods, units[b], None, g, prec[0], need_dh=need_dh,
                                                                           layers=layers[w0 + 1 - first:w0 + 1 + n - first])
        if need_dh:
            grads[w0 - first], g = _layer_backward(eng, eng.down_backward, conv(w0), x if b == 0 else taps[b - 1], conv(w0).w, zs[b], g,
                                                   prec=stage_prec, need_dx=front[b])
    return (g if need_x else None), grads


class _RpnFunction(torch.autograd.Function):
    """RPN.forward on canvases x [nb,64,gx,gy], one backbone pass per frame, stacked; the backward of the RPN from its output back
    to convolution `first` of RPN_CONV_KEYS, the first one that trains: 0 (the whole RPN, backbone_train_taps), 10 (block 3 with its
    strided convolution, backbone_stage_taps), 11 (block 3's units, backbone_block_taps) or 16 (the upsamplers alone, backbone_taps).
    weights: RPN_CONV_KEYS[first:], then the three upsamplers; they are inputs only so that autograd routes their gradients, the
    forward reads the engine's packed copy of them (PointPillars uploads it beforehand).

    prec is the pair (grad_precision of the unit backwards, grad_precision of the strided stages and upsamplers): the second is "fp32"
    unless train(grad_stages="rpn") hands the network's grad_precision to pp_down_backward_mp and pp_neck_backward_mp as well.

    The backward is _rpn_backward with InstanceNorm layers; a weight that does not require grad gets None.  Kept for the backward: y,
    x1..x3, the unit inputs and z of the levels `first` reaches, the weights, and for first = 0 the canvases, which then get level
    0's dx when they require grad.

    A 16-bit forward_precision (train(forward_precision=...)) may follow the weights as the last argument, a str: the forward then
    taps the engine's 16-bit plan; without it the forward is fp32 and makes the calls it always made.  The backward is the same
    either way."""

    @staticmethod
    def forward(ctx, eng, prec, first, x, *weights):
        ctx.fwd = weights[-1] if weights and isinstance(weights[-1], str) else None
        weights = weights[:-1] if ctx.fwd else weights
        ctx.eng, ctx.prec, ctx.first = eng, prec, first
        kept = _stacked_taps(eng, first, x, ctx.fwd or "fp32")
        ctx.save_for_backward(*([x] if first == 0 else []), *kept, *weights)
        return kept[0]

    @staticmethod
    def backward(ctx, gy):
        need, saved = ctx.needs_input_grad, ctx.saved_tensors
        if ctx.fwd:
            need = need[:-1]
        layers = [_Layer(w, n) for w, n in zip(saved[len(saved) + 4 - len(need):], need[4:])]  # the weights are the last tensors kept
        g, grads = _rpn_backward(ctx.eng, ctx.first, saved, layers, gy, need[3], ctx.prec)
        return (None, None, None, g) + tuple(dw for dw, _, _ in grads) + ((None,) if ctx.fwd else ())


class _RpnBnFunction(torch.autograd.Function):
    """_RpnFunction for the BatchNorm backbone with frozen statistics: the same forward (the tap entry points read no norm kind) and
    the same walk (_rpn_backward), whose layers carry a BackwardNorm without statistics (pp_neck_backward_affine,
    pp_unit_backward_affine, pp_down_backward_affine).  A layer is a convolution or upsampler with its BatchNorm2d: tensors holds
    (weight, gamma, beta) of RPN_CONV_KEYS[first:] and then of the three upsamplers, stats (running_mean, running_var) of the same
    layers, which get no gradient.  The folded (scale, shift) of every layer are evaluated once in the forward by the kernel that
    wrote the engine's own (pp_bn_fold), so the backward reads the values the forward used.  A layer's dgamma / dbeta come from the
    two fp64 sums of its primitive (pp_bn_affine_grad).  prec, _RpnFunction's pair (units, stages), may follow the tensors as the last
    argument (train(bn_grad_precision=...)); without it the walk is fp32 and makes the calls it always made."""

    @staticmethod
    def _split_prec(tensors):
        """tensors, possibly followed by the pair prec -> (tensors, prec or None)."""
        return (tensors[:-1], tensors[-1]) if tensors and isinstance(tensors[-1], tuple) else (tensors, None)

    @staticmethod
    def forward(ctx, eng, first, stats, x, *tensors):
        tensors, ctx.prec = _RpnBnFunction._split_prec(tensors)
        ctx.eng, ctx.first, ctx.stats, ctx.batch = eng, first, stats, False
        n = len(tensors) // 3
        folds = [eng.bn_fold(tensors[3 * i + 1], tensors[3 * i + 2], *stats[i]) for i in range(n)]
        kept = _stacked_taps(eng, first, x)
        ctx.save_for_backward(*([x] if first == 0 else []), *kept, *tensors[::3], *[t for f in folds for t in f])
        return kept[0]

    @staticmethod
    def backward(ctx, gy):
        """Shared with _RpnBnBatchFunction (ctx.batch): there a layer's norm also holds its batch mean and variance (ctx.stats: the
        pp_*_backward_bn primitives), and pp_bn_affine_grad reads those in place of the running statistics."""
        need, saved = ctx.needs_input_grad, ctx.saved_tensors
        n = (len(need) - 4) // 3
        own = saved[len(saved) - 3 * n:]  # the last tensors kept: the n weights, then every layer's (scale, shift)
        layers = []
        for i in range(n):
            need_gb = tuple(need[5 + 3 * i:7 + 3 * i])
            norm = BackwardNorm(own[n + 2 * i], own[n + 2 * i + 1], *(ctx.stats[i] if ctx.batch else ()), need_affine=any(need_gb))
            layers.append(_Layer(own[i], need[4 + 3 * i], norm, ctx.stats[i], need_gb))
        g, grads = _rpn_backward(ctx.eng, ctx.first, saved, layers, gy, need[3], ctx.prec or ("fp32", "fp32"))
        return (None, None, None, g) + tuple(t for layer in grads for t in layer) + ((None,) if ctx.prec else ())


class _RpnBnBatchFunction(torch.autograd.Function):
    """_RpnBnFunction with batch statistics (train-mode BatchNorm2d): the forward is one lock-step pass over all frames,
    pp_backbone_train_taps_bn, which hands out every layer's batch mean, biased variance and their fold with the layer's weight and
    bias; the backward is _RpnBnFunction's walk with the pp_*_backward_bn primitives.  bn_params holds weight and bias of all nineteen
    layers (the layers in front of `first` normalise with batch statistics too); tensors (and the optional prec behind them) as in
    _RpnBnFunction.  Returns the rpn output
    and the statistics mean, var f32[19,256] in Engine.bn_layers() order (not differentiable: the caller moves the running ones)."""

    @staticmethod
    def forward(ctx, eng, first, bn_params, x, *tensors):
        tensors, ctx.prec = _RpnBnFunction._split_prec(tensors)
        nconv = len(RPN_CONV_KEYS)
        taps = True if first == 0 else False if first == nconv else 2
        y, xs, units, zs, mean, var, scale, shift = eng.backbone_train_taps_bn(x, bn_params, taps=taps)
        order = [k for b in range(3) for k in RPN_CONV_KEYS[_W0[b]:_W0[b] + 1 + sum(RPN_TABLE[b][1])] + (NECK_KEYS[b],)]  # bn_layers() order
        layers = RPN_CONV_KEYS[first:] + NECK_KEYS
        rows = [(order.index(k), int(tensors[3 * i + 1].shape[0])) for i, k in enumerate(layers)]
        ctx.eng, ctx.first, ctx.batch = eng, first, True
        ctx.stats = [(mean[r, :c], var[r, :c]) for r, c in rows]
        levels = [b for b, mods in RPN_TABLE if first <= _W0[b] + 1]
        ctx.save_for_backward(*([x] if first == 0 else []), y, *xs, *[u for b in levels for u in units[b]],
                              *[zs[b] for b in levels if first <= _W0[b]], *tensors[::3], *[t[r, :c] for r, c in rows for t in (scale, shift)])
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, gy, _gmean, _gvar):
        return _RpnBnFunction.backward(ctx, gy)


class _PfnFunction(torch.autograd.Function):
    """PointNet.forward in train mode and PointPillarsScatter.forward: one pp_pfn_train_forward over the pillars of all frames (rows
    grouped by frame; frames = ((row0, row1, coors [n,3], num [1]), ...)), then pp_scatter per frame.  Returns the canvases and the
    batch statistics f64[218] (not differentiable: the caller moves the running statistics with them).  The backward is
    pp_scatter_backward per frame into that frame's rows of dfeat, then one pp_pfn_backward.  The three parameters are inputs so that
    autograd routes their gradients, and the kernels read them from the call.  The points get no gradient."""

    @staticmethod
    def forward(ctx, eng, voxels, coors, npts, frames, w, gamma, beta):
        num = eng.num_tensor(voxels.shape[0])
        feat, arg, stats = eng.pfn_train_forward(voxels, coors, npts, num, w, gamma, beta)
        canvases = torch.cat([eng.scatter(feat[a:b], c, n) for a, b, c, n in frames])
        ctx.eng, ctx.frames = eng, frames
        ctx.save_for_backward(voxels, coors, npts, num, w, gamma, feat, arg, stats)
        ctx.mark_non_differentiable(stats)
        return canvases, stats

    @staticmethod
    def backward(ctx, gcanvas, _gstats):
        voxels, coors, npts, num, w, gamma, feat, arg, stats = ctx.saved_tensors
        eng = ctx.eng
        gcanvas = gcanvas.contiguous()
        dfeat = torch.empty_like(feat)
        for f, (a, b, c, n) in enumerate(ctx.frames):
            eng.scatter_backward(gcanvas[f], c, n, out=dfeat[a:b])
        dw, dg, db = eng.pfn_backward(voxels, coors, npts, num, w, gamma, stats, feat, arg, dfeat)
        need = ctx.needs_input_grad
        return (None,) * 5 + (dw if need[5] else None, dg if need[6] else None, db if need[7] else None)


class PointPillars:
    _norm = "instance"
    grad_precision = "fp32"
    grad_stages = "units"
    forward_precision = "fp32"  # train(forward_precision=...): the precision mode the training forward runs in
    bn_grad_precision = "fp32"  # train(bn_grad_precision=...) while training a BatchNorm network
    bn_stats = None  # train(bn_stats=...) while training a BatchNorm network
    # read-only defaults for an object assembled without __init__ (no engine: the key-order and plan tests); __init__ and
    # load_state_dict give every object its own
    _block = _down = _rpn = _pfn = _pfn_stats = _bn_run = _bn_nbt = types.MappingProxyType({})
    _pfn_nbt = None
    _bn_run_up = ()          # the _version numbers of _bn_run at the last fold into the engine
    _bn_run_trained = False  # the running statistics of the RPN moved since load_state_dict
    _uploaded = types.MappingProxyType({})  # per group of _GROUPS: its tensors' _version numbers at the last upload into the engine
    _trained = frozenset()                  # the groups that have been stepped since load_state_dict

    def __init__(self, config):
        self.device = config['device']
        self._config = config
        config['_pp_norm'] = self._norm
        self._eng = engine_for(config, self._norm)
        self._sd = None
        self.training = False
        self._scope = "head"         # train(scope=...): one of SCOPES; each trains what the one before it does and one group more
        # the groups of _GROUPS as dicts of device Parameters: the head's six tensors, the three upsampler weights, block 3's five
        # unit weights, its stride-2 weight, the ten convolutions of blocks 1 and 2, the PFN's Conv1d weight and BatchNorm1d weight / bias
        self._params, self._neck, self._block, self._down, self._rpn, self._pfn = {}, {}, {}, {}, {}, {}
        self._pfn_stats = {}         # running_mean / running_var as device tensors (train(scope="all") moves them)
        self._bn_run = {}            # BatchNorm backbone: running_mean / running_var of the RPN's nineteen norms as device tensors
        self._bn_nbt = {}            # their num_batches_tracked, where the loaded dict carried it (bn_stats="moving" counts)
        self._pfn_nbt = None         # num_batches_tracked when the loaded dict carried it
        self.profile_stages = True  # the reference synchronises after every stage (:365-374)
        self.pfn_time, self.rpn_time, self.scatter_time, self.heads_time = 0.0, 0.0, 0.0, 0.0
        # like nn.Module construction, start from random initial weights (the head as wide as the config's anchors per location)
        self.load_state_dict(init_state_dict(0, norm=self._norm, num_anchor_per_loc=self._eng.num_anchor_per_loc))

    # nn.Module-style surface used by train.py:196-205
    def to(self, device):
        return self

    def eval(self):
        return self.train(False)

    def train(self, mode=True, scope="head", grad_precision="fp32", bn_stats=None, grad_stages="units", bn_grad_precision="fp32",
              forward_precision="fp32"):
        """Training mode: forward() accepts a batch of several frames and the tensors of `scope` require grad (SCOPES, from "head",
        the six head parameters, to "all", everything net.parameters() yields in the reference: the module docstring lists them);
        everything in front of the scope stays frozen.  Under "all" the PFN normalises with batch statistics and moves its running
        ones, as the reference's net.train() does.  eval() / train(False) restores the inference behaviour, with the current parameters
        and running statistics folded into the engine.
        grad_precision ("fp32" | "bf16x3" | "bf16", kept as net.grad_precision, "fp32" again after eval()): the operand precision of
        the gradient products of the backwards that grad_stages names (kept as net.grad_stages, "units" again after eval()): "units",
        the Resnet units alone (pp_unit_backward_mp), or "rpn", the three strided stages (pp_down_backward_mp) and the three
        upsamplers (pp_neck_backward_mp) as well, wherever the scope runs them.  The forward, the head backward, the PFN and every
        tensor handed around stay fp32.  InstanceNorm backbone only: on a BatchNorm network the keyword is bn_grad_precision.
        bn_grad_precision ("fp32" | "bf16x3" | "bf16", BatchNorm networks under bn_stats only, kept as net.bn_grad_precision, "fp32"
        again after eval()): the same for the BatchNorm backwards (pp_*_backward_affine_mp under "frozen", pp_*_backward_bn_mp under
        "moving"), for the backwards grad_stages names; net.grad_precision stays "fp32" on these networks, and "fp32", the default, is
        the fp32 walk bit for bit.
        bn_stats (BatchNorm networks only, kept as net.bn_stats; None keeps such a network to scope="head") governs the nineteen
        BatchNorm2d layers of the RPN; a layer's weight / bias train with the convolution whose backward primitive yields their
        gradient (a unit's leading norm with that unit's convolution, blockN.1 with the strided convolution, deconvN.1 with the
        upsampler), so "rpn" trains the 63 tensors of BN_RPN_KEYS and "all" the 66 of BN_ALL_KEYS.  "frozen" fine-tunes: every layer
        stays in eval mode and normalises with its running statistics, which do not move, as does num_batches_tracked (in torch:
        net.train(), then .eval() on every BatchNorm2d module).  "moving" is the reference's net.train(): under every scope all
        nineteen normalise with the statistics of the batch (all frames of a forward together) and move their running statistics
        (momentum 0.01, unbiased variance) and num_batches_tracked, whether or not grad is enabled; the scope decides which tensors
        get gradients, exactly as under "frozen", and eval() folds the moved statistics into the engine before the next pass.  The
        keyword is explicit because "frozen" is not what torch's net.train() alone means; "batch" is refused: "moving" is its name
        here.  Under "all" the PFN's BatchNorm1d behaves as on the InstanceNorm network whatever bn_stats says.
        forward_precision ("fp32" | "bf16x3" | "bf16" | "fp16", InstanceNorm network only, kept as net.forward_precision, "fp32" again
        after eval()): the precision mode the training forward runs in.  A 16-bit value switches the engine to that mode
        (precision(mode)) if it is not there; the training forward then runs while the engine's effective precision equals it and
        raises RuntimeError otherwise (after float(), say).  The taps are fp32, the backward and the master weights are untouched, and
        grad_precision / grad_stages combine freely with it; the PFN is fp32 in every mode."""
        if forward_precision not in FORWARD_PRECISIONS:
            raise ValueError(f"train: forward_precision must be 'fp32', 'bf16x3', 'bf16' or 'fp16', got {forward_precision!r}")
        if forward_precision != "fp32" and self._norm != "instance":
            raise ValueError("train: forward_precision is for the InstanceNorm network; a BatchNorm network trains with an fp32 forward")
        if grad_precision not in GRAD_PRECISIONS:
            raise ValueError(f"train: grad_precision must be 'fp32', 'bf16x3' or 'bf16', got {grad_precision!r}")
        if grad_stages not in GRAD_STAGES:
            raise ValueError(f"train: grad_stages must be 'units' or 'rpn', got {grad_stages!r}")
        if scope not in SCOPES:
            raise ValueError(f"train: scope must be 'head', 'neck', 'block3', 'stage3', 'rpn' or 'all', got {scope!r}")
        if bn_grad_precision not in GRAD_PRECISIONS:
            raise ValueError(f"train: bn_grad_precision must be 'fp32', 'bf16x3' or 'bf16', got {bn_grad_precision!r}")
        if bn_grad_precision != "fp32" and self._norm != "batch":
            raise ValueError("train: bn_grad_precision is for the BatchNorm networks; on the InstanceNorm backbone the keyword is grad_precision")
        if bn_grad_precision != "fp32" and bn_stats is None:
            raise ValueError("train: bn_grad_precision needs bn_stats ('frozen' or 'moving'): without it a BatchNorm network trains its head alone")
        if bn_stats is not None:
            if bn_stats not in BN_STATS:
                raise ValueError(f"train: bn_stats must be None, 'frozen' or 'moving', got {bn_stats!r}")
            if self._norm != "batch":
                raise ValueError("train: bn_stats is for the BatchNorm networks; the InstanceNorm backbone has no statistics to freeze")
            if bn_stats == "batch":
                raise NotImplementedError("train(bn_stats='batch'): training with batch statistics is bn_stats='moving' (the running "
                                          "statistics move, as under torch's net.train()); bn_stats='frozen' fine-tunes with them fixed")
            if grad_precision != "fp32":
                raise ValueError("train: on a BatchNorm network grad_precision stays 'fp32'; bn_grad_precision picks the operand precision "
                                 "of the BatchNorm backwards")
        if mode and scope != "head" and ((self._norm != "instance" and bn_stats not in ("frozen", "moving")) or (scope == "all" and len(self._pfn_stats) != 2) or
                                         any(len(getattr(self, g.attr)) != len(self._group_keys(g)) for g in self._groups(scope) if g.scope != "head")):
            raise RuntimeError(f"train(scope='{scope}'): the neck and block backward exist for the InstanceNorm backbone only" +
                               ("; on a BatchNorm network pass bn_stats='frozen' to fine-tune with frozen statistics" if self._norm == "batch" else ""))
        self.training = bool(mode)
        self._scope = scope if self.training else "head"
        self.grad_precision = grad_precision if self.training else "fp32"
        self.grad_stages = grad_stages if self.training else "units"
        self.forward_precision = forward_precision if self.training else "fp32"
        if self.forward_precision != "fp32" and self._eng.effective_precision() != self.forward_precision:
            self.precision(self.forward_precision)
        self.bn_grad_precision = bn_grad_precision if self.training else "fp32"
        self.bn_stats = bn_stats if self.training else None
        trained = self._groups(self._scope) if self.training else ()
        for g in _GROUPS.values():
            for p in getattr(self, g.attr).values():
                p.requires_grad_(g in trained)
        if not self._pfn_training():
            self._sync_pfn()  # whatever reads the engine's eval-mode PFN next (this object or framework.inference) sees the trained one
        return self

    @staticmethod
    def _groups(scope):
        """The groups train(scope=scope) trains, from the front of the network to the head."""
        return [g for g in _GROUPS.values() if SCOPES.index(g.scope) <= SCOPES.index(scope)]

    def _group_keys(self, g):
        """The state_dict names of group g in this network: on the BatchNorm backbone a group of RPN convolutions also holds the
        weight and bias of the BatchNorm2d layers that go with them (with_bn)."""
        return with_bn(g.keys) if self._norm == "batch" else g.keys

    def _trainable(self):
        every = {k: p for g in self._groups(self._scope) for k, p in getattr(self, g.attr).items()}
        if self._scope in ("rpn", "all"):
            return {k: every[k] for k in (BN_ALL_KEYS if self._norm == "batch" else ALL_KEYS) if k in every}  # the reference's order
        return every

    def named_parameters(self):
        """The trainable tensors on the device: heads.conv_{cls,box,dir}.{weight,bias}, behind rpn.deconv{1,2,3}.0.weight under
        train(scope="neck"), behind BLOCK3_KEYS (unit order) as well under train(scope="block3"), and behind rpn.block3.0.weight
        under train(scope="stage3"); under train(scope="rpn") the 25 tensors of RPN_KEYS in the reference's state_dict order, under
        train(scope="all") the 28 of ALL_KEYS.  Everything before them is frozen.  On a BatchNorm network under bn_stats="frozen" every
        RPN convolution comes with its norm's weight and bias: the 63 of BN_RPN_KEYS under "rpn", the 66 of BN_ALL_KEYS under "all"."""
        return iter(self._trainable().items())

    def parameters(self):
        return iter(self._trainable().values())

    def zero_grad(self, set_to_none=True):
        for g in _GROUPS.values():
            for p in getattr(self, g.attr).values():
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def _versions(self, attr):
        g = _GROUPS[attr]
        return tuple(t._version for d in (g.attr, g.stats) if d for t in getattr(self, d).values())

    def _moved(self, attr):
        """An optimizer stepped the group (or the running statistics moved): a _version differs from the last upload's."""
        up = self._uploaded.get(attr)
        return up is not None and self._versions(attr) != up

    def _stepped(self):
        """The groups whose current values differ from the loaded ones."""
        return [a for a in _GROUPS if a in self._trained or self._moved(a)]

    def _mark_uploaded(self, attrs=tuple(_GROUPS)):
        self._uploaded = {**self._uploaded, **{a: self._versions(a) for a in attrs}}

    def _sync_group(self, attr):
        """When the group moved, rewrite the engine's committed image of it in place, with the groups the same call carries."""
        if self._moved(attr):
            convs = ("_rpn", "_down", "_block")  # in a 16-bit mode the sixteen convolutions always go up together (_upload)
            gone_up = convs if attr in convs and self._eng.effective_precision() not in (None, "fp32") else (attr,) + _GROUPS[attr].covers
            self._trained = self._trained | {a for a in gone_up if self._moved(a)}
            self._upload(attr)
            self._mark_uploaded(gone_up)

    def _upload(self, attr):
        """The engine call that writes group attr's current values into the committed plan, chosen by the engine's effective
        precision: the group's own fp32 entry, or in a 16-bit mode the _mp entry of its family (there the sixteen convolutions always
        go up together).  The PFN is fp32 in every mode.  "fp16s" has no in-place writer."""
        mode = self._eng.effective_precision()
        if attr == "_pfn" or mode in (None, "fp32"):
            return _GROUPS[attr].upload(self)
        if mode not in FORWARD_PRECISIONS:
            raise RuntimeError(f"the network runs '{mode}', whose packed weights cannot be rewritten in place: load_state_dict(net.state_dict()) "
                               "again to commit the trained weights in this mode")
        if attr == "_params":
            return self._eng.update_head_weights(self._params, forward_precision=mode)
        if attr == "_neck":
            return self._eng.update_neck_weights(self._neck, forward_precision=mode)
        return self._eng.update_rpn_weights({**self._rpn, **self._down, **self._block}, forward_precision=mode)

    def _sync_head(self):
        """An optimizer stepped the head: rewrite the engine's packed head in place."""
        self._sync_group("_params")

    def _sync_pfn(self):
        """The same for the pillar feature net, ahead of whatever runs the eval-mode PFN: a stepped parameter or moved running
        statistics are folded into the engine's transposed weight, scale and shift (pp_update_pfn_weights)."""
        self._sync_group("_pfn")

    def _sync_neck(self):
        """The same for the three upsampler weights, block 3's five and its stride-2 weight, ahead of whatever runs the backbone; when
        a convolution of blocks 1 and 2 moved, all sixteen go up in one pp_update_rpn_weights.  On the BatchNorm backbone the groups
        hold the norms' weight / bias too: when one moved, or the running statistics did (bn_stats="moving"), all nineteen layers are
        folded again in place (pp_update_bn_fold)."""
        run = tuple(t._version for t in self._bn_run.values())
        fold = self._norm == "batch" and (any(self._moved(attr) for attr in _BACKBONE) or run != self._bn_run_up)
        for attr in _BACKBONE:
            self._sync_group(attr)
        if fold:
            self._bn_run_trained = self._bn_run_trained or run != self._bn_run_up
            self._bn_run_up = run
            self._eng.update_bn_fold({**self._bn_run, **{k: p for attr in _BACKBONE for k, p in getattr(self, attr).items()}})

    def half(self):
        """The reference deploys FP16 TensorRT engines (framework/trt_utils.py:30, networks/pointpillars8_trt.py:208-223,295-314).
        Here: fp16 MFMA operands for every convolution, upsampler and the head, fp32 accumulation, activations still fp32 in
        HBM; tolerance table in DESIGN.md.  The parity contract (<= 1e-3 vs the fp32 reference) is stated for float() / the
        default (and is also met by precision("bf16x3"))."""
        return self.precision("fp16")

    def float(self):
        return self.precision("fp32")

    def precision(self, mode):
        """ "fp32" | "bf16x3" (split-bf16: fp32-equivalent on the bf16 MFMAs) | "fp16" | "bf16" | "fp16s" (fp16 operands and fp16 tensors)."""
        self._eng.set_precision(mode)
        # a change of mode packs the loaded weights again: what was stepped goes up before it is next used (heads(), a backbone pass)
        stale = self._stepped()
        self._uploaded = {**self._uploaded, **{a: () for a in stale}}
        if self._bn_run_trained:
            self._bn_run_up = None  # the new plan folds the loaded statistics: the moved ones go up before the next pass
        if "_pfn" in stale and not self._pfn_training():
            self._sync_pfn()
        return self

    def state_dict(self):
        """The loaded tensors; those of every group that was stepped (the head's six, the three upsampler weights, the sixteen 3 x 3
        convolutions of the RPN, the pillar feature net with its running statistics) with their CURRENT values, and so the running
        statistics and num_batches_tracked of the RPN's BatchNorm2d layers once train(bn_stats="moving") has moved them."""
        sd = dict(self._sd)
        for attr in self._stepped():
            for d in (attr, _GROUPS[attr].stats):
                for k, t in (getattr(self, d).items() if d else ()):
                    sd[k] = t.detach().cpu().numpy().reshape(self._sd[k].shape)
            if attr == "_pfn" and self._pfn_nbt is not None:
                sd[PFN_NBT_KEY] = np.asarray(self._pfn_nbt, dtype=np.int64)
        if self._bn_run_trained or tuple(t._version for t in self._bn_run.values()) != self._bn_run_up:
            for k, t in self._bn_run.items():
                sd[k] = t.detach().cpu().numpy().reshape(self._sd[k].shape)
            for k, v in self._bn_nbt.items():
                sd[k] = np.asarray(v, dtype=np.int64)
        return sd

    def load_state_dict(self, sd, strict=True):
        self._sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in sd.items()}
        self._eng.load_state_dict(self._sd)
        dev_of = lambda k: torch.from_numpy(np.ascontiguousarray(self._sd[k], dtype=np.float32)).to(self._eng.device)  # noqa: E731
        trained = self._groups(self._scope) if self.training else ()
        for g in _GROUPS.values():
            setattr(self, g.attr, {k: torch.nn.Parameter(dev_of(k), requires_grad=g in trained) for k in self._group_keys(g) if k in self._sd})
        self._pfn_stats = {k: dev_of(k) for k in PFN_STAT_KEYS if k in self._sd}
        bn_run = [f"{p}.{s}" for p, _ in Engine.bn_layers() for s in Engine.BN_FIELDS[2:]] if self._norm == "batch" else ()
        self._bn_run = {k: dev_of(k) for k in bn_run if k in self._sd}
        self._pfn_nbt = int(np.asarray(self._sd[PFN_NBT_KEY])) if PFN_NBT_KEY in self._sd else None
        nbt = [f"{p}.num_batches_tracked" for p, _ in Engine.bn_layers()] if self._norm == "batch" else ()
        self._bn_nbt = {k: int(np.asarray(self._sd[k])) for k in nbt if k in self._sd}
        self._bn_run_up, self._bn_run_trained = tuple(t._version for t in self._bn_run.values()), False
        self._uploaded, self._trained = {}, frozenset()
        self._mark_uploaded()
        return self

    def _sync(self):
        if self.profile_stages:
            torch.cuda.synchronize()
        return time.time()

    def _mode_error(self, what, why):
        """The message of a training forward whose engine does not run net.forward_precision."""
        runs = self._eng.effective_precision()
        if self.forward_precision == "fp32":
            return f"{what} needs the fp32 precision mode: the network runs '{runs}' ({why}); call float()"
        return (f"{what} under train(forward_precision='{self.forward_precision}') needs the engine in that mode: the network runs '{runs}'; "
                f"call precision('{self.forward_precision}'), or train() again")

    def _pfn_training(self):
        return self.training and self._scope == "all"

    def pfn_train(self, frames):
        """PointNet in train mode and the scatter on a batch: frames = [(voxels [n,T,4], coors [n,3], num_points_per_voxel [n]), ...],
        at most max_batch of them -> canvases [nb,64,gx,gy].  BatchNorm1d normalises with the statistics of the pillars of all frames
        together and the running statistics move (momentum 0.1, unbiased variance), whether or not grad is enabled.  Differentiable
        with respect to PFN_KEYS when they require grad (train(scope="all")).  The PFN itself is fp32 in every mode; the engine must run
        net.forward_precision (the fp32 mode unless train(forward_precision=...) said otherwise)."""
        eng = self._eng
        if not 1 <= len(frames) <= eng.max_batch:
            raise ValueError(f"pfn_train: {len(frames)} frames in the batch, max_batch is {eng.max_batch}")
        if len(self._pfn) != 3 or len(self._pfn_stats) != 2:
            raise RuntimeError("pfn_train: the state_dict holds no pillar feature net")
        if eng.effective_precision() != self.forward_precision:
            raise RuntimeError(self._mode_error("PFN training", "the backward of the RPN behind it is fp32"))
        voxels = torch.cat([f[0] for f in frames]).contiguous()
        coors = torch.cat([f[1] for f in frames]).contiguous()
        npts = torch.cat([f[2] for f in frames]).contiguous()
        rows, spans = 0, []
        for _, c, _ in frames:
            spans.append((rows, rows + int(c.shape[0]), c.contiguous(), eng.num_tensor(c.shape[0])))
            rows += int(c.shape[0])
        canvases, stats = _PfnFunction.apply(eng, voxels, coors, npts, tuple(spans), *[self._pfn[k] for k in PFN_KEYS])
        n = rows * eng.T
        with torch.no_grad():  # BatchNorm1d's update, evaluated in fp64 and rounded once
            rm, rv = (self._pfn_stats[k] for k in PFN_STAT_KEYS)
            rm.copy_(((1.0 - BN_MOMENTUM) * rm.double() + BN_MOMENTUM * stats[:64]).float())
            rv.copy_(((1.0 - BN_MOMENTUM) * rv.double() + BN_MOMENTUM * (n / (n - 1.0)) * stats[64:128]).float())
        if self._pfn_nbt is not None:
            self._pfn_nbt += 1
        return canvases

    def _forward_frames(self, example):
        """Several frames collated by merge_second_batch (coordinates carry the frame index as their last column): each frame runs
        the frozen PFN / scatter / backbone, the rpn outputs are stacked and the head runs on the batch.  Under train(scope="all") the
        PFN runs in train mode over the pillars of all frames together (pfn_train)."""
        eng = self._eng
        coors = example["coordinates"]
        frame = coors[:, -1]
        nb = int(frame.max().item()) + 1 if coors.shape[0] else 1
        if not 1 <= nb <= eng.max_batch:
            raise ValueError(f"forward: {nb} frames in the batch, max_batch is {eng.max_batch}")
        neck = self._neck_grad()
        self._sync_neck()
        if self._pfn_training():
            sels = [frame == f for f in range(nb)]
            canvases = self.pfn_train([(example["voxels"][s], coors[s][:, :-1].contiguous(), example["num_points_per_voxel"][s]) for s in sels])
            return self.heads(self.rpn_train(canvases) if neck else torch.cat([eng.backbone(c) for c in canvases]))
        self._sync_pfn()
        rpn = []
        with torch.no_grad():
            for f in range(nb):
                sel = frame == f
                c = coors[sel][:, :-1].contiguous()
                num = eng.num_tensor(c.shape[0])
                feat = eng.pfn(example["voxels"][sel].contiguous(), c, example["num_points_per_voxel"][sel].contiguous(), num)
                canvas = eng.scatter(feat, c, num)
                rpn.append(canvas if neck else eng.backbone(canvas))
        return self.heads(self.rpn_train(torch.cat(rpn)) if neck else torch.cat(rpn))

    def forward(self, example):
        eng = self._eng
        if example["coordinates"].dim() == 2 and example["coordinates"].shape[1] == 4:
            return self._forward_frames(example)
        voxels = example["voxels"].contiguous()
        npts = example["num_points_per_voxel"].contiguous()
        coors = example["coordinates"].contiguous()
        num = eng.num_tensor(voxels.shape[0])
        start = time.time()
        if self._pfn_training():
            canvas = self.pfn_train([(voxels, coors, npts)])  # PFN and scatter are one Function: both are booked as pfn_time
            pfn_time = self._sync()
        else:
            self._sync_pfn()
            feat = eng.pfn(voxels, coors, npts, num)
            pfn_time = self._sync()
            canvas = eng.scatter(feat, coors, num)
        scatter_time = self._sync()
        rpn = self.rpn_train(canvas) if self._neck_grad() else self.rpn(canvas)
        rpn_time = self._sync()
        p = self.heads(rpn)
        cls, box, dr = p["cls_preds"], p["box_preds"], p["dir_preds"]
        heads_time = self._sync()
        self.pfn_time += pfn_time - start
        self.scatter_time += scatter_time - pfn_time
        self.rpn_time += rpn_time - scatter_time
        self.heads_time += heads_time - rpn_time
        return {"cls_preds": cls, "box_preds": box, "dir_preds": dr}

    __call__ = forward

    # sub-stages, named as the reference's sub-modules, for stage-wise parity tests
    def pillar_point_net(self, voxels, num_point_per_voxel, coors):
        self._sync_pfn()
        return self._eng.pfn(voxels.contiguous(), coors.contiguous(), num_point_per_voxel.contiguous(),
                             self._eng.num_tensor(voxels.shape[0]))[:voxels.shape[0]]

    def middle_feature_extractor(self, voxel_features, coords):
        return self._eng.scatter(voxel_features.contiguous(), coords.contiguous(), self._eng.num_tensor(coords.shape[0]))

    def rpn(self, x):
        self._sync_neck()
        return self._eng.backbone(x.contiguous())

    def _backbone_requires_grad(self):
        return any(p.requires_grad for attr in _BACKBONE for p in getattr(self, attr).values())

    def _neck_grad(self):
        """The training forward goes through rpn_train(): a backbone tensor gets a gradient, or bn_stats="moving" runs the lock-step pass."""
        return self.training and (self.bn_stats == "moving" or
                                  (self._scope != "head" and torch.is_grad_enabled() and self._backbone_requires_grad()))

    def rpn_train(self, x):
        """RPN.forward on canvases x [B,64,gx,gy], 1 <= B <= max_batch, one backbone pass per frame; same values as rpn() bit for
        bit.  Differentiable with respect to the three upsampler weights when they require grad (train(scope="neck")) and to block
        3's five unit weights (train(scope="block3")) and its stride-2 weight (train(scope="stage3")); under train(scope="rpn") to all
        sixteen convolutions, and then also to x itself when it requires grad (the level-0 dx: where the PFN backward starts).
        Gradients are fp32; the engine must run net.forward_precision (the fp32 mode unless train(forward_precision=...) said otherwise)."""
        eng = self._eng
        gx, gy = int(eng.grid_size[0]), int(eng.grid_size[1])
        if not isinstance(x, torch.Tensor) or x.numel() == 0 or x.numel() % (64 * gx * gy):
            raise ValueError(f"rpn_train: expected canvases [B,64,{gx},{gy}]")
        x = x.contiguous().reshape(-1, 64, gx, gy)  # a view: a canvas that requires grad stays in the graph
        if not 1 <= x.shape[0] <= eng.max_batch:
            raise ValueError(f"rpn_train: {x.shape[0]} frames in the batch, max_batch is {eng.max_batch}")
        self._sync_neck()
        moving = self.training and self.bn_stats == "moving"
        if not (torch.is_grad_enabled() and self._backbone_requires_grad()) and not moving:
            return torch.cat([eng.backbone(c) for c in x])
        if eng.effective_precision() != self.forward_precision:
            raise RuntimeError(self._mode_error("neck training", "gradients are fp32 and the packed 16-bit upsampler weights cannot be updated in place"))
        # the depth of the backward: the first convolution of the frontmost group that holds a parameter requiring grad
        req = lambda group: any(p.requires_grad for p in group.values())  # noqa: E731
        first = 0 if req(self._rpn) else _W0[2] if req(self._down) else _W0[2] + 1 if req(self._block) else len(RPN_CONV_KEYS)
        every = {**self._rpn, **self._down, **self._block}
        if first:
            x = x.detach()  # nothing in front of the stage has a backward: the graph must not reach the canvases
        if self._norm == "batch":  # every layer goes in with its norm's weight and bias
            every.update(self._neck)
            layers = RPN_CONV_KEYS[first:] + NECK_KEYS
            tensors = [every[n] for k in layers for n in (k, *bn_affine_keys(k))]
            if self.bn_grad_precision != "fp32":  # the pair (units, stages) rides behind the tensors; an fp32 run makes the calls it made
                tensors.append((self.bn_grad_precision, self.bn_grad_precision if self.grad_stages == "rpn" else "fp32"))
            if moving:
                return self._rpn_train_moving(first, x, tensors)
            stats = [tuple(self._bn_run[f"{Engine.bn_prefix(k)}.{s}"] for s in Engine.BN_FIELDS[2:]) for k in layers]
            return _RpnBnFunction.apply(eng, first, stats, x, *tensors)
        fwd = () if self.forward_precision == "fp32" else (self.forward_precision,)  # rides behind the weights; an fp32 run makes the calls it made
        return _RpnFunction.apply(eng, (self.grad_precision, self.grad_precision if self.grad_stages == "rpn" else "fp32"), first, x,
                                  *[every[k] for k in RPN_CONV_KEYS[first:]], *[self._neck[k] for k in NECK_KEYS], *fwd)

    def _rpn_train_moving(self, first, x, tensors):
        """rpn_train under bn_stats="moving": one lock-step pass with batch statistics, then BatchNorm2d's update of the running
        statistics, evaluated in fp64 and rounded once, in place (so that _sync_neck folds them again before the next eval-mode pass)."""
        eng = self._eng
        nb = int(x.shape[0])
        counts = [nb * (eng.H >> b) * (eng.W >> b) for b in range(3)]
        if min(counts) <= 1:
            raise ValueError("rpn_train: expected more than 1 value per channel when training (BatchNorm2d with batch statistics)")
        with torch.set_grad_enabled(torch.is_grad_enabled() and self._backbone_requires_grad()):
            y, mean, var = _RpnBnBatchFunction.apply(eng, first, {k: p for attr in _BACKBONE for k, p in getattr(self, attr).items()}, x, *tensors)
        with torch.no_grad():
            i = 0
            for b, mods in RPN_TABLE:
                for k in RPN_CONV_KEYS[_W0[b]:_W0[b] + 1 + sum(mods)] + (NECK_KEYS[b],):
                    p = Engine.bn_prefix(k)
                    n = float(nb * eng.H * eng.W if k in NECK_KEYS else counts[b])
                    rm, rv = self._bn_run[p + ".running_mean"], self._bn_run[p + ".running_var"]
                    c = rm.shape[0]
                    rm.copy_(((1.0 - BN2D_MOMENTUM) * rm.double() + BN2D_MOMENTUM * mean[i, :c].double()).float())
                    rv.copy_(((1.0 - BN2D_MOMENTUM) * rv.double() + BN2D_MOMENTUM * (n / (n - 1.0)) * var[i, :c].double()).float())
                    i += 1
        self._bn_nbt = {k: v + 1 for k, v in self._bn_nbt.items()}
        return y

    def heads(self, x):
        """SharedHead.forward on x [B,320,H,W], 1 <= B <= max_batch.  Differentiable with respect to x and the head parameters when
        one of them requires grad (train() for the parameters); gradients are fp32, and the engine must run net.forward_precision."""
        x = x.contiguous()
        params = list(self._params.values())
        self._sync_head()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            if self._eng.effective_precision() != self.forward_precision:
                raise RuntimeError(self._mode_error("head training", "gradients are fp32 and the packed 16-bit head weights cannot be updated in place"))
            if x.dim() != 4:
                x = x.reshape(-1, 320, self._eng.H, self._eng.W)
            cls, box, dr = _HeadFunction.apply(self._eng, x, *params)
        else:
            cls, box, dr = self._eng.head(x)
        return {"cls_preds": cls, "box_preds": box, "dir_preds": dr}
