"""networks.pointpillars8_shared.PointPillars (reference pointpillars8_shared.py:346-382): the eager
network with the InstanceNorm backbone, running PFN / scatter / RPN / head as HIP kernels.

Training surface: head fine-tuning, optionally with the neck and with block 3.  train() makes the six tensors of the anchor head
require grad; heads(x) then records a torch.autograd.Function whose backward is pp_head_backward (csrc/train.hip).
train(scope="neck") adds the three upsampler weights rpn.deconv{1,2,3}.0.weight: the training forward then runs the backbone through
pp_backbone_taps and records a second Function whose backward is pp_neck_backward (csrc/neck_train.hip).  train(scope="block3") adds
the five convolutions of the deepest Resnet block (BLOCK3_KEYS, unit order): the forward runs pp_backbone_block_taps and the
backward continues from the third upsampler's dx through five pp_unit_backward calls (csrc/block_train.hip).  train(scope="stage3")
adds block 3's stride-2 convolution rpn.block3.0.weight: the forward runs pp_backbone_stage_taps, which also hands out that conv's
pre-norm output, and the backward ends in pp_down_backward (csrc/down_train.hip).  Everything in front of it (PFN, scatter, blocks 1
and 2 with their stride-2 convolutions) is FROZEN under those scopes.

Training the whole RPN: train(scope="rpn") trains all sixteen 3 x 3 convolutions, the three upsamplers and the head (RPN_KEYS, the
reference's state_dict order, 25 tensors).  The forward runs pp_backbone_train_taps, which hands out every block's unit inputs and
every strided convolution's pre-norm output; the backward (_RpnFunction) walks RPN_TABLE from block 3 to block 1: each block's
pp_unit_backward chain, its pp_down_backward with the gradient of the stage input, to which the upsampler's dx of the level above is
added.  The gradient of block 3's input that pp_down_backward computes is consumed by block 2 here.  optimizer.step() is followed by
pp_update_rpn_weights, which also rewrites the sparse first convolution's image.  PFN and scatter stay frozen under "rpn"; rpn_train()
returns the gradient with respect to the canvases when they require grad.

Training everything: train(scope="all") adds the pillar feature net (PFN_KEYS; ALL_KEYS = the 28 tensors net.parameters() yields in the
reference, in its state_dict order) and follows the reference's train.py, whose net.train() makes BatchNorm1d normalise with batch
statistics: every training-mode forward runs pp_pfn_train_forward over the pillars of all frames of the batch (_PfnFunction), moves
running_mean / running_var (momentum 0.1, unbiased variance) and counts num_batches_tracked, whether or not grad is enabled.  The
backward consumes the canvases' gradient: pp_scatter_backward per frame, then one pp_pfn_backward (csrc/pfn_train.hip).  The eval-mode
PFN of the engine (running statistics folded into scale / shift) is rewritten by pp_update_pfn_weights before it is next used.

Mixed precision: train(..., grad_precision="bf16x3" | "bf16") runs the two gradient products of every Resnet unit backward with split
or plain bf16 operands on the bf16 MFMA (pp_unit_backward_mp); the forward, the weights, every tensor handed around and the other
backwards stay fp32, and "fp32", the default, is the fp32 path bit for bit."""
import time
import types

import numpy as np
import torch

from ..engine import Engine, engine_for
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
# the scopes that train: the upsamplers; block 3's units; block 3's strided convolution; blocks 1 and 2; the pillar feature net
_NECK_SCOPES, _BLOCK_SCOPES, _STAGE_SCOPES, _RPN_SCOPES = SCOPES[1:], SCOPES[2:], SCOPES[3:], SCOPES[4:]


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


class _NeckFunction(torch.autograd.Function):
    """RPN.forward on a list of canvases as pp_backbone_taps per frame, stacked; its backward is pp_neck_backward for the three
    upsampling branches.  The three weights are inputs only so that autograd routes their gradients; the forward reads the engine's
    packed copy of them (PointPillars uploads it beforehand).  The block outputs get no gradient: nothing in front of them trains."""

    @staticmethod
    def forward(ctx, eng, canvases, *weights):
        ctx.eng = eng
        outs = [eng.backbone_taps(c) for c in canvases]
        y, x1, x2, x3 = (torch.cat([o[i] for o in outs]) for i in range(4))
        ctx.save_for_backward(y, x1, x2, x3, *weights)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, *rest = ctx.saved_tensors
        taps, weights = rest[:3], rest[3:]
        gy = gy.contiguous()
        dws = tuple(ctx.eng.neck_backward(b, taps[b], weights[b], y, gy, need_dx=False)[0] if ctx.needs_input_grad[2 + b] else None
                    for b in range(3))
        return (None, None) + dws


class _BlockFunction(torch.autograd.Function):
    """RPN.forward as pp_backbone_block_taps per frame, stacked; its backward is pp_neck_backward for the three branches (dx for
    branch 2 only) and then pp_unit_backward for block 3's five units, from unit e back to unit a.  The weights (five of block 3,
    three upsamplers) are inputs only so that autograd routes their gradients.  Unit a's input gets no gradient: the stride-2
    convolution behind it stays frozen."""

    @staticmethod
    def forward(ctx, eng, prec, canvases, *weights):
        ctx.eng, ctx.prec = eng, prec
        outs = [eng.backbone_block_taps(c) for c in canvases]
        y, x1, x2, x3 = (torch.cat([o[i] for o in outs]) for i in range(4))
        units = [torch.stack([o[4][k] for o in outs]) for k in range(5)]  # h, m3, r3, m4, r4, each [nb,256,H/4,W/4]
        ctx.save_for_backward(y, x1, x2, x3, *units, *weights)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, *rest = ctx.saved_tensors
        taps, units, wb, wn = rest[:3], rest[3:8], rest[8:13], rest[13:16]
        eng, prec, gy = ctx.eng, ctx.prec, gy.contiguous()
        need_b, need_n = ctx.needs_input_grad[3:8], ctx.needs_input_grad[8:11]
        dwn = [None] * 3
        g = None
        for b in range(3):
            if need_n[b] or (b == 2 and any(need_b)):
                dwn[b], dx = eng.neck_backward(b, taps[b], wn[b], y, gy, need_dx=(b == 2 and any(need_b)))
                if b == 2:
                    g = dx
                if not need_n[b]:
                    dwn[b] = None
        dwb = [None] * 5
        if any(need_b):
            h, m3, r3, m4, r4 = units
            dwb[4], g_r4 = eng.unit_backward(r4, wb[4], g, dskip=g, grad_precision=prec)
            dwb[3], g_m4 = eng.unit_backward(m4, wb[3], g_r4, grad_precision=prec)
            dwb[2], g_r3 = eng.unit_backward(r3, wb[2], g_m4, dskip=g_r4, grad_precision=prec)
            dwb[1], g_m3 = eng.unit_backward(m3, wb[1], g_r3, grad_precision=prec)
            dwb[0], _ = eng.unit_backward(h, wb[0], g_m3, need_du=False, grad_precision=prec)
            dwb = [d if n else None for d, n in zip(dwb, need_b)]
        return (None, None, None) + tuple(dwb) + tuple(dwn)


class _StageFunction(torch.autograd.Function):
    """_BlockFunction with block 3's stride-2 stage in front: the forward is pp_backbone_stage_taps per frame, the backward that of
    _BlockFunction down to unit b, then unit a with its input gradient (plus the residual path's) and pp_down_backward for the weight
    of the stride-2 convolution.  Block 2's output gets no gradient: nothing in front of the stage trains."""

    @staticmethod
    def forward(ctx, eng, prec, canvases, w0, *weights):
        ctx.eng, ctx.prec = eng, prec
        outs = [eng.backbone_stage_taps(c) for c in canvases]
        y, x1, x2, x3 = (torch.cat([o[i] for o in outs]) for i in range(4))
        units = [torch.stack([o[4][k] for o in outs]) for k in range(5)]
        z3 = torch.cat([o[5] for o in outs])
        ctx.save_for_backward(y, x1, x2, x3, *units, z3, w0, *weights)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, *rest = ctx.saved_tensors
        taps, units, z3, w0, wb, wn = rest[:3], rest[3:8], rest[8], rest[9], rest[10:15], rest[15:18]
        eng, prec, gy = ctx.eng, ctx.prec, gy.contiguous()
        need_0, need_b, need_n = ctx.needs_input_grad[3], ctx.needs_input_grad[4:9], ctx.needs_input_grad[9:12]
        deep = need_0 or any(need_b)
        dwn = [None] * 3
        g = None
        for b in range(3):
            if need_n[b] or (b == 2 and deep):
                dwn[b], dx = eng.neck_backward(b, taps[b], wn[b], y, gy, need_dx=(b == 2 and deep))
                if b == 2:
                    g = dx
                if not need_n[b]:
                    dwn[b] = None
        dwb, dw0 = [None] * 5, None
        if deep:
            h, m3, r3, m4, r4 = units
            dwb[4], g_r4 = eng.unit_backward(r4, wb[4], g, dskip=g, grad_precision=prec)
            dwb[3], g_m4 = eng.unit_backward(m4, wb[3], g_r4, grad_precision=prec)
            dwb[2], g_r3 = eng.unit_backward(r3, wb[2], g_m4, dskip=g_r4, grad_precision=prec)
            dwb[1], g_m3 = eng.unit_backward(m3, wb[1], g_r3, grad_precision=prec)
            dwb[0], g_h = eng.unit_backward(h, wb[0], g_m3, dskip=g_r3, need_du=need_0, grad_precision=prec)
            dwb = [d if n else None for d, n in zip(dwb, need_b)]
            if need_0:
                dw0, _ = eng.down_backward(taps[1], w0, z3, g_h, need_dx=False)
        return (None, None, None, dw0) + tuple(dwb) + tuple(dwn)


def rpn_block_backward(eng, modules, units, weights, g, grad_precision="fp32"):
    """The backward of one block's Resnet modules (a row of RPN_TABLE): units and weights in unit order, g = dL/d(block output) ->
    (dw per unit, dL/d(block input h)).  grad_precision: the operand precision of every unit backward (Engine.unit_backward)."""
    prec = grad_precision
    dws = [None] * len(units)
    i = len(units)
    for n in reversed(modules):
        i -= n
        if n == 2:
            dws[i + 1], gm = eng.unit_backward(units[i + 1], weights[i + 1], g, grad_precision=prec)
            dws[i], g = eng.unit_backward(units[i], weights[i], gm, dskip=g, grad_precision=prec)
        else:
            dws[i], g = eng.unit_backward(units[i], weights[i], g, dskip=g, grad_precision=prec)
    return dws, g


class _RpnFunction(torch.autograd.Function):
    """RPN.forward as pp_backbone_train_taps per frame, stacked; its backward is pp_neck_backward for the three branches, each with dx,
    and then, from level 2 down to level 0 along RPN_TABLE, the block's unit chain and its strided stage (pp_down_backward); the stage's
    dx plus the upsampler's dx of the level above (in this order: upsampler + stage) is the gradient of that level's block output.
    weights: the sixteen convolutions in RPN_CONV_KEYS order, then the three upsamplers.  The canvases get level 0's dx when they
    require grad."""

    @staticmethod
    def forward(ctx, eng, prec, x, *weights):
        ctx.eng, ctx.prec = eng, prec
        outs = [eng.backbone_train_taps(c) for c in x]
        y = torch.cat([o[0] for o in outs])
        taps = [torch.cat([o[1][b] for o in outs]) for b in range(3)]
        units = [torch.stack([o[2][b][k] for o in outs]) for b, mods in RPN_TABLE for k in range(sum(mods))]
        zs = [torch.cat([o[3][b] for o in outs]) for b in range(3)]
        ctx.save_for_backward(x, y, *taps, *units, *zs, *weights)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, *rest = ctx.saved_tensors
        taps, units, zs, wc, wn = rest[:3], rest[3:16], rest[16:19], rest[19:35], rest[35:38]
        eng, gy = ctx.eng, gy.contiguous()
        need = ctx.needs_input_grad[1:]  # [1] the canvases, [2 + i] weight i
        dwn, dxn = zip(*[eng.neck_backward(b, taps[b], wn[b], y, gy, need_dx=True) for b in range(3)])
        dwc = [None] * 16
        g = None
        for b, mods in reversed(RPN_TABLE):
            n, w0 = sum(mods), (0, 4, 10)[b]  # the level's strided convolution in RPN_CONV_KEYS; its units follow
            u0 = w0 - b
            g = dxn[b] if g is None else dxn[b] + g
            dwc[w0 + 1:w0 + 1 + n], gh = rpn_block_backward(eng, mods, units[u0:u0 + n], wc[w0 + 1:w0 + 1 + n], g, ctx.prec)
            dwc[w0], g = eng.down_backward(x if b == 0 else taps[b - 1], wc[w0], zs[b], gh, need_dx=b > 0 or need[1])
        grads = [d if need[2 + i] else None for i, d in enumerate(list(dwc) + list(dwn))]
        return (None, None, g if need[1] else None) + tuple(grads)


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
    # read-only defaults for an object assembled without __init__ (no engine: the key-order tests); __init__ and load_state_dict
    # give every object its own
    _block, _block_uploaded, _block_trained = types.MappingProxyType({}), None, False
    _down, _down_uploaded, _down_trained = types.MappingProxyType({}), None, False
    _rpn, _rpn_uploaded, _rpn_trained = types.MappingProxyType({}), None, False
    _pfn, _pfn_stats, _pfn_uploaded, _pfn_trained, _pfn_nbt = types.MappingProxyType({}), types.MappingProxyType({}), None, False, None

    def __init__(self, config):
        self.device = config['device']
        self._config = config
        config['_pp_norm'] = self._norm
        self._eng = engine_for(config, self._norm)
        self._sd = None
        self._params = {}            # the six head tensors as device Parameters (parameters())
        self._uploaded = None        # their _version numbers at the last upload into the engine
        self.training = False
        self._trained = False        # the head has been stepped since load_state_dict
        self._scope = "head"         # train(scope=...): "head", "neck" (+ the three upsamplers), "block3" (+ block 3's five unit
                                     # convolutions), "stage3" (+ block 3's stride-2 convolution) or "rpn" (+ blocks 1 and 2 with
                                     # their stride-2 convolutions: the whole RPN) or "all" (+ the pillar feature net)
        self._pfn = {}               # the PFN's Conv1d weight and BatchNorm1d weight / bias as device Parameters
        self._pfn_stats = {}         # running_mean / running_var as device tensors (train(scope="all") moves them)
        self._pfn_nbt = None         # num_batches_tracked when the loaded dict carried it
        self._pfn_uploaded = None    # the _version numbers of those five at the last upload into the engine
        self._pfn_trained = False
        self._rpn = {}               # the ten convolutions of blocks 1 and 2 as device Parameters
        self._rpn_uploaded = None
        self._rpn_trained = False
        self._down = {}              # block 3's stride-2 weight as a device Parameter
        self._down_uploaded = None
        self._down_trained = False
        self._block = {}             # block 3's five weights as device Parameters
        self._block_uploaded = None
        self._block_trained = False
        self._neck = {}              # the three upsampler weights as device Parameters
        self._neck_uploaded = None
        self._neck_trained = False
        self.profile_stages = True  # the reference synchronises after every stage (:365-374)
        self.pfn_time, self.rpn_time, self.scatter_time, self.heads_time = 0.0, 0.0, 0.0, 0.0
        # like nn.Module construction, start from random initial weights
        self.load_state_dict(init_state_dict(0, norm=self._norm))

    # nn.Module-style surface used by train.py:196-205
    def to(self, device):
        return self

    def eval(self):
        return self.train(False)

    def train(self, mode=True, scope="head", grad_precision="fp32"):
        """Training mode: the six head parameters require grad and forward() accepts a batch of several frames.  scope="neck" also
        trains rpn.deconv{1,2,3}.0.weight, scope="block3" those and the five unit convolutions of block 3, scope="stage3" those and
        block 3's stride-2 convolution rpn.block3.0.weight (InstanceNorm backbone, fp32 mode); everything in front of them stays
        frozen: it has no backward.  scope="rpn" trains the whole RPN (RPN_KEYS: blocks 1 and 2 with their stride-2 convolutions as
        well); PFN and scatter stay frozen.  scope="all" trains the pillar feature net too (ALL_KEYS, what net.parameters() yields
        in the reference): the training-mode forward then normalises the PFN with batch statistics and moves the running ones, as the
        reference's net.train() does.  eval() / train(False) restores the inference behaviour, with the PFN's current parameters and
        running statistics folded into the engine.
        grad_precision ("fp32" | "bf16x3" | "bf16", kept as net.grad_precision, "fp32" again after eval()): the operand precision of
        the Resnet units' gradient products (pp_unit_backward_mp), in effect under the scopes that run them ("block3", "stage3", "rpn",
        "all") and inert under "head" and "neck".  The forward, the strided stages, the upsamplers, the head and the PFN stay fp32."""
        if grad_precision not in GRAD_PRECISIONS:
            raise ValueError(f"train: grad_precision must be 'fp32', 'bf16x3' or 'bf16', got {grad_precision!r}")
        if scope not in SCOPES:
            raise ValueError(f"train: scope must be 'head', 'neck', 'block3', 'stage3', 'rpn' or 'all', got {scope!r}")
        if mode and scope != "head" and (self._norm != "instance" or len(self._neck) != 3 or
                                         (scope in _BLOCK_SCOPES and len(self._block) != 5) or
                                         (scope in _STAGE_SCOPES and len(self._down) != 1) or
                                         (scope in _RPN_SCOPES and len(self._rpn) != len(_RPN_EXTRA_KEYS)) or
                                         (scope == "all" and (len(self._pfn) != 3 or len(self._pfn_stats) != 2))):
            raise RuntimeError(f"train(scope='{scope}'): the neck and block backward exist for the InstanceNorm backbone only")
        self.training = bool(mode)
        self._scope = scope if self.training else "head"
        self.grad_precision = grad_precision if self.training else "fp32"
        for p in self._params.values():
            p.requires_grad_(self.training)
        for p in self._neck.values():
            p.requires_grad_(self.training and self._scope in _NECK_SCOPES)
        for p in self._block.values():
            p.requires_grad_(self.training and self._scope in _BLOCK_SCOPES)
        for p in self._down.values():
            p.requires_grad_(self.training and self._scope in _STAGE_SCOPES)
        for p in self._rpn.values():
            p.requires_grad_(self.training and self._scope in _RPN_SCOPES)
        for p in self._pfn.values():
            p.requires_grad_(self.training and self._scope == "all")
        if not (self.training and self._scope == "all"):
            self._sync_pfn()  # whatever reads the engine's eval-mode PFN next (this object or framework.inference) sees the trained one
        return self

    def _trainable(self):
        if self._scope in _RPN_SCOPES:
            every = {**self._rpn, **self._down, **self._block, **self._neck, **self._params}
            if self._scope == "all":
                every.update(self._pfn)
                return {k: every[k] for k in ALL_KEYS if k in every}
            return {k: every[k] for k in RPN_KEYS if k in every}
        if self._scope == "stage3":
            return {**self._down, **self._block, **self._neck, **self._params}
        if self._scope == "block3":
            return {**self._block, **self._neck, **self._params}
        return {**self._neck, **self._params} if self._scope == "neck" else self._params

    def named_parameters(self):
        """The trainable tensors on the device: heads.conv_{cls,box,dir}.{weight,bias}, behind rpn.deconv{1,2,3}.0.weight under
        train(scope="neck"), behind BLOCK3_KEYS (unit order) as well under train(scope="block3"), and behind rpn.block3.0.weight
        under train(scope="stage3"); under train(scope="rpn") the 25 tensors of RPN_KEYS in the reference's state_dict order, under
        train(scope="all") the 28 of ALL_KEYS.  Everything before them is frozen."""
        return iter(self._trainable().items())

    def parameters(self):
        return iter(self._trainable().values())

    def zero_grad(self, set_to_none=True):
        for p in list(self._pfn.values()) + list(self._rpn.values()) + list(self._down.values()) + list(self._block.values()) + list(self._neck.values()) + list(self._params.values()):
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _sync_head(self):
        """An optimizer stepped (a parameter's _version moved since the last upload): rewrite the engine's packed head in place."""
        ver = tuple(p._version for p in self._params.values())
        if ver != self._uploaded:
            self._eng.update_head_weights(self._params)
            self._uploaded = ver

    def _neck_moved(self):
        return self._neck_uploaded is not None and tuple(p._version for p in self._neck.values()) != self._neck_uploaded

    def _block_moved(self):
        return self._block_uploaded is not None and tuple(p._version for p in self._block.values()) != self._block_uploaded

    def _down_moved(self):
        return self._down_uploaded is not None and tuple(p._version for p in self._down.values()) != self._down_uploaded

    def _rpn_moved(self):
        return self._rpn_uploaded is not None and tuple(p._version for p in self._rpn.values()) != self._rpn_uploaded

    def _pfn_versions(self):
        return tuple(t._version for t in list(self._pfn.values()) + list(self._pfn_stats.values()))

    def _pfn_moved(self):
        return self._pfn_uploaded is not None and self._pfn_versions() != self._pfn_uploaded

    def _sync_pfn(self):
        """The same for the pillar feature net, ahead of whatever runs the eval-mode PFN: a stepped parameter or moved running
        statistics are folded into the engine's transposed weight, scale and shift (pp_update_pfn_weights)."""
        if self._pfn_moved():
            self._pfn_trained = True
            self._eng.update_pfn_weights(*[self._pfn[k] for k in PFN_KEYS], *[self._pfn_stats[k] for k in PFN_STAT_KEYS])
            self._pfn_uploaded = self._pfn_versions()

    def _sync_neck(self):
        """The same for the three upsampler weights, block 3's five and its stride-2 weight, ahead of whatever runs the backbone; when
        a convolution of blocks 1 and 2 moved, all sixteen go up in one pp_update_rpn_weights."""
        if self._neck_moved():
            self._neck_trained = True
            self._eng.update_neck_weights(self._neck)
            self._neck_uploaded = tuple(p._version for p in self._neck.values())
        if self._rpn_moved():
            self._rpn_trained = True
            self._block_trained = self._block_trained or self._block_moved()
            self._down_trained = self._down_trained or self._down_moved()
            self._eng.update_rpn_weights({**self._rpn, **self._down, **self._block})
            self._rpn_uploaded = tuple(p._version for p in self._rpn.values())
            self._block_uploaded = tuple(p._version for p in self._block.values())
            self._down_uploaded = tuple(p._version for p in self._down.values())
        if self._block_moved():
            self._block_trained = True
            self._eng.update_block_weights(self._block)
            self._block_uploaded = tuple(p._version for p in self._block.values())
        if self._down_moved():
            self._down_trained = True
            self._eng.update_down_weight(2, self._down[STAGE3_KEY])
            self._down_uploaded = tuple(p._version for p in self._down.values())

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
        if self._trained or self._head_moved():
            self._uploaded = ()  # a change of mode packs the loaded weights again: the trained head is uploaded at the next heads()
        if self._neck_trained or self._neck_moved():
            self._neck_uploaded = ()  # and the trained upsamplers at the next backbone pass
        if self._block_trained or self._block_moved():
            self._block_uploaded = ()
        if self._down_trained or self._down_moved():
            self._down_uploaded = ()
        if self._rpn_trained or self._rpn_moved():
            self._rpn_uploaded = ()
        if self._pfn_trained or self._pfn_moved():
            self._pfn_uploaded = ()  # the commit folds the loaded PFN again: the trained one goes up before its next use
            if not (self.training and self._scope == "all"):
                self._sync_pfn()
        return self

    def _head_moved(self):
        return self._uploaded is not None and tuple(p._version for p in self._params.values()) != self._uploaded

    def state_dict(self):
        """The loaded tensors; the head's six, the three upsampler weights and all sixteen 3 x 3 convolutions of the RPN (blocks 1, 2
        and 3 with their stride-2 weights, RPN_CONV_KEYS) with their CURRENT values (after optimizer steps)."""
        sd = dict(self._sd)
        if self._pfn_moved() or self._pfn_trained:
            for k, t in list(self._pfn.items()) + list(self._pfn_stats.items()):
                sd[k] = t.detach().cpu().numpy().reshape(self._sd[k].shape)
            if self._pfn_nbt is not None:
                sd[PFN_NBT_KEY] = np.asarray(self._pfn_nbt, dtype=np.int64)
        if self._rpn_moved() or self._rpn_trained:
            for k, p in self._rpn.items():
                sd[k] = p.detach().cpu().numpy().reshape(self._sd[k].shape)
        if self._down_moved() or self._down_trained:
            for k, p in self._down.items():
                sd[k] = p.detach().cpu().numpy().reshape(self._sd[k].shape)
        if self._block_moved() or self._block_trained:
            for k, p in self._block.items():
                sd[k] = p.detach().cpu().numpy().reshape(self._sd[k].shape)
        if self._neck_moved() or self._neck_trained:
            for k, p in self._neck.items():
                sd[k] = p.detach().cpu().numpy().reshape(self._sd[k].shape)
        if self._head_moved() or self._trained:
            for k, p in self._params.items():
                sd[k] = p.detach().cpu().numpy().reshape(self._sd[k].shape)
        return sd

    def load_state_dict(self, sd, strict=True):
        self._sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in sd.items()}
        self._eng.load_state_dict(self._sd)
        self._params = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(self._sd[k], dtype=np.float32)).to(self._eng.device),
                                              requires_grad=self.training) for k in HEAD_KEYS if k in self._sd}
        self._uploaded = tuple(p._version for p in self._params.values())
        self._trained = False
        neck = self.training and self._scope in _NECK_SCOPES
        block = self.training and self._scope in _BLOCK_SCOPES
        self._rpn = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(self._sd[k], dtype=np.float32)).to(self._eng.device),
                                           requires_grad=self.training and self._scope in _RPN_SCOPES) for k in _RPN_EXTRA_KEYS if k in self._sd}
        self._rpn_uploaded = tuple(p._version for p in self._rpn.values())
        self._rpn_trained = False
        self._down = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(self._sd[k], dtype=np.float32)).to(self._eng.device),
                                            requires_grad=self.training and self._scope in _STAGE_SCOPES) for k in (STAGE3_KEY,) if k in self._sd}
        self._down_uploaded = tuple(p._version for p in self._down.values())
        self._down_trained = False
        self._block = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(self._sd[k], dtype=np.float32)).to(self._eng.device),
                                             requires_grad=block) for k in BLOCK3_KEYS if k in self._sd}
        self._block_uploaded = tuple(p._version for p in self._block.values())
        self._block_trained = False
        self._neck = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(self._sd[k], dtype=np.float32)).to(self._eng.device),
                                            requires_grad=neck) for k in NECK_KEYS if k in self._sd}
        self._neck_uploaded = tuple(p._version for p in self._neck.values())
        self._neck_trained = False
        dev_of = lambda k: torch.from_numpy(np.ascontiguousarray(self._sd[k], dtype=np.float32)).to(self._eng.device)  # noqa: E731
        self._pfn = {k: torch.nn.Parameter(dev_of(k), requires_grad=self.training and self._scope == "all") for k in PFN_KEYS if k in self._sd}
        self._pfn_stats = {k: dev_of(k) for k in PFN_STAT_KEYS if k in self._sd}
        self._pfn_nbt = int(np.asarray(self._sd[PFN_NBT_KEY])) if PFN_NBT_KEY in self._sd else None
        self._pfn_uploaded = self._pfn_versions()
        self._pfn_trained = False
        return self

    def _sync(self):
        if self.profile_stages:
            torch.cuda.synchronize()
        return time.time()

    def _pfn_training(self):
        return self.training and self._scope == "all"

    def pfn_train(self, frames):
        """PointNet in train mode and the scatter on a batch: frames = [(voxels [n,T,4], coors [n,3], num_points_per_voxel [n]), ...],
        at most max_batch of them -> canvases [nb,64,gx,gy].  BatchNorm1d normalises with the statistics of the pillars of all frames
        together and the running statistics move (momentum 0.1, unbiased variance), whether or not grad is enabled.  Differentiable
        with respect to PFN_KEYS when they require grad (train(scope="all")).  Needs the fp32 precision mode."""
        eng = self._eng
        if not 1 <= len(frames) <= eng.max_batch:
            raise ValueError(f"pfn_train: {len(frames)} frames in the batch, max_batch is {eng.max_batch}")
        if len(self._pfn) != 3 or len(self._pfn_stats) != 2:
            raise RuntimeError("pfn_train: the state_dict holds no pillar feature net")
        if eng.effective_precision() != "fp32":
            raise RuntimeError(f"PFN training needs the fp32 precision mode: the network runs '{eng.effective_precision()}' "
                               "(the backward of the RPN behind it is fp32); call float()")
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

    def _neck_grad(self):
        return self.training and self._scope in _NECK_SCOPES and torch.is_grad_enabled() and \
            any(p.requires_grad for p in list(self._neck.values()) + list(self._block.values()) + list(self._down.values()) +
                list(self._rpn.values()))

    def rpn_train(self, x):
        """RPN.forward on canvases x [B,64,gx,gy], 1 <= B <= max_batch, one backbone pass per frame; same values as rpn() bit for
        bit.  Differentiable with respect to the three upsampler weights when they require grad (train(scope="neck")) and to block
        3's five unit weights (train(scope="block3")) and its stride-2 weight (train(scope="stage3")); under train(scope="rpn") to all
        sixteen convolutions, and then also to x itself when it requires grad (the level-0 dx: where the PFN backward starts).
        Gradients are fp32 and need the fp32 precision mode."""
        eng = self._eng
        gx, gy = int(eng.grid_size[0]), int(eng.grid_size[1])
        if not isinstance(x, torch.Tensor) or x.numel() == 0 or x.numel() % (64 * gx * gy):
            raise ValueError(f"rpn_train: expected canvases [B,64,{gx},{gy}]")
        x = x.contiguous().reshape(-1, 64, gx, gy)  # a view: a canvas that requires grad stays in the graph
        if not 1 <= x.shape[0] <= eng.max_batch:
            raise ValueError(f"rpn_train: {x.shape[0]} frames in the batch, max_batch is {eng.max_batch}")
        self._sync_neck()
        block = any(p.requires_grad for p in self._block.values())
        stage = any(p.requires_grad for p in self._down.values())
        whole = any(p.requires_grad for p in self._rpn.values())
        if not (torch.is_grad_enabled() and (whole or stage or block or any(p.requires_grad for p in self._neck.values()))):
            return torch.cat([eng.backbone(c) for c in x])
        if eng.effective_precision() != "fp32":
            raise RuntimeError(f"neck training needs the fp32 precision mode: the network runs '{eng.effective_precision()}' "
                               "(gradients are fp32 and the packed 16-bit upsampler weights cannot be updated in place); call float()")
        if whole:
            every = {**self._rpn, **self._down, **self._block}
            return _RpnFunction.apply(eng, self.grad_precision, x, *[every[k] for k in RPN_CONV_KEYS], *[self._neck[k] for k in NECK_KEYS])
        if stage:
            return _StageFunction.apply(eng, self.grad_precision, list(x), self._down[STAGE3_KEY], *[self._block[k] for k in BLOCK3_KEYS],
                                        *[self._neck[k] for k in NECK_KEYS])
        if block:
            return _BlockFunction.apply(eng, self.grad_precision, list(x), *[self._block[k] for k in BLOCK3_KEYS], *[self._neck[k] for k in NECK_KEYS])
        return _NeckFunction.apply(eng, list(x), *[self._neck[k] for k in NECK_KEYS])

    def heads(self, x):
        """SharedHead.forward on x [B,320,H,W], 1 <= B <= max_batch.  Differentiable with respect to x and the head parameters when
        one of them requires grad (train() for the parameters); gradients are fp32 and need the fp32 precision mode."""
        x = x.contiguous()
        params = list(self._params.values())
        if self._head_moved():
            self._trained = True
            self._sync_head()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            if self._eng.effective_precision() != "fp32":
                raise RuntimeError(f"head training needs the fp32 precision mode: the network runs '{self._eng.effective_precision()}' "
                                   "(gradients are fp32 and the packed 16-bit head weights cannot be updated in place); call float()")
            if x.dim() != 4:
                x = x.reshape(-1, 320, self._eng.H, self._eng.W)
            cls, box, dr = _HeadFunction.apply(self._eng, x, *params)
        else:
            cls, box, dr = self._eng.head(x)
        return {"cls_preds": cls, "box_preds": box, "dir_preds": dr}
