"""EfficientNet-B2/B5 image encoder on hand-written gfx950 kernels.

Mirrors the public surface of the reference module of the same name (class names ``EfficientNet`` /
``MBConvBlock``, ``from_name`` / ``from_pretrained``, ``extract_features``, ``forward`` incl. the
``{"image": x}`` dict form, and -- crucially -- the ``state_dict`` key layout ``_conv_stem.weight``,
``_bn0.*``, ``_blocks.{i}._expand_conv.weight`` ...; reference: model/modules/efficientnet_custom.py and
efficient_net_custom_utils.py), but nothing below is a translation of it:

  * activations live in HBM as NHWC bf16 ``[n*h*w, c]``; every 1x1 conv is one MFMA GEMM over pixels
  * training-mode BatchNorm statistics come out of the producing kernel's epilogue, the BN+SiLU of the
    expand conv is applied while the depthwise kernel stages its LDS halo tile, the BN+SiLU+SE-gate of the
    depthwise output is applied while the project GEMM stages its A operand: the activated expanded
    tensors never exist in HBM, forward or backward (they are recomputed from the saved conv outputs)
  * one ``torch.autograd.Function`` per stem / MBConv block / head, with a hand-derived backward

Parameters are ordinary fp32 ``nn.Parameter``s held in ``nn.Conv2d`` / ``nn.BatchNorm2d`` containers (their
``forward`` is never called) so optimizers, DDP and ``load_state_dict(strict=True)`` of reference
checkpoints work unchanged.
"""
import math
from collections import namedtuple
from typing import List, Optional

import os

import torch
from torch import nn

from .... import ops

BN_MOMENTUM = 0.01      # 1 - batch_norm_momentum 0.99 [ref: efficientnet_custom.py:53, efficient_net_custom_utils.py:520]
BN_EPS = 1e-3           # [ref: efficient_net_custom_utils.py:521]

VALID_MODELS = tuple(f"efficientnet-b{i}" for i in range(9)) + ("efficientnet-l2",)

# (width, depth, nominal resolution, dropout) [ref: efficient_net_custom_utils.py:457-479]
_COEFFS = {
    "efficientnet-b0": (1.0, 1.0, 224, 0.2), "efficientnet-b1": (1.0, 1.1, 240, 0.2),
    "efficientnet-b2": (1.1, 1.2, 260, 0.3), "efficientnet-b3": (1.2, 1.4, 300, 0.3),
    "efficientnet-b4": (1.4, 1.8, 380, 0.4), "efficientnet-b5": (1.6, 2.2, 456, 0.4),
    "efficientnet-b6": (1.8, 2.6, 528, 0.5), "efficientnet-b7": (2.0, 3.1, 600, 0.5),
    "efficientnet-b8": (2.2, 3.6, 672, 0.5), "efficientnet-l2": (4.3, 5.3, 800, 0.5),
}
# repeats, kernel, stride, expand, in, out  (se_ratio 0.25 everywhere) [ref: efficient_net_custom_utils.py:502-510]
_STAGES = ((1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80),
           (3, 5, 1, 6, 80, 112), (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320))

GlobalParams = namedtuple("GlobalParams", ["width_coefficient", "depth_coefficient", "image_size", "dropout_rate",
                                           "num_classes", "batch_norm_momentum", "batch_norm_epsilon",
                                           "drop_connect_rate", "depth_divisor", "min_depth", "include_top"])
BlockArgs = namedtuple("BlockArgs", ["num_repeat", "kernel_size", "stride", "expand_ratio", "input_filters",
                                     "output_filters", "se_ratio", "id_skip"])


def _scaled_width(filters, gp):
    if not gp.width_coefficient:
        return filters
    f = filters * gp.width_coefficient
    div = gp.depth_divisor
    out = max(gp.min_depth or div, int(f + div / 2) // div * div)
    return int(out + div) if out < 0.9 * f else int(out)


def _scaled_depth(repeats, gp):
    return int(math.ceil(gp.depth_coefficient * repeats)) if gp.depth_coefficient else repeats


def _static_pad(size_hw, k, s):
    """(left, right, top, bottom) frozen for the NOMINAL feature-map size [ref: efficient_net_custom_utils.py:262-272]."""
    ih, iw = size_hw
    ph = max((math.ceil(ih / s) - 1) * s + k - ih, 0)
    pw = max((math.ceil(iw / s) - 1) * s + k - iw, 0)
    return (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)


def _down(size_hw, s):
    return (int(math.ceil(size_hw[0] / s)), int(math.ceil(size_hw[1] / s)))


def _out_extent(i, lo, hi, k, s):
    return (i + lo + hi - k) // s + 1


class _Seeds:
    """Counter-based RNG bookkeeping: every stochastic site gets (seed, stream id); re-running a forward with
    the same seed regenerates identical dropout / drop-connect masks (used by backward)."""
    base = 0x5EED

    def __init__(self):
        self.seed = _Seeds.base
        self.calls = 0

    def next(self):
        self.calls += 1
        return self.seed * 1000003 + self.calls


# ================================================================================================
#                                      autograd functions
# ================================================================================================
class StatTape:
    """BatchNorm batch statistics and squeeze-excite pooled means of ONE micro-batch's forward, in call order.
    The micro-batched step forwards most micro-batches twice with identical inputs, weights and mask seeds (first
    without a graph for the embeddings, then with a graph for the backward): the second forward computes exactly the
    same statistics again.  A tape RECORDS them in the first forward (a few MB) and the re-forward REPLAYS them: no
    statistics epilogues, no finalize launches, no squeeze pass over the depthwise output of the early stages --
    same values, bit for bit (tested), ~13 ms of a ~90 ms re-forward at 32 x 1520x912."""
    __slots__ = ("mode", "items", "pos")

    def __init__(self):
        self.mode, self.items, self.pos = "record", [], 0

    def replay(self):
        self.mode, self.pos = "replay", 0
        return self

    def put(self, v):
        self.items.append(v)
        return v

    def get(self):
        v = self.items[self.pos]
        self.pos += 1
        return v


class _BNDefer:
    """Running-statistic updates of an encoder call that runs on a SIDE stream beside another call of the same encoder
    (model/clip.py: the second image view).  Both calls update the same buffers -- r <- (1 - m) r + m s, view 1 first
    [ref: clip.py:83,108 two sequential encode_image calls] -- so the side call must not touch them: its finalize launches
    update zero-filled scratch slices instead (result: m s), and ``apply`` folds them in after the join, on the main
    stream, behind view 1's updates: r <- (1 - m) r + (m s), the same two-term form (one rounding apart from the fused
    kernel expression)."""

    def __init__(self, enc):
        offs, tot = {}, 0
        for bn in enc._bn_layers:
            offs[id(bn)] = tot
            tot += bn.num_features
        self.offs, self.total = offs, tot
        self.flat = torch.zeros(2 * tot, dtype=torch.float32, device=enc._ones_b.device)
        self.used = []

    def scratch(self, bn):
        o, c = self.offs[id(bn)], bn.num_features
        self.used.append(bn)
        return self.flat[o:o + c], self.flat[self.total + o:self.total + o + c]

    @torch.no_grad()
    def apply(self):
        if not self.used:
            return
        if self.flat.is_cuda:
            self.flat.record_stream(torch.cuda.current_stream(self.flat.device))
        dst = [bn.running_mean for bn in self.used] + [bn.running_var for bn in self.used]
        src = [self.flat[self.offs[id(bn)]:self.offs[id(bn)] + bn.num_features] for bn in self.used] + \
              [self.flat[self.total + self.offs[id(bn)]:self.total + self.offs[id(bn)] + bn.num_features] for bn in self.used]
        torch._foreach_mul_(dst, 1.0 - BN_MOMENTUM)
        torch._foreach_add_(dst, src)
        self.used = []


class _Call:
    """Everything ONE chain of one encoder forward knows beyond its tensors; made by ``EfficientNet._new_call`` and handed
    to the stem, every block and the head like ``link`` is.  Nothing of it outlives the call, so an exception leaves nothing behind.
      tape            the StatTape this forward records on / replays from, or None (both chains of forward_pair share one)
      update_running  do the finalize launches update the running statistics (and the batch counters)?
      defer           the _BNDefer whose scratch slices take those updates instead of the buffers (side chain), or None
      counters        collects the num_batches_tracked tensors: the encoder bumps them with ONE launch when the call ends
                      (None -- a block called on its own -- bumps each at once)
      seed            of the call's drop-connect / dropout masks
      head            (e, st, n, h, w, cout) of the head conv, left by _HeadFn for the feature-map forms of forward"""
    __slots__ = ("tape", "update_running", "defer", "counters", "seed", "head")

    def __init__(self, tape=None, update_running=True, defer=None, counters=None, seed=None):
        self.tape, self.update_running, self.defer, self.counters, self.seed, self.head = tape, update_running, defer, counters, seed, None

    @property
    def replaying(self):
        return self.tape is not None and self.tape.mode == "replay"

    def taped(self, active, fn):
        """fn() -- or, at a site whose values travel on the tape (``active``), its recorded value in a replay; recorded otherwise"""
        if not active or self.tape is None:
            return fn()
        return self.tape.get() if self.tape.mode == "replay" else self.tape.put(fn())


def _bn_stats(call, partials, count, bn: nn.BatchNorm2d, training: bool):
    if not training:
        return ops.bn_eval_coeffs(bn.weight, bn.bias, bn.running_mean, bn.running_var, BN_EPS)

    def finalize():
        upd = call.update_running
        rm, rv = call.defer.scratch(bn) if upd and call.defer is not None else (bn.running_mean, bn.running_var)
        st = ops.bn_finalize(partials, count, bn.weight, bn.bias, rm, rv, BN_MOMENTUM, BN_EPS, upd)
        if upd and call.counters is not None:
            call.counters.append(bn.num_batches_tracked)
        elif upd:
            bn.num_batches_tracked += 1
        return st
    return call.taped(True, finalize)


def _conv_stats(call, fn, training, *a, stats=True, **kw):
    """run a producer that can leave BatchNorm statistics partials (stats=True -> (y, partials)); a replaying tape needs none,
    nor does a backward that rebuilds y (stats=False, no call)"""
    if not stats or (training and call.replaying):
        return fn(*a, **kw), None
    return fn(*a, stats=True, **kw)


def _no_fp8_frozen(mod):
    if mod.fp8:
        raise NotImplementedError("backward through BatchNorm on running statistics (eval mode / freeze_bn) is not implemented "
                                  "for the fp8 forward (set_fp8)")


# expanded-tensor bytes per call from which the BatchNorm0 backward is folded into the expand conv's gradient GEMMs
# (ops.bn_fold_expand_bwd) instead of running the apply pass; tests set it to 0 to exercise the folded path at small sizes
LINK_STEM = os.environ.get("MC_LINK_STEM", "1") != "0"                  # stem bn0 + swish inside block 0's depthwise kernels (_StemLink)
STEM_DIRECT = os.environ.get("MC_STEM_DIRECT", "1") != "0"              # stem conv and its weight gradient straight from a channels-last image (ops.stem_conv_*), no patch matrix
STEM_FOLD_BN0 = os.environ.get("MC_STEM_FOLD_BN0", "1") != "0"          # linked direct stem: the BatchNorm0 backward apply inside the weight-gradient launch
FUSE_DW_BWD = os.environ.get("MC_FUSE_DW_BWD", "1") != "0"              # stride-1 3x3 depthwise backward as one launch (ops.dwconv_bwd_fused)
FUSE_PROJ_DGRAD = os.environ.get("MC_FUSE_PROJ_DGRAD", "1") != "0"        # projection data gradient with the SE / BatchNorm1 backward in its epilogue (ops.proj_dgrad_*)
BN_FOLD_MIN_BYTES = int(os.environ.get("MC_BN_FOLD_MIN_BYTES", 250_000_000))
BN_FOLD_S2_MIN_BYTES = int(os.environ.get("MC_BN_FOLD_S2_MIN_BYTES", 0))
# round 6: blocks whose expand conv runs INSIDE the depthwise forward launch (ops.mbconv_xdw_fwd) wherever the expanded tensor
# is not stored for a backward (graph-less forwards, recompute modes >= 1, eval): input widths up to this many channels
# (measured per block shape, scripts/xdw_ab.py: the launch wins up to cin = 64; at cin = 128 it only breaks even)
XDW_MAX_CIN = int(os.environ.get("MC_XDW_MAX_CIN", 64))
# recompute mode 3 drops the depthwise output of the stride-1 3x3 blocks up to this many expanded channels (developer sweep)
MODE3_MAX_CEXP = int(os.environ.get("MC_MODE3_MAX_CEXP", 1 << 30))


class _StemFn(torch.autograd.Function):
    """_conv_stem (3x3 s2, static pad) + _bn0 + swish [ref: efficientnet_custom.py:273]."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, mod, link=None, call=None):
        """call: the ``_Call`` of the encoder forward this is part of (None: the stem on its own).
        link (round 5): a ``_StemLink`` -- the stem then returns its RAW conv output e and block 0 (no expand conv: its
        depthwise stage reads the stem's output directly) applies bn0 + swish while it stages its LDS tiles, exactly like every
        other block does with its own expand conv; the activated 48-channel 760x456 tensor (the widest map of the network) is
        never written or read.  The backward mirrors it: block 0's depthwise data gradient finishes the bn0 + swish backward in
        its epilogue and leaves the BatchNorm reductions in the link."""
        n, _, h, wd = x.shape
        l, r, t, b = mod.stem_pad
        _, oh, ow = mod.stem_geo(n, h, wd)
        c0 = w.shape[0]
        wb = ops.stem_weight_prep(w)
        training, call = mod.batch_stats, call if call is not None else _Call()
        ctx.direct = STEM_DIRECT and ops.stem_direct_ok(x, c0, l, t)
        if ctx.direct:
            e, part = _conv_stats(call, ops.stem_conv_fwd, training, x, wb, l, t, oh, ow)
        else:                                                      # any other layout: through the patch matrix
            e, part = _conv_stats(call, ops.linear_fwd, training, ops.stem_im2col(x, l, t, oh, ow), wb)
        st = _bn_stats(call, part, n * oh * ow, mod._bn0, training)
        ctx.mod, ctx.st, ctx.geo, ctx.frozen = mod, st, (n, h, wd, oh, ow, c0), not training
        ctx.raw = (x.mean, x.std) if isinstance(x, ops.RawImages) else None
        ctx.save_for_backward(x.data if ctx.raw else x, e)
        ctx.link = link
        if link is not None:
            link.st, link.part = st, None
            return e.detach()               # (a new tensor object: autograd must not return a saved input as the output)
        return ops.bnact_apply(e, n, oh * ow, c0, st.scale, st.shift, 1)

    @staticmethod
    def backward(ctx, dy):
        x, e = ctx.saved_tensors
        if ctx.raw:
            x = ops.RawImages(x, *ctx.raw)
        n, h, wd, oh, ow, c0 = ctx.geo
        mod = ctx.mod
        link = ctx.link
        fold = None
        if ctx.frozen:
            _no_fp8_frozen(mod)
        if ctx.frozen and link is not None:
            # frozen bn0: de = scale0 * dZ0 is never formed -- the conv's weight gradient is taken from dZ0 and row-scaled
            de = dy.contiguous()
            _, dgamma, dbeta = ops.bn_bwd_coefs(link.part, 0, ctx.st, mod._bn0.weight, frozen=True)
            link.part = None
        elif ctx.frozen:
            de, dgamma, dbeta = ops.bnact_bwd(e, n, oh * ow, c0, ctx.st, mod._bn0.weight, 1, g=dy.contiguous(), frozen=True)
        elif link is not None:
            # dy is already dZ0 = dL/d bn0(e) (block 0's data-gradient epilogue), link.part its BatchNorm-backward reductions
            if ctx.direct and STEM_FOLD_BN0:
                # the stem has no data gradient: de = A*dZ0 + B*e + C is only the weight gradient's operand, formed inside that launch
                de = dy.contiguous()
                fold, dgamma, dbeta = ops.bn_bwd_coefs(link.part, n * oh * ow, ctx.st, mod._bn0.weight)
            else:
                de, dgamma, dbeta = ops.bnact_bwd(e, n, oh * ow, c0, ctx.st, mod._bn0.weight, 0, g=dy.contiguous(), partials=link.part)
            link.part = None
        else:
            de, dgamma, dbeta = ops.bnact_bwd(e, n, oh * ow, c0, ctx.st, mod._bn0.weight, 1, g=dy.contiguous())
        l, r, t, b = mod.stem_pad
        if ctx.direct:
            dw = ops.stem_conv_wgrad(de, x, l, t, oh, ow, bn=(e, fold) if fold is not None else None)     # [c0, 32]
        else:
            patches = ops.stem_im2col(x, l, t, oh, ow)             # recomputed, not stored
            dw = ops.linear_wgrad(de, patches)
        if ctx.frozen and link is not None:
            dw = ops.rowscale_f32_(dw, ctx.st.scale)
        gw, gg, gb = ops.deliver_param_grads((mod._conv_stem.weight, mod._bn0.weight, mod._bn0.bias),
                                             (dw[:, :27].reshape(c0, 3, 3, 3), dgamma, dbeta))
        return None, gw, gg, gb, None, None, None        # (autograd drops the Nones of trailing arguments that were not passed)


class _StemLink:
    """hand-over between the stem and block 0 when the stem's bn0 + swish lives in block 0's depthwise kernels: the stem's
    BatchNorm coefficients (forward) and the BatchNorm-backward reductions block 0's data gradient leaves (backward)"""
    __slots__ = ("st", "part")

    def __init__(self):
        self.st, self.part = None, None


def _expand_conv(call, pl, x, we, stats=True):
    """_expand_conv of one block: (e [rows, cexp] bf16, BatchNorm0 column-statistic partials) (deterministic: the backward's
    rebuild, stats=False and no call, reproduces the forward's tensor bit for bit)."""
    if pl.fp8_expand:
        # config #5: fp8 (e4m3, per-tensor scale) activations and weights on the fp8 MFMA; BatchNorm statistics
        # and everything downstream stay on the bf16 / fp32 path; backward uses the bf16 tensors (straight-through)
        return ops.linear_fwd_fp8(x, we, stats=True)
    return _conv_stats(call, ops.linear_fwd, pl.batch_stats, x, we, stats=stats)


def _depthwise(call, blk, pl, x, e, we, wkkc, pro0, stats=True):
    """depthwise stage of one block: (d [n*oh*ow, cexp] bf16, BatchNorm1 partials) from the block input x (fused expand +
    depthwise launch: from the UNROUNDED expand output) or from e / the linked stem output x (pro0 = the BatchNorm0 + swish
    prologue).  The backward rebuilds d through this very function (stats=False): same launch, bit for bit."""
    if pl.xdw:
        return _conv_stats(call, ops.mbconv_xdw_fwd, pl.batch_stats, x, we, pro0, wkkc, *pl.dw, stats=stats)
    return _conv_stats(call, ops.dwconv_fwd, pl.batch_stats, e if blk.args.expand != 1 else x, wkkc, *pl.dw, stats=stats, pro=pro0)


def _project_conv(call, pl, d, act1, st1, gate, wp, stats=True):
    """_project_conv of one block: (p [n*oh*ow, cout] bf16, BatchNorm2 partials)"""
    ohw = pl.oh * pl.ow
    if pl.fp8_project:
        wg = ops.gate_weights(wp, gate)                           # [n, cout, cexp] bf16: the SE gate folded into the weights
        return ops.linear_fwd_fp8(act1, wg, stats=True, batch_w=(pl.n, ohw))
    # stored activation: only the SE gate is applied; else BN1 + SiLU + gate while the GEMM stages its A operand
    src, pro = (act1, (None, None, gate, ohw)) if pl.keep_act else (d, (st1.scale, st1.shift, gate, ohw))
    return _conv_stats(call, ops.linear_fwd, pl.batch_stats, src, wp, stats=stats, pro=pro)


class _MBConvFn(torch.autograd.Function):
    """One MBConvBlock, forward + hand-derived backward [ref: efficientnet_custom.py:91-132].  Every path choice of the pair is
    made once, by ``MBConvBlock.plan``, when the forward runs; the backward reads the plan stored with the graph."""

    @staticmethod
    def forward(ctx, x, rowscale, blk, n, h, w, recording, link, call, *params):
        a = blk.args
        pl = blk.plan(n, h, w, recording)
        # bstat: BatchNorm on batch statistics (statistics epilogues, finalize launches, their tape entries); training: the module's
        # mode -- the stochastic pieces and the tape entries of the squeeze-excite values (frozen BatchNorm: bstat off, training on)
        training, bstat, ohw = pl.training, pl.batch_stats, pl.oh * pl.ow
        wkkc = blk.w_taps()
        e = we = st0 = gram = None
        if a.expand != 1:
            we = blk.w_expand()
            if pl.xdw:
                # e never exists in HBM: BatchNorm0's batch statistics come from the Gram matrix of the block input (one pass
                # over x, 6 x narrower than e), from the statistics tape of a re-forward, or from the running statistics (eval).
                # x^T x and colsum(x) of the Gram statistics pass are what the folded BatchNorm0 backward of this block needs
                # again: they stay in the graph (a few KB) and travel on the statistics tape to the re-forward's backward
                part0 = None

                def gram_pass():
                    nonlocal part0
                    part0, xtx = ops.bn_gram_partials(x, we, n * h * w)
                    return xtx
                gram = call.taped(True, gram_pass) if bstat else None
            else:
                e, part0 = _expand_conv(call, pl, x, we)
            st0 = _bn_stats(call, part0, n * h * w, blk._bn0, bstat)
            pro0 = (st0.scale, st0.shift)
        else:
            # block 0 behind a linked stem: x is the stem's RAW conv output, its bn0 + swish is this block's prologue
            pro0 = (link.st.scale, link.st.shift) if link is not None else None
        d, part1 = _depthwise(call, blk, pl, x, e, we, wkkc, pro0)
        st1 = _bn_stats(call, part1, n * ohw, blk._bn1, bstat)
        # Late stages (project conv on the tiled GEMM): the squeeze pass also stores A = silu(bn1(d)); the project GEMM
        # and its weight gradient then apply only the SE gate instead of re-evaluating BN+SiLU per output tile.
        # (that pass runs in a replay too: act1 is needed; in the early stages the squeeze pass only produces the taped means)
        if pl.keep_act:
            pooled, act1 = ops.bnact_pool(d, n, ohw, a.cexp, st1.scale, st1.shift, 1, keep_act=True)
        else:
            pooled, act1 = call.taped(training, lambda: ops.bnact_pool(d, n, ohw, a.cexp, st1.scale, st1.shift, 1)), None
        # (every block: a replay saves the squeeze-excite MLP's two launches)
        gate = call.taped(training, lambda: ops.se_fwd(pooled, blk._se_reduce.weight.view(a.cse, a.cexp), blk._se_reduce.bias,
                                                       blk._se_expand.weight.view(a.cexp, a.cse), blk._se_expand.bias))
        wp = blk.w_project()
        p, part2 = _project_conv(call, pl, d, act1, st1, gate, wp)
        st2 = _bn_stats(call, part2, n * ohw, blk._bn2, bstat)
        y = ops.bnact_apply(p, n, ohw, a.cout, st2.scale, st2.shift, 0,
                            rowscale=rowscale if a.skip else None, res=x if a.skip else None)
        # what the plan does not store (recompute modes, see EfficientNet.set_recompute) the backward rebuilds from the block
        # input x and the saved BatchNorm coefficients; efree is repeated beside the tensors for whoever audits a graph node
        ctx.blk, ctx.plan, ctx.saved = blk, pl, dict(
            x=x, e=e if pl.store_e else None, d=d if pl.store_d else None, act1=act1 if pl.store_d else None,
            p=p if pl.store_p else None, we=we, wkkc=wkkc, wp=wp, pro0=pro0, link=link, st0=st0, st1=st1, st2=st2, gram=gram,
            pooled=pooled, gate=gate, efree=pl.efree, rowscale=rowscale if a.skip else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        blk, pl, sv = ctx.blk, ctx.plan, ctx.saved
        a = blk.args
        n, h, w, oh, ow = pl.n, pl.h, pl.w, pl.oh, pl.ow
        hw, ohw = h * w, oh * ow
        k, s, l, t = a.k, a.s, a.pad[0], a.pad[2]
        dy = dy.contiguous()
        x, e, d, p, act1, link, pro0 = sv["x"], sv["e"], sv["d"], sv["p"], sv["act1"], sv["link"], sv["pro0"]
        st0, st1, st2, gate, pooled = sv["st0"], sv["st1"], sv["st2"], sv["gate"], sv["pooled"]
        # frozen BatchNorm (running statistics): dx = scale*dz at every site, the reductions only feed dgamma / dbeta
        frozen = not pl.batch_stats
        if frozen:
            _no_fp8_frozen(blk)

        def expand_bwd(g, w_t):
            """(dx, dWe) of the expand conv from the gradient g of its output; w_t: the [cin, cexp] weight image of the data gradient"""
            if pl.xbwd:                                      # one pass over g for both gradients (round 5)
                return ops.xbwd_rows(g, x, w_t, residual=dy if a.skip else None)
            return ops.linear_dgrad(g, sv["we"], residual=dy if a.skip else None, w_t=w_t), ops.linear_wgrad(g, x)
        if a.expand != 1 and e is None and not (pl.efree or pl.efree_s2):     # (recompute modes: same kernels, statistics epilogues off)
            e = _expand_conv(None, pl, x, sv["we"], stats=False)[0]
        if d is None:
            d = _depthwise(None, blk, pl, x, e, sv["we"], sv["wkkc"], pro0, stats=False)[0]
            if pl.keep_act:
                act1 = ops.bnact_pool(d, n, ohw, a.cexp, st1.scale, st1.shift, 1, keep_act=True)[1]
        if p is None:                                        # mode 4: the projection conv again, from the rebuilt d
            p = _project_conv(None, pl, d, act1, st1, gate, sv["wp"], stats=False)[0]
        # y = bn2(p) * rowscale + x
        dp, dg2, db2 = ops.bnact_bwd(p, n, ohw, a.cout, st2, blk._bn2.weight, 0, g=dy, rowscale=sv["rowscale"], frozen=frozen)
        # project 1x1: p = A1 . wp^T, A1 = silu(bn1(d)) * gate   (A1 is recomputed inside the wgrad GEMM)
        wp_t = blk.w_project(transposed=True)                # [cexp, cout]
        # Early stages (row-streaming shapes, whole 16-row groups per image): dA1 = dp . wp never goes to memory -- the
        # projection's data-gradient GEMM runs TWICE with an elementwise epilogue over d, first for the squeeze-excite /
        # BatchNorm1 sums, then (once the SE backward has produced d loss / d pooled) for the BatchNorm1 + swish backward
        # itself: 1 + 2 passes over the depthwise-site tensor instead of 1 (dgrad) + 2 (sums) + 3 (apply)
        da1 = None if pl.fuse_proj_dgrad else ops.linear_dgrad(dp, sv["wp"], w_t=wp_t)
        if act1 is not None:
            dwp = ops.linear_wgrad(dp, act1, pro=(None, None, gate, ohw))
            del act1
        else:
            dwp = ops.linear_wgrad(dp, d, pro=(st1.scale, st1.shift, gate, ohw))
        # squeeze-excite
        # ONE pass over (d, dA1) yields d loss / d gate AND the ingredients of the bn1-backward reductions
        sums = ops.proj_dgrad_se_sums(dp, wp_t, d, st1, n, ohw) if pl.fuse_proj_dgrad else ops.bnact_se_sums(d, da1, n, ohw, a.cexp, st1, 1)
        dpooled, dw1, db1, dw2, dbse2 = ops.se_bwd(pooled, gate, sums[0], blk._se_reduce.weight.view(a.cse, a.cexp),
                                                   blk._se_reduce.bias, blk._se_expand.weight.view(a.cexp, a.cse),
                                                   blk._se_expand.bias)
        # bn1 + swish: upstream of swish output = dA1 * gate + dpooled / (oh*ow)
        part1 = ops.bn_partials_from_se_sums(sums, gate, dpooled, 1.0 / ohw)
        if pl.fuse_proj_dgrad:
            coef1, dg1, db1n = ops.bn_bwd_coefs(part1, n * ohw, st1, blk._bn1.weight, frozen=frozen)
            dd = ops.proj_dgrad_bn_apply(dp, wp_t, d, st1, coef1, gate, dpooled, 1.0 / ohw, ohw)
        else:
            dd, dg1, db1n = ops.bnact_bwd(d, n, ohw, a.cexp, st1, blk._bn1.weight, 1, g=da1, mul=gate, add=dpooled,
                                          add_scale=1.0 / ohw, partials=part1, frozen=frozen)
        del da1
        # depthwise
        del d
        dw_in = e if a.expand != 1 else x
        wflip = blk.w_taps(flipped=True) if s == 1 else None   # 180 degree rotation
        # round 5: stride-1 3x3 blocks run the WHOLE depthwise backward as one launch (conv_lane.hip MODE 3): data gradient with
        # the bn0 + swish epilogue AND the weight gradient from one staging of (dd, e) -- 3 passes over the expanded tensor
        # instead of 5; where that launch is not preferred: weight gradient + data gradient as two launches.  fused_dw5: the same
        # launch for the stride-1 5x5 blocks (12-wave instances), asked for through predicates of its own
        if not (pl.fused_dw or pl.fused_dw5 or pl.efree_s2):
            dwdw = ops.dwconv_bwd_weight(dw_in, dd, *pl.dw, pro=pro0)
        grads = {}
        if a.expand != 1:
            # the data-gradient kernel finishes the bn0 + swish backward in its epilogue -- it reads e at the output
            # position, writes dZ0 = dA0 * silu'(bn0(e)) and leaves the BatchNorm-backward reductions behind, so the
            # separate reduce pass over (e, dA0) is gone and the apply pass is a plain linear combination (stride 1: the
            # forward kernel on flipped taps; stride 2, round 3: the marching super-pixel kernel -- dA0 of the stride-2
            # blocks, the largest tensors of the network, is never written)
            if pl.fused_dw or pl.fused_dw5:
                dz0, part0, dwdw = ops.dwconv_bwd_fused(dd, e, st0, wflip, n, h, w, a.cexp, k, l, t, oh, ow,
                                                        xw=(x, sv["we"]) if pl.efree else None)
            elif pl.efree_s2:
                # stride-2 3x3 blocks in the recompute modes: e is neither rebuilt nor read -- the data-gradient launch forms
                # the e rows of the pixels it completes from x and is the weight gradient too (three launches -> one)
                dz0, part0, dwdw = ops.dwconv_bwd_data(dd, sv["wkkc"], *pl.dw, epi=(None, st0), xw=(x, sv["we"]), dw=True)
            else:
                dz0, part0 = ops.dwconv_bwd_data(dd, sv["wkkc"], *pl.dw, w_kkc_flipped=wflip, epi=(e, st0))
            del dd
            if frozen:
                # de = scale0 * dZ0 is never formed: dx = dZ0 (diag(scale0) We) through a 16-bit image of the row-scaled weight,
                # dWe = diag(scale0) (dZ0^T x) -- no pass over an expanded-size tensor beyond the two GEMMs' read of dZ0
                del e, dw_in
                _, dg0, db0 = ops.bn_bwd_coefs(part0, n * hw, st0, blk._bn0.weight, frozen=True)
                ws_t = ops.bn_frozen_weight_t(blk._expand_conv.weight.view(a.cexp, a.cin), st0.scale)      # [cin, cexp]
                dx, dwe = expand_bwd(dz0, ws_t)
                dwe = ops.rowscale_f32_(dwe, st0.scale)
                de = None
            elif pl.fold_bn0:
                # bn0 backward is linear in (dZ0, e) and e = x We^T: it is folded into the operands of the expand conv's
                # two gradient GEMMs (ops.bn_fold_expand_bwd) -- de is never formed, e is not read again.  Three passes
                # over the expanded tensor against ~10 small launches and 6 passes over the (6x smaller) block input:
                # pays from ~0.25 GB of expanded tensor per call (B5 at 32 x 1520 x 912: blocks 4-12 from 0.4 GB on one stream; with
                # the three launch chains of round 5 the small launches overlap and the blocks at 95 x 57 / c = 3072 join)
                del e, dw_in
                coef0, dg0, db0 = ops.bn_bwd_coefs(part0, n * hw, st0, blk._bn0.weight)
                dx, dwe = ops.bn_fold_expand_bwd(dz0, x, blk._expand_conv.weight.view(a.cexp, a.cin), sv["we"], coef0,
                                                 db0, n * hw, residual=dy if a.skip else None, gram=sv["gram"])
                de = None
            else:
                de, dg0, db0 = ops.bnact_bwd(e, n, hw, a.cexp, st0, blk._bn0.weight, 0, g=dz0, partials=part0)
                del e, dw_in
            del dz0
        elif link is not None:
            # linked stem: this launch finishes the STEM's bn0 + swish backward (x is the stem's raw conv output): what goes
            # back is dZ0 = dL/d bn0(x), the BatchNorm reductions travel in the link
            da0, link.part = ops.dwconv_bwd_data(dd, sv["wkkc"], *pl.dw, w_kkc_flipped=wflip, epi=(x, link.st))
            del dd
        else:
            da0 = ops.dwconv_bwd_data(dd, sv["wkkc"], *pl.dw, w_kkc_flipped=wflip)
            del dd
        if a.expand != 1:
            if de is not None:
                dx, dwe = expand_bwd(de, blk.w_expand(transposed=True))
            grads["_expand_conv.weight"] = dwe.view(a.cexp, a.cin, 1, 1)
            grads["_bn0.weight"], grads["_bn0.bias"] = dg0, db0
        else:
            dx = da0
            if a.skip:
                dx = ops.bnact_apply(da0, n, hw, a.cin, blk._ones, blk._zeros, 0, res=dy)
        grads["_depthwise_conv.weight"] = ops.transpose_f32(dwdw).view(a.cexp, 1, k, k)
        grads["_bn1.weight"], grads["_bn1.bias"] = dg1, db1n
        grads["_se_reduce.weight"], grads["_se_reduce.bias"] = dw1.view(a.cse, a.cexp, 1, 1), db1
        grads["_se_expand.weight"], grads["_se_expand.bias"] = dw2.view(a.cexp, a.cse, 1, 1), dbse2
        grads["_project_conv.weight"] = dwp.view(a.cout, a.cexp, 1, 1)
        grads["_bn2.weight"], grads["_bn2.bias"] = dg2, db2
        ctx.saved = None
        return (dx,) + (None,) * 8 + ops.deliver_param_grads(ops.cached_params(blk), [grads[nm] for nm in blk._param_names])


class _HeadFn(torch.autograd.Function):
    """_conv_head (1x1) + _bn1 + swish + global average pool [ref: efficientnet_custom.py:283, 307-309]."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, mod, n, h, wd, call):
        cin, cout = w.shape[1], w.shape[0]
        wb = ops.cast_bf16(w.view(cout, cin))
        if mod.fp8 and cin % 16 == 0:
            e, part = ops.linear_fwd_fp8(x, wb, stats=True)
        else:
            e, part = _conv_stats(call, ops.linear_fwd, mod.batch_stats, x, wb)
        st = _bn_stats(call, part, n * h * wd, mod._bn1, mod.batch_stats)
        pooled = ops.bnact_pool(e, n, h * wd, cout, st.scale, st.shift, 1)
        ctx.mod, ctx.st, ctx.geo, ctx.frozen = mod, st, (n, h, wd, cin, cout), not mod.batch_stats
        ctx.save_for_backward(x, e, wb)
        call.head = (e, st, n, h, wd, cout)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        x, e, wb = ctx.saved_tensors
        n, h, wd, cin, cout = ctx.geo
        mod = ctx.mod
        if ctx.frozen:
            _no_fp8_frozen(mod)
        de, dgamma, dbeta = ops.bnact_bwd(e, n, h * wd, cout, ctx.st, mod._bn1.weight, 1, add=dpooled.contiguous(),
                                          add_scale=1.0 / (h * wd), frozen=ctx.frozen)
        dx = ops.linear_dgrad(de, wb, w_t=ops.cast_transpose_bf16(mod._conv_head.weight.view(cout, cin)))
        dw = ops.linear_wgrad(de, x)
        gw, gg, gb = ops.deliver_param_grads((mod._conv_head.weight, mod._bn1.weight, mod._bn1.bias),
                                             (dw.view(cout, cin, 1, 1), dgamma, dbeta))
        return dx, gw, gg, gb, None, None, None, None, None


class _DropoutFn(torch.autograd.Function):
    """nn.Dropout on the pooled features [ref: efficientnet_custom.py:310-312]; Philox mask, regenerated in backward."""

    @staticmethod
    def forward(ctx, x, p, seed, sid):
        ctx.cfg = (p, seed, sid)
        return ops.dropout_f32(x.contiguous(), p, seed, sid)

    @staticmethod
    def backward(ctx, dy):
        p, seed, sid = ctx.cfg
        return ops.dropout_f32(dy.contiguous(), p, seed, sid), None, None, None


# ================================================================================================
#                                           modules
# ================================================================================================
class _BN(nn.BatchNorm2d):
    """Parameter/buffer container with the reference's BatchNorm2d keys; arithmetic happens in HIP kernels."""

    def __init__(self, c):
        super().__init__(c, momentum=BN_MOMENTUM, eps=BN_EPS)

    def forward(self, x):                 # pragma: no cover
        raise RuntimeError("BatchNorm arithmetic runs inside the fused HIP kernels, not here")


class _Conv(nn.Conv2d):
    """Parameter container (OIHW fp32) mirroring Conv2dStaticSamePadding's keys."""

    def __init__(self, cin, cout, k, stride=1, groups=1, bias=False):
        super().__init__(cin, cout, k, stride, 0, 1, groups, bias)

    def forward(self, x):                 # pragma: no cover
        raise RuntimeError("convolutions run inside the HIP kernels, not here")


_Geo = namedtuple("_Geo", ["idx", "expand", "k", "s", "cin", "cexp", "cout", "cse", "pad", "skip"])
# one call of an MBConv block (MBConvBlock.plan); dw = (n, h, w, cexp, k, s, pad_l, pad_t, oh, ow), the argument run of ops.dwconv_*
_Plan = namedtuple("_Plan", ["n", "h", "w", "oh", "ow", "training", "xdw", "efree", "fp8_expand", "keep_act", "fp8_project",
                             "store_e", "store_d", "store_p", "fuse_proj_dgrad", "fused_dw", "fold_bn0", "xbwd", "dw", "efree_s2",
                             "batch_stats", "fused_dw5"])
# training: the module's mode (stochastic pieces, the statistics tape's squeeze-excite entries); batch_stats: BatchNorm on batch
# statistics = training and not frozen (statistics epilogues, finalize, running-statistic updates, Gram pairs and every path whose
# backward reads them).  Frozen (batch_stats off) the backward is the running-statistics one: dx = scale*dz at every site


class MBConvBlock(nn.Module):
    """Mobile inverted residual bottleneck with squeeze-excite [ref: efficientnet_custom.py:36-140]."""

    def __init__(self, block_args: BlockArgs, global_params: GlobalParams, image_size=None, idx: int = 0):
        super().__init__()
        self._block_args = block_args
        a = block_args
        s = a.stride if isinstance(a.stride, int) else a.stride[0]
        cin, cexp = a.input_filters, a.input_filters * a.expand_ratio
        cse = max(1, int(a.input_filters * a.se_ratio))
        self.has_se = True
        self.id_skip = a.id_skip
        if a.expand_ratio != 1:
            self._expand_conv = _Conv(cin, cexp, 1)
            self._bn0 = _BN(cexp)
        self._depthwise_conv = _Conv(cexp, cexp, a.kernel_size, s, groups=cexp)
        self._bn1 = _BN(cexp)
        self._se_reduce = _Conv(cexp, cse, 1, bias=True)
        self._se_expand = _Conv(cse, cexp, 1, bias=True)
        self._project_conv = _Conv(cexp, a.output_filters, 1)
        self._bn2 = _BN(a.output_filters)
        self.args = _Geo(idx, a.expand_ratio, a.kernel_size, s, cin, cexp, a.output_filters, cse,
                         _static_pad(image_size, a.kernel_size, s),
                         bool(a.id_skip and s == 1 and cin == a.output_filters))
        self._param_names = [n for n, _ in self.named_parameters()]
        self.fp8 = False
        self.frozen_bn = False            # EfficientNet.freeze_bn
        self.recompute = 0
        self.register_buffer("_ones", torch.ones(cin), persistent=False)
        self.register_buffer("_zeros", torch.zeros(cin), persistent=False)

    @property
    def batch_stats(self):
        """do this block's BatchNorm layers use (and update from) batch statistics?  Otherwise: the running statistics"""
        return self.training and not self.frozen_bn

    def out_geo(self, n, h, w):
        """(n, oh, ow) of this block's output for an (n, h, w) input"""
        a = self.args
        l, r, t, b = a.pad
        return n, _out_extent(h, t, b, a.k, a.s), _out_extent(w, l, r, a.k, a.s)

    def xdw_capable(self):
        """the shape-independent half of ``plan().xdw``: may the expand conv run inside the depthwise launch (ops.mbconv_xdw_fwd)?"""
        a = self.args
        return bool(ops.XDW) and a.expand != 1 and a.cin <= XDW_MAX_CIN and not self.fp8

    def plan(self, n, h, w, recording):
        """Every path choice of ONE call of this block on an (n, h, w) input, forward and backward, from the block's mode (training /
        recompute / fp8), the module-level switches and thresholds as they stand NOW and the library's (cached) shape predicates.
        ``_MBConvFn.forward`` stores the plan with the graph; the backward reads only that.

        recording: is an autograd graph being recorded?  (autograd runs Function.forward with grad mode off and reports
        needs_input_grad from requires_grad alone: ``forward`` passes ``torch.is_grad_enabled()``.)  A block that may store its
        expanded tensor e runs the two-launch forward when recording (e rounded to 16 bits, stored), the fused one otherwise.
        Grad mode is only a proxy for "e must be stored": under ``torch.utils.checkpoint`` (first pass under no_grad, recompute
        with grad on) the two passes would take different forwards and differ in the last bits.  Such a caller first sets
        recompute mode >= 1 on the ``xdw_capable`` blocks, as ``EfficientNet.xdw_reforward_modes`` does for the micro-batched step."""
        a, rc, expand, bstat = self.args, self.recompute, self.args.expand != 1, self.batch_stats
        _, oh, ow = self.out_geo(n, h, w)
        rows, orows = n * h * w, n * oh * ow
        dw = (n, h, w, a.cexp, a.k, a.s, a.pad[0], a.pad[2], oh, ow)
        fusable = self.xdw_capable() and ops.mbconv_xdw_ok(n, h, w, a.cin, *dw[3:])
        # stride-1 3x3 blocks whose backward forms its e rows from x as well (ops.dwconv_bwd_fused with xw) and folds the
        # BatchNorm0 backward into the expand conv's gradient GEMMs never need e anywhere: an E-free plan IS fused forward +
        # fused depthwise backward + fold (enough expanded bytes for the fold to be the chosen BatchNorm0 backward)
        # (batch statistics only: both E-free forms fold BatchNorm0 through the forward's Gram pair, which a frozen forward -- running
        # statistics -- does not produce; the frozen BatchNorm0 backward needs neither fold nor Gram pair, see _MBConvFn.backward)
        efree = bool(fusable and ops.EFREE and FUSE_DW_BWD and a.k == 3 and a.s == 1 and bstat
                     and 2 * rows * a.cexp >= BN_FOLD_MIN_BYTES and ops.dwconv_bwd_fused_ok(*dw, cin=a.cin))
        # ... and where no backward needs e stored (no graph, or a recompute mode that rebuilds it) the forward is fused too
        xdw = efree or (fusable and (rc >= 1 or not recording))
        keep_act = not ops._rows_ok(orows, a.cout, a.cexp, None, 0)
        fold = fused_dw = fused_dw5 = fuse_proj = xbwd = False
        if recording:
            fuse_proj = bool(FUSE_PROJ_DGRAD and ops.proj_dgrad_fusable(orows, a.cexp, a.cout, oh * ow))
            fused_dw = efree or bool(FUSE_DW_BWD and expand and ops.dwconv_bwd_fused_ok(*dw))
            fused_dw5 = bool(FUSE_DW_BWD and expand and ops.dwconv_bwd_fused5_ok(*dw))
            fold = expand and bstat and (efree or 2 * rows * a.cexp >= (BN_FOLD_MIN_BYTES if a.s == 1 else max(BN_FOLD_MIN_BYTES, BN_FOLD_S2_MIN_BYTES)))
            xbwd = expand and not fold and ops.xbwd_rows_ok(rows, a.cexp, a.cin)
        # stride-2 3x3 blocks whose e is not stored (recompute modes >= 1): the backward forms the e rows from x inside the data-
        # gradient launch, which is the weight gradient too (ops.dwconv_bwd_data with xw), and folds BatchNorm0: e is not rebuilt
        efree_s2 = bool(recording and fusable and ops.EFREE_S2 and a.k == 3 and a.s == 2 and bstat and rc >= 1 and fold
                        and ops.dwconv_bwd_s2_xw_ok(*dw, cin=a.cin, force=ops.EFREE_S2 >= 2))
        return _Plan(n, h, w, oh, ow, self.training, xdw, efree,
                     fp8_expand=bool(expand and self.fp8 and a.cin % 16 == 0 and not ops._rows_ok(rows, a.cexp, a.cin, None, 0)),
                     keep_act=keep_act, fp8_project=keep_act and self.fp8 and a.cexp % 16 == 0 and a.cout > 64,
                     store_e=expand and rc == 0 and not xdw, store_d=rc < 2, store_p=rc < 4,
                     fuse_proj_dgrad=fuse_proj, fused_dw=fused_dw, fold_bn0=fold, xbwd=xbwd, dw=dw, efree_s2=efree_s2,
                     batch_stats=bstat, fused_dw5=fused_dw5)

    def w_expand(self, transposed=False):
        """cached 16-bit image of the expand conv's weight, [cexp, cin] or transposed.  (Forward, backward and
        ``EfficientNet.warm_weight_images`` all ask w_*: the cache key holds pointer, shape and strides of the view)"""
        v = self._expand_conv.weight.view(self.args.cexp, self.args.cin)
        return ops.cast_transpose_bf16(v) if transposed else ops.cast_bf16(v)

    def w_taps(self, flipped=False):
        """cached fp32 depthwise taps [k*k, cexp], or rotated by 180 degrees (stride-1 data gradient)"""
        v = self._depthwise_conv.weight.view(self.args.cexp, self.args.k * self.args.k)
        return ops.flipped_taps_f32(v) if flipped else ops.transpose_f32(v, cache=True)

    def w_project(self, transposed=False):
        """cached 16-bit image of the project conv's weight: [cout, cexp], or transposed [cexp, cout] (backward)"""
        v = self._project_conv.weight.view(self.args.cout, self.args.cexp)
        return ops.cast_transpose_bf16(v) if transposed else ops.cast_bf16(v)

    def forward(self, inputs, n, h, w, rowscale=None, link=None, call=None):
        """link: the ``_StemLink`` of a linked stem whose raw output this call reads (block 0); call: the ``_Call`` of the encoder
        forward this is part of (None: the block on its own); grad mode: see ``plan``"""
        return _MBConvFn.apply(inputs, rowscale, self, n, h, w, torch.is_grad_enabled(), link,
                               call if call is not None else _Call(), *ops.cached_params(self))


class EfficientNet(nn.Module):
    """[ref: efficientnet_custom.py:143-411]"""

    def __init__(self, blocks_args: List[BlockArgs] = None, global_params: GlobalParams = None):
        super().__init__()
        assert isinstance(blocks_args, list) and len(blocks_args) > 0
        self._global_params, self._blocks_args = global_params, blocks_args
        gp = global_params
        size = (gp.image_size, gp.image_size) if isinstance(gp.image_size, int) else tuple(gp.image_size)
        c0 = _scaled_width(32, gp)
        self._conv_stem = _Conv(3, c0, 3, 2)
        self._bn0 = _BN(c0)
        self.stem_pad = _static_pad(size, 3, 2)
        size = _down(size, 2)
        self._blocks = nn.ModuleList([])
        for ba in blocks_args:
            ba = ba._replace(input_filters=_scaled_width(ba.input_filters, gp),
                             output_filters=_scaled_width(ba.output_filters, gp),
                             num_repeat=_scaled_depth(ba.num_repeat, gp))
            s = ba.stride if isinstance(ba.stride, int) else ba.stride[0]
            self._blocks.append(MBConvBlock(ba, gp, size, idx=len(self._blocks)))
            size = _down(size, s)
            if ba.num_repeat > 1:
                ba = ba._replace(input_filters=ba.output_filters, stride=1)
            for _ in range(ba.num_repeat - 1):
                self._blocks.append(MBConvBlock(ba, gp, size, idx=len(self._blocks)))
        head_out = _scaled_width(1280, gp)
        self._conv_head = _Conv(ba.output_filters, head_out, 1)
        self._bn1 = _BN(head_out)
        self._dropout_p = gp.dropout_rate if gp.include_top else 0.0
        self.out_dim = head_out
        self.fp8 = False
        self._frozen_bn = False
        self.rng = _Seeds()
        self.register_buffer("_ones_b", torch.ones(1), persistent=False)
        self._bn_layers = [m for m in self.modules() if isinstance(m, _BN)]
        # what reaches a forward through ``module(x)`` rather than as an argument; read by ``_new_call`` alone
        self._tape = None                 # set_stat_tape
        self.update_running = True        # False: forwards leave running statistics and batch counters alone (the engine's re-forwards)
        self._side_defer = self._side_counters = None         # side_call_begin .. side_call_end

    # ---------------------------------------------------------------------------- construction API
    @classmethod
    def from_name(cls, model_name, in_channels=3, **override_params):
        cls._check_model_name_is_valid(model_name)
        if in_channels != 3:
            raise NotImplementedError("the gfx950 stem kernel is specialised for 3 input channels")
        w, d, res, p = _COEFFS[model_name]
        gp = GlobalParams(width_coefficient=w, depth_coefficient=d, image_size=res, dropout_rate=p, num_classes=1000,
                          batch_norm_momentum=0.99, batch_norm_epsilon=BN_EPS, drop_connect_rate=0.2, depth_divisor=8,
                          min_depth=None, include_top=True)
        if override_params:
            gp = gp._replace(**override_params)
        blocks = [BlockArgs(r, k, s, e, i, o, 0.25, True) for (r, k, s, e, i, o) in _STAGES]
        return cls(blocks, gp)

    @classmethod
    def from_pretrained(cls, model_name, weights_path=None, advprop=False, in_channels=3, num_classes=1000,
                        **override_params):
        """Builds the network; ImageNet weights are loaded only from a local ``weights_path`` (the reference
        downloads them, efficient_net_custom_utils.py:584-615 -- there is no network on the target boxes)."""
        model = cls.from_name(model_name, num_classes=num_classes, **override_params)
        if isinstance(weights_path, str):
            sd = torch.load(weights_path, map_location="cpu")
            sd.pop("_fc.weight", None)
            sd.pop("_fc.bias", None)
            ret = model.load_state_dict(sd, strict=False)
            assert not ret.unexpected_keys, ret.unexpected_keys
        return model

    @classmethod
    def get_image_size(cls, model_name):
        cls._check_model_name_is_valid(model_name)
        return _COEFFS[model_name][2]

    @classmethod
    def _check_model_name_is_valid(cls, model_name):
        if model_name not in VALID_MODELS:
            raise ValueError("model_name should be one of: " + ", ".join(VALID_MODELS))

    def set_fp8(self, on: bool = True):
        """BASELINE config #5: forward of the late-stage 1x1 convolutions (expand / project / head on the tiled MFMA path)
        with per-tensor-scaled OCP e4m3 activations and weights on gfx950's fp8 MFMA [ref: efficientnet_custom.py:104,
        122,283 are the convolutions concerned]; statistics, depthwise stages and the whole backward stay bf16 / fp32."""
        if on and self._frozen_bn:
            raise NotImplementedError("set_fp8 with frozen BatchNorm statistics (freeze_bn) is not implemented")
        self.fp8 = bool(on)
        for blk in self._blocks:
            blk.fp8 = bool(on)
        return self

    def freeze_bn(self, on: bool = True):
        """Frozen BatchNorm: every BatchNorm site of the encoder normalises with its RUNNING statistics, in ``train()`` mode too,
        and leaves ``running_mean`` / ``running_var`` / ``num_batches_tracked`` untouched; the backward is torch's for a
        BatchNorm in eval mode (dx = gamma*rsqrt(running_var + eps)*dz, dgamma = sum dz*xhat, dbeta = sum dz).  A site uses batch
        statistics iff ``self.training and not self.frozen_bn``: ``eval()`` alone gives the same arithmetic (forward and, with
        autograd on, backward), ``freeze_bn()`` + ``train()`` keeps drop-connect and dropout live -- the usual way to fine-tune or
        continue pre-training at a small per-GPU batch; a micro-batched step and a full-batch step are then the same function of
        the weights.  The flag survives ``train()`` / ``eval()``, is not part of ``state_dict()`` and covers the whole encoder:
        the per-layer ``.training`` flags of the ``_bn*`` submodules are NOT consulted (as before).  Not implemented together
        with ``set_fp8``.  Returns self."""
        if on and self.fp8:
            raise NotImplementedError("freeze_bn with the fp8 forward (set_fp8) is not implemented")
        self._frozen_bn = bool(on)
        for blk in self._blocks:
            blk.frozen_bn = bool(on)
        return self

    @property
    def frozen_bn(self) -> bool:
        return self._frozen_bn

    @property
    def batch_stats(self) -> bool:
        """do the BatchNorm sites use (and update from) batch statistics?  (``training and not frozen_bn``)"""
        return self.training and not self._frozen_bn

    def set_recompute(self, mode: int = 0):
        """Activation memory of a kept autograd graph against backward work (the micro-batched contrastive step keeps as
        many micro-batch graphs as fit and re-runs the forward of the others): 0 = every MBConv block stores its expanded
        tensor e and its depthwise output d (the two big ones, ~72 % of the graph); 1 = e is rebuilt in the backward by
        one more expand GEMM from the block input; 2 = e and d (and the stored late-stage activation) are rebuilt
        (expand GEMM + depthwise forward); 3 = mode 1 everywhere plus mode 2 on the blocks whose depthwise stage is a
        stride-1 3x3 (the depthwise kernels that run near HBM rate: 45 % of the d bytes of B5 for ~1.5 % more work);
        4 = mode 2 plus the projection conv's output p (needed first thing in the backward, by BatchNorm2): rebuilt from the
        rebuilt d -- the graph of a block is then its input x alone.
        Same kernels on the same operands: gradients agree across modes to the spread of the atomically reduced ones."""
        assert mode in (0, 1, 2, 3, 4)
        for blk in self._blocks:
            a = blk.args
            blk.recompute = int(mode) if mode != 3 else (2 if (a.k == 3 and a.s == 1 and a.expand != 1 and a.cexp <= MODE3_MAX_CEXP) else 1)
        return self

    def xdw_reforward_modes(self):
        """Micro-batched step (engine._step_micro): the graph-less first forward of a micro-batch runs its narrow-input blocks
        through the fused expand + depthwise launch (no expanded tensor).  Its re-forward -- same inputs, replayed statistics,
        graph recorded -- must produce the SAME embeddings, so those blocks take recompute mode 1 there (fused forward, the
        expanded tensor rebuilt by one GEMM in the backward) instead of the two-launch forward that rounds e to 16 bits first.
        Returns the list of (block, previous mode) to restore."""
        changed = []
        for blk in self._blocks:
            if blk.recompute == 0 and blk.xdw_capable():
                changed.append((blk, blk.recompute))
                blk.recompute = 1
        return changed

    def set_swish(self, memory_efficient=True):
        """No-op: the swish is always the fused, recompute-in-backward form."""

    # ---------------------------------------------------------------------------- forward
    def stem_geo(self, n, h, w):
        """(n, oh, ow) of the stem's output (= block 0's input) for n images of h x w"""
        l, r, t, b = self.stem_pad
        return n, _out_extent(h, t, b, 3, 2), _out_extent(w, l, r, 3, 2)

    def _stem(self, x, call=None):
        """stem of one chain -> (output, its _StemLink or None, output geometry).  Block 0 has no expand conv (every EfficientNet-
        B*): the stem's bn0 + swish then runs inside block 0's depthwise kernels, which get the link with the stem's RAW output"""
        b0 = self._blocks[0].args
        link = _StemLink() if (LINK_STEM and b0.expand == 1 and not b0.skip and b0.s == 1) else None
        y = _StemFn.apply(x, self._conv_stem.weight, self._bn0.weight, self._bn0.bias, self, link, call)
        return y, link, self.stem_geo(x.shape[0], *x.shape[2:])

    def _drop_connect_scales(self, n, device, seed):
        """keep/keep_prob per (block, sample) [ref: efficient_net_custom_utils.py:129-154]; rate = 0.2*idx/len."""
        rate = self._global_params.drop_connect_rate
        out = []
        nb = len(self._blocks)
        for i, blk in enumerate(self._blocks):
            p = rate * float(i) / nb if rate else 0.0
            if not (self.training and p > 0.0 and blk.args.skip):
                out.append(None)
                continue
            out.append(ops.dropout_f32(self._ones_b.expand(n).contiguous(), p, seed, 1000 + i))
        return out

    def set_stat_tape(self, tape):
        """install (or remove: None) the tape the next forwards of THIS encoder record on / replay from (engine._step_micro)"""
        self._tape = tape

    def _new_call(self, defer=None):
        """the context of one chain of a forward that starts now (draws its seed); the one reader of the encoder's ambient state"""
        held = self._side_counters
        return _Call(self._tape, self.update_running, defer if defer is not None else self._side_defer,
                     held if held is not None else [], self.rng.next())

    def _end_call(self, call):
        """bump the batch counters the call collected with one multi-tensor launch (116 one-element add launches per forward
        otherwise) -- unless a side-call bracket holds them back for ``side_call_end``"""
        if call.counters and call.counters is not self._side_counters:
            with torch.no_grad():
                torch._foreach_add_(call.counters, 1)

    def _run(self, inputs):
        """one forward on the current stream -> (pooled features before dropout, its ``_Call``)"""
        if not inputs.is_cuda:
            raise RuntimeError("mammo_clip_amd.EfficientNet runs only on a HIP device (no CPU fallback)")
        x = inputs if isinstance(inputs, ops.RawImages) or inputs.dtype == torch.float32 else inputs.float()
        call = self._new_call()
        y, link, (n, h, w) = self._stem(x, call)
        scales = self._drop_connect_scales(n, x.device, call.seed)
        for blk, rs in zip(self._blocks, scales):
            y = blk(y, n, h, w, rs, link if blk.args.idx == 0 else None, call)
            n, h, w = blk.out_geo(n, h, w)
        pooled = _HeadFn.apply(y, self._conv_head.weight, self._bn1.weight, self._bn1.bias, self, n, h, w, call)
        self._end_call(call)
        return pooled, call

    # ---------------------------------------------------------------------------- side-stream calls (model/clip.py)
    def warm_weight_images(self, backward: bool):
        """Build (or find) every cached weight image the forward -- and, with ``backward``, the backward -- of this encoder
        reads, on the CURRENT stream: two calls of the encoder on different streams then only ever hit the cache (an image
        built by one chain while the other chain is in flight would be read without an ordering between the streams).  The
        blocks' images come from the accessors their autograd function uses (``MBConvBlock.w_*``)."""
        for blk in self._blocks:
            if blk.args.expand != 1:
                blk.w_expand()
                if backward:
                    blk.w_expand(transposed=True)
            blk.w_taps()
            if backward and blk.args.s == 1:
                blk.w_taps(flipped=True)
            blk.w_project()
            if backward:
                blk.w_project(transposed=True)
        cout, cin = self._conv_head.weight.shape[0], self._conv_head.weight.shape[1]
        ops.cast_bf16(self._conv_head.weight.view(cout, cin))
        if backward:
            ops.cast_transpose_bf16(self._conv_head.weight.view(cout, cin))

    def side_call_begin(self):
        """the next forward of this encoder runs on a side stream beside another one: BatchNorm running statistics and batch
        counters are left to ``side_call_end`` (after the join, on the main stream)"""
        self._side_counters = []
        self._side_defer = _BNDefer(self) if self.batch_stats else None

    def side_call_end(self):
        d, c = self._side_defer, self._side_counters
        self._side_defer = self._side_counters = None
        if d is not None:
            d.apply()
        if c:
            with torch.no_grad():
                torch._foreach_add_(c, 1)

    def forward_pair(self, x1, x2, side):
        """Both image views of a batch [ref: clip.py:83,108 -- two sequential ``encode_image`` calls] as two chains issued
        BLOCK BY BLOCK in alternation: view 1 on the current stream, view 2 on ``side``.  Each chain is exactly the
        launch sequence of ``forward`` on its input (same seeds: two consecutive draws, view 1 first; per-view BatchNorm
        statistics; view 2's running-statistic updates and both views' batch counters applied after the join, view 1
        first), so every result equals two sequential calls; what changes is the ISSUE order -- the two chains are in flight
        side by side from the first launch on, in the forward and (autograd replays the creation order backwards) in the
        backward.  Returns the two pooled feature tensors."""
        if not (x1.is_cuda and x2.is_cuda):
            raise RuntimeError("mammo_clip_amd.EfficientNet runs only on a HIP device (no CPU fallback)")
        main = torch.cuda.current_stream(x1.device)
        conv = lambda x: x if isinstance(x, ops.RawImages) or x.dtype == torch.float32 else x.float()   # noqa: E731
        # view 2's dtype conversion (fp16 / bf16 / integer inputs) is a launch of its own: it is issued on the SIDE stream,
        # where chain 2 reads its result (on the main stream, behind the fork, nothing ordered it before the side
        # chain's stem); the inputs themselves were produced on the main stream before the caller's fork -- the explicit wait
        # below also covers callers that built them after it (model/clip.py: ``batch["image_views"].to(device)``)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            x2c = conv(x2)
        xs = [conv(x1), x2c]
        for t_ in (x2.data if isinstance(x2, ops.RawImages) else x2,):
            if torch.is_tensor(t_) and t_.is_cuda:
                t_.record_stream(side)          # allocated on the main stream, read by the side chain (allocator reuse)
        def chain(i):
            """switch the issue point to chain i"""
            torch.cuda.set_stream(side if i else main)

        ys, scales, links = [None, None], [None, None], [None, None]
        try:
            chain(1)
            defer = _BNDefer(self) if self.batch_stats else None      # (zero-filled scratch: allocated and cleared on the side stream)
            calls = [self._new_call(), self._new_call(defer)]         # (two consecutive seeds, view 1 first; one tape)
            for i in (0, 1):
                chain(i)
                ys[i], links[i], (n, h, w) = self._stem(xs[i], calls[i])
                scales[i] = self._drop_connect_scales(n, xs[i].device, calls[i].seed)
            for bi, blk in enumerate(self._blocks):
                for i in (0, 1):
                    chain(i)
                    ys[i] = blk(ys[i], n, h, w, scales[i][bi], links[i] if bi == 0 else None, calls[i])
                n, h, w = blk.out_geo(n, h, w)
            pooled = [None, None]
            for i in (0, 1):
                chain(i)
                pooled[i] = _HeadFn.apply(ys[i], self._conv_head.weight, self._bn1.weight, self._bn1.bias, self, n, h, w, calls[i])
                if self.training and self._dropout_p > 0.0:
                    pooled[i] = _DropoutFn.apply(pooled[i], self._dropout_p, calls[i].seed, 999)
        finally:
            torch.cuda.set_stream(main)
        main.wait_stream(side)
        if defer is not None:
            defer.apply()
        for c in calls:
            self._end_call(c)
        pooled[1].record_stream(main)
        return pooled[0], pooled[1]

    @staticmethod
    def _feature_map(call):
        """head conv + BN + swish of a finished call as an NCHW fp32 map"""
        e, st, n, h, w, cout = call.head
        fmap = ops.bnact_apply(e, n, h * w, cout, st.scale, st.shift, 1)
        return ops.cast_f32(fmap).view(n, h, w, cout).permute(0, 3, 1, 2)

    def extract_features(self, inputs):
        """Final feature map after head conv + BN + swish, NCHW fp32 (API parity; not on the training hot path)."""
        return self._feature_map(self._run(inputs)[1])

    def forward(self, inputs):
        """[ref: efficientnet_custom.py:287-313]: pooled features [b, out_dim] (fp32); the dict form
        ``{"image": x}`` returns (pooled, raw_feature_map)."""
        want_map = isinstance(inputs, dict) and "image" in inputs
        pooled, call = self._run(inputs["image"] if want_map else inputs)
        if self.training and self._dropout_p > 0.0:
            pooled = _DropoutFn.apply(pooled, self._dropout_p, call.seed, 999)
        return (pooled, self._feature_map(call)) if want_map else pooled
