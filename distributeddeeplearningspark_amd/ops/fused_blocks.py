"""Fused ResNet bottleneck (GPU): the whole conv-BN-ReLU x3 + shortcut block is ONE
autograd node whose backward is scheduled by hand.

What the fusion buys over composing per-op autograd nodes:
  * the block-input gradient ``dX = dgrad(conv1) + dShortcut`` is produced by the
    conv1 data-gradient GEMM epilogue (residual add), instead of a separate add kernel;
  * every BN uses the statistics the producing conv's epilogue accumulated;
  * the BN backward ReLU masks are recomputed from the conv outputs (mode 2) except
    where a residual enters (mode 1), so no extra activation tensor is read;
  * bn3's backward of an identity block folds through conv3 (``_FOLD_BN3``, default on; a module flag for
    tests, not an environment knob): the next block's conv1 data-gradient stores the block-output gradient
    under bn3's ReLU mask with its column sums, and conv3's weight / data gradients come from the small
    products g^T y2, y2^T y2 (``fold_conv_bn_backward``, csrc/kernels/bn_fold.hip) — no dx sweep, no read of
    conv3's output.  Only where it pays (``_FOLD_MIN_ELEMS``), never in deterministic mode, and only when the
    gradient that arrives is the very tensor the producer wrote; otherwise the sweeps run as before;
  * the forward of such a block never writes conv3's output either (``_FOLD_BN3_FWD``): bn3's batch statistics
    follow from S = y2^T y2 and s = sum y2 (one read of the 4x narrower y2, ``gram_colsum``; the folded backward
    needs both anyway), and conv3 applies bn3, the shortcut and the ReLU in its own epilogue, writing the block
    output and the ReLU bit mask (``_convbn3_fold_forward``).  A backward that cannot fold recomputes conv3's
    output first (``_recompute_yc``);
  * a projection block whose shortcut conv is 1x1 / stride 1 (``_FOLD_DOWN``, ResNet-50's ``layer1.0``) folds both
    bn3 and the shortcut's BN the same way: both BNs' statistics from the Gram matrices of the 4x narrower y2 and
    x, ONE two-product GEMM that writes the block output and its mask (``_fold_down_forward``) — neither pre-BN
    tensor is written — and ``fold_conv_bn_backward`` once per unit on the same pre-masked gradient;
  * all workspaces come from the per-step statistics pool;
  * parameter-gradient hooks (for the overlapped RCCL all-reduce) fire per layer in
    backward order as soon as each layer's gradients are final.
Reference semantics are unchanged: ``relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + sc(x))``.
"""
from __future__ import annotations

import weakref

import torch

from . import conv as CV
from . import determinism as _det
from . import gemm as G
from . import zpad as ZP
from ._native import C
from .norm import new_stats_workspace, partials_workspace, pool_epoch
from .streams import on_grad_stream


class _ConvBNState:
    """Per-(conv,BN) forward results needed by the backward.  ``pre_reduced``: the BN-backward
    partial sums [32, 2, C] already accumulated by the producer of this BN's output gradient
    (the next block's conv1 data-gradient epilogue), so ``bn_backward`` skips its reduce sweep.
    ``pre_reduced = (ws, d, premasked)``; ``premasked``: ``d`` was stored under this BN's ReLU mask and ``ws``
    holds only its column sums (what the folded bn3 backward needs, see ``_fold_bn3_backward``).
    ``fold``: this is the bn3 of an identity bottleneck that may fold (set by the forward).
    ``gram``: (S, s, statistics-pool epoch) of a forward that folded bn3 into conv3's epilogue — ``yc`` is None then."""

    __slots__ = ("g", "yc", "y", "mean", "invstd", "scale", "shift", "mode", "mask", "pre_reduced", "fold", "gram",
                 "__weakref__")

    def __init__(self):
        self.pre_reduced = None
        self.fold = False
        self.gram = None


# Block outputs -> the (ConvBN unit, state) of the BN that produced them (weak references only): the
# next bottleneck looks its input up here so that, in backward, its conv1 data-gradient (which
# produces THIS BN's output gradient) can also accumulate this BN's backward partial sums.
_PRODUCERS: dict = {}


def _register_output(y, unit, st):
    _PRODUCERS[y.data_ptr()] = (weakref.ref(y), unit, weakref.ref(st))
    if len(_PRODUCERS) > 4096:  # stale entries of freed tensors
        for k in [k for k, v in _PRODUCERS.items() if v[0]() is None]:
            del _PRODUCERS[k]


def _producer_of(x):
    e = _PRODUCERS.get(x.data_ptr())
    if e is None or e[0]() is not x:
        return None
    st = e[2]()
    return None if st is None else (e[1], st)


def _bn_forward(layer_bn, yc, stats, resid, relu, training, mask=None, apply=True, res_affine=None):
    """Finalize the fused statistics into scale/shift (+ running stats) and, with ``apply``, write
    ``relu(yc * scale + shift + resid)``; ``res_affine = (scale_r, shift_r)`` normalises a pre-BN
    residual on the fly (the downsample shortcut's BN rides in its consumer's apply sweep)."""
    Cc = yc.shape[-1]
    M = yc.numel() // Cc
    dev = yc.device
    bn = layer_bn
    gamma = None if bn.gamma is None else bn.gamma.master
    beta = None if bn.beta is None else bn.beta.master
    rm, rv = bn._states["moving_mean"], bn._states["moving_variance"]
    # one allocation for the four per-channel vectors (host cost per BN: VGG-16 runs launch-bound)
    scale, shift, mean, invstd = torch.empty(4, Cc, dtype=torch.float32, device=dev).unbind(0)
    if stats is None:  # deterministic mode: no fused (atomic) statistics; fixed-order partial rows instead
        stats = partials_workspace(M, Cc, dev)
        C().bn_stats(yc, stats, Cc)
    C().bn_finalize(stats, M, Cc, gamma, beta, bn.epsilon, 1.0 - bn.momentum, rm, rv, mean, invstd, scale, shift)
    if not apply:
        return None, mean, invstd, scale, shift
    y = torch.empty_like(yc)
    rs, rt = res_affine if res_affine is not None else (None, None)
    C().bn_apply(yc, scale, shift, resid, y, Cc, relu, mask, rs, rt)
    return y, mean, invstd, scale, shift


def convbn_forward(unit, x, resid=None, relu=True, apply=True, res_affine=None):
    """conv (fused statistics) + BN (+resid)(+relu) for a ``models.resnet.ConvBN`` unit.
    ``apply=False``: statistics and scale/shift only (``st.y`` is None: the consumer applies them)."""
    conv, bn = unit.conv, unit.bn
    N, H, W, Ci = x.shape
    kh, kw = conv.kernel_size
    p = conv.padding if isinstance(conv.padding, tuple) else (kh // 2, kw // 2)
    g = CV.geometry(N, H, W, Ci, conv.filters, kh, kw, conv.strides, p, conv.dilation_rate)
    stats = new_stats_workspace(conv.filters, x.device)
    yc = CV.conv_fwd_native(x, conv.kernel.data, g, stats=stats)
    st = _ConvBNState()
    st.g, st.yc = g, yc
    # ReLU after a residual add: the backward mask cannot be recomputed from yc alone, so the
    # apply pass stores it as bits (mode 3) instead of the backward re-reading the bf16 output
    bits = relu and resid is not None
    st.mask = torch.empty(-(-yc.numel() // 32) * 4, dtype=torch.uint8, device=yc.device) if bits else None
    st.y, st.mean, st.invstd, st.scale, st.shift = _bn_forward(bn, yc, stats, resid, relu, True, st.mask, apply,
                                                               res_affine)
    st.mode = 0 if not relu else (2 if resid is None else (3 if bits else 1))
    return st


def bn_backward(unit, st, dy, want_dres, red2=None, dy_mask=None, reduced=None):
    """BN backward of ``st`` for output gradient ``dy``: (dx, dres or None).

    ``red2 = (x2, mean2, ws2)``: the dx sweep also writes the reduce partials of a second BN fed by the
    masked gradient (``bn_bwd_dx_red``; the ResNet downsample BN).  ``dy_mask``: the gradient this BN
    sees is ``dy`` under that ReLU bit mask (mode 3), i.e. the masked gradient is never materialised;
    ``reduced``: the partial-sum workspace already holds this BN's reduce (the red2 of the producer)."""
    bn = unit.bn
    Cc = st.yc.shape[-1]
    M = st.yc.numel() // Cc
    mode = st.mode
    y = st.y if st.mode == 1 else (st.mask if st.mode == 3 else None)
    if dy_mask is not None:
        if st.mode != 0:
            raise ValueError("bn_backward: dy_mask applies to a BN without its own ReLU")
        mode, y = 3, dy_mask
    pre, st.pre_reduced = st.pre_reduced, None
    if reduced is not None:
        ws = reduced
    elif pre is not None and not pre[2] and _same_tensor(pre[1], dy):
        # partial sums already accumulated by dy's producer (no reduce sweep) — valid only when dy IS the
        # gradient that producer reduced: a second consumer of this BN's output makes autograd sum the
        # gradients into a new tensor, and then the sweep runs on the sum
        ws = pre[0]
    else:
        ws = partials_workspace(M, Cc, dy.device)
        C().bn_bwd_reduce(dy, st.yc, y, st.scale, st.shift, st.mean, ws, Cc, mode)
    coef = torch.empty(3 * Cc, dtype=torch.float32, device=dy.device)
    C().bn_bwd_finalize(ws, M, Cc, None if bn.gamma is None else bn.gamma.master, st.mean, st.invstd,
                        None if bn.gamma is None else bn.gamma.grad, None if bn.beta is None else bn.beta.grad, coef)
    dyc = torch.empty_like(dy)
    dres = torch.empty_like(dy) if want_dres else None
    if red2 is not None:
        if dres is not None:
            raise ValueError("bn_backward: red2 replaces dres")
        C().bn_bwd_dx_red(dy, st.yc, y, st.scale, st.shift, coef, dyc, Cc, mode, red2[0], red2[1], red2[2])
    else:
        C().bn_bwd_dx(dy, st.yc, y, st.scale, st.shift, coef, dyc, dres, Cc, mode)
    if bn.grad_hook is not None:
        bn.grad_hook()
    return dyc, dres


def conv_backward(unit, st, dyc, x, need_dx, resid=None, resid_mask=None, bnr=None, rsub=None):
    conv = unit.conv
    # the weight gradient only feeds the optimizer / all-reduce: it runs on the side stream
    # (ops/streams.py) beside the data-gradient and BatchNorm sweeps of the layers below
    # (every tensor the side-stream kernel reads is recorded on that stream: the main stream may
    # drop them before the side stream has run)
    with on_grad_stream(dyc.device, dyc, x, default=False):
        CV.conv_wgrad_native(dyc, x, st.g, conv.kernel.grad)
    dx = None
    if need_dx:
        dx = CV.conv_dgrad_native(dyc, conv.kernel.data, st.g, resid=resid, resid_mask=resid_mask, bnr=bnr, rsub=rsub)
    # the hook comes after the last read of the weights: on one GPU it may start the optimizer on this bucket
    # (parallel/ddp.py DataParallel.solo), which rewrites them
    if conv.grad_hook is not None:
        conv.grad_hook()
    return dx


class _BottleneckFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, block):
        ctx.prev = _producer_of(x) if _FUSE_BNR else None  # the BN whose output is this block's input
        x = x.contiguous()
        gdn = _fold_down_geometry(block, x) if block.down is not None else None
        if gdn is not None:
            # both pre-BN tensors of the block's tail stay unwritten: the shortcut conv runs inside the output GEMM
            s1 = convbn_forward(block.c1, x, relu=True)
            s2 = convbn_forward(block.c2, s1.y, relu=True)
            s_down, s3 = _fold_down_forward(block, x, s2.y, *gdn)
            s3.fold = True  # the next block's conv1 data-gradient pre-masks (backward: fold_dn)
        else:
            # the downsample BN is not applied on its own: its scale/shift normalise the shortcut inside
            # the block-output apply sweep (one write + one read of the shortcut tensor saved)
            s_down = convbn_forward(block.down, x, relu=False, apply=False) if block.down is not None else None
            sc = s_down.yc if s_down is not None else x
            s1 = convbn_forward(block.c1, x, relu=True)
            s2 = convbn_forward(block.c2, s1.y, relu=True)
            g3 = _fold_fwd_geometry(block.c3, s2.y) if s_down is None else None
            if g3 is not None:
                s3 = _convbn3_fold_forward(block.c3, s2.y, sc, g3)
            else:
                s3 = convbn_forward(block.c3, s2.y, resid=sc, relu=True,
                                    res_affine=None if s_down is None else (s_down.scale, s_down.shift))
            s3.fold = s_down is None and s3.mode == 3 and _fold_gate(s3.g)
        ctx.block, ctx.states = block, (s_down, s1, s2, s3)
        ctx.save_for_backward(x)
        ctx.needs_dx = ctx.needs_input_grad[0]
        _register_output(s3.y, block.c3, s3)
        return s3.y

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        b = ctx.block
        s_down, s1, s2, s3 = ctx.states
        dout = dout.contiguous()
        # identity shortcut: its gradient is dout masked by the block-output ReLU; instead of the BN
        # backward writing it out, conv1's data-gradient epilogue adds dout under the bit mask
        masked_sc = s_down is None and s3.mode == 3 and s1.g.is_pointwise
        # downsample shortcut: its BN's input gradient is dout under bn3's ReLU mask.  bn3's dx sweep also
        # writes that BN's reduce partials (it reads dout and the mask anyway; + a read of the shortcut's
        # pre-BN tensor), and the shortcut BN's dx sweep re-applies the mask to dout — so the masked
        # gradient is never written, and the shortcut BN runs no reduce sweep
        fuse_down = _FUSE_DOWN and s_down is not None and s3.mode == 3 and s_down.mode == 0
        ws_d = None
        # identity block whose output gradient arrived pre-masked with its column sums (the next block's conv1
        # data-gradient, BNR premask): bn3's backward folds through conv3 — no dx sweep, no read of yc3
        pre3 = s3.pre_reduced
        fold = (_FOLD_BN3 and s3.fold and not _det.enabled() and pre3 is not None and pre3[2]
                and _same_tensor(pre3[1], dout) and b.c3.bn.gamma is not None)
        # projection block whose forward folded both BNs (_fold_down_forward): the same, once per unit; the
        # shortcut's turn comes where its backward always ran (below), on the same gradient and column sums
        fold_dn = fold and s_down is not None and s_down.gram is not None
        fold = fold and s_down is None
        ws_g = None
        if fold_dn:
            s3.pre_reduced = None
            ws_g = pre3[0]
            bnr2 = _bnr_mode2(s2, dout.device)
            d2 = _fold_unit_backward(b.c3, s3, s2.y, dout, ws_g, bnr2)
        elif fold:
            s3.pre_reduced = None
            bnr2 = _bnr_mode2(s2, dout.device)
            d2 = _fold_bn3_backward(b.c3, s3, s2, dout, pre3[0], bnr2)
            dsc = dout  # pre-masked: it is the shortcut's gradient as it stands
        else:
            if s3.yc is None:
                # the forward never wrote conv3's output (nor the shortcut conv's, in a folding projection block)
                # and this backward does not fold (a second consumer, a producer that did not pre-mask, the
                # network's last block): recompute, then the sweeps as before
                _recompute_yc(b.c3, s3, s2)
                if s_down is not None and s_down.yc is None:
                    _recompute_yc(b.down, s_down, x)
            if fuse_down:
                Cd = s_down.yc.shape[-1]
                ws_d = partials_workspace(s_down.yc.numel() // Cd, Cd, dout.device)
                d3c, dsc = bn_backward(b.c3, s3, dout, False, red2=(s_down.yc, s_down.mean, ws_d))
            else:
                d3c, dsc = bn_backward(b.c3, s3, dout, want_dres=not masked_sc)
        # the data-gradients of conv3 and conv2 produce bn2's / bn1's output gradients: their epilogues also
        # accumulate those BNs' backward partial sums (ReLU mask recomputed from yc), so bn_backward skips the
        # reduce sweep wherever the kernel that ran could take it (bnr["done"])
        if not (fold or fold_dn):
            bnr2 = _bnr_mode2(s2, dout.device)
            d2 = conv_backward(b.c3, s3, d3c, s2.y, True, bnr=bnr2)
        _take_reduced(s2, bnr2, d2)
        d2c, _ = bn_backward(b.c2, s2, d2, False)
        bnr1 = _bnr_mode2(s1, dout.device)
        d1 = conv_backward(b.c2, s2, d2c, s1.y, True, bnr=bnr1)
        _take_reduced(s1, bnr1, d1)
        d1c, _ = bn_backward(b.c1, s1, d1, False)
        rsub = None
        if fold_dn:
            # [M, Ci] as it stands: conv1's data-gradient adds it as the plain residual
            # (no BN behind it takes a per-channel offset out again: its column sums are made to vanish)
            dsc = _fold_unit_backward(b.down, s_down, x, dout, ws_g, None, need_dx=ctx.needs_dx, exact_colsum=True)
        elif s_down is not None:
            if fuse_down:
                ddc, _ = bn_backward(b.down, s_down, dout, False, dy_mask=s3.mask, reduced=ws_d)
            else:
                ddc, _ = bn_backward(b.down, s_down, dsc, False)
            gd = s_down.g
            if (_HALF_RES_SC and ctx.needs_dx and s1.g.is_pointwise and gd.KH == 1 and gd.KW == 1
                    and (gd.sh, gd.sw) == (2, 2) and (gd.ph, gd.pw) == (0, 0)):
                # stride-2 1x1 shortcut: its data-gradient stays at half resolution ([N, H/2, W/2, Cin], a plain
                # GEMM) and conv1's dgrad epilogue adds it at the even pixels — instead of a scatter GEMM that
                # writes a full-resolution tensor of 3/4 zeros which that epilogue then reads back
                wd = b.down.conv.kernel.data
                dsc = G.linear_dgrad(ddc.view(gd.M, gd.Co), wd.view(gd.Co, gd.Ci))
                rsub = (gd.H, gd.W)
                conv_backward(b.down, s_down, ddc, x, False)  # weight gradient + hook, after the last weight read
            else:
                dsc = conv_backward(b.down, s_down, ddc, x, ctx.needs_dx)
        # dX = dgrad(conv1) + dShortcut: the residual add rides in the conv1 dgrad epilogue, and so do the
        # backward partial sums of the BN that produced X (previous block's bn3, mode 3) when that GEMM
        # runs on the streaming kernel — that BN's backward then skips its reduce sweep over dX and yc
        bnr = None
        if ctx.needs_dx and ctx.prev is not None and ctx.prev[1].mode == 3 and not _det.enabled():
            pst = ctx.prev[1]
            # a folding identity block wants the masked gradient and its column sums only (neither x nor the mean
            # is read: after a folded forward there is no x); without premask the reduce needs x = conv3's output
            premask = bool(_FOLD_BN3 and pst.fold and s1.g.is_pointwise)
            if premask or pst.yc is not None:
                bnr = {"x": pst.yc, "mask": pst.mask, "mean": pst.mean,
                       "ws": new_stats_workspace(pst.g.Co, dout.device), "premask": premask}
        if _TEST_MUTATION is not None and _TEST_MUTATION[0] == "drop_shortcut" and _TEST_MUTATION[1] in (None, b.name):
            # test-only fault (tests/test_gpu_determinism.py): the block's input gradient loses its shortcut term
            masked_sc, dsc, rsub = False, None, None
        if masked_sc:
            dx = conv_backward(b.c1, s1, d1c, x, ctx.needs_dx, resid=dout, resid_mask=s3.mask, bnr=bnr)
        else:
            dx = conv_backward(b.c1, s1, d1c, x, ctx.needs_dx, resid=dsc, bnr=bnr, rsub=rsub)
        if bnr is not None and bnr.get("done"):
            ctx.prev[1].pre_reduced = (bnr["ws"], dx, bool(bnr["premask"]))
        ctx.states = ctx.prev = None
        return dx, None, None



_FUSE_BNR = True
# test-only fault injection for the discriminating gradient checks: ("drop_shortcut", block name or None)
_TEST_MUTATION = None
# bn1 / bn2 of every bottleneck: reduce fused into the conv2 / conv3 data-gradient epilogues
_FUSE_BNR_INNER = True
_HALF_RES_SC = True
# downsample BN backward fed by bn3's dx sweep (bn_bwd_dx_red): no masked-gradient tensor, no reduce sweep
_FUSE_DOWN = True
# stem: BN backward through the max pool without materialising the pool's gradient (pool3s2_bn_bwd)
_FUSE_STEM_BWD = True
_STEM_PARTIALS = 2048  # workgroups (= partial rows) of its reduce


def _bnr_mode2(st, device):
    """BN-backward reduce request for a ReLU BN without residual (mode 2) — see ``gemm.linear_dgrad``."""
    if not _FUSE_BNR_INNER or st.mode != 2 or _det.enabled():
        return None
    return {"x": st.yc, "scale": st.scale, "shift": st.shift, "mean": st.mean,
            "ws": new_stats_workspace(st.yc.shape[-1], device)}


def _take_reduced(st, bnr, d):
    if bnr is not None and bnr.get("done"):
        st.pre_reduced = (bnr["ws"], d, False)


# bn3's backward of identity bottlenecks folded through conv3 (csrc/kernels/bn_fold.hip): monkeypatchable
_FOLD_BN3 = True
# it trades ~2.9 sweeps of the [M, Co] tensor for seven launch-sized kernels: folds where that tensor has at
# least this many elements (measured per ResNet-50 stage at batch 256, docs/PERFORMANCE.md)
_FOLD_MIN_ELEMS = 1 << 26


def _fold_gate(g) -> bool:
    return g.is_pointwise and g.Ci % 64 == 0 and g.Co % 128 == 0 and g.M * g.Co >= _FOLD_MIN_ELEMS


# the forward of a folding block: bn3 in conv3's epilogue, conv3's output never written.  Only effective with
# _FOLD_BN3 (which restores the unfolded step when off); monkeypatchable
_FOLD_BN3_FWD = True


def _fold_fwd_geometry(unit, x2):
    """conv3's geometry when this identity block's forward folds bn3 into conv3's epilogue, else None: the flags,
    not in deterministic mode, a bn3 with a scale (as the backward's fold asks), the backward's gate, and a shape the streaming kernel's column-scale epilogue has."""
    if not (_FOLD_BN3 and _FOLD_BN3_FWD) or _det.enabled() or x2.device.type != "cuda":
        return None
    if unit.bn.gamma is None:  # the backward never folds without a scale: every step would recompute conv3's output
        return None
    conv = unit.conv
    N, H, W, Ci = x2.shape
    kh, kw = conv.kernel_size
    if (kh, kw) != (1, 1):
        return None
    p = conv.padding if isinstance(conv.padding, tuple) else (0, 0)
    g = CV.geometry(N, H, W, Ci, conv.filters, kh, kw, conv.strides, p, conv.dilation_rate)
    if not (_fold_gate(g) and G.stream_colscale_ok(g.Co, g.Ci) and x2.is_contiguous()):
        return None
    return g


def _convbn3_fold_forward(unit, x2, resid, g):
    """conv3 + bn3 + identity shortcut + ReLU of a folding block without conv3's output: S = x2^T x2 and
    s = sum x2 (``gram_colsum``) -> bn3's batch sums (``bn_fold_fwd_stats``) -> ``bn_finalize`` as ever -> ONE
    GEMM that applies scale / shift / shortcut / ReLU in its epilogue and writes y and the ReLU bit mask."""
    M, Co, Ci = g.M, g.Co, g.Ci
    dev = x2.device
    x2m = x2.view(M, Ci)
    st = _fold_fwd_stats(unit, x2m, g)
    st.mask = torch.empty(-(-M * Co // 32) * 4, dtype=torch.uint8, device=dev)
    y = torch.empty((g.N, g.H, g.W, Co), dtype=torch.bfloat16, device=dev)
    G.linear_fwd(x2m, unit.conv.kernel.data.view(Co, Ci), bias=st.shift, relu=True, out=y.view(M, Co),
                 resid=resid.view(M, Co), colscale=st.scale, relu_mask_out=st.mask)
    st.y, st.mode = y, 3
    return st


def _recompute_yc(unit, s3, s2):
    """The 1x1 conv output of a unit whose forward did not write it (plain forward GEMM), for the unfolded sweeps:
    conv3 from ``s2`` (the state in front of it), or a folding projection block's shortcut conv from ``s2`` = the
    block input itself."""
    geo = s3.g
    xin = s2.y if isinstance(s2, _ConvBNState) else s2
    w = unit.conv.kernel.data.view(geo.Co, geo.Ci)
    yc = torch.empty((geo.N, geo.H, geo.W, geo.Co), dtype=torch.bfloat16, device=xin.device)
    G.linear_fwd(xin.view(geo.M, geo.Ci), w, out=yc.view(geo.M, geo.Co))
    s3.yc = yc


# a projection bottleneck whose shortcut conv is 1x1 / stride 1 folds bn3 AND the shortcut's BN (forward and
# backward); only effective with _FOLD_BN3 and _FOLD_BN3_FWD; monkeypatchable
_FOLD_DOWN = True
# its own size gate on the [M, Co] block output (ResNet-50 at batch 256: layer1.0 only, 2^27.6 elements)
_FOLD_DOWN_MIN_ELEMS = 1 << 27


def _pointwise_geometry(conv, xshape):
    N, H, W, Ci = xshape
    kh, kw = conv.kernel_size
    if (kh, kw) != (1, 1):
        return None
    p = conv.padding if isinstance(conv.padding, tuple) else (0, 0)
    g = CV.geometry(N, H, W, Ci, conv.filters, kh, kw, conv.strides, p, conv.dilation_rate)
    return g if g.is_pointwise else None


def _fold_down_geometry(block, x):
    """(conv3's geometry, the shortcut conv's) when this projection block folds both BNs of its tail, else None:
    the flags, not in deterministic mode, both BNs with a scale, both convs 1x1 / stride 1 over the same pixels
    with 64 input channels (the two-product GEMM's shape), a stride-1 main path, and the size gate."""
    if not (_FOLD_BN3 and _FOLD_BN3_FWD and _FOLD_DOWN) or _det.enabled() or x.device.type != "cuda":
        return None
    if block.c3.bn.gamma is None or block.down.bn.gamma is None or x.dtype != torch.bfloat16:
        return None
    N, H, W, _ = x.shape
    if any(tuple(u.conv.strides) != (1, 1) for u in (block.c1, block.c2)):
        return None
    gd = _pointwise_geometry(block.down.conv, x.shape)
    g3 = _pointwise_geometry(block.c3.conv, (N, H, W, block.c2.conv.filters))
    if gd is None or g3 is None or gd.Co != g3.Co or gd.Co % 128:
        return None
    if not G.stream_dual_ok(g3.Co, g3.Ci, gd.Ci) or g3.M * g3.Co < _FOLD_DOWN_MIN_ELEMS:
        return None
    return g3, gd


def _fold_fwd_stats(unit, xm, g):
    """State of a 1x1 conv + BN whose output is not written: the BN's batch statistics from S = x^T x and s = sum x
    (``gram_colsum`` -> ``bn_fold_fwd_stats`` -> ``bn_finalize`` as ever, running statistics included)."""
    conv, bn = unit.conv, unit.bn
    M, Co, Ci = g.M, g.Co, g.Ci
    dev = xm.device
    # S | s: zeroed fp32 from the per-step statistics pool, which hands no memory out twice within a step, so
    # they live until this step's backward (the epoch tells a backward that runs after a later reset)
    ps = new_stats_workspace(-(-(Ci * Ci + Ci) // 64), dev).view(-1)
    S, s = ps[: Ci * Ci].view(Ci, Ci), ps[Ci * Ci : Ci * Ci + Ci]
    C().gram_colsum(xm, S, s)
    stats = new_stats_workspace(Co, dev)
    C().bn_fold_fwd_stats(conv.kernel.data.view(Co, Ci), S, s, M, stats)
    gamma = None if bn.gamma is None else bn.gamma.master
    beta = None if bn.beta is None else bn.beta.master
    rm, rv = bn._states["moving_mean"], bn._states["moving_variance"]
    st = _ConvBNState()
    st.g, st.yc, st.y, st.mask = g, None, None, None
    st.scale, st.shift, st.mean, st.invstd = torch.empty(4, Co, dtype=torch.float32, device=dev).unbind(0)
    C().bn_finalize(stats, M, Co, gamma, beta, bn.epsilon, 1.0 - bn.momentum, rm, rv, st.mean, st.invstd, st.scale,
                    st.shift)
    st.gram = (S, s, pool_epoch(dev))
    return st


def _fold_down_forward(block, x, y2, g3, gd):
    """Tail of a folding projection block: y = relu(bn3(conv3 y2) + bn_d(conv_d x)) from the two narrow inputs.
    Returns (shortcut state, bn3 state): neither has a conv output (``yc`` None), both keep their Gram."""
    M, Co = g3.M, g3.Co
    if tuple(y2.shape) != (g3.N, g3.H, g3.W, g3.Ci):
        raise RuntimeError("folding projection block: conv2's output does not match conv3's geometry")
    y2 = y2.contiguous()
    s3 = _fold_fwd_stats(block.c3, y2.view(M, g3.Ci), g3)
    sd = _fold_fwd_stats(block.down, x.view(M, gd.Ci), gd)
    s3.mask = torch.empty(-(-M * Co // 32) * 4, dtype=torch.uint8, device=x.device)
    y = torch.empty((g3.N, g3.H, g3.W, Co), dtype=torch.bfloat16, device=x.device)
    G.linear_dual_fwd(y2.view(M, g3.Ci), block.c3.conv.kernel.data.view(Co, g3.Ci), s3.scale,
                      x.view(M, gd.Ci), block.down.conv.kernel.data.view(Co, gd.Ci), sd.scale,
                      shift1=s3.shift, shift2=sd.shift, relu=True, out=y.view(M, Co), relu_mask_out=s3.mask)
    s3.y, s3.mode, sd.mode = y, 3, 0
    return sd, s3


def fold_conv_bn_backward(w, gw, g2, y2, ws_g, mean, invstd, gamma, dgamma, dbeta, bnr2=None, out=None, gram=None,
                          need_dx=True, exact_colsum=False):
    """Backward of ``yc = y2 w^T -> BN`` (a 1x1 conv and the BN behind it) from the BN's output gradient ``g2``
    [M, Co], already under the BN's ReLU mask, and its column sums ``ws_g`` ([32, 2, Co], row [:, 0]): with the
    BN's dx = A g + B yc + K,
        d2 = g (A.w) + y2 Gm + kv,  gw += A.P + B.(w S) + K x s,  P = g^T y2, S = y2^T y2, s = sum_p y2
    (csrc/kernels/bn_fold.hip) — neither yc nor dx is read or written.  ``dgamma`` / ``dbeta`` accumulate as in
    ``bn_bwd_finalize``; ``bnr2``: fused BN-backward reduce of d2 (``gemm.linear_dgrad``).
    ``gram = (S, s)``: the forward formed them already (``gram_colsum``): neither the S product nor the
    ``bn_stats`` sweep over y2 is launched.  ``need_dx = False``: parameter gradients only (d2 is None).
    ``exact_colsum``: kv is re-formed from the rounded bf16 WA and Gm (``bn_fold_kv``) so that the column sums of d2
    vanish as the BN's dx demands; for a d2 with no BN behind it to remove a per-channel offset (a shortcut's).
    Returns (d2 [M, Ci] bf16, sums [2, Co]: sum g and sum g (yc - mean))."""
    M, Co = g2.shape
    Ci = y2.shape[1]
    dev = g2.device
    # P | S | s: zeroed fp32 accumulators (the two split-K products, the column sums), from the statistics pool
    if gram is not None:
        S, s = gram
        P = new_stats_workspace(-(-(Co * Ci) // 64), dev).view(-1)[: Co * Ci].view(Co, Ci)
        G.linear_wgrad(g2, y2, P)
        wsy = None
    else:
        ps = new_stats_workspace(-(-(Co * Ci + Ci * Ci + Ci) // 64), dev).view(-1)
        P, S = ps[: Co * Ci].view(Co, Ci), ps[Co * Ci : Co * Ci + Ci * Ci].view(Ci, Ci)
        s = ps[Co * Ci + Ci * Ci : Co * Ci + Ci * Ci + Ci]
        G.linear_wgrad(g2, y2, P)
        G.linear_wgrad(y2, y2, S)
        wsy = partials_workspace(M, Ci, dev)
        C().bn_stats(y2, wsy, Ci)
    f32 = torch.empty(5 * Co + Ci, dtype=torch.float32, device=dev)
    sums, coef, kv = f32[: 2 * Co], f32[2 * Co : 5 * Co], f32[5 * Co :]
    C().bn_fold_sums(w, P, ws_g, mean, wsy, sums, s)
    C().bn_bwd_finalize(sums, M, Co, gamma, mean, invstd, dgamma, dbeta, coef)
    b16 = torch.empty(2 * Co * Ci + Ci * Ci, dtype=torch.bfloat16, device=dev)
    WA, WAt, Gm = b16[: Co * Ci].view(Co, Ci), b16[Co * Ci : 2 * Co * Ci].view(Ci, Co), b16[2 * Co * Ci :].view(Ci, Ci)
    C().bn_fold_coef(w, P, S, s, coef, WA, WAt, Gm, kv, gw)
    if not need_dx:
        return None, sums.view(2, Co)
    if exact_colsum:
        C().bn_fold_kv(WA, Gm, sums[:Co], s, M, kv)
    r = G.linear_fwd(y2, Gm, bias=kv)
    if out is None:
        out = torch.empty((M, Ci), dtype=torch.bfloat16, device=dev)
    G.linear_dgrad(g2, WA, out=out, resid=r, bnr=bnr2, wt=WAt)
    return out, sums.view(2, Co)


def _fold_bn3_backward(unit, s3, s2, g, ws_g, bnr2):
    """conv3 + bn3 backward of an identity bottleneck from the pre-masked output gradient ``g`` and its column
    sums ``ws_g`` (``fold_conv_bn_backward``).  Returns d2."""
    return _fold_unit_backward(unit, s3, s2.y, g, ws_g, bnr2)


def _fold_unit_backward(unit, st, xin, g, ws_g, bnr2, need_dx=True, exact_colsum=False):
    """1x1 conv + BN backward of one folding unit (conv3 + bn3 from y2; a projection block's shortcut conv + its BN
    from the block input) from the pre-masked block-output gradient ``g`` and its column sums ``ws_g``
    (``fold_conv_bn_backward``), then the unit's gradient hooks.  Returns the unit's input gradient [N, H, W, Ci],
    or None without ``need_dx``."""
    conv, bn = unit.conv, unit.bn
    geo = st.g
    M, Co, Ci = geo.M, geo.Co, geo.Ci
    dx = torch.empty((geo.N, geo.H, geo.W, Ci), dtype=torch.bfloat16, device=g.device) if need_dx else None
    gram = None
    if st.gram is not None and st.gram[2] == pool_epoch(g.device):  # the pool has not been reset since the forward
        gram = st.gram[:2]
    fold_conv_bn_backward(conv.kernel.data.view(Co, Ci), conv.kernel.grad.view(Co, Ci), g.view(M, Co), xin.view(M, Ci),
                          ws_g, st.mean, st.invstd, bn.gamma.master, bn.gamma.grad,
                          None if bn.beta is None else bn.beta.grad, bnr2=bnr2,
                          out=None if dx is None else dx.view(M, Ci), gram=gram, need_dx=need_dx,
                          exact_colsum=exact_colsum)
    if bn.grad_hook is not None:
        bn.grad_hook()
    if conv.grad_hook is not None:  # after the last read of the weights (see conv_backward)
        conv.grad_hook()
    return dx


def _same_tensor(a, b) -> bool:
    """b is the very gradient tensor a (same storage, shape and version), not a sum formed from it."""
    return (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()
            and a._version == b._version)


def bottleneck(block, x, anchor):
    """``anchor``: any parameter view requiring grad (makes the node part of the graph)."""
    return _BottleneckFn.apply(x, anchor, block)


def convbn_relu(unit, x, anchor, relu=True):
    """Single fused conv+BN(+ReLU) unit as one autograd node (the ResNet stem)."""
    if not x.requires_grad and _stem_s2d_ok(unit.conv, x.shape[-1]):
        return _StemS2DFn.apply(x, anchor, unit, relu)
    return _ConvBNFn.apply(x, anchor, unit, relu)


_STEM_S2D = True  # space-to-depth stem (tests switch it off to compare with the plain 7x7 conv)
_STEM_POOL = True  # stem conv + BN + ReLU + max pool as one node


def _stem_s2d_ok(conv, Ci) -> bool:
    """7x7 / stride 2 / pad 3 stem on <= 4 channels: run as a 4x4 stride-1 conv after a
    block-2 space-to-depth (12 of 16 channels used instead of 3 of 8, K = 256 instead of 392)."""
    return (_STEM_S2D and Ci <= 4 and tuple(conv.kernel_size) == (7, 7)
            and tuple(conv.strides) == (2, 2) and tuple(conv.dilation_rate) == (1, 1)
            and (conv.padding == (3, 3) or conv.padding == 3 or conv.padding == "same"))


def _s2d_weight(w):
    """[Co, 7, 7, C] -> [Co, 4, 4, 16]: W'[A][B][(2a+b)C + ch] = W[2A+a][2B+b][ch] (zero past 7)."""
    Co, _, _, Cc = w.shape
    w8 = torch.nn.functional.pad(w, (0, 0, 0, 1, 0, 1))  # [Co, 8, 8, C]
    w4 = w8.view(Co, 4, 2, 4, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(Co, 4, 4, 4 * Cc)
    return torch.nn.functional.pad(w4, (0, 16 - 4 * Cc)).contiguous()


def _s2d_weight_grad(g4, Cc):
    """Inverse of _s2d_weight for gradients: [Co, 4, 4, 16] -> [Co, 7, 7, C]."""
    Co = g4.shape[0]
    g = g4[..., : 4 * Cc].reshape(Co, 4, 4, 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(Co, 8, 8, Cc)
    return g[:, :7, :7, :]


_S2D_TABLES: dict = {}


def _s2d_table(t):
    """(int32 [Co, 4, 4, 16] table, extent): entry i of the space-to-depth filter is element table[i] of
    ``t``'s storage from ``t.data_ptr()`` (its own strides: the arena's padded views work), -1 = zero.
    The same table gathers the bf16 filter (forward) and scatters the fp32 gradient back (backward)."""
    key = (tuple(t.shape), tuple(t.stride()), str(t.device))
    hit = _S2D_TABLES.get(key)
    if hit is None:
        offs = torch.zeros((), dtype=torch.int64)
        for d, (n, st) in enumerate(zip(t.shape, t.stride())):
            offs = offs.unsqueeze(-1) + torch.arange(n, dtype=torch.int64) * st
        Co, _, _, Cc = t.shape
        o8 = torch.nn.functional.pad(offs, (0, 0, 0, 1, 0, 1), value=-1)
        o4 = o8.view(Co, 4, 2, 4, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(Co, 4, 4, 4 * Cc)
        tab = torch.nn.functional.pad(o4, (0, 16 - 4 * Cc), value=-1).contiguous()
        hit = _S2D_TABLES[key] = (tab.to(torch.int32).to(t.device), int(offs.max()) + 1)
    return hit


def _s2d_weight_dev(w):
    """``_s2d_weight`` as one table-driven HIP gather (no pad / permute / copy kernels per step)."""
    if not (w.is_cuda and w.dtype == torch.bfloat16):
        return _s2d_weight(w)
    tab, ext = _s2d_table(w)
    out = torch.empty(tab.shape, dtype=w.dtype, device=w.device)
    C().gather_bf16(w, tab, out, ext)
    return out


def _s2d_weight_grad_into(conv, g, dyc, xs, Cc):
    """Stem weight gradient: the 4x4 conv's gradient into a zeroed scratch, scattered (added) into the
    7x7 filter's gradient by the gather table's adjoint — HIP launches only."""
    gw = conv.kernel.grad
    tmp = torch.empty((g.Co, 4, 4, 16), dtype=torch.float32, device=dyc.device)
    if not gw.is_cuda:
        tmp.zero_()
        CV.conv_wgrad_native(dyc, xs, g, tmp)
        gw.add_(_s2d_weight_grad(tmp, Cc))
        return
    C().zero_ranges([tmp])
    CV.conv_wgrad_native(dyc, xs, g, tmp)
    tab, ext = _s2d_table(gw)
    C().scatter_add_f32(tmp, tab, gw, ext)


class _StemPoolFn(torch.autograd.Function):
    """ResNet stem conv (7x7 s2 p3 through space-to-depth) + BN + ReLU + 3x3/2 max pool as ONE node:
    the BN affine and ReLU are applied by the pool as it loads the conv output (maxpool_fwd with
    scale/shift), so the stem's BN-apply sweep — a write and a re-read of the largest activation of
    the network (batch 256: 411 MB each way) — is gone.  Backward: pool gather -> BN backward (ReLU
    mask recomputed from the conv output, mode 2) -> weight gradient, as before."""

    @staticmethod
    def forward(ctx, x, anchor, unit, k, s, p):
        x = x.contiguous()
        N, H, W, Cc = x.shape
        conv = unit.conv
        Ho, Wo = (H + 6 + 1) // 2, (W + 6 + 1) // 2
        xs = torch.empty((N, Ho, Wo, 16), dtype=x.dtype, device=x.device)
        C().s2d_pad(x, xs, 3)
        w4 = _s2d_weight_dev(conv.kernel.data.detach())
        g = CV.geometry(N, Ho, Wo, 16, conv.filters, 4, 4, (1, 1), (0, 0), (1, 1))
        stats = new_stats_workspace(conv.filters, x.device)
        yc = CV.conv_fwd_native(xs, w4, g, stats=stats)
        st = _ConvBNState()
        st.g, st.yc = g, yc
        st.y, st.mean, st.invstd, st.scale, st.shift = _bn_forward(unit.bn, yc, stats, None, True, True, apply=False)
        st.mode = 2
        _, Hc, Wc, Co = yc.shape
        Hp, Wp = (Hc + 2 * p - k) // s + 1, (Wc + 2 * p - k) // s + 1
        y = torch.empty((N, Hp, Wp, Co), dtype=yc.dtype, device=yc.device)
        am = torch.empty((N, Hp, Wp, Co), dtype=torch.uint8, device=yc.device)
        C().maxpool_fwd(yc, y, am, k, k, s, s, p, p, st.scale, st.shift)
        ctx.unit, ctx.st, ctx.cc, ctx.pool = unit, st, Cc, (k, s, p)
        ctx.save_for_backward(xs, am)
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, am = ctx.saved_tensors
        unit, st = ctx.unit, ctx.st
        k, s, p = ctx.pool
        dy = dy.contiguous()
        N, H, W, Co = st.yc.shape
        if _FUSE_STEM_BWD and (k, s, p) == (3, 2, 1) and C().pool3s2_bn_bwd_ok(N, H, W, Co, dy.shape[1], dy.shape[2], 3):
            # the BN output gradient (the pool's gather) is recomputed from dy + argmax by the reduce and the dx
            # sweeps instead of being written (411 MB at batch 256) and read back by both
            bn = unit.bn
            M = N * H * W
            ws = torch.empty((_STEM_PARTIALS, 2, Co), dtype=torch.float32, device=dy.device)  # one row per workgroup
            C().pool3s2_bn_bwd(dy, am, st.yc, st.scale, st.shift, st.mean, ws, None)
            coef = torch.empty(3 * Co, dtype=torch.float32, device=dy.device)
            C().bn_bwd_finalize(ws, M, Co, None if bn.gamma is None else bn.gamma.master, st.mean, st.invstd,
                                None if bn.gamma is None else bn.gamma.grad, None if bn.beta is None else bn.beta.grad,
                                coef)
            dyc = torch.empty_like(st.yc)
            C().pool3s2_bn_bwd(dy, am, st.yc, st.scale, st.shift, st.mean, coef, dyc)
            if bn.grad_hook is not None:
                bn.grad_hook()
        else:
            d = torch.empty_like(st.yc)
            C().maxpool_bwd(dy, am, d, k, k, s, s, p, p)
            dyc, _ = bn_backward(unit, st, d, False)
        conv = unit.conv
        g = st.g
        with on_grad_stream(dy.device, dyc, xs, default=False):
            _s2d_weight_grad_into(conv, g, dyc, xs, ctx.cc)
        if conv.grad_hook is not None:
            conv.grad_hook()
        ctx.st = None
        return None, None, None, None, None, None  # the stem input is data: no gradient


def stem_pool(unit, x, anchor, k=3, s=2, p=1):
    """Stem conv+BN+ReLU followed by a k x k / s max pool, fused when the space-to-depth stem applies
    (``_STEM_POOL = False`` keeps the separate apply + pool); returns None when not applicable."""
    if (not _STEM_POOL or x.requires_grad or not _stem_s2d_ok(unit.conv, x.shape[-1])
            or unit.conv.filters % 8):
        return None
    return _StemPoolFn.apply(x, anchor, unit, k, s, p)


class _StemS2DFn(torch.autograd.Function):
    """ResNet stem conv (7x7 s2 p3, 3 channels) + BN (+ReLU) through space-to-depth."""

    @staticmethod
    def forward(ctx, x, anchor, unit, relu):
        x = x.contiguous()
        N, H, W, Cc = x.shape
        conv = unit.conv
        Ho, Wo = (H + 6 + 1) // 2, (W + 6 + 1) // 2
        xs = torch.empty((N, Ho, Wo, 16), dtype=x.dtype, device=x.device)
        C().s2d_pad(x, xs, 3)
        w4 = _s2d_weight_dev(conv.kernel.data.detach())
        g = CV.geometry(N, Ho, Wo, 16, conv.filters, 4, 4, (1, 1), (0, 0), (1, 1))
        stats = new_stats_workspace(conv.filters, x.device)
        yc = CV.conv_fwd_native(xs, w4, g, stats=stats)
        st = _ConvBNState()
        st.g, st.yc = g, yc
        st.y, st.mean, st.invstd, st.scale, st.shift = _bn_forward(unit.bn, yc, stats, None, relu, True)
        st.mode = 2 if relu else 0
        ctx.unit, ctx.st, ctx.cc = unit, st, Cc
        ctx.save_for_backward(xs)
        return st.y

    @staticmethod
    def backward(ctx, dy):
        (xs,) = ctx.saved_tensors
        unit, st = ctx.unit, ctx.st
        dyc, _ = bn_backward(unit, st, dy.contiguous(), False)
        conv = unit.conv
        g = st.g
        with on_grad_stream(dy.device, dyc, xs, default=False):
            _s2d_weight_grad_into(conv, g, dyc, xs, ctx.cc)
        if conv.grad_hook is not None:
            conv.grad_hook()
        ctx.st = None
        return None, None, None, None  # the stem input is data: no gradient


def _seq_conv_forward(ctx, x, unit):
    """Conv half of a Sequential conv -> BN node (``_ConvBNFn`` / ``_ConvBNPoolFn``): the conv output with
    its BN statistics fused into the epilogue; records on ``ctx`` what the backward needs."""
    # a conv -> BN -> ReLU chain (VGG): this conv's data-gradient epilogue accumulates the backward
    # partial sums of the BN that produced x (mode 2), whose backward then skips its reduce sweep
    ctx.prev = _producer_of(x) if _FUSE_BNR else None
    x = x.contiguous()
    Ci = x.shape[-1]
    ctx.ci = Ci
    kp = unit.conv.kernel
    if Ci % 8:  # stem: pad 3 -> 8 channels (16-B vectors); the arena keeps the filter padded (params.py)
        cp = -(-Ci // 8) * 8
        x = ZP.padded(x, cp)
        w = kp.pdata if kp.pshape[1:] == (*kp.shape[1:3], cp) and kp.pshape[0] == kp.shape[0] \
            else torch.nn.functional.pad(kp.data.detach(), (0, cp - Ci))
    else:
        w = kp.data
    conv = unit.conv
    N, H, W, Cp = x.shape
    kh, kw = conv.kernel_size
    p = conv.padding if isinstance(conv.padding, tuple) else (kh // 2, kw // 2)
    g = CV.geometry(N, H, W, Cp, conv.filters, kh, kw, conv.strides, p, conv.dilation_rate)
    stats = new_stats_workspace(conv.filters, x.device)
    yc = CV.conv_fwd_native(x, w, g, stats=stats)
    st = _ConvBNState()
    st.g, st.yc = g, yc
    ctx.unit, ctx.st, ctx.w, ctx.x = unit, st, w, x
    ctx.needs_dx = ctx.needs_input_grad[0]
    return st, stats


def _seq_conv_backward(ctx, dyc):
    """Weight gradient (side stream) and data gradient of the conv half, given the conv output's gradient."""
    unit, x = ctx.unit, ctx.x
    conv = unit.conv
    g = ctx.st.g
    with on_grad_stream(dyc.device, dyc, x, default=False):
        if g.Ci != ctx.ci and ctx.w is not conv.kernel.pdata:
            tmp = torch.zeros((g.Co, g.KH, g.KW, g.Ci), dtype=torch.float32, device=dyc.device)
            CV.conv_wgrad_native(dyc, x, g, tmp)
            conv.kernel.grad.add_(tmp[..., : ctx.ci])
        else:  # padded storage: it takes the zero-padded channels' (zero) gradients as is
            CV.conv_wgrad_native(dyc, x, g, conv.kernel.pgrad if ctx.w is conv.kernel.pdata else conv.kernel.grad)
    dx = None
    if ctx.needs_dx:
        bnr = None if ctx.prev is None else _bnr_mode2(ctx.prev[1], dyc.device)
        dx = CV.conv_dgrad_native(dyc, ctx.w, g, bnr=bnr)
        if bnr is not None:
            _take_reduced(ctx.prev[1], bnr, dx)
        dx = ZP.logical(dx, ctx.ci)
    if conv.grad_hook is not None:  # after the last read of the weights (see conv_backward)
        conv.grad_hook()
    ctx.st = ctx.prev = ctx.x = None
    return dx


class _ConvBNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, unit, relu):
        st, stats = _seq_conv_forward(ctx, x, unit)
        st.y, st.mean, st.invstd, st.scale, st.shift = _bn_forward(unit.bn, st.yc, stats, None, relu, True)
        st.mode = 2 if relu else 0
        _register_output(st.y, unit, st)
        return st.y

    @staticmethod
    def backward(ctx, dy):
        dyc, _ = bn_backward(ctx.unit, ctx.st, dy.contiguous(), False)
        return _seq_conv_backward(ctx, dyc), None, None, None


_SEQ_POOL = True  # Sequential conv -> BN -> ReLU -> 2x2 / 2 max pool as one node (tests compare with False)


class _ConvBNPoolFn(torch.autograd.Function):
    """VGG block tail conv -> BN -> ReLU -> 2x2 / stride-2 max pool as ONE node: the pool applies the BN
    affine + ReLU as it loads the conv output (no BN-apply sweep, the full-resolution activation is never
    written); backward: the BN's output gradient is the pool's scatter of the pooled gradient by the argmax
    bytes, recomputed inside the reduce and dx sweeps (``pool_bn_bwd``, k = 2) instead of written by a pool
    backward and read twice."""

    @staticmethod
    def forward(ctx, x, anchor, unit):
        st, stats = _seq_conv_forward(ctx, x, unit)
        st.y, st.mean, st.invstd, st.scale, st.shift = _bn_forward(unit.bn, st.yc, stats, None, True, True,
                                                                    apply=False)
        st.mode = 2
        N, Hc, Wc, Co = st.yc.shape
        y = torch.empty((N, Hc // 2, Wc // 2, Co), dtype=st.yc.dtype, device=st.yc.device)
        ctx.am = torch.empty(y.shape, dtype=torch.uint8, device=y.device)
        C().maxpool_fwd(st.yc, y, ctx.am, 2, 2, 2, 2, 0, 0, st.scale, st.shift)
        return y

    @staticmethod
    def backward(ctx, dy):
        st, bn = ctx.st, ctx.unit.bn
        dy = dy.contiguous()
        N, H, W, Co = st.yc.shape
        M = N * H * W
        # one partial row per workgroup, each workgroup one pass over its 256 / (C / 8) rows of 2x2 blocks
        rows = -(-(N * (H // 2) * (W // 2)) // max(1, 256 // (Co // 8)))
        ws = torch.empty((min(_STEM_PARTIALS, rows), 2, Co), dtype=torch.float32, device=dy.device)
        C().pool3s2_bn_bwd(dy, ctx.am, st.yc, st.scale, st.shift, st.mean, ws, None, 2)
        coef = torch.empty(3 * Co, dtype=torch.float32, device=dy.device)
        C().bn_bwd_finalize(ws, M, Co, bn.gamma.master, st.mean, st.invstd, bn.gamma.grad, bn.beta.grad, coef)
        dyc = torch.empty_like(st.yc)
        C().pool3s2_bn_bwd(dy, ctx.am, st.yc, st.scale, st.shift, st.mean, coef, dyc, 2)
        if bn.grad_hook is not None:
            bn.grad_hook()
        ctx.am = None
        return _seq_conv_backward(ctx, dyc), None, None


def convbn_relu_pool(unit, x, anchor):
    """Sequential conv -> BN -> ReLU -> MaxPooling2D(2, 2) as one node, or None when it does not apply."""
    conv = unit.conv
    if not _SEQ_POOL or conv.filters % 8 or conv.filters > 2048 or tuple(conv.strides) != (1, 1):
        return None
    if not (x.is_cuda and x.dtype == torch.bfloat16) or x.shape[1] % 2 or x.shape[2] % 2:
        return None
    return _ConvBNPoolFn.apply(x, anchor, unit)


_ = G
