"""ResNet / ResNeXt-FPN backbones with fp16 storage and fp32 accumulation -- BASELINE config 5's
precision -- as native programs of this repo's kernels: every convolution of the network in the
arrangement of the reference's only fp16 route, CudnnConvOp<float16> with fp32 math
(caffe2/caffe2/operators/conv_op_cudnn.cc:631-636, :1115-1124), for the networks of
detectron/lib/modeling/ResNet.py:85-130,221-283 and FPN.py:116-250.

Mixed precision in the usual arrangement (head_pipeline.DistillHeadsF16): fp32 master
parameters, momentum and parameter gradients (NativeResNetFPN's flat buffers, SGD and all-reduce
unchanged); filters re-rounded to fp16 every step; activations and their gradients
channel-blocked fp16, Xb[n][c/8][y][x][8]; gradients carry the subnets' dynamic loss scale S and
every filter / bias gradient is multiplied by 1/S on its way into the fp32 buffers.

Kernels:
  * pointwise layers (bottleneck 1x1s, projection shortcuts, laterals): gemm_f16.hip -- bias,
    shortcut Sum, ReLU, FPN's top-down upsample + Sum (forward) and the ReluGradient mask / gradient
    Sum (data gradient) in the epilogue; filter gradient = conv3x3_wgrad_f16_kernel<true>;
  * 3x3 / stride 1: conv3x3_f16.hip (forward, masked data gradient, filter + bias gradient);
  * ResNeXt's grouped 3x3 (the X-101-64x4d teacher): grouped_f16.hip, forward; with wide_groups=True also the
    X-101-32x8d teacher, whose three 64-wide res5 layers take that file's 64-wide entry points;
  * stride-2 3x3 layers (P6, P7, ResNeXt's first blocks): the stride-1 layer + the even positions;
  * the 7x7 / 2 stem: the fp32 implicit GEMM on the fp32 image (Cin = 3), then bias + ReLU +
    3x3 / 2 max pool written blocked fp16 (ssad_stem_pool_f16);
  * everything else: one-slot-per-thread passes on blocked tensors (ssad_f16_elementwise).
"""
import torch

from . import kernels as K
from . import program as PR
from .backbone_pipeline import NativeResNetFPN
from .engines import emit_conv3x3_f16, emit_conv3x3_wgrad_f16, emit_f16_packs

KL_PW, KL_C3, KL_W3, KL_W1, KL_GR, KL_EW, KL_PACK = 57, 58, 59, 60, 61, 62, 63


class NativeResNetFPNF16(NativeResNetFPN):
    """heads_io (optional): dict(fpn_out=[5 blocked fp16 tensors the FPN levels are written into],
    d_fpn_in=([5], [5]) the two blocked fp16 gradient sets to be summed (cls / bbox subnet),
    inv_scale=1-element float32 device tensor holding 1 / loss scale).  Without it the network owns
    its FPN outputs (self.fpn, blocked fp16) and gradient inputs (self.d_fpn).
    wide_groups: accept a ResNeXt whose res5 groups are 64 wide (x101-32x8d): those layers get the GROUPED_F16_CG64
    records, every narrower layer the records it always had.  Off by default (the architecture is then refused, as
    before); no effect on any other architecture.  Forward only, like every grouped fp16 network."""

    F16 = True

    def __init__(self, arch="r50", N=2, image_hw=(640, 896), device="cuda", train=True, heads_io=None,
                 wide_groups=False, **kw):
        self.wide_groups = bool(wide_groups)
        self._io = heads_io or {}
        super().__init__(arch, N, image_hw, device, train=train, **kw)

    # P6 / P7 always as the stride-1 layer + the even positions (NativeResNetFPN._emit_p6p7)
    _strided_own = False

    def _act(self, N, Cc, H, W):
        """Blocked fp16 activation [N][C/8][H][W][8].  (The image and the stem's convolution stay fp32: _t.)"""
        t = torch.empty((N, (Cc + 7) // 8, H, W, 8), dtype=torch.float16, device=self.device)
        self._bufs.append(t)
        return t

    def poison(self, value=float("nan")):
        for t in self._bufs:
            t.fill_(value)
        self._packed_frozen = False

    # -- emit helpers ------------------------------------------------------------------------
    def _pw(self, P, x, w, y, Cc, M, bias=None, res=None, mask=None, relu=False, res_up=False, stride=1):
        d = K.PwF16()
        d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
        d.bias = bias.data_ptr() if bias is not None else None
        d.residual = res.data_ptr() if res is not None else None
        d.mask = mask.data_ptr() if mask is not None else None
        d.N, d.C, d.M = y.shape[0], Cc, M
        d.Ho, d.Wo, d.Hi, d.Wi, d.stride = y.shape[2], y.shape[3], x.shape[2], x.shape[3], stride
        d.flags = (K.CONV_RELU if relu else 0) | (K.PW_F16_RES_UPSAMPLE2 if res_up else 0)
        px = y.shape[0] * y.shape[2] * y.shape[3]
        P.add(PR.PW_F16, KL_PW, p=(d,), work=2.0 * px * Cc * M,
              keep=[t for t in (x, w, y, bias, res, mask) if t is not None])

    def _conv3(self, P, probs, Cout, Cin, flags, engine=None, fold=False):
        """probs: [(x, y, mask or None, packed, bias or None)]: independent 3x3 convolutions of one
        (Cout, Cin) in one launch (conv3x3_f16_kernel: one engine, no |max| words)."""
        emit_conv3x3_f16(P, KL_C3, probs, Cin, Cout, flags)

    def _ew16(self, P, mode, a, b, y, Cc, stride=1, acc=0):
        P.add(PR.F16_EW, KL_EW, i=(mode, y.shape[0], Cc, y.shape[2], y.shape[3], stride, acc), p=(a, b, y),
              work=2.0 * (y.numel() + a.numel() + (b.numel() if b is not None else 0)))

    def _wgrad3(self, P, x, dy, layer):
        emit_conv3x3_wgrad_f16(P, KL_W3, [x], [dy], layer.gw, layer.gb, layer.cin, layer.cout, self.inv_scale,
                               self._aux)

    def _wgrad1(self, P, x, dy, layer):
        """Filter gradient of a pointwise layer; the kernel sums the bias gradient of a layer that has one."""
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        nb = K.lib().ssad_conv1x1_wgrad_f16_workspace_bytes(N, layer.cin, H, W, layer.cout)
        stream, ws = self._aux(P)
        P.add(PR.PW_F16_WGRAD, KL_W1, i=(N, layer.cin, H, W, layer.cout, 0), f=(1.0,), l=(nb,),
              p=(x, dy, self.inv_scale, layer.gw, layer.gb, ws.need(nb)),
              work=2.0 * N * H * W * layer.cin * layer.cout, keep=[x, dy], stream=stream)

    # -- the operations of NativeResNetFPN's walk of the network, in fp16 storage ---------------------------------
    # Sums go to a fresh buffer, never in place: an auxiliary stream may still be reading the operands.
    def _stem_pool(self, P, st, z, y):
        N, Cc, oh, ow = z.shape
        P.add(PR.STEM_POOL_F16, KL_EW, i=(N, Cc, oh, ow), p=(z, st.b, y), work=4.0 * z.numel() + 2.0 * y.numel())

    def _subsample(self, P, x, y, Cc, stride):
        self._ew16(P, K.EW_SUBSAMPLE, x, None, y, Cc, stride=stride)

    def _subsample_grad(self, P, dy, dx, Cc, stride, acc=False):
        self._ew16(P, K.EW_SUBSAMPLE_GRAD, dy, None, dx, Cc, stride=stride, acc=int(acc))

    def _relu(self, P, x, y, Cc):
        self._ew16(P, K.EW_RELU, x, None, y, Cc)

    def _relu_grad(self, P, y, dy, dz, Cc):
        self._ew16(P, K.EW_RELU_GRAD, y, dy, dz, Cc)

    def _sum2(self, P, a, b, Cc):
        s = self._like(a)
        self._ew16(P, K.EW_SUM2, a, b, s, Cc)
        return s

    def _topdown_grad(self, P, fine, coarse):
        s = self._like(coarse)
        self._ew16(P, K.EW_UPSAMPLE_GRAD, fine, coarse, s, self.D)
        return s

    def _pointwise(self, P, l, x, y, res=None, relu=False):
        self._pw(P, x, l.pf, y, l.cin, l.cout, bias=l.b, res=res, relu=relu)

    def _lateral(self, P, l, c, t, top=None):
        """The top-down upsample + Sum in the GEMM's epilogue (FPN.py:283-306)."""
        self._pw(P, c, l.pf, t, l.cin, l.cout, bias=l.b, res=top, res_up=top is not None)

    def _pointwise_grad(self, P, l, dy, like=None, mask=None, res=None, into=None, fold=False):
        """The gradient `into` holds goes in as the residual operand; the result is a new buffer either way."""
        assert res is None or into is None
        dx = self._like(like if into is None else into)
        self._pw(P, dy, l.pd, dx, l.cout, l.cin, res=res if into is None else into, mask=mask)
        return dx

    def _grouped3(self, P, l, x, y):
        """The stride-1 layer into a full-size buffer, then every stride-th position (ReLU commutes with that)."""
        N, Cc, H, W = self.N, l.cin, x.shape[2], x.shape[3]
        yf = y if l.stride == 1 else self._act(N, Cc, H, W)
        P.add(PR.GROUPED_F16_CG64 if l.wcin == 64 else PR.GROUPED_F16, KL_GR, i=(N, Cc, H, W, l.group, 1),
              p=(x, l.pf, l.b, yf), work=2.0 * 9 * Cc * l.wcin * N * H * W, keep=[x, yf])
        if l.stride != 1:
            self._subsample(P, yf, y, Cc, l.stride)

    def _fpn_level(self, k, h, w):
        outs = self._io.get("fpn_out")
        return outs[k] if outs is not None else self._act(self.N, self.D, h, w)

    def _fpn_grads(self, P):
        """(Times the loss scale.)  With heads_io the program sums the two subnets' parts itself."""
        d_fpn = super()._fpn_grads(P)
        din = self._io.get("d_fpn_in")
        if din is not None:
            for a, b, d in zip(din[0], din[1], d_fpn):
                self._ew16(P, K.EW_SUM2, a, b, d, self.D)
        return d_fpn

    def _emit_p6p7(self, P, c5):
        if c5.shape[2] % 4 or c5.shape[3] % 4:
            raise K.KernelError("fp16 backbone: P6 / P7 need even res5 / P6 maps")
        return super()._emit_p6p7(P, c5)

    # -- program construction --------------------------------------------------------------------
    def _build(self):
        self._aux_streams()
        L, dev, lib = self._layers, self.device, K.lib()
        inv = self._io.get("inv_scale")
        self.inv_scale = inv if inv is not None else torch.ones(1, dtype=torch.float32, device=dev)
        prep, P = PR.Program(), PR.Program()
        self.prep, self.prog = prep, P
        P.mark("pack")
        h16 = dict(dtype=torch.float16, device=dev)
        # every fp16 filter of a program in ONE launch (ssad_f16_pack_filters): as 111 launches of 5-13 us (R-101
        # student) they were a serial chain at the head of every step
        packs = {True: [], False: []}              # trainable (every step) / frozen (once): (w, wf, wd, M, C, taps)
        for l in L.values():
            tgt = P if l.train else prep
            if l.k == 1 or (l.k == 3 and l.group == 1):
                n = (lib.ssad_pw_f16_filter_halves if l.k == 1 else lib.ssad_f16_filter_halves)(l.cout, l.cin)
                l.pf = torch.empty(n, **h16)
                l.pd = torch.empty(n, **h16) if l.train else None
                packs[bool(l.train)].append((l.w, l.pf, l.pd, l.cout, l.cin, 1 if l.k == 1 else 9))
            elif l.k == 3:
                cg64 = l.wcin == 64                                  # (only behind wide_groups: check_f16_grouped)
                n = (lib.ssad_grouped_conv3x3_f16_cg64_filter_halves if cg64
                     else lib.ssad_grouped_conv3x3_f16_filter_halves)(l.cout, l.group)
                l.pf = torch.empty(n, **h16)
                tgt.add(PR.GROUPED_F16_CG64_PACK if cg64 else PR.GROUPED_F16_PACK, KL_PACK, i=(l.cout, l.group),
                        p=(l.w, l.pf), work=4.0 * l.w.numel() + 2.0 * n)
            else:                                                    # stem: fp32 [147][64] (Cin = 3)
                l.wt = self._t(l.cin * l.k * l.k, l.cout)
                tgt.add(PR.TRANSPOSE_FILTER, 54, i=(l.cout, l.cin * l.k * l.k, l.cout), p=(l.w, l.wt),
                        work=8.0 * l.w.numel())
        for train, tgt in ((True, P), (False, prep)):
            emit_f16_packs(tgt, KL_PACK, packs[train])
        prep.build()
        self._packed_frozen = False
        P.mark("forward")
        self._emit_passes(P)
        self._bind_workspaces()
        P.build()

    # -- running (fp32 NCHW views for tests and callers outside the fp16 domain) ----------------------
    def fpn_f32(self):
        """The five FPN levels as float32 NCHW tensors (a conversion, not part of the step)."""
        return [K.f16_unpack_activations(p, self.D) for p in self.fpn]

    def backward(self, d_fpn=None, scale=1.0):
        """d_fpn: optional float32 NCHW gradients (they are rounded to blocked fp16 times `scale`);
        with heads_io the program sums the subnets' blocked gradients itself."""
        if d_fpn is not None:
            for dst, src in zip(self.d_fpn, d_fpn):
                K.f16_pack_activations(src, scale, out=dst)
        super().backward()
