"""ResNet-FPN backbone (row f1) as a native program of this repo's kernels -- forward, backward
through res3..res5 + FPN, and the SGD update, with no torch operator in the step.

Structure of the network: detectron/lib/modeling/ResNet.py:85-130,221-283 (bottleneck stages
3-4-{6,23}-3, stride on the first 1x1 as with the MSRA weights, frozen BN = AffineChannel,
folded into the convolution that precedes it: W' = s W, bias = b; stem + res2 frozen,
TRAIN.FREEZE_CONV_BODY / FREEZE_AT = 2).  The body's convolutions have no bias of their own
(ResNet.py:270-283, no_bias=1) and AffineChannel's scale and bias are never trained
(caffe2/modules/detectron/affine_channel_op.cc: the gradient operator produces dX only), so
here the folded biases of res3..res5 are frozen values, not parameters, and the update of a
folded filter multiplies its gradient rows by s^2 (ssad_sgd_segment.row_scale) -- W' = s W
then follows the reference's update of W exactly: s (W - lr (s dW' + wd W)) = W' - lr (s^2 dW'
+ wd W').  Only the FPN's own convolutions (FPN.py:116-250) carry trained biases. and FPN.py:116-250 for RetinaNet (laterals on
res3..res5, top-down nearest upsampling + Sum, 3x3 output convs, P6 = conv3x3/2 on res5,
P7 = conv3x3/2 on relu(P6)).

Kernels:
  * every pointwise convolution (bottleneck 1x1s, projection shortcuts, laterals): the fp32-MFMA
    GEMM of csrc/kernels/gemm_conv.hip with bias / shortcut Sum / ReLU in its epilogue (forward),
    the ReluGradient mask and gradient accumulation in its epilogue (data gradient), and the
    split-reduction filter gradient;
  * every 3x3 / stride 1 convolution: the Winograd engine of the subnets (forward, data
    gradient with the fused ReluGradient mask, filter + bias gradient);
  * the stride-2 pointwise layers run on ssad_subsample's output (shared by c1 and the
    projection); P6 / P7 (3x3 / stride 2) run at their own size: implicit GEMM with split-K forward,
    flattened-batch GEMMs + gather-form col2im for the gradients (csrc/kernels/conv_strided.hip;
    SSAD_STRIDED_3X3=winograd: the stride-1 Winograd layer + subsampling of rounds 1-2, 4x the flops);
  * the 7x7 / stride 2 stem: an implicit GEMM (K = 147, no column buffer), then bias + ReLU + 3x3/2 max pool
    in one pass (ssad_max_pool3x3s2_bias_relu).

_emit_forward / _emit_backward are the one statement of the network for both precisions: what is computed in which
order.  How an operation is emitted is a method ("the operations of the walk"); backbone_f16.NativeResNetFPNF16
overrides those and defines no walk of its own.

All activations, gradients and packed filters are allocated once; the step is
Program.run() calls (ssad_program_run) -- a few segments when data parallel, so that a stage's
gradient bucket is all-reduced while the earlier stages are still in backward.
"""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import kernels as K
from . import program as PR
from .data_parallel import BucketedAllReduce
from .engines import (AmaxTable, Engine, Switches, backbone_engine, backbone_wgrad_split, emit_conv3x3,
                      emit_conv3x3_wgrad, emit_packs, emit_sgd_flat, filter_floats, same_engine)
from .modeling.resnet_fpn import ChannelRatioError, channel_widths

# pixels (all images) a pointwise launch needs before the split-operand GEMM pays (see NativeResNetFPN._gemm)
GEMM_SPLIT_MIN_PIXELS = 8192

ARCHS = {"r50": (3, 4, 6, 3), "r101": (3, 4, 23, 3), "x101-64x4d": (3, 4, 23, 3), "x101-32x8d": (3, 4, 23, 3)}
# ResNeXt (ResNet.py:247-258): name -> (groups, width per group); the stride sits on the 3x3
# (RESNETS.STRIDE_1X1 = False).  By default forward only: the frozen teachers of BASELINE config 5 (64x4d) and of the
# reference's retinanet_X-101-32x8d-FPN configurations (groups 8, 16, 32 and 64 channels wide at res2..res5); trained
# with NativeResNetFPN(..., grouped_grad=True).
GROUPED = {"x101-64x4d": (64, 4), "x101-32x8d": (32, 8)}


def check_f16_grouped(arch, wide_groups=False):
    """The fp16-storage backbone's grouped 3x3 (grouped_f16.hip) serves groups of up to 32 channels; a ResNeXt whose
    res5 groups (8 x width per group) are wider is an fp32 network only -- unless wide_groups asks for the 64-wide
    entry points (ssad_grouped_conv3x3_f16_cg64), which take res5 groups of exactly 64.  Raises KernelError; touches no
    device."""
    if arch in GROUPED and 8 * GROUPED[arch][1] > (64 if wide_groups else 32):
        raise K.KernelError("native backbone: %s has no fp16-storage backbone: the fp16 grouped kernel stops at "
                            "32-wide groups and its res5 groups are %d wide; use the fp32 backbone"
                            % (arch, 8 * GROUPED[arch][1]))


def student_widths(arch, channel_ratio, fpn_dim=256):
    """Widths of a network of RESNETS.CHANNEL_RATIO = channel_ratio (modeling.resnet_fpn.channel_widths: the
    reference's expressions, truncation included) after the checks that need no device: a ratio other than 1 is for
    the plain ResNets (the grouped 3x3 kernel is written for the ResNeXt teacher's widths) and must give widths that
    are positive multiples of 16.  Raises KernelError."""
    if arch not in ARCHS:
        raise K.KernelError("native backbone: architectures %s" % sorted(ARCHS))
    groups, width = GROUPED.get(arch, (1, 64))
    if float(channel_ratio) != 1.0 and arch in GROUPED:
        raise K.KernelError("native backbone: channel_ratio %r with the grouped architecture %s is not supported "
                            "(the grouped 3x3 kernel serves the full-width ResNeXt teacher only)" % (channel_ratio, arch))
    try:
        return channel_widths(channel_ratio, groups, width, fpn_dim)
    except ChannelRatioError as e:
        raise K.KernelError("native backbone: %s" % e)


class _Layer(object):
    __slots__ = ("name", "k", "cin", "cout", "stride", "train", "group", "affine", "w", "b", "gw", "gb", "wt",
                 "pf", "pd", "s2", "engine")

    def __init__(self, name, k, cin, cout, stride, train, group=1, affine=False):
        self.name, self.k, self.cin, self.cout, self.stride, self.train = name, k, cin, cout, stride, train
        self.group = group
        self.affine = affine       # followed by a frozen AffineChannel (folded): the bias is not a parameter
        self.w = self.b = self.gw = self.gb = self.wt = self.pf = self.pd = self.s2 = None
        self.engine = None         # engines.Engine of an ungrouped stride-1 3x3 layer (forward and data gradient)

    @property
    def wcin(self):
        """Input channels one filter sees ([cout][cin / group][k][k], conv_op_impl.h:43-47)."""
        return self.cin // self.group


class NativeResNetFPN(object):
    def __init__(self, arch="r50", N=2, image_hw=(640, 896), device="cuda", train=True, src=None,
                 fpn_dim=256, lr=1e-5, momentum=0.9, weight_decay=1e-4, process_group=None, world_size=1,
                 affine_scales=None, skip_flag=None, overlap_wgrad=None, channel_ratio=1.0, grouped_grad=False):
        """channel_ratio: RESNETS.CHANNEL_RATIO (ResNet.py:99-124, FPN.py:122,501), the width multiplier of a thin
        student; fpn_dim is FPN.DIM before the ratio, self.D = int(fpn_dim * channel_ratio) what the network builds
        (and the subnets inherit).  The stem stays 64 wide.
        grouped_grad: allow train=True on a grouped architecture (a ResNeXt student: the grouped 3x3 layers of
        res3..res5 get the data and filter gradients of grouped_conv3x3_grad.hip).  Off by default: a ResNeXt is then
        the frozen teacher only, as before.  No effect on the plain ResNets; fp32 backbone, channel_ratio 1 only."""
        if grouped_grad and getattr(self, "F16", False):
            raise K.KernelError("native backbone: grouped_grad with the fp16-storage backbone is not supported (the "
                                "grouped 3x3 gradient kernels are fp32); use the fp32 backbone")
        if float(channel_ratio) != 1.0 and getattr(self, "F16", False):
            raise K.KernelError("native backbone: channel_ratio %r with the fp16-storage backbone is not supported "
                                "(backbone_f16's kernels were written for the full widths); use the fp32 backbone"
                                % (channel_ratio,))
        self.widths = student_widths(arch, channel_ratio, fpn_dim)       # (before anything touches the library)
        if getattr(self, "F16", False):
            check_f16_grouped(arch, getattr(self, "wide_groups", False))
        self.channel_ratio = float(channel_ratio)
        self.grouped_grad = bool(grouped_grad)
        if arch in GROUPED and train and not grouped_grad:
            raise K.KernelError("native backbone: %s is forward only (the frozen teacher); its grouped 3x3 has no "
                                "gradient kernels" % arch)
        self.arch, self.N, self.hw, self.device, self.train = arch, N, tuple(image_hw), device, train
        self.D = self.widths.fpn_dim
        self.momentum, self.weight_decay = momentum, weight_decay
        self.dp = BucketedAllReduce(process_group, world_size)
        self.timing = None
        H, W = self.hw
        if H % 128 or W % 128:
            raise K.KernelError("native backbone: image sides must be multiples of 128 (16-pixel-multiple "
                                "maps down to res5; 640x896 and 512x768 are)")
        self._layers = OrderedDict()
        self._bufs = []
        self._define_layers()
        self._alloc_params(src, affine_scales)
        self.lr = torch.full((1,), lr, dtype=torch.float32, device=device)
        # device int (or None): when non-zero at execution time the update is dropped (a
        # mixed-precision step whose gradients overflowed, head_pipeline.DistillHeadsF16)
        self.skip_flag = skip_flag
        self._overlap_wgrad = overlap_wgrad
        self.switches = Switches.read()           # the one read of the engine switches
        self._build()

    @classmethod
    def layer_shapes(cls, arch, channel_ratio=1.0, fpn_dim=256):
        """{layer name: filter shape (cout, cin / group, k, k)} of the network, without building it (utils/net.py
        checks a weights file against it before anything is allocated)."""
        nat = cls.__new__(cls)
        nat.arch, nat.train = arch, False
        nat.widths = student_widths(arch, channel_ratio, fpn_dim)
        nat.D = nat.widths.fpn_dim
        nat._layers = OrderedDict()
        nat._define_layers()
        return OrderedDict((n, (l.cout, l.wcin, l.k, l.k)) for n, l in nat._layers.items())

    # -- network definition -------------------------------------------------------------
    def _define_layers(self):
        L = self._layers

        def add(name, k, cin, cout, stride=1, train=True, group=1):
            L[name] = _Layer(name, k, cin, cout, stride, train and self.train, group,
                             affine=name.startswith(("stem", "res")))
        groups, width = GROUPED.get(self.arch, (1, 64))
        wd = getattr(self, "widths", None) or channel_widths(1.0, groups, width, self.D)
        add("stem.0", 7, 3, wd.stem, 2, train=False)
        cin = wd.stem
        self.blocks = []                       # (stage, j, cin, cmid, cout, stride, has_proj, trainable)
        for si, nblk in enumerate(ARCHS[self.arch]):
            stage = si + 2
            cmid, cout = wd.inner[si], wd.stage[si]
            tr = stage > 2                     # FREEZE_AT = 2: the stem and res2 stay frozen
            for j in range(nblk):
                # by stage index.  (ResNet.py:173-175 tells the first stage by dim_in == 64; at ratio 0.25 res2 also
                # leaves 64 channels and the reference's res3_0 gets stride 1 -- its levels then disagree with its own
                # anchor strides.  Not restated here: P3..P7 stay at strides 8..128.  DESIGN 3.13.)
                stride = 2 if (j == 0 and si > 0) else 1
                pre = "res%d.%d" % (stage, j)
                s1, s3 = (stride, 1) if groups == 1 else (1, stride)        # STRIDE_1X1
                add(pre + ".c1", 1, cin, cmid, s1, tr)
                add(pre + ".c2", 3, cmid, cmid, s3, tr, groups)
                add(pre + ".c3", 1, cmid, cout, 1, tr)
                proj = cin != cout or stride != 1
                if proj:
                    add(pre + ".proj", 1, cin, cout, stride, tr)
                self.blocks.append((stage, j, cin, cmid, cout, stride, proj, tr and self.train))
                cin = cout
        for i, c in enumerate(reversed(wd.stage[1:])):           # res5, res4, res3
            add("lat.%d" % i, 1, c, self.D)
        for i in range(3):
            add("out.%d" % i, 3, self.D, self.D)
        add("p6", 3, wd.stage[3], self.D, 2)
        add("p7", 3, self.D, self.D, 2)

    def _bucket_order(self):
        """Trainable layers in the order the backward pass finishes them, grouped into the
        all-reduce buckets FPN, res5, res4, res3 ("backbone 4-6 buckets")."""
        groups = OrderedDict([("fpn", []), ("res5", []), ("res4", []), ("res3", [])])
        for name in ("p7", "p6", "out.0", "out.1", "out.2", "lat.0", "lat.1", "lat.2"):
            groups["fpn"].append(name)
        for stage in (5, 4, 3):
            n = ARCHS[self.arch][stage - 2]
            for j in range(n - 1, -1, -1):
                for part in ("c3", "proj", "c2", "c1"):
                    name = "res%d.%d.%s" % (stage, j, part)
                    if name in self._layers:
                        groups["res%d" % stage].append(name)
        return groups

    # Folded AffineChannel scale of the random initialisation: the last layer of every bottleneck
    # carries s = 0.25 (frozen-BN scales have no statistics with random weights; the damped residual
    # branch keeps activations O(1) through 16 / 33 blocks, the job a trained model's BN does).
    INIT_C3_SCALE = 0.25

    def _default_init(self):
        """Random weights of the network's shapes (there are no checkpoints on the box): He-normal
        filters (fan in) with zero bias for the body, Xavier-uniform for the FPN's own layers
        (FPN.py:116-250 uses XavierFill there).  Returns ({name.weight / name.bias: tensor},
        {name: folded affine scale})."""
        gen = torch.Generator().manual_seed(7)
        sd, scales = {}, {}
        for l in self._layers.values():
            shape = (l.cout, l.wcin, l.k, l.k)
            fan_in = l.wcin * l.k * l.k
            if l.affine:
                w = torch.randn(shape, generator=gen) * float(np.sqrt(2.0 / fan_in))
                if l.name.endswith(".c3"):
                    w *= self.INIT_C3_SCALE
                    scales[l.name] = self.INIT_C3_SCALE
            else:
                bound = float(np.sqrt(6.0 / (fan_in + l.cout * l.k * l.k)))
                w = (torch.rand(shape, generator=gen) * 2.0 - 1.0) * bound
            sd[l.name + ".weight"] = w
            sd[l.name + ".bias"] = torch.zeros(l.cout)
        return sd, scales

    def _alloc_params(self, src, affine_scales=None):
        """src: None (random initialisation), a {name.weight / name.bias: tensor} dict or a module
        whose state_dict() has those names (filters with the AffineChannel scale folded in);
        affine_scales: {layer name: s (float or [cout] tensor)} of the folded scales (default 1)."""
        dev = self.device
        L = self._layers
        scales = dict(affine_scales or {})
        # weights from outside (a checkpoint, utils/net.py): every trainable folded filter gets a scale slot, so
        # that load_from() can install other AffineChannel scales later without rebuilding the program.  The
        # random initialisation keeps slots only where its scale is not 1 (bench.py's path, unchanged).
        all_slots = src is not None or affine_scales is not None
        if src is None:
            sd, init_scales = self._default_init()
            for k, v in init_scales.items():
                scales.setdefault(k, v)
        else:
            sd = src if isinstance(src, dict) else src.state_dict()
            sd = {k: v.detach() for k, v in sd.items()}
            if any((l.name + ".weight") not in sd for l in L.values()):
                # a weights file that holds only part of the network (the reference's standard TRAIN.WEIGHTS
                # is an ImageNet body without fpn_* / retnet_* blobs): what it lacks keeps the initialisation
                init_sd, init_scales = self._default_init()
                for l in L.values():
                    if (l.name + ".weight") not in sd:
                        sd[l.name + ".weight"], sd[l.name + ".bias"] = init_sd[l.name + ".weight"], init_sd[l.name + ".bias"]
                        if l.name in init_scales:
                            scales.setdefault(l.name, init_scales[l.name])
        # the folded scales as given (utils/net.py writes them back as <conv>_bn_s when saving)
        self.affine_scale_values = {k: torch.as_tensor(v, dtype=torch.float32).reshape(-1).cpu().clone()
                                    for k, v in scales.items() if k in L and L[k].affine}
        groups = self._bucket_order() if self.train else OrderedDict()
        order = [L[n] for g in groups.values() for n in g]
        assert all(l.train for l in order) and (not self.train or len(order) == sum(l.train for l in L.values()))

        # frozen values: filters + biases of frozen layers, and the folded affine biases of the
        # trainable body layers
        def fsize(l):
            return (0 if l.train else l.cout * l.wcin * l.k * l.k) + (l.cout if (not l.train or l.affine) else 0)

        f32 = dict(dtype=torch.float32, device=dev)
        self.frozen_flat = torch.empty(sum(fsize(l) for l in L.values()), **f32)
        off = 0
        for l in L.values():
            if not l.train:
                nw = l.cout * l.wcin * l.k * l.k
                l.w = self.frozen_flat[off:off + nw].view(l.cout, l.wcin, l.k, l.k)
                off += nw
            if not l.train or l.affine:
                l.b = self.frozen_flat[off:off + l.cout]
                off += l.cout
        n_train = sum(l.cout * l.wcin * l.k * l.k + (0 if l.affine else l.cout) for l in order)
        self.params_flat = torch.empty(n_train, **f32)
        self.grads_flat = torch.zeros(n_train, **f32)
        self.moms_flat = torch.zeros(n_train, **f32)
        self.bucket, self.segments = OrderedDict(), []
        off = 0
        for gname, names in groups.items():
            start = off
            for n in names:
                l = L[n]
                nw = l.cout * l.wcin * l.k * l.k
                l.w = self.params_flat[off:off + nw].view(l.cout, l.wcin, l.k, l.k)
                l.gw = self.grads_flat[off:off + nw].view(l.cout, l.wcin, l.k, l.k)
                sc = scales.get(n)
                if sc is None and all_slots and l.affine:
                    sc = 1.0
                if sc is not None and l.affine:
                    sc = torch.as_tensor(sc, dtype=torch.float32).reshape(-1).to(dev)
                    l.s2 = (sc * sc).expand(l.cout).contiguous() if sc.numel() == 1 else (sc * sc).contiguous()
                self.segments.append((off, nw, 0, l.wcin * l.k * l.k, l.s2))
                off += nw
                if not l.affine:
                    l.b = self.params_flat[off:off + l.cout]
                    l.gb = self.grads_flat[off:off + l.cout]
                    self.segments.append((off, l.cout, 1, 0, None))
                    off += l.cout
            self.bucket[gname] = self.grads_flat[start:off]
        for l in L.values():
            l.w.copy_(sd[l.name + ".weight"].to(device=dev, dtype=torch.float32))
            l.b.copy_(sd[l.name + ".bias"].to(device=dev, dtype=torch.float32))

    def load_from(self, src, affine_scales=None, strict=True):
        """Copy parameters from a {name.weight / name.bias: tensor} dict or a module with such a
        state_dict() (filters with the AffineChannel scale folded in).  strict=False: a layer the
        dict does not hold keeps its current values (detectron/lib/utils/net.py:96-99 logs
        "<name> not found" and leaves the initialised blob alone).  affine_scales: {layer: s} of
        the folded scales when they differ from the ones the network was built with -- the update of
        a trainable folded filter multiplies its gradient rows by s^2 (see the module docstring), so
        the network needs a scale slot for that layer (built with src= / affine_scales=)."""
        sd = src if isinstance(src, dict) else src.state_dict()
        for l in self._layers.values():
            if not strict and (l.name + ".weight") not in sd:
                continue
            l.w.copy_(sd[l.name + ".weight"].detach().to(device=self.device, dtype=torch.float32))
            l.b.copy_(sd[l.name + ".bias"].detach().to(device=self.device, dtype=torch.float32))
        if affine_scales is not None:
            for name, sc in affine_scales.items():
                l = self._layers.get(name)
                if l is None or not l.affine:
                    raise K.KernelError("load_from: %r is not a layer followed by an AffineChannel" % (name,))
                sc = torch.as_tensor(sc, dtype=torch.float32).reshape(-1)
                if sc.numel() == 1:
                    sc = sc.expand(l.cout)
                if sc.numel() != l.cout:
                    raise K.KernelError("load_from: %d scales for the %d channels of %s" % (sc.numel(), l.cout, name))
                self.affine_scale_values[name] = sc.cpu().clone()
                if not l.train:
                    continue
                if l.s2 is None:
                    if bool((sc == 1).all()):
                        continue
                    raise K.KernelError("load_from: %s has no scale slot (the network was built from the random "
                                        "initialisation); build it with src= / affine_scales=" % name)
                l.s2.copy_((sc * sc).to(self.device))
        self._packed_frozen = False

    # -- small emit helpers -------------------------------------------------------------------
    def _t(self, *shape):
        t = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._bufs.append(t)
        return t

    def _like(self, t):
        u = torch.empty_like(t)
        self._bufs.append(u)
        return u

    def _act(self, N, Cc, H, W):
        """An activation or gradient buffer of the network in this precision's layout: here NCHW fp32."""
        return self._t(N, Cc, H, W)

    # |max| words of the split-operand engines (engines.AmaxTable): one word per tensor.  The producers of the forward
    # pass fold (every activation is written exactly once there) and, in the backward pass, those of the three gradients
    # inside a bottleneck block (fold=True at their call sites); the other gradient buffers are also summed in place by
    # element-wise kernels, which would leave a folded word stale: their first split-engine reader measures them.
    AMAX_WORDS = 4096

    def poison(self, value=float("nan")):
        """Fill every activation / gradient / scratch buffer (debugging aid: anything the step
        reads before it writes shows up as NaN in the results)."""
        for t in self._bufs:
            t.fill_(value)
        for w in self.wss.values():
            w.view(torch.float32)[: w.numel() // 4].fill_(value)
        self._packed_frozen = False

    def _gemm(self, P, a, lda, x, y, Kc, M, bias=None, res=None, mask=None, relu=False, acc=False, klass=50, final=True,
              fold=False):
        """final=False: y is modified in place afterwards (the top-down sum of the FPN): its |max| is not folded in.
        fold=True: a backward-pass output that is written once and read only by split-engine calls (the gradients inside
        a bottleneck block): folded like a forward activation."""
        d = K.gemm_conv_desc(a, lda, x, y, Kc, M, bias, res, mask, relu, acc)
        px = x.numel() // Kc
        # SSAD_SPLIT_CONV bit 128: the compute-bound pointwise layers (K, M >= 256: res4, res5, the laterals) on the
        # split-operand GEMM that splits x on the fly (gemm_split.hip, gemm_fly_kernel).  (With a split PASS over x in
        # front of the GEMM the step got 1.2-1.5 ms slower, profiles/r06_experiments.md section 3.)  Thresholds from
        # same-box A/B pairs: K, M >= 128 costs the step +1.6 ms, >= 64 +3.2 ms (those layers are HBM-bound); at batch 2
        # (config 2: < 8192 pixels per launch from res4 up) the call's three extra small launches cost more than the
        # GEMM saves (+1.0 ms on a 12 ms step).
        if self.switches.split_conv & 128 and Kc >= 256 and M >= 256 and px >= GEMM_SPLIT_MIN_PIXELS and klass == 50:
            nb = K.lib().ssad_conv1x1_gemm_split_workspace_bytes(C.byref(d))
            if nb:
                am = self._amax
                xa = am.addr(am.measure(P, [[x]], Kc))
                ya = am.addr(am.reserve([[y]])) if (self._fwd or fold) and final and not acc else None
                P.add(PR.GEMM_CONV_SPLIT, 71, p=(d, self._split.need(nb), self._packed_a(a, lda, Kc, M), xa, ya),
                      l=(nb,), work=2.0 * px * Kc * M, keep=[t for t in (a, x, y, bias, res, mask) if t is not None])
                return
        P.add(PR.GEMM_CONV, klass, p=(d,), work=2.0 * px * Kc * M,
              keep=[t for t in (a, x, y, bias, res, mask) if t is not None])

    def _packed_a(self, a, lda, Kc, M):
        """The split copy of a pointwise filter operand a[Kc][lda] (made by the program's one GEMM_SPLIT_PACK op: per
        step for a trained layer, once for a frozen one)."""
        key = (a.data_ptr(), lda, Kc, M)
        if key not in self._gemm_packs:
            dst = self._t(K.lib().ssad_gemm_split_filter_floats(Kc, M))
            train = self._a_train[a.data_ptr()]
            self._gemm_packs[key] = dst
            (self._gpack_train if train else self._gpack_frozen).append((a, lda, Kc, M, dst))
        return self._gemm_packs[key]

    # timing class of a 3x3 launch by (trained network?, engine)
    KLASS3 = {(True, Engine.DIRECT): 18, (True, Engine.F22): 48, (True, Engine.F24): 46, (True, Engine.SPLIT): 66,
              (False, Engine.DIRECT): 18, (False, Engine.F22): 48, (False, Engine.F24): 47, (False, Engine.SPLIT): 67}

    def _conv3(self, P, probs, Cout, Cin, flags, engine, fold=False):
        """probs: [(x, y, mask or None, packed, bias or None)]: independent 3x3 convolutions of one (Cout, Cin) in one
        launch on one engine."""
        emit_conv3x3(P, self.KLASS3[self.train, engine], probs, Cout, Cin, flags, engine, self._amax, self._split,
                     fold=self._fwd or fold)

    def _wgrad3(self, P, x, dy, layer):
        emit_conv3x3_wgrad(P, (49, 70), [x], [dy], layer.gw, layer.gb, layer.cout, layer.cin,
                           backbone_wgrad_split(self.switches, layer.cout, layer.cin), self._amax, self._aux)

    def _emit_grouped_packs(self, P, layers):
        """One GROUPED_PACKS record: the forward and data-gradient packs of every trained grouped layer."""
        tab = self._grouped_pack_table = K.grouped_pack_entries([(l.w, l.pf, l.pd, l.cout, l.group) for l in layers])
        P.add(PR.GROUPED_PACKS, 77, i=(len(layers),), p=(tab,),
              work=4.0 * sum(l.w.numel() + l.pf.numel() + l.pd.numel() for l in layers),
              keep=[t for l in layers for t in (l.w, l.pf, l.pd)])

    def _wgrad_grouped(self, P, x, dy, layer):
        """Filter gradient of a grouped 3x3 layer (x: what the layer read, at its own size; dy at the output's): on an
        auxiliary stream like the others.  No bias gradient: the folded AffineChannel bias is frozen."""
        N, Cc, H, W = x.shape
        nb = K.lib().ssad_grouped_conv3x3_wgrad_workspace_bytes(N, Cc, H, W, layer.group, layer.stride)
        if not nb:
            raise K.KernelError("native backbone: %s: the grouped filter gradient refuses N %d, %d channels in %d groups, "
                                "%d x %d, stride %d" % (layer.name, N, Cc, layer.group, H, W, layer.stride))
        stream, ws = self._aux(P)
        P.add(PR.GROUPED_WGRAD, 76, i=(N, Cc, H, W, layer.group, layer.stride), l=(nb,),
              p=(x, dy, layer.gw, ws.need(nb)), keep=[x, dy],
              work=2.0 * 9 * Cc * layer.wcin * N * dy.shape[2] * dy.shape[3], stream=stream)

    def _dgrad_grouped(self, P, dy, dx, relu_x, layer):
        """dx = ReluGradient(relu_x, grouped 3x3 data gradient of dy); H, W are dx's (the layer's input).  The kernel
        folds no |max| word: dx's split-engine readers measure it (AmaxTable.measure in _gemm / _wgrad1)."""
        N, Cc, H, W = dx.shape
        P.add(PR.GROUPED_DGRAD, 75, i=(N, Cc, H, W, layer.group, layer.stride), p=(dy, layer.pd, relu_x, dx),
              work=2.0 * 9 * Cc * layer.wcin * N * dy.shape[2] * dy.shape[3])

    def _wgrad1(self, P, x, dy, layer):
        """Filter gradient of a pointwise layer, and the bias gradient of one that trains its bias (the laterals)."""
        N, Cc = x.shape[0], x.shape[1]
        pix = x.shape[2] * x.shape[3]
        # SSAD_SPLIT_CONV bit 256: the compute-bound pointwise filter gradients (C, M >= 256, the launch's pixels as for
        # the forward GEMM) on the split-operand engine (gemm_split.hip, wpoint_split_kernel)
        split = (bool(self.switches.split_conv & 256) and Cc >= 256 and layer.cout >= 256
                 and N * pix >= GEMM_SPLIT_MIN_PIXELS and pix % 8 == 0)
        if split and not K.lib().ssad_conv1x1_wgrad_split_workspace_bytes(N, Cc, pix, layer.cout):
            split = False           # (a tensor of 2 GiB or more: the exact engine)
        size_fn = K.lib().ssad_conv1x1_wgrad_split_workspace_bytes if split else K.lib().ssad_conv1x1_wgrad_workspace_bytes
        nb = size_fn(N, Cc, pix, layer.cout)
        xa = da = None
        if split:            # (measured on the main stream, before the fork)
            xa = self._amax.addr(self._amax.measure(P, [[x]], Cc))
            da = self._amax.addr(self._amax.measure(P, [[dy]], layer.cout))
        stream, ws = self._aux(P)
        P.add(PR.CONV1X1_WGRAD, 72 if split else 52, i=(N, Cc, pix, layer.cout, 0, 1 if split else 0), l=(nb,),
              p=(x, dy, layer.gw, ws.need(nb), xa, da), work=2.0 * N * pix * Cc * layer.cout, keep=[x, dy], stream=stream)
        if layer.gb is not None:
            self._bias_grad(P, dy, layer)

    def _bias_grad(self, P, dz, layer, rowsum=None):
        """db[c] = sum over n, pixels of dz; from the [N][C] plane sums when a ReluGradient pass
        already produced them."""
        self._aux(P)
        if rowsum is not None:
            P.add(PR.CHANNEL_SUM, 51, i=(rowsum.shape[0], rowsum.shape[1], 1, 0), p=(rowsum, layer.gb),
                  work=4.0 * rowsum.numel(), stream=self._wstream)
        else:
            # plane sums with one workgroup per (image, channel) -- N x C workgroups instead of the C of
            # ssad_channel_sum -- then the sum over the images of the tiny [N][C] table
            N, Cc = dz.shape[0], dz.shape[1]
            rows = self._t(N, Cc)
            P.add(PR.RELU_GRAD_ROWSUM, 51, i=(N, Cc, dz.shape[2] * dz.shape[3]), p=(None, dz, None, rows),
                  work=4.0 * dz.numel(), stream=self._wstream, keep=[dz, rows])
            P.add(PR.CHANNEL_SUM, 51, i=(N, Cc, 1, 0), p=(rows, layer.gb), work=4.0 * rows.numel(),
                  stream=self._wstream)

    def _conv_s2(self, P, x, y, layer):
        """y = conv3x3 / stride 2 / pad 1 (x) + bias at the layer's own size (FPN.py:193-224)."""
        N, Cc, H, W = x.shape
        oh, ow = y.shape[2], y.shape[3]
        d = K.gemm_conv_desc(layer.wt, layer.cout, x, y, Cc * 9, layer.cout, bias=layer.b)
        d.P = oh * ow
        nb = K.lib().ssad_conv_implicit_gemm_workspace_bytes(N, layer.cout, Cc, H, W, 3, 2, 1)
        ws = self._t(max(nb // 4, 4))
        P.add(PR.CONV_IMPLICIT_WS, 64, i=(Cc, H, W, 3, 2, 1), p=(d, ws), l=(nb,),
              work=2.0 * 9 * Cc * layer.cout * N * oh * ow, keep=[layer.wt, x, y, layer.b])

    def _wgrad_s2(self, P, x, dy, layer):
        N, Cc, H, W = x.shape
        nb = K.lib().ssad_conv_kxk_wgrad_workspace_bytes(N, Cc, H, W, layer.cout, 3, 2, 1)
        assert nb > 0
        stream, ws = self._aux(P)
        P.add(PR.CONV_KXK_WGRAD, 65, i=(N, Cc, H, W, layer.cout, 3, 2, 1), l=(nb, 0), p=(x, dy, layer.gw, ws.need(nb)),
              keep=[x, dy], work=2.0 * 9 * Cc * layer.cout * N * dy.shape[2] * dy.shape[3], stream=stream)
        self._bias_grad(P, dy, layer)

    def _dgrad_s2(self, P, layer, dy, dx, mask=None):
        N, Cc, H, W = dx.shape
        nb = K.lib().ssad_conv_kxk_dgrad_workspace_bytes(N, Cc, H, W, layer.cout, 3, 2, 1)
        assert nb > 0
        if self._dgrad_ws is None or self._dgrad_ws.numel() * 4 < nb:
            self._dgrad_ws = self._t(nb // 4)          # main stream only: the two layers run one after the other
        P.add(PR.CONV_KXK_DGRAD, 64, i=(N, Cc, H, W, layer.cout, 3, 2, 1), l=(nb, 0),
              p=(layer.w, dy, dx, self._dgrad_ws, mask), keep=[dy, dx],
              work=2.0 * 9 * Cc * layer.cout * N * dy.shape[2] * dy.shape[3])

    def _aux(self, P):
        """Filter / bias gradients do not feed the data-gradient chain: they run on an auxiliary
        stream behind a FORK (everything they read has been enqueued on the main stream), so that
        they fill the last partial round of workgroups of the chain's kernels and vice versa.  They
        share one workspace, which is safe because they are serialised on that one stream; nothing
        they read is modified by the main stream before the segment's JOIN (gradients that meet are
        written to fresh buffers, not accumulated in place).  -> (the stream, its Workspace)"""
        self._wstream = self._wstreams[self._wnext % len(self._wstreams)]
        self._wnext += 1
        if self._wstream:
            P.fork(self._wstream)
        return self._wstream, self._aux_ws[self._wstream]

    def _ew(self, P, code, i=(), p=(), l=(), f=(), nbytes=0.0):
        P.add(code, 51, i=i, p=p, l=l, f=f, work=nbytes)

    # -- program construction ----------------------------------------------------------------------
    def _aux_streams(self):
        ov = self._overlap_wgrad
        on = os.environ.get("SSAD_OVERLAP_WGRAD", "1") == "1" if ov is None else ov
        # filter / bias gradients go round-robin over this many auxiliary streams (each with its own
        # workspace): the small reduce launch that ends one filter gradient then runs beside the next
        # one's main kernel instead of in front of it
        nws = 2      # 1 was indistinguishable, 3 worse
        self._wstreams = list(range(1, nws + 1)) if on else [0]
        self._wstream, self._wnext = self._wstreams[0], 0
        self._aux_ws = {k: PR.Workspace() for k in self._wstreams}
        # the split-engine launches of this network run one after the other on its main stream: one workspace
        self._split = PR.Workspace()

    def _emit_sgd(self, P):
        emit_sgd_flat(P, 55, self.segments, self.params_flat, self.grads_flat, self.moms_flat, self.lr, self.momentum,
                      self.weight_decay, self.skip_flag)

    def _bind_workspaces(self):
        self.wss = {k: w.bind(self.device) for k, w in self._aux_ws.items()}
        self.ws = self.wss[self._wstreams[0]]
        self.split_ws = self._split.bind(self.device)

    def _build(self):
        self._aux_streams()
        # FPN's stride-2 3x3 layers (P6, P7) at their own size: implicit GEMM with split-K forward, flattened-batch
        # GEMMs for the gradients (conv_strided.hip).  SSAD_STRIDED_3X3=winograd: rounds 1-2's stride-1 Winograd
        # layer + subsampling (4x the direct-form flops), kept for A/B runs.
        self._strided_own = os.environ.get("SSAD_STRIDED_3X3", "own") != "winograd"
        self._dgrad_ws = None
        L = self._layers
        lib = K.lib()
        # packed filters: frozen layers once (prepare program), trainable layers every step (pack segment)
        prep, P = PR.Program(), PR.Program()
        self.prep, self.prog = prep, P
        packs = {True: {}, False: {}}          # {trained?: {Engine: pack entries}}: P packs every step, prep once
        self._amax = AmaxTable(self.AMAX_WORDS, self.device)
        self.amax = self._amax.tensor
        self._gemm_packs, self._gpack_train, self._gpack_frozen, self._a_train = {}, [], [], {}
        tr_frozen, tr_train = [], []          # (w, wt, M, K, ldm): every transposed filter of a program in one launch
        gr_train = []                         # trained grouped 3x3 layers: their forward + data-gradient packs in one launch
        P.mark("pack")
        for l in L.values():
            tgt = P if l.train else prep
            trs = tr_train if l.train else tr_frozen
            if l.k == 1:
                ldm = (l.cout + 3) // 4 * 4
                l.wt = self._t(l.cin, ldm)
                trs.append((l.w, l.wt, l.cout, l.cin, ldm))
                self._a_train[l.wt.data_ptr()] = self._a_train[l.w.data_ptr()] = l.train
            elif l.k == 3 and l.group > 1 and l.train:           # ResNeXt student: both packs, every step, one launch
                l.pf = self._t(lib.ssad_grouped_conv3x3_filter_floats(l.cout, l.group))
                l.pd = self._t(lib.ssad_grouped_conv3x3_dgrad_filter_floats(l.cout, l.group))
                gr_train.append(l)
            elif l.k == 3 and l.group > 1:                       # ResNeXt: MFMA operand order, packed once
                l.pf = self._t(lib.ssad_grouped_conv3x3_filter_floats(l.cout, l.group))
                tgt.add(PR.GROUPED_PACK, 54, i=(l.cout, l.group), p=(l.w, l.pf), work=4.0 * (l.w.numel() + l.pf.numel()))
            elif l.k == 3 and l.stride == 2 and self._strided_own:
                # P6 / P7 at their own size: the implicit GEMM's [Cin * 9][Cout] operand (the data and filter
                # gradients read the filter in its natural layout)
                l.wt = self._t(l.cin * 9, l.cout)
                trs.append((l.w, l.wt, l.cout, l.cin * 9, l.cout))
            elif l.k == 3:
                l.engine = backbone_engine(self.switches, l.train, l.cout, l.cin)
                l.pf = self._t(filter_floats(l.engine)(l.cout, l.cin))
                # (every trainable 3x3 sends a gradient further down)
                l.pd = self._t(filter_floats(l.engine)(l.cin, l.cout)) if l.train else None
                packs[l.train].setdefault(l.engine, []).append((l.w, l.cout, l.cin, l.pf, l.pd))
            else:                                                    # stem: [147][64]
                l.wt = self._t(l.cin * l.k * l.k, l.cout)
                trs.append((l.w, l.wt, l.cout, l.cin * l.k * l.k, l.cout))
        # one launch per program for all transposes (ssad_transpose_filters): as 34 launches of ~5 us they were a
        # serial chain at the start of every step, each waiting for a CU slot behind the other stream's persistent
        # kernels (tools/step_timeline.py: the main stream sat idle for ~7 ms there)
        for tgt, trs in ((prep, tr_frozen), (P, tr_train)):
            if trs:
                tab = (K.TransposeEntry * len(trs))()
                for i, (w, wt, M, Kc, ldm) in enumerate(trs):
                    tab[i] = K.TransposeEntry(w.data_ptr(), wt.data_ptr(), M, Kc, ldm, 0)
                tgt.add(PR.TRANSPOSE_FILTERS, 54, i=(len(trs),), p=(tab,),
                        work=8.0 * sum(M * Kc for (_, _, M, Kc, _) in trs), keep=[t for e in trs for t in e[:2]])
        if gr_train:
            # as per-layer launches the two packs of an X-101's 30 trained grouped layers were a serial chain of 60
            # kernels of a few microseconds at the head of the step (the transposes' story above)
            self._emit_grouped_packs(P, gr_train)
        for tgt, train in ((prep, False), (P, True)):
            emit_packs(tgt, 54, packs[train], (Engine.F22, Engine.F24, Engine.SPLIT, Engine.DIRECT))
        # the pointwise filters' split copies (which layers need one is known once the passes are emitted: the table is
        # filled in below)
        gp_max = 2 * sum(1 for l in L.values() if l.k == 1)
        gtab = {True: (K.GemmPackEntry * max(gp_max, 1))(), False: (K.GemmPackEntry * max(gp_max, 1))()}
        gidx = {True: P.add(PR.GEMM_SPLIT_PACK, 74, i=(0,), p=(gtab[True],)),
                False: prep.add(PR.GEMM_SPLIT_PACK, 74, i=(0,), p=(gtab[False],))}
        self._packed_frozen = False
        P.mark("forward")
        P.add(PR.FILL, 51, p=(self.amax,), f=(0.0,), l=(self.AMAX_WORDS,), work=4.0 * self.AMAX_WORDS)
        self._emit_passes(P)
        for train, entries, prog in ((True, self._gpack_train, P), (False, self._gpack_frozen, prep)):
            for k, (a, lda, Kc, M, dst) in enumerate(entries):
                gtab[train][k] = K.GemmPackEntry(a.data_ptr(), dst.data_ptr(), lda, Kc, M)
            op = prog.ops[gidx[train]]
            op.i[0] = len(entries)
            op.work = 8.0 * sum(Kc * M for (_, _, Kc, M, _) in entries)
        prep.build()
        self._bind_workspaces()
        P.build()

    def _emit_passes(self, P):
        """The walk into P (behind the "forward" mark): forward, and for a trained network backward and the update."""
        self._fwd = True              # (every activation is written once there: its producer folds its |max| word)
        self._emit_forward(P)
        self._fwd = False
        P.mark("backward")
        if self.train:
            self._emit_backward(P)
            P.mark("sgd")
            self._emit_sgd(P)
        P.mark("end")

    # -- the operations of the walk, as this precision emits them (backbone_f16 overrides these) -------------------
    # An operation that sums or accumulates returns the tensor that holds the result -- here its in-place operand, in
    # fp16 a fresh buffer -- and the walk goes on with what it was handed.  Cc: the channels of the tensors (a blocked
    # fp16 tensor's shape does not tell).
    def _stem_pool(self, P, st, z, y):
        """y = 3x3 / 2 max pool of relu(z + bias)."""
        N, Cc, oh, ow = z.shape
        self._ew(P, PR.STEM_POOL, i=(N, Cc, oh, ow, 1), p=(z, st.b, y), nbytes=4.0 * 1.25 * z.numel())

    def _subsample(self, P, x, y, Cc, stride):
        """y = every stride-th position of x."""
        self._ew(P, PR.SUBSAMPLE, i=(self.N, Cc, x.shape[2], x.shape[3], stride), p=(x, y), nbytes=8.0 * y.numel())

    def _subsample_grad(self, P, dy, dx, Cc, stride, acc=False):
        """dx = dy at every stride-th position, zero elsewhere; acc: added to what dx holds."""
        self._ew(P, PR.SUBSAMPLE_GRAD, i=(self.N, Cc, dx.shape[2], dx.shape[3], stride, int(acc)), p=(dy, dx),
                 nbytes=(12.0 if acc else 4.0) * dx.numel())

    def _relu(self, P, x, y, Cc):
        self._ew(P, PR.RELU, p=(x, y), l=(x.numel(),), nbytes=8.0 * x.numel())

    def _relu_grad(self, P, y, dy, dz, Cc):
        """dz = ReluGradient(y, dy)."""
        self._ew(P, PR.RELU_GRAD, p=(y, dy, dz), l=(y.numel(),), nbytes=12.0 * y.numel())

    def _sum2(self, P, a, b, Cc):
        """a + b -> the tensor that holds the sum (a, in place)."""
        ptrs = (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())
        P.add(PR.SUM_N, 51, i=(2,), l=(a.numel(),), p=(ptrs, a), work=12.0 * a.numel(), keep=[a, b])
        return a

    def _topdown_grad(self, P, fine, coarse):
        """coarse + the 2 x 2 sums of fine (fine = lateral + up(coarse) in the forward pass) -> the tensor that holds it."""
        up = self._like(coarse)
        self._ew(P, PR.UPSAMPLE_GRAD, i=(self.N, self.D, coarse.shape[2], coarse.shape[3], 2), p=(fine, up),
                 nbytes=5.0 * fine.numel())
        return self._sum2(P, coarse, up, self.D)

    def _pointwise(self, P, l, x, y, res=None, relu=False):
        """y = W x + bias (+ res), through ReLU when asked."""
        self._gemm(P, l.wt, l.wt.shape[1], x, y, l.cin, l.cout, bias=l.b, res=res, relu=relu)

    def _lateral(self, P, l, c, t, top=None):
        """t = W c + bias (+ top, upsampled 2 x nearest: in place behind the GEMM)."""
        self._gemm(P, l.wt, l.wt.shape[1], c, t, l.cin, l.cout, bias=l.b, final=top is None)
        if top is not None:
            self._ew(P, PR.UPSAMPLE, i=(self.N, l.cout, top.shape[2], top.shape[3], 2), p=(top, t, t), nbytes=9.0 * t.numel())

    def _pointwise_grad(self, P, l, dy, like=None, mask=None, res=None, into=None, fold=False):
        """W^T dy (+ res), through the ReluGradient mask when given, in a new buffer shaped like `like` -- or, into=:
        added to the gradient that tensor already holds.  -> the tensor that holds the result (into itself)."""
        dx = self._like(like) if into is None else into
        self._gemm(P, l.w.view(l.cout, l.cin), l.cin, dy, dx, l.cout, l.cin, res=res, mask=mask, acc=into is not None,
                   fold=fold)
        return dx

    def _grouped3(self, P, l, x, y):
        """y = relu(grouped 3x3 of x + bias) at the layer's stride."""
        P.add(PR.GROUPED_CONV3X3, 56, i=(self.N, l.cin, x.shape[2], x.shape[3], l.group, l.stride, 1),
              p=(x, l.pf, l.b, y), work=2.0 * 9 * l.cin * l.wcin * self.N * y.shape[2] * y.shape[3])

    def _fpn_level(self, k, h, w):
        """The buffer of FPN level k (0: P3 ... 4: P7)."""
        return self._act(self.N, self.D, h, w)

    def _fpn_grads(self, P):
        """The gradients w.r.t. the FPN levels (subnet gradients, summed): written by the caller."""
        return [self._like(p) for p in self.fpn]

    # -- forward ----------------------------------------------------------------------------------------
    def _emit_forward(self, P):
        """The network, once for both precisions: what is computed in which order.  How an operation is emitted is the
        methods' above."""
        L, N, D = self._layers, self.N, self.D
        H, W = self.hw
        self.image = self._t(N, 3, H, W)
        # stem (fp32 in either precision: Cin = 3): 7x7 / 2 as an implicit GEMM (K = 147 gathered by the DMA: no column
        # buffer), then bias + ReLU + 3x3 / 2 max pool in one pass.  Image groups keep every buffer offset below 2 GiB.
        st = L["stem.0"]
        oh, ow = H // 2, W // 2
        kk = 3 * 49
        self.stem_z = self._t(N, st.cout, oh, ow)
        grp = max(1, min(N, int((1 << 31) - 1) // (st.cout * oh * ow * 4)))
        for n0 in range(0, N, grp):
            n1 = min(N, n0 + grp)
            d = K.gemm_conv_desc(st.wt, st.cout, self.image[n0:n1], self.stem_z[n0:n1], kk, st.cout)
            d.P = oh * ow
            P.add(PR.CONV_IMPLICIT, 53, i=(3, H, W, 7, 2, 3), p=(d,), work=2.0 * (n1 - n0) * oh * ow * kk * st.cout,
                  keep=[st.wt, self.image, self.stem_z])
        x = self._act(N, st.cout, oh // 2, ow // 2)
        self._stem_pool(P, st, self.stem_z, x)
        self.saved = {}
        stage_out = {}
        for (stage, j, cin, cmid, cout, stride, proj, tr) in self.blocks:
            pre = "res%d.%d" % (stage, j)
            l1, l2, l3 = L[pre + ".c1"], L[pre + ".c2"], L[pre + ".c3"]
            h, w = x.shape[2] // stride, x.shape[3] // stride
            xs = x
            if stride != 1:                                   # shared by c1 (ResNet) and the projection
                xs = self._act(N, cin, h, w)
                self._subsample(P, x, xs, cin, stride)
            a = xs if l1.stride == stride else x              # ResNeXt strides on the 3x3: c1 sees the full map
            y1 = self._act(N, cmid, a.shape[2], a.shape[3])
            y2, y = self._act(N, cmid, h, w), self._act(N, cout, h, w)
            self._pointwise(P, l1, a, y1, relu=True)
            if l2.group > 1:
                self._grouped3(P, l2, y1, y2)
            else:
                self._conv3(P, [(y1, y2, None, l2.pf, l2.b)], cmid, cmid, K.CONV_RELU, l2.engine)
            sc = xs
            if proj:
                sc = self._act(N, cout, h, w)
                self._pointwise(P, L[pre + ".proj"], xs, sc)
            self._pointwise(P, l3, y2, y, res=sc, relu=True)
            self.saved[pre] = dict(x=x, xs=xs, y1=y1, y2=y2, y=y, c1_in=a)
            x = y
            stage_out[stage] = y
        c3, c4, c5 = self.c345 = (stage_out[3], stage_out[4], stage_out[5])
        # FPN: laterals, each but the first summed with the level above (nearest upsampling); 3x3 output convolutions
        t5, t4, t3 = (self._act(N, D, c.shape[2], c.shape[3]) for c in (c5, c4, c3))
        self._lateral(P, L["lat.0"], c5, t5)
        self._lateral(P, L["lat.1"], c4, t4, top=t5)
        self._lateral(P, L["lat.2"], c3, t3, top=t4)
        p5, p4, p3 = (self._fpn_level(k, t.shape[2], t.shape[3]) for k, t in ((2, t5), (1, t4), (0, t3)))
        self._conv3(P, [(t, p, None, L[name].pf, L[name].b)                # three filters, one launch
                        for t, p, name in ((t5, p5, "out.0"), (t4, p4, "out.1"), (t3, p3, "out.2"))], D, D, 0,
                   same_engine(L[name].engine for name in ("out.0", "out.1", "out.2")))
        p6, p7, r6, p6f, p7f = (self._emit_p6p7_own if self._strided_own else self._emit_p6p7)(P, c5)
        self.fpn = [p3, p4, p5, p6, p7]                   # finest first (synth.LEVEL_SHAPES_*)
        self._fpn_saved = dict(t3=t3, t4=t4, t5=t5, r6=r6, p6f=p6f, p7f=p7f)

    def _emit_p6p7(self, P, c5):
        """P6 = conv3x3 / 2 (c5), P7 = conv3x3 / 2 (relu(P6)) as the stride-1 layer + the even positions (fp32:
        SSAD_STRIDED_3X3=winograd).  -> p6, p7, relu(p6), the two full-size maps"""
        N, D = self.N, self.D
        l6, l7 = self._layers["p6"], self._layers["p7"]
        p6f = self._act(N, D, c5.shape[2], c5.shape[3])
        self._conv3(P, [(c5, p6f, None, l6.pf, l6.b)], D, l6.cin, 0, l6.engine)
        p6 = self._fpn_level(3, c5.shape[2] // 2, c5.shape[3] // 2)
        self._subsample(P, p6f, p6, D, 2)
        r6 = self._like(p6)
        self._relu(P, p6, r6, D)
        p7f = self._like(p6)
        self._conv3(P, [(r6, p7f, None, l7.pf, l7.b)], D, D, 0, l7.engine)
        p7 = self._fpn_level(4, (p6.shape[2] + 1) // 2, (p6.shape[3] + 1) // 2)
        self._subsample(P, p7f, p7, D, 2)
        return p6, p7, r6, p6f, p7f

    def _emit_p6p7_own(self, P, c5):
        """The same at the layers' own size (conv_strided.hip; fp32 only, the default).  -> as _emit_p6p7"""
        N, D = self.N, self.D
        p6 = self._t(N, D, (c5.shape[2] - 1) // 2 + 1, (c5.shape[3] - 1) // 2 + 1)
        self._conv_s2(P, c5, p6, self._layers["p6"])
        r6 = self._like(p6)
        self._relu(P, p6, r6, D)
        p7 = self._t(N, D, (p6.shape[2] - 1) // 2 + 1, (p6.shape[3] - 1) // 2 + 1)
        self._conv_s2(P, r6, p7, self._layers["p7"])
        return p6, p7, r6, None, None

    # -- backward ------------------------------------------------------------------------------------------
    def _emit_backward(self, P):
        L, N, D = self._layers, self.N, self.D
        c3, c4, c5 = self.c345
        S = self._fpn_saved
        t3, t4, t5 = S["t3"], S["t4"], S["t5"]
        self.d_fpn = self._fpn_grads(P)
        d3, d4, d5, d6, d7 = self.d_fpn
        dc5 = self._like(c5)
        (self._emit_p6p7_own_grad if self._strided_own else self._emit_p6p7_grad)(P, c5, d6, d7, dc5)
        # output convs: filter gradients and the three data gradients in one launch
        dt5, dt4, dt3 = self._like(t5), self._like(t4), self._like(t3)
        if L["out.0"].engine == Engine.SPLIT:
            # one pass for the three filter gradients and the data gradient
            self._amax.measure(P, [[d5], [d4], [d3]], D)
        for t, d, name in ((t5, d5, "out.0"), (t4, d4, "out.1"), (t3, d3, "out.2")):
            self._wgrad3(P, t, d, L[name])
        self._conv3(P, [(d, dt, None, L[name].pd, None)
                        for d, dt, name in ((d5, dt5, "out.0"), (d4, dt4, "out.1"), (d3, dt3, "out.2"))], D, D, 0,
                   same_engine(L[name].engine for name in ("out.0", "out.1", "out.2")))
        # top-down path: t3 = lat2(c3) + up(t4), t4 = lat1(c4) + up(t5)
        dt4 = self._topdown_grad(P, dt3, dt4)
        dt5 = self._topdown_grad(P, dt4, dt5)
        # laterals: filter / bias gradients; data gradients meet the stage outputs' other consumers (c5's: P6)
        grads_into = {}
        for stage, c, dt, name, into in ((5, c5, dt5, "lat.0", dc5), (4, c4, dt4, "lat.1", None),
                                         (3, c3, dt3, "lat.2", None)):
            self._wgrad1(P, c, dt, L[name])
            grads_into[stage] = self._pointwise_grad(P, L[name], dt, like=c, into=into)
        P.mark("bwd_fpn_done")
        dy = None
        dy_is_dz = False          # dy already went through this block's ReluGradient (previous GEMM's epilogue)
        for (stage, j, cin, cmid, cout, stride, proj, tr) in reversed(self.blocks):
            if not tr:
                break
            pre = "res%d.%d" % (stage, j)
            l1, l2, l3 = L[pre + ".c1"], L[pre + ".c2"], L[pre + ".c3"]
            sv = self.saved[pre]
            x, xs, y1, y2, y = sv["x"], sv["xs"], sv["y1"], sv["y2"], sv["y"]
            if j == ARCHS[self.arch][stage - 2] - 1:
                # the stage's output feeds the lateral (already in grads_into) and, for res3 / res4,
                # the next stage's first block, whose input gradient was accumulated onto it
                dy = grads_into[stage]
                dy_is_dz = False
            if dy_is_dz:
                # the block below (later in the forward order) produced dy with this block's
                # ReluGradient mask already applied in its GEMM epilogue: no elementwise pass
                dz = dy
            else:
                # dz = ReluGradient(y, dy).  (No bias gradients in the body: the folded AffineChannel
                # biases are frozen values, affine_channel_op.cc.)
                dz = self._like(y)
                self._relu_grad(P, y, dy, dz, cout)
            self._wgrad1(P, y2, dz, l3)
            dz2 = self._pointwise_grad(P, l3, dz, like=y2, mask=y2, fold=True)
            dz1 = self._like(y1)
            if l2.group > 1:
                # ResNeXt (fp32 only): y1 (and so dz1) is at c1's input size, dz2 at the block's output size (stride on
                # the 3x3)
                self._wgrad_grouped(P, y1, dz2, l2)
                self._dgrad_grouped(P, dz2, dz1, y1, l2)
            else:
                self._wgrad3(P, y1, dz2, l2)                               # + bias gradient of c2
                self._conv3(P, [(dz2, dz1, y1, l2.pd, None)], cmid, cmid, K.CONV_MASK_AUX, l2.engine, fold=True)
            sv["dz2"], sv["dz1"] = dz2, dz1
            c1_in = sv["c1_in"]                                            # xs; the full map x in a ResNeXt
            self._wgrad1(P, c1_in, dz1, l1)
            if proj:
                lp = L[pre + ".proj"]
                self._wgrad1(P, xs, dz, lp)
                if not (stage == 3 and j == 0):              # (the first trainable block sends nothing further down)
                    # into the previous stage's output gradient, which already holds the lateral's part
                    if c1_in is xs:
                        dxs = self._pointwise_grad(P, l1, dz1, like=xs)
                        dxs = self._pointwise_grad(P, lp, dz, into=dxs)
                    else:
                        # ResNeXt, stride 2: the two parts of the input gradient live at different sizes.  W1^T dz1 is
                        # x-shaped: straight onto the previous stage's output gradient; Wp^T dz is xs-shaped: scattered
                        # onto it afterwards.  Always in this order: same bits.  (In place, unlike _aux's rule for
                        # gradients that meet: no auxiliary-stream launch reads that buffer -- the lateral's filter
                        # gradient reads the stage output and dt -- and its first reader, the previous stage's
                        # ReluGradient, is emitted on the main stream behind both writes.)
                        grads_into[stage - 1] = self._pointwise_grad(P, l1, dz1, into=grads_into[stage - 1])
                        dxs = self._pointwise_grad(P, lp, dz, like=xs)
                    self._subsample_grad(P, dxs, grads_into[stage - 1], cin, stride, acc=True)
                dy = None
                dy_is_dz = False
            else:
                # identity shortcut: dx = dz + W1^T dz1 (dz through the residual operand into a fresh
                # buffer: the auxiliary stream may still be reading dz)
                # x is the previous block's output y: its ReluGradient mask goes into this epilogue
                dy = self._pointwise_grad(P, l1, dz1, like=dz, mask=x, res=dz, fold=True)
                dy_is_dz = True
            if j == 0:
                P.mark("bwd_res%d_done" % stage)

    def _emit_p6p7_grad(self, P, c5, d6, d7, dc5):
        """Backward of _emit_p6p7: both filter gradients, and c5's part of the data gradient written to dc5."""
        D, S = self.D, self._fpn_saved
        l6, l7 = self._layers["p6"], self._layers["p7"]
        r6 = S["r6"]
        # P7 = sub(conv(relu(p6)))
        d7f = self._like(S["p7f"])
        self._subsample_grad(P, d7, d7f, D, 2)
        self._wgrad3(P, r6, d7f, l7)
        dr6 = self._like(r6)
        self._conv3(P, [(d7f, dr6, r6, l7.pd, None)], D, D, K.CONV_MASK_AUX, l7.engine)   # masked by p6 > 0
        d6 = self._sum2(P, d6, dr6, D)
        # P6 = sub(conv(c5))
        d6f = self._like(S["p6f"])
        self._subsample_grad(P, d6, d6f, D, 2)
        self._wgrad3(P, c5, d6f, l6)
        self._conv3(P, [(d6f, dc5, None, l6.pd, None)], l6.cin, D, 0, l6.engine)

    def _emit_p6p7_own_grad(self, P, c5, d6, d7, dc5):
        """Backward of _emit_p6p7_own."""
        l6, l7 = self._layers["p6"], self._layers["p7"]
        r6 = self._fpn_saved["r6"]
        # P7 = conv_s2(relu(p6)): filter gradient, then the data gradient masked by p6 > 0, added to P6's own
        self._wgrad_s2(P, r6, d7, l7)
        dr6 = self._like(r6)
        self._dgrad_s2(P, l7, d7, dr6, mask=r6)
        d6 = self._sum2(P, d6, dr6, self.D)
        # P6 = conv_s2(c5)
        self._wgrad_s2(P, c5, d6, l6)
        self._dgrad_s2(P, l6, d6, dc5)

    # -- running ---------------------------------------------------------------------------------------------
    def prepare(self):
        """Pack the frozen filters (once, and again after load_from)."""
        if not self._packed_frozen:
            self.prep.run(timing=None)
            self._packed_frozen = True

    def pack(self):
        self.prepare()
        self.prog.run("pack", "forward", timing=self.timing)

    def forward(self, images):
        """images: [N, 3, H, W] float32.  Returns the five FPN levels (finest first)."""
        if images.data_ptr() != self.image.data_ptr():
            self.image.copy_(images)
        self.prepare()
        self.prog.run("forward", "backward", timing=self.timing)
        return self.fpn

    def backward(self, d_fpn=None):
        """d_fpn: gradients w.r.t. the five levels (or already written into self.d_fpn).  Each
        stage's gradient bucket is all-reduced as soon as its last filter gradient is enqueued."""
        if d_fpn is not None:
            for dst, src in zip(self.d_fpn, d_fpn):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
        marks = ["backward", "bwd_fpn_done", "bwd_res5_done", "bwd_res4_done", "bwd_res3_done"]
        names = ["fpn", "res5", "res4", "res3"]
        for k in range(4):
            self.prog.run(marks[k], marks[k + 1], timing=self.timing)
            self.dp.issue(self.bucket[names[k]])
        # (the program has nothing between bwd_res3_done and sgd)

    def sgd_step(self):
        self.dp.wait()
        self.prog.run("sgd", "end", timing=self.timing)

    def broadcast_params(self, src=0):
        """detectron/lib/utils/net.py:185-208 broadcasts every blob of model.params from GPU 0: here the
        trained parameters and their history, the FROZEN values (conv1 / res2 filters, every folded
        AffineChannel bias) and the s^2 row scales of the folded trainable filters -- a replica that
        did not load the weights file itself must not keep its own initialisation in any of them.
        The un-folded scales kept for saving (`affine_scale_values`, host side) follow as an object."""
        if not self.dp.active:
            return
        slots = [l.s2 for l in self._layers.values() if l.s2 is not None]
        self.dp.broadcast([self.params_flat, self.moms_flat, self.frozen_flat] + slots, src=src)
        import torch.distributed as dist
        box = [self.affine_scale_values]
        dist.broadcast_object_list(box, src=src, group=self.dp.pg)
        self.affine_scale_values = box[0]
        self._packed_frozen = False

    SCALE_MOMENTUM = True             # cfg.SOLVER.SCALE_MOMENTUM (config.py:634)
    SCALE_MOMENTUM_THRESHOLD = 1.1    # config.py:638

    def update_lr(self, new_lr):
        """UpdateWorkspaceLr + _CorrectMomentum (detector.py:594-648) for the backbone's flat
        buffers: same rule as DistillHeads.update_lr."""
        cur_lr = float(self.lr.item())
        new_lr = float(np.float32(new_lr))
        if cur_lr == new_lr or not self.train:
            return new_lr
        eps = 1e-10
        ratio = max(new_lr / max(cur_lr, eps), cur_lr / max(new_lr, eps))
        self.lr.fill_(new_lr)
        if self.SCALE_MOMENTUM and cur_lr > 1e-7 and ratio > self.SCALE_MOMENTUM_THRESHOLD:
            K.scale_(self.moms_flat, new_lr / cur_lr)
        return new_lr


class NativeDistillModel(object):
    """One iteration of the whole detector on one GPU with native backbones: teacher forward
    (its own stream), student forward, subnets + losses (head_pipeline.DistillHeads), student
    backward, gradient all-reduce (when data parallel) and both SGD updates -- every launch one
    of this repo's kernels, enqueued by ssad_program_run."""

    def __init__(self, heads, student_arch="r50", teacher_arch="r101", N=16, image_hw=(640, 896), device="cuda",
                 process_group=None, world_size=1, lr=None, momentum=0.9, weight_decay=1e-4, two_streams=None,
                 overlap_wgrad=None, student_src=None, teacher_src=None, student_scales=None,
                 student_channel_ratio=1.0, student_grouped_grad=False, teacher_wide_groups=False):
        """lr: None = the subnets' learning rate (one schedule for the whole detector,
        optimizer.py:95-130).  two_streams / overlap_wgrad: None = environment
        (SSAD_NATIVE_TWO_STREAMS / SSAD_OVERLAP_WGRAD, default on).  *_src: initial weights
        (NativeResNetFPN._alloc_params), student_scales: the folded AffineChannel scales.
        student_channel_ratio: RESNETS.CHANNEL_RATIO of the student (a thin student under a full-width teacher:
        the teacher is built from its own cfg, model_builder.py:384 switch_to_teacher(), ratio 1).  `heads` must have
        been built for the two widths: HeadConfig.fpn_dim = the student's FPN dimension, teacher_fpn_dim = the
        teacher's (head_pipeline.DistillHeads).
        student_grouped_grad: NativeResNetFPN's grouped_grad for the student (a ResNeXt student; fp32 backbones only).
        teacher_wide_groups: NativeResNetFPNF16's wide_groups for the fp16 teacher (x101-32x8d, whose res5 groups are 64
        wide); the fp32 backbones run that teacher already and ignore it."""
        import os
        self.heads = heads
        self.student_channel_ratio = float(student_channel_ratio)
        self.has_teacher = teacher_arch not in (None, "none")
        assert self.has_teacher == bool(getattr(heads, "distill", True))
        if self.has_teacher and getattr(heads, "Dt", 256) != 256:
            raise K.KernelError("NativeDistillModel: the teacher is full width (FPN dimension 256), its subnets were "
                                "built for %d" % heads.Dt)
        lr = float(heads.lr.item()) if lr is None else lr
        self.f16 = bool(getattr(heads, "F16", False))
        # fp16 subnets that exchange blocked fp16 tensors with the backbone: the backbones run in the
        # same precision (config 5: every convolution of the net, conv_op_cudnn.cc:631-636)
        self.backbone_f16 = self.f16 and bool(getattr(heads, "blocked_io", False))
        if self.backbone_f16 and self.student_channel_ratio != 1.0:
            raise K.KernelError("NativeDistillModel: student_channel_ratio %r with the fp16-storage backbones is not "
                                "supported (backbone_f16's kernels were written for the full widths)"
                                % (student_channel_ratio,))
        if self.backbone_f16 and student_grouped_grad:
            raise K.KernelError("NativeDistillModel: student_grouped_grad with the fp16-storage backbones is not "
                                "supported (the grouped 3x3 gradient kernels are fp32); use the fp32 backbone")
        if self.backbone_f16:
            check_f16_grouped(student_arch)
            if self.has_teacher:
                check_f16_grouped(teacher_arch, teacher_wide_groups)
        want_s = student_widths(student_arch, student_channel_ratio).fpn_dim      # (raises before any allocation)
        if getattr(heads, "D", want_s) != want_s:
            raise K.KernelError("NativeDistillModel: the subnets were built for FPN dimension %d, a %s student of "
                                "channel_ratio %r has %d" % (heads.D, student_arch, student_channel_ratio, want_s))
        kw = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, process_group=process_group,
                  world_size=world_size, affine_scales=student_scales,
                  skip_flag=heads.ls_counters if self.f16 else None, overlap_wgrad=overlap_wgrad)
        if self.backbone_f16:
            from .backbone_f16 import NativeResNetFPNF16
            self.student = NativeResNetFPNF16(
                student_arch, N, image_hw, device, train=True, src=student_src, channel_ratio=student_channel_ratio,
                heads_io=dict(fpn_out=heads.in_blk["student"], inv_scale=heads.ls_state[1:2],
                              d_fpn_in=(heads.dbuf["cls"][0], heads.dbuf["bbox"][0])), **kw)
            self.teacher = NativeResNetFPNF16(
                teacher_arch, N, image_hw, device, train=False, src=teacher_src, process_group=process_group,
                world_size=world_size, heads_io=dict(fpn_out=heads.in_blk["teacher"]),
                wide_groups=teacher_wide_groups) if self.has_teacher else None
        else:
            self.student = NativeResNetFPN(student_arch, N, image_hw, device, train=True, src=student_src,
                                           channel_ratio=student_channel_ratio,
                                           grouped_grad=student_grouped_grad, **kw)
            self.teacher = NativeResNetFPN(teacher_arch, N, image_hw, device, train=False, src=teacher_src,
                                           process_group=process_group,
                                           world_size=world_size) if self.has_teacher else None
        # every replica starts from rank 0's values: trained AND frozen (utils/net.py:185-208)
        self.student.broadcast_params()
        if self.teacher is not None:
            self.teacher.broadcast_params()
        if two_streams is None:
            two_streams = os.environ.get("SSAD_NATIVE_TWO_STREAMS", "1") == "1"
        self.side = torch.cuda.Stream() if (two_streams and self.has_teacher) else None      # normal priority: high measured worse
        # the teacher's forward pass is enqueued BEFORE the student's filter packs (attribute kept for A/B in tests)
        self._teacher_first = True
        # The frozen teacher's forward pass depends on the images only -- not on the student's update.  Ordered after
        # the previous step's last READER of the teacher's output buffers (the subnets' forward launches) instead of
        # after everything the previous step enqueued, it may start while the previous step's backward pass is still
        # running whenever the launching thread is ahead of the GPU (it is: ~5 steps in steady state).  Taken only
        # when `images` cannot have a pending writer on the current stream (step(): `images_event`, or the same
        # unmodified tensor as the step before); otherwise the teacher waits for the current stream as before.
        # SSAD_TEACHER_AHEAD=0: the teacher waits for the whole previous step (rounds 2-3).
        # Measured (same-call A/B, 20 steps): config 3 (fp32) 95.7 -> 93.4 ms/step; config 5 (fp16 backbones, small
        # HBM-bound launches) 26.07 -> 26.8 ms -- there the teacher beside the backward pass costs more than it
        # fills, so the fp16 backbones keep the old order by default.
        self._teacher_ahead = os.environ.get("SSAD_TEACHER_AHEAD", "0" if self.backbone_f16 else "1") == "1"
        self._t_fpn_read = None               # event: the subnets have consumed the teacher's FPN levels
        self._images_ref, self._images_version = None, -1
        # gradient w.r.t. an FPN level = cls-subnet part + bbox-subnet part (the fp16 backbone's own
        # program starts with that sum, on the blocked tensors)
        Q = self.sum_prog = PR.Program()
        self._ptrs = []
        if not self.backbone_f16:
            # (a shared tower, HeadConfig.share_cls_bbox_tower: only the cls subnet reaches the FPN levels -- one term)
            parts = [heads.d_fpn[t] for t in ("cls", "bbox") if t in heads.d_fpn]
            for d, *terms in zip(self.student.d_fpn, *parts):
                ptrs = (C.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
                Q.add(PR.SUM_N, 51, i=(len(terms),), l=(d.numel(),), p=(ptrs, d), work=4.0 * (len(terms) + 1) * d.numel(),
                      keep=terms + [d])
        Q.build()
        if self.f16:
            # mixed precision: the backbone's reduced gradients join the subnets' finiteness check
            # (an overflowing step must drop BOTH updates; the flag is cleared after both)
            Q = self.check_prog = PR.Program()
            n = self.student.grads_flat.numel()
            Q.add(PR.CHECK_FINITE, 38, l=(n,), p=(self.student.grads_flat, heads.ls_counters), work=4.0 * n)
            Q.build()
        self._timing = None

    def update_lr(self, new_lr):
        """One learning-rate schedule for subnets and backbone (detector.py:594-648)."""
        self.heads.update_lr(new_lr)
        return self.student.update_lr(new_lr)

    @property
    def timing(self):
        return self._timing

    @timing.setter
    def timing(self, t):
        self._timing = t
        self.student.timing = t
        if self.teacher is not None:
            self.teacher.timing = t if self.side is None else None   # one timing object per stream

    def describe(self):
        if self.backbone_f16:
            return ("backbones = native programs of this repo's kernels in fp16 storage / fp32 accumulation "
                    "(pointwise convs: pw_f16_kernel with fused bias / shortcut / ReLU / FPN upsample-add; 3x3: "
                    "conv3x3_f16_kernel; ResNeXt grouped 3x3: grouped_f16_kernel; stem: fp32 implicit GEMM + fp16 "
                    "pool; no torch operator in the step)")
        return ("backbones = native programs of this repo's kernels (pointwise convs: fp32-MFMA GEMM with fused "
                "bias / shortcut / ReLU; 3x3: Winograd engine; stem: im2col + GEMM + fused bias/ReLU/pool; "
                "no torch operator in the step)")

    def step(self, images, labels, bbox_targets, fg_num, update=True, images_event=None):
        """One iteration.  update=False stops after the gradient exchange (every parameter
        gradient is then readable: the SGD launch overwrites the gradient buffers with the
        applied update, as MomentumSGDUpdate does, momentum_sgd_op_gpu.cu:22-38)."""
        h, st, te = self.heads, self.student, self.teacher
        # The frozen teacher needs nothing of this step but the images: its forward pass goes to the side stream
        # FIRST, so that the ~35 (fp32) / ~110 (fp16) small filter-pack launches of the student -- a serial chain
        # of 5-10 us kernels that leaves the chip empty -- run beside it instead of in front of it.
        t_fpn = None
        early = self._teacher_first and te is not None and self.side is not None
        if early:
            cur = torch.cuda.current_stream()
            # Running ahead is only safe when nothing enqueued on the current stream can still be WRITING `images`:
            # the caller says so with `images_event` (recorded by the input pipeline after its copy), or the tensor
            # is the very OBJECT the previous step already read, unmodified since (same version counter).  The
            # model keeps a reference to that tensor: a fresh batch tensor can then never be mistaken for it (its
            # storage cannot be handed out again by the caching allocator while the reference lives, and a fresh
            # tensor's version counter starts at 0 just like the old one's -- address + version alone would match
            # a new batch whose host-to-device copy is still queued on the current stream, which the side stream
            # does not wait for).  Anything else -- new tensor, view, in-place update -- takes the full wait.
            known = images_event is not None or (images is self._images_ref and
                                                 images._version == self._images_version)
            self._images_ref, self._images_version = images, images._version
            if self._teacher_ahead and self._t_fpn_read is not None and known:
                self.side.wait_event(self._t_fpn_read)      # the previous step's readers of the teacher's FPN buffers
                if images_event is not None:
                    self.side.wait_event(images_event)
            else:
                self.side.wait_stream(cur)
            with torch.cuda.stream(self.side):
                t_fpn = te.forward(images)
        h.pack_student()
        st.pack()
        if te is not None and not early:
            if self.side is not None:
                self.side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self.side):
                    t_fpn = te.forward(images)
            else:
                t_fpn = te.forward(images)
        s_fpn = st.forward(images)
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)
        if self.backbone_f16:
            t_fpn = s_fpn = None              # already in the subnets' blocked input buffers
        h.forward_all(t_fpn, s_fpn)
        h.cls_losses(labels, fg_num)
        h.bbox_losses_fwd_bwd(bbox_targets, fg_num)
        if self.side is not None and self._teacher_ahead:
            # the teacher's FPN levels have been read (forward_all); recorded behind the loss launches, which are
            # HBM-bound and short (0.45 ms): the next step's teacher starts beside the backward pass, not beside them
            if self._t_fpn_read is None:
                self._t_fpn_read = torch.cuda.Event()
            self._t_fpn_read.record(torch.cuda.current_stream())
        h.backward()
        self.sum_prog.run(timing=self._timing)
        st.backward()
        if not update:
            h.wait_gradients()
            st.dp.wait()
            return h.losses
        if self.f16:
            h.wait_gradients()
            st.dp.wait()
            h.prog.run("sgd", "sgd_update", timing=self._timing)          # subnet gradients finite?
            self.check_prog.run(timing=self._timing)                       # backbone gradients finite?
            h.prog.run("sgd_update", "ls_update", timing=self._timing)    # both updates honour the flag
            st.sgd_step()
            h.prog.run("ls_update", "end", timing=self._timing)           # scale moves, flag cleared
        else:
            h.sgd_step()
            st.sgd_step()
        return h.losses
