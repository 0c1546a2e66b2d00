"""Fused execution of the hot path: teacher heads forward, student heads
forward, PowSum + SigmoidAdaptiveDistillLoss, student heads backward, gradient
all-reduce and SGD -- the per-GPU work of one training iteration of
`build_generic_retinanet_model_dissstillation`
(detectron/lib/modeling/model_builder.py:373-411) restricted to the subnets.

Same arithmetic as running the operator graph of modeling/retinanet_heads.py
through the workspace (tests check that), but scheduled MI355X-first:

  * the five FPN levels that share a filter run as ONE launch per layer
    (the reference runs 5 cuDNN calls; its DAG executor overlaps them at best);
  * Relu / ReluGradient / Sigmoid live in conv epilogues, the 5-way gradient
    Sum over levels (caffe2/python/core.py:706-741) in the wgrad reduction;
  * filters are repacked once per step, not once per level;
  * all activations, gradients, parameters, parameter gradients and momenta
    are pre-allocated once (HBM is 288 GB; nothing is allocated in the step);
    parameter gradients live in two flat buckets (cls subnet, bbox subnet) so
    the data-parallel exchange is two large RCCL all-reduces that overlap the
    remaining backward instead of ~20 per-tensor ones
    (detectron/lib/modeling/optimizer.py:72-92).

torch provides device memory, streams and torch.distributed only.
"""
import dataclasses
import os
from collections import OrderedDict

import numpy as np
import torch

import ctypes as C

from . import kernels as K
from . import program as PR
from . import synth
from .data_parallel import BucketedAllReduce
from .engines import (AmaxTable, Engine, Switches, emit_conv3x3, emit_conv3x3_f16, emit_conv3x3_wgrad,
                      emit_conv3x3_wgrad_f16, emit_f16_packs, emit_packs, emit_sgd_flat, filter_floats, same_engine,
                      subnet_engine, subnet_wgrad_split)
from .modeling.retinanet_heads import HeadConfig, retinanet_bias_init


def cls_group(cfg):
    """Channels of cls_pred per anchor: the foreground classes of the sigmoid head, or all classes with the
    background for the softmax head (RETINANET.SOFTMAX, retinanet_heads.py:78-80)."""
    return cfg.num_classes if cfg.softmax else cfg.num_classes - 1


def head_towers(cfg):
    """The towers the subnets own: with RETINANET.SHARE_CLS_BBOX_TOWER there is no box tower and bbox_pred reads
    the classification tower (retinanet_heads.py:164-171)."""
    return ("cls",) if cfg.share_cls_bbox_tower else ("cls", "bbox")


def head_param_specs(cfg):
    """(name, shape, is_bias, bucket) in the order the backward pass finishes
    them: prediction layers, then tower layers from the deepest to the first,
    cls and bbox subnet interleaved (their layers of equal depth run in the
    same launches).  Bucket "late" (ready first) = predictions + upper half of
    the towers, bucket "early" = lower half.  A shared tower (HeadConfig.share_cls_bbox_tower) has no
    retnet_bbox_conv_* entries; a class-specific bbox_pred (HeadConfig.class_specific_bbox) has
    4 * (num_classes - 1) * A outputs."""
    A, C, D = cfg.num_anchors, cls_group(cfg), cfg.fpn_dim
    specs = []

    def add(stem, cout, bucket):
        specs.append((stem + "_w", (cout, D, 3, 3), False, bucket))
        specs.append((stem + "_b", (cout,), True, bucket))
    add("retnet_cls_pred_fpn%d" % cfg.k_min, A * C, "late")
    add("retnet_bbox_pred_fpn%d" % cfg.k_min, cfg.bbox_regr_dim * A, "late")
    for i in range(cfg.num_convs - 1, -1, -1):
        bucket = "late" if i >= cfg.num_convs // 2 else "early"
        for tower in head_towers(cfg):
            add("retnet_%s_conv_n%d_fpn%d" % (tower, i, cfg.k_min), D, bucket)
    return specs


class FlatParams(object):
    """Parameters (or gradients / momenta) of both subnets in one flat
    buffer; `bucket[name]` is the contiguous slice of one all-reduce bucket."""

    def __init__(self, cfg, device, init=None):
        self.specs = head_param_specs(cfg)
        total = sum(int(np.prod(s)) for _, s, _, _ in self.specs)
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.views = OrderedDict()
        self.offsets = {}
        self.bucket = {}
        off = 0
        starts = {}
        for name, shape, _, tower in self.specs:
            n = int(np.prod(shape))
            starts.setdefault(tower, off)
            self.views[name] = self.flat[off:off + n].view(shape)
            self.offsets[name] = off
            off += n
            self.bucket[tower] = self.flat[starts[tower]:off]
        if init is not None:
            for name, arr in init.items():
                self.views[name].copy_(torch.as_tensor(arr))

    def __getitem__(self, name):
        return self.views[name]


class DistillHeads(object):
    """One training iteration of the RetinaNet subnets as a native program
    (program.Program -> ssad_program_run).  distill=False is plain RetinaNet training
    (BASELINE config 2: model_builder.py:98-100,413 without the distillation wrapper): no
    teacher, no PowSum / SigmoidAdaptiveDistillLoss, only SigmoidFocalLoss + SelectSmoothL1Loss.
    HeadConfig.softmax (RETINANET.SOFTMAX, distill=False only): cls_pred has A * num_classes rows, initialised with
    the builder's prior bias, and the loss segment is ONE SOFTMAX_FOCAL_FUSED record (SoftmaxFocalLoss and its
    gradient in one pass over the logits) + SelectSmoothL1Loss; DESIGN 3.11a.
    HeadConfig.share_cls_bbox_tower (RETINANET.SHARE_CLS_BBOX_TOWER): no box tower in the student (nor in the teacher):
    bbox_pred reads the last classification activation and that activation's gradient is the sum of both prediction
    layers' data gradients under one ReLU mask.  HeadConfig.class_specific_bbox (RETINANET.CLASS_SPECIFIC_BBOX):
    bbox_pred, its gradient and its filter are 4 * (num_classes - 1) * A wide; DESIGN 3.14."""

    F16 = False

    def __init__(self, cfg=None, N=2, shapes=synth.LEVEL_SHAPES_600, device="cuda",
                 student_init=None, teacher_init=None, teacher_bbox_tower=True,
                 lr=0.01, momentum=0.9, weight_decay=1e-4, process_group=None, world_size=1,
                 distill=True, overlap_wgrad=None, blocked_io=False, teacher_fpn_dim=None, shared_accumulate=None):
        """teacher_fpn_dim: FPN dimension of the TEACHER's subnets when it differs from cfg.fpn_dim (the student's):
        a thin student of RESNETS.CHANNEL_RATIO r has int(FPN.DIM * r) channels on every level while the teacher,
        built from its own cfg, keeps FPN.DIM.  The two networks' towers then have different (Cout, Cin) and run as
        separate launches, each under the engine rules of its own width (fp32 pipeline only).
        shared_accumulate (shared tower only; None: environment SSAD_SHARED_ACCUM, default on -- the same-call A/B is in
        DESIGN 3.14): bbox_pred's data gradient adds itself to cls_pred's in its epilogue (CONV_ACCUM_AUX) where it runs
        on the F(2x4) engine; off, or on any other engine: two unmasked data gradients, SUM_N and RELU_GRAD records."""
        self.cfg = cfg or HeadConfig()
        self.N, self.shapes, self.device = N, list(shapes), device
        self.distill = bool(distill)
        if self.cfg.softmax and self.distill:
            raise K.KernelError(
                "DistillHeads: HeadConfig.softmax with distill=True is not supported: SigmoidAdaptiveDistillLoss does "
                "not take a softmax head (HeadConfig.softmax); the reference's distillation loss is sigmoid-shaped "
                "too.  Build the softmax head with distill=False")
        if self.cfg.softmax and self.F16:
            raise K.KernelError("DistillHeadsF16: HeadConfig.softmax is not supported (there is no fp16 softmax "
                                "head; the fp32 pipeline DistillHeads runs it)")
        for switch in ("share_cls_bbox_tower", "class_specific_bbox"):
            if getattr(self.cfg, switch) and self.F16:
                raise K.KernelError("DistillHeadsF16: HeadConfig.%s is not supported (the fp16 subnets run two towers "
                                    "and a 4 * A wide bbox_pred; the fp32 pipeline DistillHeads runs it)" % switch)
        self.towers = head_towers(self.cfg)
        self.box_tower = self.towers[-1]      # the tower bbox_pred reads
        if shared_accumulate is None:
            shared_accumulate = os.environ.get("SSAD_SHARED_ACCUM", "1") == "1"
        self._shared_accumulate = bool(shared_accumulate) and self.cfg.share_cls_bbox_tower
        self.teacher_bbox_tower = teacher_bbox_tower and self.distill
        self.switches = Switches.read().for_subnets(self.distill, self.F16)     # the one read of the engine switches
        self.split_conv = self.switches.split_conv
        self.momentum, self.weight_decay = momentum, weight_decay
        self.pg, self.world_size = process_group, world_size
        self.dp = BucketedAllReduce(process_group, world_size)
        cfg = self.cfg
        # C: cls_pred channels per anchor (softmax head: the background included)
        self.A, self.C, self.D = cfg.num_anchors, cls_group(cfg), cfg.fpn_dim
        self.Dt = int(teacher_fpn_dim) if (teacher_fpn_dim and self.distill) else self.D
        if self.Dt != self.D and self.F16:
            raise K.KernelError("DistillHeadsF16: teacher_fpn_dim %d != fpn_dim %d is not supported (the fp16 subnets "
                                "run teacher and student towers as one launch of one width)" % (self.Dt, self.D))
        t_cfg = cfg if self.Dt == self.D else dataclasses.replace(cfg, fpn_dim=self.Dt)
        self._plan_engines(cfg, t_cfg if self.distill else None)
        if cfg.softmax and student_init is None:
            # the builder's GivenTensorFill prior: the background channel of every anchor (retinanet_heads.py:39-52)
            student_init = {"retnet_cls_pred_fpn%d_b" % cfg.k_min:
                            np.asarray(retinanet_bias_init(cfg)[1]["values"], np.float32).reshape(-1)}
        self.params = FlatParams(cfg, device, student_init)
        self.teacher = FlatParams(t_cfg, device, teacher_init) if self.distill else None
        self.grads = FlatParams(cfg, device)
        self.moms = FlatParams(cfg, device)
        nlev = len(self.shapes)
        f32 = dict(dtype=torch.float32, device=device)
        self.lr = torch.full((1,), lr, **f32)
        self.one = torch.ones(nlev, **f32)
        self.losses = torch.zeros(nlev, **f32)           # distillation loss per level
        self.focal_losses = torch.zeros(nlev, **f32)
        self.bbox_losses = torch.zeros(nlev, **f32)
        self.normalizer = torch.zeros(1, **f32)
        self.fg_num = torch.ones(1, **f32)               # bound copy of the step's fg_num
        self.preserved = OrderedDict()     # blobs of a loaded weights file the subnets do not own
        self.timing = None                 # program.Timing while bench.py measures
        self.t_packed = None
        self._teacher_packed = False
        self._overlap_wgrad = overlap_wgrad      # None: environment (SSAD_OVERLAP_WGRAD, default on)
        # fp16 pipeline only: the FPN levels arrive (and their gradients leave) channel-blocked fp16
        # in this object's own buffers -- in_blk[...] is written by the backbone program, dbuf[t][0]
        # read by it (backbone_f16.NativeResNetFPNF16): no NCHW fp32 round trip at the boundary
        self.blocked_io = bool(blocked_io) and self.F16
        self._alloc_buffers()
        self._build_programs()

    # -- buffers ------------------------------------------------------------------
    def _lv(self, ch):
        return [torch.empty((self.N, ch, h, w), dtype=torch.float32, device=self.device)
                for (h, w) in self.shapes]

    def _alloc_buffers(self):
        cfg, lv, D = self.cfg, self._lv, self.D
        # inputs are bound per step (the FPN tensors belong to the caller); these placeholders
        # give the level tables valid addresses until the first bind
        self.fpn_in = lv(D)
        self.t_fpn_in = self.fpn_in if self.Dt == D else lv(self.Dt)
        self.labels = [torch.zeros((self.N, self.A, h, w), dtype=torch.int32, device=self.device)
                       for (h, w) in self.shapes]
        # student activations (kept for backward) and their gradients
        R = cfg.bbox_regr_dim * self.A
        self.act = {t: [lv(D) for _ in range(cfg.num_convs)] for t in self.towers}
        self.cls_logits, self.bbox_pred = lv(self.A * self.C), lv(R)
        self.d_cls_logits = lv(self.A * self.C)
        self.d_bbox_pred = lv(R)
        # one gradient set per tower depth (not ping-pong): the filter gradient of a layer runs on an
        # auxiliary stream while the data-gradient chain continues, so its dY must stay intact
        self.dbuf = {t: [lv(D) for _ in range(cfg.num_convs + 1)] for t in self.towers}
        self.d_fpn = {t: lv(D) for t in self.towers}
        # shared tower: "accumulate" where bbox_pred's data gradient runs on the engine that has the epilogue, else "two_pass"
        self.shared_form = None
        if cfg.share_cls_bbox_tower:
            accum = self._shared_accumulate and self.dgrad_engine[self._layers("bbox")[-1]] == Engine.F24
            self.shared_form = "accumulate" if accum else "two_pass"
        if self.shared_form == "two_pass":
            # two-pass form: the two prediction layers' unmasked data gradients and their sum; the sum, masked, is
            # dbuf["cls"][num_convs] (no operand of a launch aliases its output)
            self.d_shared = {t: lv(D) for t in ("cls", "bbox", "sum")}
        if self.distill:
            # teacher scratch: two ping-pong feature sets per tower + probabilities
            Dt = self.Dt
            self.t_buf = {t: [lv(Dt), lv(Dt)] for t in self.towers}
            self.t_prob = lv(self.A * self.C)
            self.t_bbox = lv(R) if self.teacher_bbox_tower else None

    # -- layer bookkeeping ----------------------------------------------------------
    def _layers(self, tower):
        cfg = self.cfg
        names = ["retnet_%s_conv_n%d_fpn%d" % (tower, i, cfg.k_min) for i in range(cfg.num_convs)]
        if tower not in self.towers:      # shared tower: the box subnet is its prediction layer alone
            names = []
        names.append("retnet_%s_pred_fpn%d" % (tower, cfg.k_min))
        return names

    def _plan_engines(self, cfg, t_cfg):
        """The engine of every convolution, before a buffer or a record exists: fwd_engine[who, layer] for the forward
        launches of who = "student" | "teacher" (t_cfg None: no teacher), dgrad_engine[layer] for the student's data
        gradients.  Filters are packed for these engines (_alloc_packed) and the launches read them on these
        (_emit_forward, _emit_backward): nothing else decides."""
        self.fwd_engine, self.dgrad_engine = {}, {}
        for who, c in (("student", cfg), ("teacher", t_cfg)):
            for name, shape, is_bias, _ in head_param_specs(c) if c is not None else ():
                if not is_bias:
                    layer, (cout, cin) = name[:-2], shape[:2]
                    self.fwd_engine[who, layer] = subnet_engine(self.switches, who, layer, cout, cin, "fwd")
                    if who == "student":
                        self.dgrad_engine[layer] = subnet_engine(self.switches, who, layer, cout, cin, "dgrad")

    def _px(self):
        return self.N * sum(h * w for h, w in self.shapes)

    # -- program construction ---------------------------------------------------------
    @staticmethod
    def _rows(problems):
        """problems: [(xs, outs or None, masks or None, packed or None, bias or None)], one tensor per level in xs / outs /
        masks -> kernels.conv_levels()'s rows, the problems' levels one after the other"""
        return [(x, outs[l] if outs is not None else None, masks[l] if masks is not None else None, packed, bias)
                for xs, outs, masks, packed, bias in problems for l, x in enumerate(xs)]

    # |max| words of the split-operand engines (engines.AmaxTable): a launch's block holds its problems' level lists one
    # after the other, so that a filter gradient (one tower's levels) finds the words of the launch that produced or
    # first read its tensors; a reader measures through its own level table.
    AMAX_WORDS = 2048

    # timing class of a launch by (role, engine); "teacher_...": a launch of the teacher's problems alone.  The direct
    # engine has one class for every role (18).
    KLASS = {("tower", Engine.F22): 2, ("tower", Engine.F24): 23, ("tower", Engine.SPLIT): 28,
             ("teacher_tower", Engine.F22): 2, ("teacher_tower", Engine.F24): 21, ("teacher_tower", Engine.SPLIT): 28,
             ("cls_pred", Engine.F22): 3, ("cls_pred", Engine.F24): 22, ("cls_pred", Engine.SPLIT): 26,
             ("teacher_cls_pred", Engine.F22): 3, ("teacher_cls_pred", Engine.F24): 20,
             ("teacher_cls_pred", Engine.SPLIT): 25,
             ("bbox_pred", Engine.F22): 4, ("teacher_bbox_pred", Engine.F22): 4,
             # a class-specific bbox_pred (>= 128 outputs) runs on cls_pred's engines
             ("bbox_pred", Engine.F24): 30, ("teacher_bbox_pred", Engine.F24): 30,
             ("bbox_pred", Engine.SPLIT): 31, ("teacher_bbox_pred", Engine.SPLIT): 31,
             ("pred_dgrad", Engine.F22): 16, ("pred_dgrad", Engine.F24): 24, ("pred_dgrad", Engine.SPLIT): 27,
             ("tower_dgrad", Engine.F22): 16, ("tower_dgrad", Engine.F24): 24, ("tower_dgrad", Engine.SPLIT): 29}

    def _emit_conv(self, P, problems, Cout, Cin, flags, role, engine, teacher=False, fold=True):
        """One launch of independent convolutions of equal (Cout, Cin) on one engine; every output's |max| is folded
        (fold=False: the output is not final -- a later launch accumulates into it -- so no word is kept for it)."""
        klass = 18 if engine == Engine.DIRECT else self.KLASS[("teacher_" if teacher else "") + role, engine]
        return emit_conv3x3(P, klass, self._rows(problems), Cout, Cin, flags, engine, self._amax, self._split,
                            levels=len(self.shapes), own_table=True, fold=fold)

    def _emit_group(self, P, probs, role, flags, bind=False):
        """probs: [(who, layer, problem)], forward convolutions that may share launches: one launch per (Cout, Cin,
        planned engine), the teacher's own launches first.  bind: the problems read the bound FPN levels."""
        groups = OrderedDict()
        for who, layer, prob in probs:
            cout, cin = (self.teacher if who == "teacher" else self.params)[layer + "_w"].shape[:2]
            groups.setdefault((cout, cin, self.fwd_engine[who, layer]), []).append((who, prob))
        for (cout, cin, engine), members in sorted(groups.items(), key=lambda g: any(w != "teacher" for w, _ in g[1])):
            # The teacher's towers on F(2x4) in a launch of their own, the student's of the same width on F(2x2): the
            # student's half alone is 19.5 + 4.5 rounds of the 256 CUs where the four towers together were 39 + 9.
            # These launches have the chip to themselves, so their partial rounds are split.
            tail = engine == Engine.F22 and any(k[:2] == (cout, cin) and k[2] != engine for k in groups)
            _, arr = self._emit_conv(P, [p for _, p in members], cout, cin, flags | (K.CONV_SPLIT_TAIL if tail else 0),
                                     role, engine, teacher=all(w == "teacher" for w, _ in members))
            if bind:
                slots = [(w, l) for w, p in members for l in range(len(p[0]))]
                self._in_slots.extend((arr, k, w, l) for k, (w, l) in enumerate(slots))

    def _emit_wgrad(self, P, xs, dys, name, Cout, klass):
        exact = 19 if self.fwd_engine["student", name] == Engine.DIRECT else klass
        return emit_conv3x3_wgrad(P, (exact, {5: 68, 6: 69, 7: 40}.get(klass, klass)), xs, dys, self.grads[name + "_w"],
                                  self.grads[name + "_b"], Cout, self.D, subnet_wgrad_split(self.switches, Cout, self.D),
                                  self._amax, self._fork, own_table=True)

    def _fork(self, P):
        """The filter gradients' stream and workspace, behind everything enqueued so far (the producer of dys)."""
        if self._wstream:
            P.fork(self._wstream)
        return self._wstream, self._wgrad

    PACK_ORDER = (Engine.SPLIT, Engine.F24, Engine.F22, Engine.DIRECT)

    def _alloc_packed(self, params, who):
        """Packed-filter buffers of who's layers ("student": forward and data gradient, "teacher": forward), each in
        the layout of the engine planned to read it -> ({layer: (fwd, dgrad or None)}, what _emit_pack needs: here
        {Engine: pack entries})."""
        packed, packs = {}, {}
        for tower in ("cls", "bbox"):
            for name in self._layers(tower):
                w = params[name + "_w"]
                cout, cin = w.shape[0], w.shape[1]
                ef, ed = self.fwd_engine[who, name], self.dgrad_engine[name] if who == "student" else None
                pf = torch.empty(filter_floats(ef)(cout, cin), dtype=torch.float32, device=self.device)
                pd = None
                if ed is not None:
                    pd = torch.empty(filter_floats(ed)(cin, cout), dtype=torch.float32, device=self.device)
                packed[name] = (pf, pd)
                for e in {ef, ed} - {None}:
                    packs.setdefault(e, []).append((w, cout, cin, pf if e == ef else None, pd if e == ed else None))
        return packed, packs

    def _emit_pack(self, P, packs):
        emit_packs(P, 1, packs, self.PACK_ORDER)

    def _build_programs(self):
        # filter gradients on an auxiliary stream beside the data-gradient chain (program.py FORK / JOIN)
        ov = self._overlap_wgrad
        self._wstream = 1 if (os.environ.get("SSAD_OVERLAP_WGRAD", "1") == "1" if ov is None else ov) else 0
        # one workspace for the split-engine convolutions (they run one after the other on the program's stream), one
        # for the filter gradients
        self._split, self._wgrad = PR.Workspace(), PR.Workspace()
        self._amax = AmaxTable(self.AMAX_WORDS, self.device)
        self.amax = self._amax.tensor
        self._in_slots = []          # (table, index, which): entries that read the bound inputs
        # filters (the teacher's are frozen: packed by a program of their own, run when they change)
        self.packed, s_packs = self._alloc_packed(self.params, "student")
        if self.distill:
            self.t_packed_pairs, t_packs = self._alloc_packed(self.teacher, "teacher")
            self.t_packed = {k: v[0] for k, v in self.t_packed_pairs.items()}
            T = self.prog_teacher_pack = PR.Program()
            self._emit_pack(T, t_packs)
            T.build()
        P = self.prog = PR.Program()
        P.mark("pack")
        self._emit_pack(P, s_packs)
        P.mark("forward")
        if self.switches.split_conv:      # the table of |max| words serves the split-operand engines
            P.add(PR.FILL, 11, p=(self.amax,), f=(0.0,), l=(self.AMAX_WORDS,), work=4.0 * self.AMAX_WORDS)
        self._emit_forward(P)
        P.mark("losses")
        self._emit_losses(P)
        P.mark("backward")
        self._emit_backward(P)
        P.mark("sgd")
        self._emit_sgd(P)
        P.mark("end")
        # the distillation-only variant of the loss segment (no supervised losses: the caller
        # supplies the gradient of the box predictions)
        if self.distill:
            Q = self.prog_distill_only = PR.Program()
            self._emit_losses(Q, supervised=False)
            Q.build()
        self.split_ws, self.wgrad_ws = self._split.bind(self.device), self._wgrad.bind(self.device)
        P.build()

    # -- forward --------------------------------------------------------------------------
    def _emit_forward(self, P):
        """Teacher (test mode) and student subnets.  The tower layers of equal depth
        (teacher/student x cls/bbox) are independent convolutions of the same shape, so each
        depth is ONE launch of up to 20 (level, filter) problems: 12 480 equal workgroups fill
        the 256 CUs to 99 % where five separate launches would each leave a partial last wave.
        Teacher cls_pred carries the Sigmoid epilogue (retinanet_heads.py:153-163)."""
        cfg = self.cfg
        tx = {t: self.t_fpn_in for t in self.towers}
        sx = {t: self.fpn_in for t in self.towers}
        for i in range(cfg.num_convs):
            probs = []
            for t in self.towers:
                name = self._layers(t)[i]
                if self.distill and (t == "cls" or self.teacher_bbox_tower):
                    out = self.t_buf[t][i & 1]
                    probs.append(("teacher", name, (tx[t], out, None, self.t_packed_for(name), self.teacher[name + "_b"])))
                    tx[t] = out
                out = self.act[t][i]
                probs.append(("student", name, (sx[t], out, None, self.packed[name][0], self.params[name + "_b"])))
                sx[t] = out
            # (a thin student under a full-width teacher: two widths, so two launches per depth)
            self._emit_group(P, probs, "tower", K.CONV_RELU, bind=i == 0)
        cp, bp = self._layers("cls")[-1], self._layers("bbox")[-1]
        if self.distill:
            self._emit_group(P, [("teacher", cp, (tx["cls"], self.t_prob, None, self.t_packed_for(cp), self.teacher[cp + "_b"]))],
                             "cls_pred", K.CONV_SIGMOID)
        self._emit_group(P, [("student", cp, (sx["cls"], self.cls_logits, None, self.packed[cp][0], self.params[cp + "_b"]))],
                         "cls_pred", 0)
        bt = self.box_tower
        probs = [("student", bp, (sx[bt], self.bbox_pred, None, self.packed[bp][0], self.params[bp + "_b"]))]
        if self.teacher_bbox_tower:
            probs.append(("teacher", bp, (tx[bt], self.t_bbox, None, self.t_packed_for(bp), self.teacher[bp + "_b"])))
        self._emit_group(P, probs, "bbox_pred", 0)

    def t_packed_for(self, name):
        return self.t_packed[name]

    # -- losses -----------------------------------------------------------------------------
    def _distill_kw(self):
        cfg = self.cfg
        return dict(gamma=cfg.distill_gamma, alpha=cfg.distill_alpha, beta=cfg.distill_beta,
                    num_classes=self.C, ignored_label=cfg.ignored_label,
                    scale=cfg.loss_scale * cfg.temperature * cfg.temperature)

    def _cls_table(self, outs):
        arr = (K.DistillLevel * len(self.shapes))()
        for l, x in enumerate(self.cls_logits):
            N, Dd, H, W = x.shape
            arr[l] = K.DistillLevel(x.data_ptr(), self.t_prob[l].data_ptr() if self.distill else 0,
                                    self.labels[l].data_ptr(), outs[l].data_ptr(), N, Dd, H, W)
        self._label_tables.append(arr)
        return arr

    def _emit_losses(self, P, supervised=True):
        """PowSum normaliser (adaptive: computed from the teacher's probabilities,
        retinanet_heads.py:325-329) and the classification / box losses with their gradients
        w.r.t. the predictions (loss gradients = 1.0, utils/blob.py:166-172).  With the
        supervised losses present, both classification losses of the student and their summed
        gradient come from ONE pass over the logits (the reference: 2 forward ops + 2 gradient
        ops + an autograd Sum per level)."""
        cfg, L = self.cfg, K.lib()
        if not hasattr(self, "_label_tables"):
            self._label_tables, self._sl1_tables = [], []
        nlev = len(self.shapes)
        n_logits = sum(x.numel() for x in self.cls_logits)
        n_labels = sum(x.numel() for x in self.labels)
        if self.distill:
            ptrs = (C.c_void_p * nlev)(*[t.data_ptr() for t in self.t_prob])
            sizes = (C.c_int64 * nlev)(*[t.numel() for t in self.t_prob])
            nb = L.ssad_pow_sum_workspace_bytes(nlev)
            ws = torch.zeros(nb, dtype=torch.uint8, device=self.device)     # arrival counters: zero once
            P.add(PR.POW_SUM, 8, i=(nlev,), f=(cfg.logits_power,), l=(nb,), p=(ptrs, sizes, self.normalizer, ws),
                  work=4.0 * n_logits, keep=list(self.t_prob))
        DP = K.DistillParams(**{k: v for k, v in self._distill_kw().items()})
        FP = K.FocalParams(cfg.focal_gamma, cfg.focal_alpha, self.C, cfg.loss_scale)
        if self.distill and supervised:
            if cfg.focal_gamma != 2.0:
                raise K.KernelError("the fused distillation + focal pass specialises focal gamma == 2")
            arr = self._cls_table(self.d_cls_logits)
            nb = L.ssad_cls_losses_fused_workspace_bytes(nlev)
            ws = torch.zeros(nb, dtype=torch.uint8, device=self.device)     # arrival counters: zero once
            P.add(PR.CLS_LOSSES_FUSED, 9, i=(nlev,), l=(nb,),
                  p=(arr, self.normalizer, self.fg_num, DP, FP, self.losses, self.focal_losses, ws),
                  work=12.0 * n_logits + 4.0 * n_labels)
        elif self.distill:
            nb = L.ssad_distill_loss_workspace_bytes(nlev)
            ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
            arr_f = self._cls_table([self.losses[l:l + 1] for l in range(nlev)])
            P.add(PR.DISTILL_FWD, 12, i=(nlev,), l=(nb,), p=(arr_f, self.normalizer, DP, ws),
                  work=8.0 * n_logits + 4.0 * n_labels)
            arr_b = self._cls_table(self.d_cls_logits)
            P.add(PR.DISTILL_BWD, 13, i=(nlev, 1), p=(arr_b, self.normalizer, self.one, DP),
                  work=12.0 * n_logits + 4.0 * n_labels)
        elif cfg.softmax:
            # SoftmaxFocalLoss and its gradient in one pass over the logits: the probabilities stay in registers
            # (no P pointer), the loss gradient 1.0 is folded in on the host
            arr = (K.SoftmaxFocalLevel * nlev)()
            for l, x in enumerate(self.cls_logits):
                N, Dd, H, W = x.shape
                arr[l] = K.SoftmaxFocalLevel(x.data_ptr(), self.labels[l].data_ptr(), 0,
                                             self.d_cls_logits[l].data_ptr(), N, Dd, H, W)
            self._label_tables.append(arr)
            SP = K.FocalParams(cfg.focal_gamma, cfg.focal_alpha, cfg.num_classes, cfg.loss_scale)
            nb = L.ssad_softmax_focal_loss_fused_workspace_bytes(nlev)
            ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
            P.add(PR.SOFTMAX_FOCAL_FUSED, 17, i=(nlev,), f=(1.0,), l=(nb,),
                  p=(arr, self.fg_num, SP, self.focal_losses, ws),
                  work=8.0 * n_logits + 4.0 * n_labels, keep=list(self.cls_logits) + list(self.d_cls_logits))
        else:
            nb = L.ssad_distill_loss_workspace_bytes(nlev)
            ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
            arr_f = self._cls_table([self.focal_losses[l:l + 1] for l in range(nlev)])
            P.add(PR.FOCAL_FWD, 14, i=(nlev,), l=(nb,), p=(arr_f, self.fg_num, FP, ws),
                  work=4.0 * n_logits + 4.0 * n_labels)
            arr_b = self._cls_table(self.d_cls_logits)
            P.add(PR.FOCAL_BWD, 15, i=(nlev, 1), p=(arr_b, self.fg_num, self.one, FP),
                  work=8.0 * n_logits + 4.0 * n_labels)
        if supervised:
            # SelectSmoothL1Loss per level (retinanet_heads.py:268-280) and its gradient
            tab = (K.SmoothL1Level * nlev)()
            for l, pred in enumerate(self.bbox_pred):
                N, Dd, H, W = pred.shape
                tab[l] = K.SmoothL1Level(pred.data_ptr(), 0, 0, self.bbox_losses[l:l + 1].data_ptr(),
                                         self.d_bbox_pred[l].data_ptr(), N, Dd, H, W, 0)
            self._sl1_tables.append(tab)
            nb = L.ssad_select_smooth_l1_workspace_bytes(nlev)
            ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
            P.add(PR.SMOOTH_L1, 10, i=(nlev, 1), f=(cfg.bbox_reg_beta, cfg.loss_scale * cfg.bbox_reg_weight),
                  l=(nb,), p=(tab, self.fg_num, self.one, ws),
                  work=4.0 * sum(x.numel() for x in self.d_bbox_pred),
                  keep=list(self.bbox_pred) + list(self.d_bbox_pred))

    # -- backward -------------------------------------------------------------------------------
    def _emit_backward(self, P):
        """Backward of both subnets, depth by depth from the prediction layers down.  Per depth:
        the two weight gradients (each already one workgroup per CU) and ONE data-gradient
        launch for both towers.  For tower layers the data gradient carries the ReluGradient
        mask, which is the layer's own post-ReLU input.  The program is cut where a gradient
        bucket is complete (mark "backward_late_done"): its all-reduce is issued there."""
        cfg, D = self.cfg, self.D
        nl = cfg.num_convs
        shared = cfg.share_cls_bbox_tower
        # shared tower, accumulate form: cls_pred's data gradient lands unmasked in the tower's gradient buffer and bbox_pred's
        # adds itself under the one ReLU mask in its own epilogue -- where bbox_pred's data gradient is on the F(2x4)
        # engine, the one engine with that epilogue (subnet_engine: the class-agnostic 36-wide layer by default)
        dy = {"cls": self.d_cls_logits, "bbox": self.d_bbox_pred}
        for t, klass_w in (("cls", 6), ("bbox", 7)):
            name = self._layers(t)[-1]
            x_in = self.act[t if t in self.towers else self.box_tower][nl - 1]
            Cout = self.params[name + "_b"].numel()
            self._emit_wgrad(P, x_in, dy[t], name, Cout, klass_w)
            engine = self.dgrad_engine[name]
            if self.shared_form == "accumulate":
                out = self.dbuf["cls"][nl]
                if t == "cls":
                    self._emit_conv(P, [(dy[t], out, None, self.packed[name][1], None)], D, Cout, 0, "pred_dgrad", engine,
                                    fold=False)
                else:
                    self._emit_conv(P, [(dy[t], out, x_in, self.packed[name][1], None)], D, Cout,
                                    K.CONV_MASK_AUX | K.CONV_ACCUM_AUX, "pred_dgrad", engine)
            elif shared:
                # both data gradients land unmasked in buffers of their own and are summed below
                out = self.d_shared[t]
                self._emit_conv(P, [(dy[t], out, None, self.packed[name][1], None)], D, Cout, 0, "pred_dgrad", engine,
                                fold=False)
            else:
                out = self.dbuf[t][nl]
                self._emit_conv(P, [(dy[t], out, x_in, self.packed[name][1], None)], D, Cout, K.CONV_MASK_AUX,
                                "pred_dgrad", engine)
            dy[t] = out
        if self.shared_form == "two_pass":
            # d(last tower activation) = ReluGradient(cls_pred's + bbox_pred's data gradient): the reference's gradient
            # Sum of a blob read by two convolutions, then the tower's ReluGradient (one mask for the sum)
            x_in, out = self.act["cls"][nl - 1], self.dbuf["cls"][nl]
            for a, b, s_, d, x in zip(dy["cls"], dy["bbox"], self.d_shared["sum"], out, x_in):
                ptrs = (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())
                P.add(PR.SUM_N, 39, i=(2,), l=(d.numel(),), p=(ptrs, s_), work=12.0 * d.numel(), keep=[a, b, s_])
                P.add(PR.RELU_GRAD, 39, p=(x, s_, d), l=(d.numel(),), work=12.0 * d.numel(), keep=[x, s_, d])
        if shared:
            dy = {"cls": self.dbuf["cls"][nl]}
        for li in range(nl - 1, -1, -1):
            probs = []
            for t in self.towers:
                name = self._layers(t)[li]
                x_in = self.act[t][li - 1] if li > 0 else self.fpn_in
                _, arr = self._emit_wgrad(P, x_in, dy[t], name, D, 5)
                if li == 0:
                    for l in range(len(x_in)):
                        self._in_slots.append((arr, l, "student", l))
                out = self.dbuf[t][li] if li > 0 else self.d_fpn[t]
                probs.append((dy[t], out, x_in if li > 0 else None, self.packed[name][1], None))
                dy[t] = out
            self._emit_conv(P, probs, D, D, K.CONV_MASK_AUX if li > 0 else 0, "tower_dgrad",
                            same_engine(self.dgrad_engine[self._layers(t)[li]] for t in self.towers))
            if li == nl // 2:
                P.mark("backward_late_done")
        if "backward_late_done" not in P.marks:
            P.mark("backward_late_done")

    # -- update -----------------------------------------------------------------------------------
    def _emit_sgd(self, P, skip_flag=None):
        if "sgd_update" not in P.marks:
            P.mark("sgd_update")            # fp32: nothing precedes the update ("sgd" == "sgd_update")
        emit_sgd_flat(P, 11, [(self.params.offsets[name], int(np.prod(shape)), is_bias, 0, None)
                              for name, shape, is_bias, _ in self.params.specs],
                      self.params.flat, self.grads.flat, self.moms.flat, self.lr, self.momentum, self.weight_decay,
                      skip_flag)
        P.mark("ls_update")                 # fp32: nothing follows the update

    # -- input binding ------------------------------------------------------------------------------
    def _bind(self, student_fpn=None, teacher_fpn=None, labels=None, bbox_targets=None, fg_num=None):
        """Point the program at this step's input tensors (they belong to the caller and may
        move between steps); only entries whose address changed are rewritten."""
        if student_fpn is not None or teacher_fpn is not None:
            s = list(student_fpn) if student_fpn is not None else self.fpn_in
            t = list(teacher_fpn) if teacher_fpn is not None else self.t_fpn_in
            dev_type = torch.device(self.device).type
            for x in list(s) + list(t if self.distill else []):
                if x.dtype != torch.float32 or not x.is_contiguous() or x.device.type != dev_type:
                    raise K.KernelError("FPN levels must be contiguous float32 tensors on %s" % dev_type)
            if any(tuple(a.shape) != tuple(b.shape) for a, b in zip(s, self.fpn_in)) or (
                    self.distill and any(tuple(a.shape) != tuple(b.shape) for a, b in zip(t, self.t_fpn_in))):
                raise K.KernelError("FPN levels do not match the shapes this pipeline was built for")
            self._rebind_inputs(s, t)
            self.fpn_in, self.t_fpn_in = s, t
            self._bound_in = (s, t)                     # keep the tensors alive
        if labels is not None:
            for l, g in enumerate(labels):
                if g.dtype != torch.int32 or not g.is_contiguous() or tuple(g.shape) != tuple(self.labels[l].shape):
                    raise K.KernelError("labels[%d] must be contiguous int32 %r" % (l, tuple(self.labels[l].shape)))
            for arr in self._label_tables:
                for l, g in enumerate(labels):
                    arr[l].labels = g.data_ptr()
            self.labels = list(labels)
        if fg_num is not None:
            self.fg_num.copy_(fg_num.reshape(1), non_blocking=True)
        if bbox_targets is not None:
            for tab in self._sl1_tables:
                for l, (Y, Lc) in enumerate(bbox_targets):
                    M = Y.shape[0] if Y.numel() else 0
                    if M:
                        K._f32c(Y, "Y"); K._f32c(Lc, "L")
                        if tuple(Y.shape) != (M, 4) or tuple(Lc.shape) != (M, 4):
                            raise K.KernelError("bbox targets must be (Y [M,4], L [M,4])")
                    tab[l].Y = Y.data_ptr() if M else 0
                    tab[l].L = Lc.data_ptr() if M else 0
                    tab[l].M = M
            self._bound_targets = bbox_targets

    def _rebind_inputs(self, s, t):
        for arr, k, who, l in self._in_slots:
            arr[k].x = (s if who == "student" else t)[l].data_ptr()

    # -- segments (the names the full model drives) ---------------------------------------------------
    def pack_student(self, want_dgrad=True):
        self.prog.run("pack", "forward", timing=self.timing)

    def pack_teacher(self):
        """The teacher is frozen: packed once (and again after its weights are loaded)."""
        if self.distill:
            self.prog_teacher_pack.run()
            self._teacher_packed = True

    def forward_all(self, teacher_fpn, student_fpn):
        if self.distill and not self._teacher_packed:
            self.pack_teacher()
        self._bind(student_fpn=student_fpn, teacher_fpn=teacher_fpn if self.distill else None)
        self.prog.run("forward", "losses", timing=self.timing)
        return self.cls_logits, self.bbox_pred

    def cls_losses(self, labels, fg_num):
        """With bbox_losses_fwd_bwd: the full reference loss set (kept as two calls for the
        full model's driver; both run in the one "losses" segment)."""
        self._pending_labels, self._pending_fg = labels, fg_num
        return self.losses, self.focal_losses

    def bbox_losses_fwd_bwd(self, bbox_targets, fg_num):
        self._bind(labels=self._pending_labels, bbox_targets=bbox_targets, fg_num=fg_num)
        self.prog.run("losses", "backward", timing=self.timing)
        return self.d_bbox_pred

    def distill_loss(self, labels):
        """Distillation loss only (forward + gradient w.r.t. the logits)."""
        self._bind(labels=labels)
        self.prog_distill_only.run(timing=self.timing)
        return self.losses

    def backward(self, d_bbox_pred=None):
        if d_bbox_pred is not None and d_bbox_pred is not self.d_bbox_pred:
            for dst, src in zip(self.d_bbox_pred, d_bbox_pred):
                dst.copy_(src)
        self.prog.run("backward", "backward_late_done", timing=self.timing)
        self._allreduce_async("late")
        self.prog.run("backward_late_done", "sgd", timing=self.timing)
        self._allreduce_async("early")
        return self.d_fpn

    # -- data parallel ------------------------------------------------------------------
    def _allreduce_async(self, tower):
        if tower in self.grads.bucket:
            self.dp.issue(self.grads.bucket[tower])

    def wait_gradients(self):
        self.dp.wait()

    def broadcast_params(self, src=0):
        """Initial parameter sync (detectron/lib/utils/net.py:185-208 walks all of model.params, which in a
        distillation model holds the teacher's blobs too): student parameters, their history and the frozen
        teacher's parameters."""
        if not self.dp.active:
            return
        tensors = [self.params.flat, self.moms.flat]
        if self.teacher is not None:
            tensors.append(self.teacher.flat)
            self._teacher_packed = False         # repack from the received values
        self.dp.broadcast(tensors, src=src)

    # -- learning rate (detector.py:594-648) ------------------------------------------
    SCALE_MOMENTUM = True             # cfg.SOLVER.SCALE_MOMENTUM (config.py:634)
    SCALE_MOMENTUM_THRESHOLD = 1.1    # config.py:638

    def update_lr(self, new_lr):
        """UpdateWorkspaceLr: set the step's learning rate; when it changes by more
        than the threshold the update history V (= mu*V + lr*grad, so it carries
        the old lr) is rescaled by new/old in one pass over the flat momentum
        buffer (_CorrectMomentum runs one Scale op per parameter)."""
        cur_lr = float(self.lr.item())
        new_lr = float(np.float32(new_lr))
        if cur_lr == new_lr:
            return new_lr
        eps = 1e-10
        ratio = max(new_lr / max(cur_lr, eps), cur_lr / max(new_lr, eps))
        self.lr.fill_(new_lr)
        if self.SCALE_MOMENTUM and cur_lr > 1e-7 and ratio > self.SCALE_MOMENTUM_THRESHOLD:
            K.scale_(self.moms.flat, new_lr / cur_lr)
        return new_lr

    def sgd_step(self):
        """Wait for the reduced gradients, then the whole model's update in one launch."""
        self.wait_gradients()
        self.prog.run("sgd", "end", timing=self.timing)

    # -- one iteration --------------------------------------------------------------------
    def step(self, student_fpn, teacher_fpn, labels, d_bbox_pred=None, update=True,
             bbox_targets=None, fg_num=None):
        """One iteration.  With `bbox_targets` and `fg_num` the student's supervised losses are
        part of the step (the full reference graph); without them only the distillation loss
        drives the cls subnet and `d_bbox_pred` must supply the box-subnet gradient."""
        if bbox_targets is None and not self.distill:
            raise K.KernelError("student-only training needs bbox_targets and fg_num")
        self.pack_student()
        self.forward_all(teacher_fpn, student_fpn)
        if bbox_targets is not None:
            self.cls_losses(labels, fg_num)
            self.bbox_losses_fwd_bwd(bbox_targets, fg_num)
            d_bbox_pred = None
        else:
            self.distill_loss(labels)
        self.backward(d_bbox_pred)
        if update:
            self.sgd_step()
        else:
            self.wait_gradients()
        return self.losses


class DistillHeadsF16(DistillHeads):
    """The same iteration with fp16 storage and fp32 accumulation in the subnet convolutions
    (BASELINE config 5's precision; the reference's only fp16 route is CudnnConvOp<float16>
    with fp32 math, caffe2/operators/conv_op_cudnn.cc:631-636).  Mixed precision in the usual
    arrangement: fp32 master parameters, momentum and parameter gradients (FlatParams, SGD and
    the all-reduce are unchanged); filters re-rounded to fp16 every step; activations between
    the layers channel-blocked fp16; prediction layers write NCHW fp32 for the fp32 loss
    kernels; the gradient of the logits is multiplied by a loss scale before it is rounded to
    fp16 (its elements are ~1e-6) and every result leaving the fp16 domain -- filter / bias
    gradients, the gradient w.r.t. the FPN levels -- is divided by it again.

    The loss scale is DYNAMIC and lives on the device (ssad_loss_scale_update): after the
    gradient all-reduce one pass checks the flat fp32 gradient buffer for Inf / NaN; on
    overflow the SGD launch drops the step (every rank sees the same reduced buffer, so all
    ranks drop it together) and the scale is halved, after LOSS_SCALE_GROWTH_INTERVAL clean
    steps it is doubled.  Nothing of this visits the host."""

    F16 = True
    LOSS_SCALE = 8192.0                 # initial value
    LOSS_SCALE_GROWTH_INTERVAL = 2000
    LOSS_SCALE_MIN, LOSS_SCALE_MAX = 1.0, 65536.0

    def _blk(self, ch):
        return [torch.empty((self.N, (ch + 7) // 8, h, w, 8), dtype=torch.float16, device=self.device)
                for (h, w) in self.shapes]

    def _alloc_buffers(self):
        cfg, lv, blk, D = self.cfg, self._lv, self._blk, self.D
        self.fpn_in = lv(D)
        self.t_fpn_in = self.fpn_in
        self.labels = [torch.zeros((self.N, self.A, h, w), dtype=torch.int32, device=self.device)
                       for (h, w) in self.shapes]
        self.act = {t: [blk(D) for _ in range(cfg.num_convs)] for t in ("cls", "bbox")}
        self.cls_logits, self.bbox_pred = lv(self.A * self.C), lv(4 * self.A)
        self.d_cls_logits, self.d_bbox_pred = lv(self.A * self.C), lv(4 * self.A)
        self.dy_pred = {"cls": blk(self.A * self.C), "bbox": blk(4 * self.A)}
        self.dbuf = {t: [blk(D) for _ in range(cfg.num_convs + 1)] for t in ("cls", "bbox")}
        self.d_fpn = {t: lv(D) for t in ("cls", "bbox")}
        self.in_blk = {"student": blk(D)}
        if self.distill:
            self.in_blk["teacher"] = blk(D)
            self.t_buf = {"cls": [blk(D), blk(D)], "bbox": [blk(D), blk(D)]}
            self.t_prob = lv(self.A * self.C)
            self.t_bbox = lv(4 * self.A) if self.teacher_bbox_tower else None
        # {scale, 1/scale} and {overflow flag, clean steps}
        self.ls_state = torch.tensor([self.LOSS_SCALE, 1.0 / self.LOSS_SCALE], dtype=torch.float32,
                                     device=self.device)
        self.ls_counters = torch.zeros(2, dtype=torch.int32, device=self.device)

    @property
    def loss_scale(self):
        return float(self.ls_state[0])

    def _alloc_packed(self, params, who):
        """-> ({layer: (fwd, dgrad or None)}, what _emit_pack needs: here kernels.f16_pack_entries()'s entries)"""
        packed, ops, want_dgrad = {}, [], who == "student"
        for tower in ("cls", "bbox"):
            for name in self._layers(tower):
                w = params[name + "_w"]
                M, Cc = w.shape[0], w.shape[1]
                n = K.lib().ssad_f16_filter_halves(M, Cc)
                wf = torch.empty(n, dtype=torch.float16, device=self.device)
                wd = torch.empty(n, dtype=torch.float16, device=self.device) if want_dgrad else None
                packed[name] = (wf, wd)
                ops.append((w, wf, wd, M, Cc, 9))
        return packed, ops

    def _emit_pack(self, P, entries):
        """All of a network's filters in one launch (ssad_f16_pack_filters)."""
        emit_f16_packs(P, 33, entries)

    def _emit_conv16(self, P, problems, Cin, Cout, flags, klass):
        emit_conv3x3_f16(P, klass, self._rows(problems), Cin, Cout, flags)

    def _emit_forward(self, P):
        cfg, D = self.cfg, self.D
        AC, A4 = self.A * self.C, 4 * self.A
        self._in_ops = []
        act_bytes = lambda x: 6.0 * x.numel()
        for who in (("student", "teacher") if self.distill else ("student",)) if not self.blocked_io else ():
            src = self.fpn_in if who == "student" else self.t_fpn_in
            for l, (x, xb) in enumerate(zip(src, self.in_blk[who])):
                idx = P.add(PR.F16_PACK_ACT, 32, i=(x.shape[0], x.shape[1], x.shape[2], x.shape[3]), f=(1.0,),
                            p=(x, None, xb), work=act_bytes(x))
                self._in_ops.append((idx, who, l))
        tx = {"cls": self.in_blk.get("teacher"), "bbox": self.in_blk.get("teacher")}
        sx = {"cls": self.in_blk["student"], "bbox": self.in_blk["student"]}
        for i in range(cfg.num_convs):
            # the tower layers of equal depth (teacher / student x cls / bbox) are independent
            # convolutions of one shape: ONE launch of up to 20 (level, filter) problems
            probs = []
            for t in ("cls", "bbox"):
                name = self._layers(t)[i]
                if self.distill and (t == "cls" or self.teacher_bbox_tower):
                    out = self.t_buf[t][i & 1]
                    probs.append((tx[t], out, None, self.t_packed_for(name), self.teacher[name + "_b"]))
                    tx[t] = out
                out = self.act[t][i]
                probs.append((sx[t], out, None, self.packed[name][0], self.params[name + "_b"]))
                sx[t] = out
            self._emit_conv16(P, probs, D, D, K.CONV_RELU, 34)
        cp, bp = self._layers("cls")[-1], self._layers("bbox")[-1]
        F32 = K.F16_OUT_NCHW_F32
        if self.distill:
            self._emit_conv16(P, [(tx["cls"], self.t_prob, None, self.t_packed_for(cp), self.teacher[cp + "_b"])],
                              D, AC, K.CONV_SIGMOID | F32, 35)
        self._emit_conv16(P, [(sx["cls"], self.cls_logits, None, self.packed[cp][0], self.params[cp + "_b"])],
                          D, AC, F32, 35)
        self._emit_conv16(P, [(sx["bbox"], self.bbox_pred, None, self.packed[bp][0], self.params[bp + "_b"])],
                          D, A4, F32, 36)
        if self.teacher_bbox_tower:
            self._emit_conv16(P, [(tx["bbox"], self.t_bbox, None, self.t_packed_for(bp), self.teacher[bp + "_b"])],
                              D, A4, F32, 36)

    def _emit_wgrad16(self, P, xbs, dybs, name, Cin, Cout):
        emit_conv3x3_wgrad_f16(P, 37, xbs, dybs, self.grads[name + "_w"], self.grads[name + "_b"], Cin, Cout,
                               self.ls_state[1:2], self._fork)

    def _emit_backward(self, P):
        cfg, D = self.cfg, self.D
        nl, nlev = cfg.num_convs, len(self.shapes)
        S, Sinv = self.ls_state[0:1], self.ls_state[1:2]
        dy = {}
        for t, src in (("cls", self.d_cls_logits), ("bbox", self.d_bbox_pred)):
            for l in range(nlev):
                x = src[l]
                P.add(PR.F16_PACK_ACT, 32, i=tuple(x.shape), f=(1.0,), p=(x, S, self.dy_pred[t][l]),
                      work=6.0 * x.numel())
            dy[t] = self.dy_pred[t]
        for t, klass in (("cls", 35), ("bbox", 36)):
            name = self._layers(t)[-1]
            x_in = self.act[t][nl - 1]
            Cout = self.params[name + "_b"].numel()
            self._emit_wgrad16(P, x_in, dy[t], name, D, Cout)
            out = self.dbuf[t][nl]
            self._emit_conv16(P, [(dy[t], out, x_in, self.packed[name][1], None)], Cout, D,
                              K.CONV_MASK_AUX, klass)
            dy[t] = out
        for li in range(nl - 1, -1, -1):
            probs = []
            for t in ("cls", "bbox"):
                name = self._layers(t)[li]
                x_in = self.act[t][li - 1] if li > 0 else self.in_blk["student"]
                self._emit_wgrad16(P, x_in, dy[t], name, D, D)
                out = self.dbuf[t][li]
                probs.append((dy[t], out, x_in if li > 0 else None, self.packed[name][1], None))
                dy[t] = out
            self._emit_conv16(P, probs, D, D, K.CONV_MASK_AUX if li > 0 else 0, 34)
            if li == nl // 2:
                P.mark("backward_late_done")
        for t in ("cls", "bbox") if not self.blocked_io else ():
            for l in range(nlev):
                xb, x = dy[t][l], self.d_fpn[t][l]
                P.add(PR.F16_UNPACK_ACT, 32, i=tuple(x.shape), f=(1.0,), p=(xb, Sinv, x), work=6.0 * x.numel())
        if "backward_late_done" not in P.marks:
            P.mark("backward_late_done")

    def _emit_sgd(self, P):
        # "sgd": finiteness check of the reduced gradients | "sgd_update": the update, dropped on
        # overflow | "ls_update": the scale moves and the flag is cleared.  A model that owns more
        # gradients than the subnets' (backbone_pipeline.NativeDistillModel) runs its own checks on
        # the same flag between "sgd" and "sgd_update" and its own updates before "ls_update".
        n = self.grads.flat.numel()
        P.add(PR.CHECK_FINITE, 38, l=(n,), p=(self.grads.flat, self.ls_counters), work=4.0 * n)
        P.mark("sgd_update")
        DistillHeads._emit_sgd(self, P, self.ls_counters)          # the update is skipped on overflow
        P.add(PR.LOSS_SCALE_UPDATE, 38, i=(self.LOSS_SCALE_GROWTH_INTERVAL,),
              f=(2.0, 0.5, self.LOSS_SCALE_MIN, self.LOSS_SCALE_MAX), p=(self.ls_state, self.ls_counters))

    def _rebind_inputs(self, s, t):
        for idx, who, l in self._in_ops:
            self.prog.set_ptr(idx, 0, (s if who == "student" else t)[l])
