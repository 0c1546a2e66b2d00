#!/usr/bin/env python3
"""Fingerprints of the native programs over a matrix of engine switches.

A program is the list of launch records a pipeline builds once (program.Program); which engine a convolution runs
on, which layout its filter is packed in and which timing class it is booked under are all fields of those
records and of the tables they point to.  This script builds every configuration below over CPU tensors
(addresses only, nothing is launched), writes each program down with its addresses made canonical, and hashes the
listing.  tests/test_program_fingerprints.py rebuilds the configurations and compares: a change that is meant to
leave the programs alone (a refactoring of the engine rules) must leave every hash alone.

It uses only Program.ops / .keep / .marks and the pipelines' constructors, so it runs against any commit:

    python tests/golden/make_program_fingerprints.py --write       # tests/golden/program_fingerprints.json and
                                                                   # backbone_buffers.json
    python tests/golden/make_program_fingerprints.py --dump NAME   # one configuration's readable listing
    python tests/golden/make_program_fingerprints.py --list

A mismatch is located by diffing `--dump NAME` of the two commits.

A record names a tensor that is not in Program.keep only by its order of appearance, so the listing does not pin the
shape of an activation or gradient buffer.  backbone_buffers.json does: for every configuration that builds a backbone
(an object with _bufs), the count of its buffers and a sha256 over the sorted list of their (dtype, shape).  Order of
allocation is free.

Canonical addresses: a ctypes table of Program.keep is T<ordinal of first appearance>(+offset); an address inside
the storage of a tensor of Program.keep is S<ordinal of first appearance of that storage>+<byte offset>; any other
address is U<ordinal of first appearance>.  The contents of a table are listed, field by field, where it first
appears; its c_void_p fields are canonical in the same way.  A storage's size is listed where it first appears (a
packed filter's size is its layout's).
"""
import argparse
import bisect
import contextlib
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "program_fingerprints.json")
OUT_BUFFERS = os.path.join(HERE, "backbone_buffers.json")

SWITCHES = ("SSAD_SPLIT_CONV", "SSAD_STUDENT_F24", "SSAD_TEACHER_F24", "SSAD_CONV_ENGINE", "SSAD_STRIDED_3X3")
SHAPES = [(10, 14), (5, 7)]
PROGRAMS = ("prog", "prog_teacher_pack", "prog_distill_only", "prep")


# ---------------------------------------------------------------------------------------------------------------
# the listing
# ---------------------------------------------------------------------------------------------------------------
class _Canon(object):
    """Address -> canonical name, over every program of one configuration."""

    def __init__(self, programs):
        import torch
        self.tables, self.storages = {}, {}            # start address -> (size, object)
        for P in programs:
            for v in P.keep:
                if isinstance(v, torch.Tensor):
                    st = v.untyped_storage()
                    if st.nbytes() > 0:
                        self.storages[st.data_ptr()] = (st.nbytes(), None)
                elif isinstance(v, (C.Structure, C.Array, C._SimpleCData)):
                    self.tables[C.addressof(v)] = (C.sizeof(v), v)
        self.t_starts, self.s_starts = sorted(self.tables), sorted(self.storages)
        self.t_ord, self.s_ord, self.u_ord = {}, {}, {}
        self.pending = []                              # tables named but not yet listed
        self.new_storages = []                         # storages named but their sizes not yet listed

    @staticmethod
    def _find(starts, ranges, a):
        k = bisect.bisect_right(starts, a) - 1
        if k >= 0 and a < starts[k] + ranges[starts[k]][0]:
            return starts[k]
        return None

    def name(self, a):
        if not a:
            return "0"
        t = self._find(self.t_starts, self.tables, a)
        if t is not None:
            if t not in self.t_ord:
                self.t_ord[t] = len(self.t_ord)
                self.pending.append(t)
            return "T%d" % self.t_ord[t] + ("+%d" % (a - t) if a != t else "")
        s = self._find(self.s_starts, self.storages, a)
        if s is not None:
            if s not in self.s_ord:
                self.s_ord[s] = len(self.s_ord)
                self.new_storages.append(s)
            return "S%d+%d" % (self.s_ord[s], a - s)
        return "U%d" % self.u_ord.setdefault(a, len(self.u_ord))

    def value(self, v):
        """One ctypes value, written down."""
        if isinstance(v, C.c_void_p):
            return self.name(v.value)
        if isinstance(v, C.Array):
            if issubclass(v._type_, C.c_void_p):
                return "[" + " ".join(self.name(x) for x in v) + "]"
            if issubclass(v._type_, (C.Structure, C.Array)):
                return "[" + " ".join(self.value(x) for x in v) + "]"
            return "[" + " ".join(repr(x) for x in v) + "]"
        if isinstance(v, C.Structure):
            parts = []
            for fname, ftype in v._fields_:
                x = getattr(v, fname)
                if issubclass(ftype, C.c_void_p):
                    parts.append("%s=%s" % (fname, self.name(x)))
                elif issubclass(ftype, (C.Structure, C.Array)):
                    parts.append("%s=%s" % (fname, self.value(x)))
                else:
                    parts.append("%s=%r" % (fname, x))
            return "{" + " ".join(parts) + "}"
        if isinstance(v, C._SimpleCData):
            return repr(v.value)
        return repr(v)

    def drain(self, lines):
        """List the tables named since the last call (a table may name further tables)."""
        while self.pending:
            t = self.pending.pop(0)
            v = self.tables[t][1]
            head = "  T%d %s" % (self.t_ord[t], type(v).__name__)
            if isinstance(v, C.Array) and issubclass(v._type_, (C.Structure, C.Array)):
                lines.append(head)
                for k, x in enumerate(v):
                    lines.append("    [%d] %s" % (k, self.value(x)))
            else:
                lines.append(head + " " + self.value(v))
        for s in self.new_storages:
            lines.append("  S%d %d bytes" % (self.s_ord[s], self.storages[s][0]))
        del self.new_storages[:]


def listing(objects):
    """Readable listing of every program of the objects of one configuration -> (lines, op count)."""
    named = []
    for k, obj in enumerate(objects):
        for attr in PROGRAMS:
            P = getattr(obj, attr, None)
            if P is not None:
                named.append(("%d.%s" % (k, attr), P))
    canon = _Canon([P for _, P in named])
    lines, nops = [], 0
    for title, P in named:
        lines.append("program %s: %d ops, marks %s" % (title, len(P.ops), " ".join("%s=%d" % kv for kv in P.marks.items())))
        nops += len(P.ops)
        for k, o in enumerate(P.ops):
            lines.append("%4d code=%d klass=%d stream=%d i=%s f=%s l=%s work=%r p=%s" % (
                k, o.code, o.klass, o.stream, list(o.i), [repr(x) for x in o.f], list(o.l), o.work,
                [canon.name(a) for a in o.p]))
            canon.drain(lines)
    return lines, nops


# ---------------------------------------------------------------------------------------------------------------
# the configurations
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**env):
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@contextlib.contextmanager
def _gemm_split_min_pixels(n):
    """backbone_pipeline.GEMM_SPLIT_MIN_PIXELS = n around a build: at 128 x 128, N = 1 the default keeps every
    pointwise layer off the split-operand route."""
    from ssad_amd import backbone_pipeline as BP
    saved, BP.GEMM_SPLIT_MIN_PIXELS = BP.GEMM_SPLIT_MIN_PIXELS, n
    try:
        yield
    finally:
        BP.GEMM_SPLIT_MIN_PIXELS = saved


def _matrix():
    return [dict(SSAD_SPLIT_CONV=s, SSAD_STUDENT_F24=f, SSAD_TEACHER_F24=t)
            for s in (0, 3, 15, 47, 511) for f in (0, 1, 3, 7, 15) for t in (0, 1, 2)]


def _tag(env):
    return "split%d_sf%d_tf%d" % (env["SSAD_SPLIT_CONV"], env["SSAD_STUDENT_F24"], env["SSAD_TEACHER_F24"])


def configurations():
    """[(name, environment, builder -> list of pipeline objects)]"""
    from ssad_amd.backbone_f16 import NativeResNetFPNF16
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    from ssad_amd.head_pipeline import DistillHeads, DistillHeadsF16
    from ssad_amd.modeling.retinanet_heads import HeadConfig

    def heads(cls=DistillHeads, cfg=None, shapes=SHAPES, **kw):
        return lambda: [cls(cfg or HeadConfig(num_gpus=1), N=1, shapes=shapes, device="cpu", **kw)]

    def backbone(arch="r50", cls=NativeResNetFPN, **kw):
        return lambda: [cls(arch, 1, (128, 128), "cpu", **kw)]

    def pointwise(arch="r50", **kw):
        """The pointwise layers on the split-operand route (GEMM_CONV_SPLIT, split CONV1X1_WGRAD)."""
        def build():
            with _gemm_split_min_pixels(0):
                return backbone(arch, **kw)()
        return build

    def f16_pair():
        shapes = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
        h = DistillHeadsF16(HeadConfig(num_gpus=1), N=1, shapes=shapes, device="cpu", blocked_io=True)
        st = NativeResNetFPNF16("r50", 1, (128, 128), "cpu", train=True,
                                heads_io=dict(fpn_out=h.in_blk["student"], inv_scale=h.ls_state[1:2],
                                              d_fpn_in=(h.dbuf["cls"][0], h.dbuf["bbox"][0])),
                                skip_flag=h.ls_counters)
        te = NativeResNetFPNF16("x101-64x4d", 1, (128, 128), "cpu", train=False,
                                heads_io=dict(fpn_out=h.in_blk["teacher"]))
        return [h, st, te]

    out = []
    for env in _matrix():
        for distill in (True, False):
            out.append(("heads_%s_%s" % (_tag(env), "distill" if distill else "plain"), env, heads(distill=distill)))
    out.append(("heads_direct", dict(SSAD_CONV_ENGINE="direct"), heads()))
    out.append(("heads_no_teacher_bbox_tower", {}, heads(teacher_bbox_tower=False)))
    out.append(("heads_no_overlap_wgrad", {}, heads(overlap_wgrad=False)))
    for dim in (128, 64):
        for tag, env in (("default", {}), ("split0", dict(SSAD_SPLIT_CONV=0))):
            out.append(("heads_thin%d_%s" % (dim, tag), env,
                        heads(cfg=HeadConfig(num_gpus=1, fpn_dim=dim), teacher_fpn_dim=256)))
    out.append(("heads_f16", {}, heads(cls=DistillHeadsF16)))
    for env in _matrix()[::7]:
        for train in (True, False):
            out.append(("r50_%s_%s" % (_tag(env), "train" if train else "frozen"), env, backbone(train=train)))
    for ratio in (0.5, 0.25):
        out.append(("r50_ratio%d_train" % int(ratio * 100), {}, backbone(train=True, channel_ratio=ratio)))
    out.append(("r101_frozen", {}, backbone("r101", train=False)))
    out.append(("x101_64x4d_frozen", {}, backbone("x101-64x4d", train=False)))
    out.append(("r50_strided_winograd_train", dict(SSAD_STRIDED_3X3="winograd"), backbone(train=True)))
    out.append(("f16_pair", {}, f16_pair))
    for bits in (511, 255):
        out.append(("r50_pointwise_split%d_train" % bits, dict(SSAD_SPLIT_CONV=bits), pointwise(train=True)))
    for arch in ("r50", "r101", "x101-64x4d"):
        out.append(("%s_pointwise_split511_frozen" % arch.replace("-", "_"), dict(SSAD_SPLIT_CONV=511),
                    pointwise(arch, train=False)))
    # one level: a launch's whole key and its per-problem key coincide in the |max| word table
    for distill in (True, False):
        out.append(("heads_one_level_%s" % ("distill" if distill else "plain"), {},
                    heads(shapes=[(5, 7)], distill=distill)))
    # without the auxiliary streams, and the fp16 backbone without the heads' hand-over
    out.append(("r50_no_overlap_wgrad_train", {}, backbone(train=True, overlap_wgrad=False)))
    out.append(("heads_f16_no_overlap_wgrad", {}, heads(cls=DistillHeadsF16, overlap_wgrad=False)))
    out.append(("f16_r50_own_io_train", {}, backbone(cls=NativeResNetFPNF16, train=True)))
    out.append(("f16_r50_own_io_no_overlap_wgrad_train", {},
                backbone(cls=NativeResNetFPNF16, train=True, overlap_wgrad=False)))
    # the fp16 subnets without a teacher and on blocked input, the frozen fp16 teachers (the second one has the
    # GROUPED_F16_CG64 records) and a trained ResNeXt, the one program with a GROUPED_PACKS table
    out.append(("heads_f16_plain", {}, heads(cls=DistillHeadsF16, distill=False)))
    out.append(("heads_f16_blocked_one_level", {}, heads(cls=DistillHeadsF16, shapes=[(5, 7)], blocked_io=True)))
    out.append(("f16_r101_frozen", {}, backbone("r101", cls=NativeResNetFPNF16, train=False)))
    out.append(("f16_x101_32x8d_wide_frozen", {},
                backbone("x101-32x8d", cls=NativeResNetFPNF16, train=False, wide_groups=True)))
    out.append(("x101_64x4d_grouped_grad_train", {}, backbone("x101-64x4d", train=True, grouped_grad=True)))
    # branches of the two backbone walks that the matrix above reaches at one width or in one precision only
    wino = dict(SSAD_STRIDED_3X3="winograd")
    out.append(("x101_32x8d_frozen", {}, backbone("x101-32x8d", train=False)))
    out.append(("x101_32x8d_grouped_grad_train", {}, backbone("x101-32x8d", train=True, grouped_grad=True)))
    out.append(("r101_train", {}, backbone("r101", train=True)))
    out.append(("r50_strided_winograd_frozen", wino, backbone(train=False)))
    out.append(("x101_64x4d_strided_winograd_grouped_grad_train", wino,
                backbone("x101-64x4d", train=True, grouped_grad=True)))
    out.append(("f16_r50_frozen", {}, backbone(cls=NativeResNetFPNF16, train=False)))
    out.append(("f16_r101_train", {}, backbone("r101", cls=NativeResNetFPNF16, train=True)))
    out.append(("f16_x101_64x4d_frozen", {}, backbone("x101-64x4d", cls=NativeResNetFPNF16, train=False)))
    return out


def buffer_record(obj):
    """[count, sha256 over the sorted (dtype, shape) list] of a backbone's activation / gradient / scratch buffers."""
    shapes = sorted((str(t.dtype), tuple(t.shape)) for t in obj._bufs)
    return [len(shapes), hashlib.sha256(repr(shapes).encode()).hexdigest()]


def record(env, build):
    """-> ([sha256 of the listing, op count], [buffer_record of every object that has _bufs])"""
    with _env(**env):
        objects = build()
        lines, nops = listing(objects)
    return ([hashlib.sha256("\n".join(lines).encode()).hexdigest(), nops],
            [buffer_record(o) for o in objects if hasattr(o, "_bufs")])


@functools.lru_cache(maxsize=None)
def records():
    """Every configuration built once -> ({name: fingerprint}, {name: buffer records} of those that build a backbone)"""
    fp, bufs = {}, {}
    for name, env, build in configurations():
        fp[name], b = record(env, build)
        if b:
            bufs[name] = b
    return fp, bufs


def fingerprints():
    return records()[0]


def backbone_buffers():
    return records()[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="write %s" % os.path.relpath(OUT, ROOT))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--out-buffers", default=OUT_BUFFERS)
    ap.add_argument("--dump", metavar="NAME", help="print one configuration's listing")
    ap.add_argument("--list", action="store_true", help="print the configurations' names")
    args = ap.parse_args()
    if args.list:
        print("\n".join(name for name, _, _ in configurations()))
        return
    if args.dump:
        for name, env, build in configurations():
            if name == args.dump:
                with _env(**env):
                    print("\n".join(listing(build())[0]))
                return
        raise SystemExit("no configuration %r (--list)" % args.dump)
    fp, bufs = records()
    if args.write:
        commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
        for path, conf in ((args.out, fp), (args.out_buffers, bufs)):
            with open(path, "w") as f:
                json.dump({"parent": commit, "configurations": conf}, f, indent=0, sort_keys=True)
                f.write("\n")
    print("%d configurations, %d distinct fingerprints, %d with backbone buffers" % (
        len(fp), len({v[0] for v in fp.values()}), len(bufs)))


if __name__ == "__main__":
    main()
