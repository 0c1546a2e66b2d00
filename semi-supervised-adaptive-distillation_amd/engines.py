"""Which engine runs a 3x3 convolution of the native fp32 pipelines (head_pipeline.DistillHeads,
backbone_pipeline.NativeResNetFPN): the engine type, the one read of the environment switches, the rules of each
pipeline, the table of |max| words of the split-operand engines (AmaxTable) and the one emitter of each launch record
the pipelines share: the 3x3 records and filter packs of the fp32 programs (emit_conv3x3, emit_conv3x3_wgrad,
emit_packs), those of the fp16 ones (emit_conv3x3_f16, emit_conv3x3_wgrad_f16, emit_f16_packs) and the flat SGD update
(emit_sgd_flat).  An emitter holds its record's slot order, work formula and keep list; the tables come from the
builders of kernels.py.

A pipeline reads the switches once, at construction, asks the rule for every convolution before it allocates
anything, packs each filter in the layout of the planned engine and launches the planned engine on it.  DESIGN.md
section 3.7a has the rules as tables.
"""
import collections
import enum
import os

import torch

from . import kernels as K
from . import program as PR


class Engine(enum.IntEnum):
    """i[4] of a CONV3X3 record (csrc/pipeline/program.cc)."""
    DIRECT = 0      # conv3x3.hip: any width, the parity floor
    F22 = 1         # conv3x3_winograd.hip, F(2x2, 3x3): 4 multiplies per output, from 32 outputs
    F24 = 2         # conv3x3_winograd24.hip, F(2x4, 3x3): 3 multiplies per output, fp32 error ~2e-6 of the output scale
    SPLIT = 3       # conv3x3_split.hip: fp32 operands as hi + lo fp16, three fp16 MFMAs per pair; meets the direct
    #                 kernel's parity floor where F(2x4) needs 2e-5


# WINO_PACK_FILTERS numbers its layouts in i[1] (absent = 0 = F(2x2)); the direct engine's packs are PACK_FILTER records
_PACK_LAYOUT = {Engine.F22: 0, Engine.F24: 2, Engine.SPLIT: 3}


def filter_floats(engine):
    """The library function (cout, cin) -> floats of a filter packed for this engine (0: the engine refuses the widths)."""
    L = K.lib()
    return {Engine.DIRECT: L.ssad_conv_packed_filter_floats, Engine.F22: L.ssad_conv_wino_filter_floats,
            Engine.F24: L.ssad_conv_wino24_filter_floats, Engine.SPLIT: L.ssad_conv_split_filter_floats}[engine]


class Switches(collections.namedtuple("Switches", "wino teacher_f24 student_f24 split_conv")):
    """The four engine switches as the environment gives them.

    SSAD_CONV_ENGINE=direct (wino False): the subnets on the direct kernel everywhere.

    SSAD_TEACHER_F24: the frozen teacher on the F(2x4) engine (admissible where nothing back-propagates): 1 (default)
    its cls_pred layer and its backbone's 3x3 layers of >= 128 outputs; 2: also its tower layers, which then leave
    the launch they shared with the student's; 0 = everything on F(2x2) as in rounds 1-4.

    SSAD_STUDENT_F24, a bit mask (default 15; DESIGN 3.10e has the error and step-time A/B): the TRAINED networks on
    F(2x4): 1 = the subnets' data gradients, 2 = cls_pred forward, 4 = tower forward (with the teacher's towers, one
    launch), 8 = the backbone's 3x3 layers of >= 128 channels, forward and data gradient (the filter gradient keeps
    its F(3x3, 2x2) engine).

    SSAD_SPLIT_CONV, a bit mask: the split-operand engines where they measured faster than F(2x4) at config 3's size:
    1 = cls_pred forward (student and teacher), 2 = its data gradient, 4 = tower forward (both networks, one launch per
    depth), 8 = tower data gradients, 16 = the backbones' >= 256-wide 3x3 layers, 32 = the subnets' >= 128-wide filter
    gradients (conv3x3_wgrad_split.hip), 64 = the backbones' >= 256-wide ones, 128 = the backbones' pointwise layers
    with K, M >= 256 on the split-operand GEMM, 256 = their filter gradients (gemm_split.hip); 0 = off.  Default 511:
    same-box A/B of the step 86.0 -> 83.9 ms for bits 1-16 (every bit pays in the step although the isolated launches
    are level with F(2x4): the step is power-bound, and the engine spends less of it; bit 16 alone -0.1 ... -1.3 ms in
    four pairs), 82.6 -> 78.3 ms for bits 32 + 64, 78.9 -> 73.5 ms for bit 128, 72.6 -> 70.4 ms for bit 256
    (profiles/r06_experiments.md)."""
    __slots__ = ()

    @classmethod
    def read(cls, env=None):
        env = os.environ if env is None else env
        return cls(env.get("SSAD_CONV_ENGINE", "winograd").lower() != "direct", int(env.get("SSAD_TEACHER_F24", "1")),
                   int(env.get("SSAD_STUDENT_F24", "15")), int(env.get("SSAD_SPLIT_CONV", "511")))

    def for_subnets(self, distill, f16=False):
        """What the subnets make of the switches.  The fp16-storage subnets have kernels of their own, and the direct
        engine has no variants: all masks 0.  The towers of one depth (teacher + student) are ONE launch on ONE
        engine when their widths agree: bit 4 of SSAD_STUDENT_F24 takes the teacher's towers along; with the teacher
        pinned to F(2x2) (SSAD_TEACHER_F24=0) a distillation step keeps the shared launch there and bit 4 is void."""
        if f16 or not self.wino:
            return self._replace(teacher_f24=0, student_f24=0, split_conv=0)
        teacher, student = self.teacher_f24, self.student_f24 & 7
        if student & 4:
            if teacher:
                teacher = 2
            elif distill:
                student &= ~4
        return self._replace(teacher_f24=teacher, student_f24=student)


def subnet_engine(sw, who, name, cout, cin, which):
    """Engine of one subnet convolution.  sw: Switches.for_subnets(); who = "teacher" | "student"; name: the layer's
    (retnet_{cls,bbox}_{conv_n<i>,pred}_fpn<k>); which = "fwd" (a launch cin -> cout) | "dgrad" (cout -> cin)."""
    fwd = which == "fwd"
    if not sw.wino or (cout if fwd else cin) < 32:
        return Engine.DIRECT           # narrower than one 32-row tile of the Winograd engines
    pred = "_pred_" in name
    if sw.split_conv & ((1 if fwd else 2) if pred else (4 if fwd else 8)) and _bbox_pred_on_split(name, cout, cin, fwd):
        return Engine.SPLIT
    if who == "teacher":
        f24 = fwd and cout >= 128 and sw.teacher_f24 >= (1 if pred else 2)
    elif fwd:
        f24 = cout >= 128 and sw.student_f24 & (2 if pred else 4)
    else:
        f24 = cin >= 128 and sw.student_f24 & 1
    return Engine.F24 if f24 else Engine.F22


def _bbox_pred_on_split(name, cout, cin, fwd):
    """bbox_pred of the class-agnostic head (4 * A = 36 outputs) stays off the split-operand engine.  A class-specific
    one (RETINANET.CLASS_SPECIFIC_BBOX: 4 * (num_classes - 1) * A outputs, 2880 at 81 classes, 11 tower layers' flops)
    goes where cls_pred goes from 128 outputs -- the width from which the subnets' filter gradients take that engine
    too (subnet_wgrad_split) -- provided the engine's pack-size function accepts the widths of this launch."""
    if "bbox_pred" not in name:
        return True
    if cout < 128:
        return False
    return filter_floats(Engine.SPLIT)(*((cout, cin) if fwd else (cin, cout))) > 0


def backbone_engine(sw, train, cout, cin):
    """Engine of a backbone's ungrouped stride-1 3x3 layer, forward and (trained) data gradient alike.  sw: the
    switches as read.  An engine whose pack-size function refuses the layer's widths (forward, and the data
    gradient's transposed widths when it is trained) sends the layer to the next engine of the chain, the rule of the
    split filter gradient."""
    def accepts(engine):
        return filter_floats(engine)(cout, cin) > 0 and (not train or filter_floats(engine)(cin, cout) > 0)
    f24_on = bool(sw.student_f24 & 8) if train else sw.teacher_f24 >= 1
    if sw.split_conv & 16 and f24_on and cout >= 256 and cin >= 256 and accepts(Engine.SPLIT):
        return Engine.SPLIT
    if f24_on and cout >= 128 and (cin >= 128 or not train) and accepts(Engine.F24):
        return Engine.F24
    if cout < 32 or cin < 32 or not accepts(Engine.F22):
        # narrower than one 32-row tile of the F(2x2) engine (res2 of a quarter-width student, 16 -> 16)
        return Engine.DIRECT
    return Engine.F22


def subnet_wgrad_split(sw, cout, cin):
    """A subnet filter gradient on the split-operand engine (conv3x3_wgrad_split.hip)?  SSAD_SPLIT_CONV bit 32
    (default): the >= 128-wide ones (towers, cls_pred)."""
    return bool(sw.split_conv & 32) and cout >= 128 and cin >= 64


def backbone_wgrad_split(sw, cout, cin):
    """A backbone 3x3 filter gradient on the split-operand engine?  SSAD_SPLIT_CONV bit 64 (default): the >= 256-wide
    ones (the 128-wide res3 layers are level with the F(3x3, 2x2) engine there: 2 blocks of dW, 128 slabs to reduce)."""
    return bool(sw.split_conv & 64) and cout >= 256 and cin >= 256


def same_engine(engines):
    """The one engine of a launch; problems planned on different engines cannot share one."""
    engines = set(engines)
    if len(engines) != 1:
        raise K.KernelError("one launch, several engines: %s" % sorted(e.name for e in engines))
    return engines.pop()


conv_table = K.conv_levels         # the name this table's builder had here


def emit_packs(P, klass, packs, order):
    """packs: {Engine: [(w, cout, cin, packed_fwd or None, packed_dgrad or None)]}: one WINO_PACK_FILTERS launch per
    layout, one PACK_FILTER record per filter of the direct engine, in this order of engines."""
    for engine in order:
        entries = packs.get(engine, ())
        moved = [4 * (w.numel() + sum(t.numel() for t in (pf, pd) if t is not None)) for w, _, _, pf, pd in entries]
        if engine == Engine.DIRECT:
            for (w, cout, cin, pf, pd), nbytes in zip(entries, moved):
                P.add(PR.PACK_FILTER, klass, i=(cout, cin), p=(w, pf, pd), work=nbytes)
        elif entries:
            P.add(PR.WINO_PACK_FILTERS, klass, i=(len(entries), _PACK_LAYOUT[engine]), p=(K.pack_entries(entries),),
                  work=sum(moved),
                  keep=[t for w, _, _, pf, pd in entries for t in (w, pf, pd) if t is not None])


class AmaxTable(object):
    """The |max| words of one pipeline's split-operand engines: `tensor` (int32, zeroed by the pipeline's ONE fill at
    the start of its forward segment), the next free word and {tensor addresses: word}.  A stale or unwritten word is
    a wrong power-of-two scale, so: a launch's words are one block of consecutive words in its operand order; the
    block is found again by the whole group list, by each group and -- where a group is one tensor -- by the tensor
    (a filter gradient reads one tower's levels, or one tensor, of the launch that produced or first read them); a
    tensor nobody folded is measured once, on the main stream, in front of its first reader, and a later reader on an
    auxiliary stream is handed the word.  Tensors go by address: every activation / gradient buffer of a program is
    allocated once and written once per step before its readers."""

    def __init__(self, words, device):
        self.words, self.next, self.word = words, 0, {}
        self.tensor = torch.zeros(words, dtype=torch.int32, device=device)

    def addr(self, k):
        return self.tensor.data_ptr() + 4 * k

    def find(self, groups):
        return self.word.get(tuple(t.data_ptr() for g in groups for t in g))

    def reserve(self, groups):
        """First word of a fresh block for groups = [[tensor]]: their PRODUCER's epilogue folds the |max| in, or
        measure() writes them.  (The freshest words serve later readers.)"""
        base = k = self.next
        self.next += sum(len(g) for g in groups)
        if self.next > self.words:
            raise K.KernelError("|max| table full")
        self.word[tuple(t.data_ptr() for g in groups for t in g)] = base
        for g in groups:
            self.word[tuple(t.data_ptr() for t in g)] = k
            k += len(g)
        return base

    def measure(self, P, groups, channels, table=None, field=0):
        """First word of the groups' block: found, or measured here on the main stream into a fresh block -- through
        `table` (the reading launch's own ssad_conv_level[], field 0 = x, 1 = aux), else one tensor by SPLIT_ABSMAX
        and several through a level table of their own."""
        base = self.find(groups)
        if base is None:
            base = self.reserve(groups)
            ts = [t for g in groups for t in g]
            nbytes = 4.0 * sum(t.numel() for t in ts)
            if table is None and len(ts) == 1:
                P.add(PR.SPLIT_ABSMAX, 73, p=(ts[0], self.addr(base)), l=(ts[0].numel(),), work=nbytes, stream=0)
            else:
                if table is None:
                    table, field = K.conv_levels([(t, None, None, None, None) for t in ts]), 0
                P.add(PR.SPLIT_ABSMAX_LEVELS, 73, i=(len(ts), channels, field), p=(table, self.addr(base)),
                      work=nbytes, keep=ts, stream=0)
        return base


def _pixels(xs):
    return sum(x.shape[0] * x.shape[2] * x.shape[3] for x in xs)


def emit_conv3x3(P, klass, rows, cout, cin, flags, engine, amax, ws, levels=1, own_table=False, fold=True):
    """One CONV3X3 record: independent convolutions of one (cout, cin) on one engine.  rows: K.conv_levels()'s, `levels`
    consecutive rows per problem.  The split-operand engine takes its workspace `ws`, the words of its inputs (found
    or measured: through its own table when own_table) and, when fold, fresh words its epilogue folds the outputs'
    |max| into.  -> (record index, table)"""
    arr = K.conv_levels(rows)
    ptrs, sizes = (arr, None, None), ()
    if engine == Engine.SPLIT:
        nb = K.lib().ssad_conv3x3_split_workspace_bytes(arr, len(arr), cin)
        groups = lambda f: [[r[f] for r in rows[k:k + levels]] for k in range(0, len(rows), levels)]
        xa = amax.addr(amax.measure(P, groups(0), cin, arr if own_table else None))
        ya = amax.addr(amax.reserve(groups(1))) if fold else None
        ptrs, sizes = (arr, None, None, ws.need(nb), xa, ya), (nb,)
    return P.add(PR.CONV3X3, klass, i=(len(arr), cout, cin, flags, engine), l=sizes, p=ptrs,
                 work=2.0 * 9 * cout * cin * _pixels(r[0] for r in rows),
                 keep=[t for r in rows for t in r if t is not None]), arr


def emit_conv3x3_wgrad(P, klasses, xs, dys, gw, gb, cout, cin, split, amax, fork, own_table=False):
    """One CONV3X3_WGRAD record over the levels xs / dys that share the filter gradient gw (+ bias gradient gb).
    split: the pipeline's rule wants the split-operand engine (a level of 2 GiB or more still goes to the exact
    one); klasses = (exact, split) timing classes.  The operands' words are found or measured on the main stream;
    then fork(P) emits the pipeline's fork and returns the record's (stream, Workspace).  -> (record index, table)"""
    arr = K.conv_levels([(x, None, dy, None, None) for x, dy in zip(xs, dys)])
    L = K.lib()
    nb = L.ssad_conv3x3_wgrad_split_workspace_bytes(arr, len(arr), cout, cin) if split else 0
    split = nb > 0
    xa = da = None
    if split:
        xa = amax.addr(amax.measure(P, [list(xs)], cin, arr if own_table else None, 0))
        da = amax.addr(amax.measure(P, [list(dys)], cout, arr if own_table else None, 1))
    else:
        nb = L.ssad_conv3x3_wgrad_workspace_bytes(arr, len(arr), cout, cin)
    stream, ws = fork(P)
    return P.add(PR.CONV3X3_WGRAD, klasses[split], i=(len(arr), cout, cin, 0, int(split)), l=(nb,),
                 p=(arr, gw, gb, ws.need(nb), xa, da), work=2.0 * 9 * cout * cin * _pixels(xs),
                 keep=list(xs) + list(dys), stream=stream), arr


def emit_conv3x3_f16(P, klass, rows, cin, cout, flags):
    """One F16_CONV3X3 record: independent fp16 convolutions of one (cin, cout), kernels.f16_levels()'s rows.
    -> (record index, table)"""
    arr = K.f16_levels(rows)
    return P.add(PR.F16_CONV3X3, klass, i=(len(arr), cin, cout, flags), p=(arr, None, None),
                 work=2.0 * 9 * cout * cin * _pixels(r[0] for r in rows),
                 keep=[t for r in rows for t in r if t is not None]), arr


def emit_conv3x3_wgrad_f16(P, klass, xs, dys, gw, gb, cin, cout, inv_scale, fork):
    """One F16_WGRAD record over the levels xs / dys that share the filter gradient gw (+ bias gradient gb), both times
    the device scalar inv_scale; fork(P) as for emit_conv3x3_wgrad.  -> (record index, table)"""
    arr = K.f16_wgrad_levels(xs, dys)
    nb = K.lib().ssad_conv3x3_wgrad_f16_levels_workspace_bytes(arr, len(arr), cin, cout)
    stream, ws = fork(P)
    return P.add(PR.F16_WGRAD, klass, i=(len(arr), cin, cout, 0), f=(1.0,), l=(nb,),
                 p=(arr, inv_scale, gw, gb, ws.need(nb)), work=2.0 * 9 * cout * cin * _pixels(xs),
                 keep=list(xs) + list(dys), stream=stream), arr


def emit_f16_packs(P, klass, entries):
    """One F16_PACK_FILTERS record: kernels.f16_pack_entries()'s entries in one launch; nothing for an empty list."""
    if entries:
        P.add(PR.F16_PACK_FILTERS, klass, i=(len(entries),), p=(K.f16_pack_entries(entries),),
              work=sum(4.0 * e[0].numel() + 2.0 * sum(t.numel() for t in e[1:3] if t is not None) for e in entries),
              keep=[t for e in entries for t in e[:3] if t is not None])


def emit_sgd_flat(P, klass, segments, params, grads, moms, lr, momentum, weight_decay, skip_flag):
    """One SGD_FLAT record: the momentum update of the flat buffers by kernels.sgd_segments()'s segments; skip_flag: a
    device word that drops the update when it is set, or None."""
    return P.add(PR.SGD_FLAT, klass, i=(len(segments),), f=(momentum, weight_decay),
                 p=(params, grads, moms, lr, K.sgd_segments(segments), skip_flag), work=4.0 * 6 * params.numel(),
                 keep=[s[4] for s in segments if s[4] is not None])
