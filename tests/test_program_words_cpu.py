"""The two things a native program's split-operand launches depend on besides their own record: the |max| word
table (engines.AmaxTable: a stale or unwritten word is a wrong power-of-two scale, so fp16 operands saturate or lose
their low half silently) and the workspaces the launches share (program.Workspace: a wrong slot or a missed maximum
is an out-of-bounds write on the device).  Programs are built over CPU tensors; nothing is launched."""
import ctypes

import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import backbone_pipeline as BP, kernels as K, program as PR
from ssad_amd.backbone_f16 import NativeResNetFPNF16
from ssad_amd.engines import AmaxTable
from ssad_amd.kernels import conv_levels as conv_table
from ssad_amd.head_pipeline import DistillHeads, DistillHeadsF16
from ssad_amd.modeling.retinanet_heads import HeadConfig

SHAPES = [(10, 14), (5, 7)]
SWITCHES = ("SSAD_SPLIT_CONV", "SSAD_STUDENT_F24", "SSAD_TEACHER_F24", "SSAD_CONV_ENGINE", "SSAD_STRIDED_3X3",
            "SSAD_OVERLAP_WGRAD")


def _heads(cls=DistillHeads, shapes=SHAPES, **kw):
    return cls(HeadConfig(num_gpus=1), N=1, shapes=shapes, device="cpu", **kw)


def _backbone(arch="r50", cls=BP.NativeResNetFPN, **kw):
    return cls(arch, 1, (128, 128), "cpu", **kw)


BUILDERS = {
    "heads_distill": lambda: _heads(),
    "heads_plain": lambda: _heads(distill=False),
    "heads_one_level_distill": lambda: _heads(shapes=[(5, 7)]),
    "heads_one_level_plain": lambda: _heads(shapes=[(5, 7)], distill=False),
    "r50_pointwise_train": lambda: _backbone(train=True),
    "r101_frozen": lambda: _backbone("r101", train=False),
    "heads_f16": lambda: _heads(DistillHeadsF16),
    "f16_r50_train": lambda: _backbone(cls=NativeResNetFPNF16, train=True),
}


@pytest.fixture
def build(monkeypatch):
    """name -> the pipeline under the default switches, its pointwise layers on the split-operand route (at 128 x 128,
    N = 1 the default GEMM_SPLIT_MIN_PIXELS keeps them all off it)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(BP, "GEMM_SPLIT_MIN_PIXELS", 0)
    return lambda name: BUILDERS[name]()


# ---------------------------------------------------------------------------------------------------------------
# word dataflow
# ---------------------------------------------------------------------------------------------------------------
def _word_reads(o):
    """[(first word's address, words)] a record reads"""
    if o.code == PR.CONV3X3 and o.i[4] == 3:
        return [(o.p[4], o.i[0])]
    if o.code == PR.CONV3X3_WGRAD and o.i[4] == 1:
        return [(o.p[4], o.i[0]), (o.p[5], o.i[0])]
    if o.code == PR.GEMM_CONV_SPLIT:
        return [(o.p[3], 1)]
    if o.code == PR.CONV1X1_WGRAD and o.i[5] == 1:
        return [(o.p[4], 1), (o.p[5], 1)]
    return []


def _word_writes(o):
    if o.code == PR.SPLIT_ABSMAX:
        return [(o.p[1], 1)]
    if o.code == PR.SPLIT_ABSMAX_LEVELS:
        return [(o.p[1], o.i[0])]
    if o.code == PR.CONV3X3 and o.i[4] == 3 and o.p[5]:
        return [(o.p[5], o.i[0])]
    if o.code == PR.GEMM_CONV_SPLIT and o.p[4]:
        return [(o.p[4], 1)]
    return []


@pytest.mark.parametrize("name", ["heads_distill", "heads_plain", "heads_one_level_distill", "heads_one_level_plain",
                                  "r50_pointwise_train", "r101_frozen"])
def test_every_word_read_was_written_once_by_an_earlier_record(build, name):
    obj = build(name)
    lo, hi = obj.amax.data_ptr(), obj.amax.data_ptr() + 4 * obj.AMAX_WORDS
    assert obj.amax.dtype == torch.int32 and obj.amax.numel() == obj.AMAX_WORDS
    fills = [k for k, o in enumerate(obj.prog.ops) if o.code == PR.FILL and o.p[0] == lo]
    assert len(fills) == 1 and obj.prog.ops[fills[0]].l[0] == obj.AMAX_WORDS      # ONE fill, of the whole table
    written, reads = set(), 0
    for k, o in enumerate(obj.prog.ops):
        assert k > fills[0] or not (_word_reads(o) or _word_writes(o)), "record %d touches the table before its fill" % k
        # (a record reads before its epilogue folds)
        for addr, n in _word_reads(o):
            assert addr, "record %d (code %d) reads a NULL word" % (k, o.code)
            assert lo <= addr and addr + 4 * n <= hi and (addr - lo) % 4 == 0, "record %d reads outside the table" % k
            missing = [a for a in range(addr, addr + 4 * n, 4) if a not in written]
            assert not missing, "record %d (code %d) reads %d words nobody wrote" % (k, o.code, len(missing))
            reads += n
        for addr, n in _word_writes(o):
            assert o.stream == 0, "record %d writes words off the main stream" % k
            assert lo <= addr and addr + 4 * n <= hi and (addr - lo) % 4 == 0, "record %d writes outside the table" % k
            words = set(range(addr, addr + 4 * n, 4))
            assert not words & written, "record %d (code %d) writes a word a second time" % (k, o.code)
            written |= words
    assert reads > 0
    if name == "r50_pointwise_train":      # the routes the 128 x 128 default size keeps closed are open here
        assert sum(o.code == PR.GEMM_CONV_SPLIT for o in obj.prog.ops) == 47
        assert sum(o.code == PR.CONV1X1_WGRAD and o.i[5] == 1 for o in obj.prog.ops) == 24


# ---------------------------------------------------------------------------------------------------------------
# the word table
# ---------------------------------------------------------------------------------------------------------------
def _t(*shape):
    return torch.zeros(shape)


def test_a_measured_group_is_found_again_without_a_second_record():
    am, P = AmaxTable(64, "cpu"), PR.Program()
    a, b = _t(1, 8, 4, 4), _t(1, 8, 2, 2)
    base = am.measure(P, [[a, b]], 8)
    assert base == 0 and len(P.ops) == 1 and P.ops[0].p[1] == am.addr(0) == am.tensor.data_ptr()
    assert am.measure(P, [[a, b]], 8) == base and am.find([[a, b]]) == base and len(P.ops) == 1
    assert am.find([[b, a]]) is None and am.addr(3) == am.tensor.data_ptr() + 12


def test_a_part_of_a_block_is_found_by_its_own_key():
    am = AmaxTable(64, "cpu")
    cls, bbox = [_t(1, 8, 4, 4), _t(1, 8, 2, 2)], [_t(1, 8, 4, 4), _t(1, 8, 2, 2)]
    x = _t(1, 8, 3, 3)
    assert am.reserve([[x]]) == 0
    base = am.reserve([cls, bbox])                      # one launch, two problems of two levels
    assert base == 1 and am.find([cls, bbox]) == 1 and am.find([cls]) == 1 and am.find([bbox]) == 3
    assert am.find([[cls[0]]]) is None                  # (a level alone is no key of a two-level problem)
    one = [[_t(1, 8, 4, 4)], [_t(1, 8, 2, 2)]]          # one tensor per problem: every tensor is a key
    assert am.reserve(one) == 5 and am.find([one[0]]) == 5 and am.find([one[1]]) == 6 and am.next == 7
    # a launch of ONE problem: its whole key and its problem's key coincide
    assert am.reserve([cls]) == 7 and am.find([cls]) == 7


def test_a_remeasured_tensors_alias_moves_to_the_new_word():
    am, P = AmaxTable(64, "cpu"), PR.Program()
    a, b = _t(1, 8, 4, 4), _t(1, 8, 4, 4)
    assert am.measure(P, [[a]], 8) == 0 and am.measure(P, [[b]], 8) == 1
    assert am.measure(P, [[a], [b]], 8) == 2 and len(P.ops) == 3        # together: a fresh block, measured again
    assert am.find([[a]]) == 2 and am.find([[b]]) == 3                  # the freshest measurement serves later readers
    assert am.measure(P, [[b]], 8) == 3 and len(P.ops) == 3


def test_one_tensor_measures_with_split_absmax_and_several_through_a_table():
    am, P = AmaxTable(64, "cpu"), PR.Program()
    a, b, c = _t(2, 8, 4, 4), _t(2, 8, 2, 2), _t(2, 8, 1, 1)
    am.measure(P, [[a]], 8)
    o = P.ops[0]
    assert (o.code, o.klass, o.stream) == (PR.SPLIT_ABSMAX, 73, 0)
    assert (o.p[0], o.p[1], o.l[0], o.work) == (a.data_ptr(), am.addr(0), a.numel(), 4.0 * a.numel())
    am.measure(P, [[b], [c]], 8)
    o = P.ops[1]
    assert (o.code, o.klass, o.stream, list(o.i[:3])) == (PR.SPLIT_ABSMAX_LEVELS, 73, 0, [2, 8, 0])
    assert o.p[1] == am.addr(1) and o.work == 4.0 * (b.numel() + c.numel())
    lv = ctypes.cast(o.p[0], ctypes.POINTER(K.ConvLevel))              # a level table of the pass's own
    assert [lv[k].x for k in range(2)] == [b.data_ptr(), c.data_ptr()] and (lv[1].N, lv[1].H, lv[1].W) == (2, 1, 1)
    # a reader's own table: one tensor goes through it too, with the reader's field index
    d, e = _t(1, 8, 4, 4), _t(1, 8, 4, 4)
    own = conv_table([(d, None, e, None, None)])
    P.keep.append(own)
    am.measure(P, [[e]], 8, own, 1)
    o = P.ops[2]
    assert (o.code, list(o.i[:3]), o.p[0], o.p[1]) == (PR.SPLIT_ABSMAX_LEVELS, [1, 8, 1], ctypes.addressof(own), am.addr(3))


def test_one_word_past_the_table_raises():
    am = AmaxTable(4, "cpu")
    am.reserve([[_t(1), _t(1)], [_t(1), _t(1)]])                        # exactly full
    with pytest.raises(K.KernelError, match="table full"):
        am.reserve([[_t(1)]])
    h = _heads()
    with pytest.raises(K.KernelError, match="table full"):
        h._amax.measure(PR.Program(), [[_t(1) for _ in range(h.AMAX_WORDS + 1 - h._amax.next)]], 1)
    assert DistillHeads.AMAX_WORDS == 2048 and BP.NativeResNetFPN.AMAX_WORDS == 4096


# ---------------------------------------------------------------------------------------------------------------
# workspaces
# ---------------------------------------------------------------------------------------------------------------
# pointer slot of the workspace in the records that take one (csrc/pipeline/program.cc); its bytes are l[0]
WS_SLOT = {PR.CONV3X3_WGRAD: 3, PR.GEMM_CONV_SPLIT: 1, PR.CONV1X1_WGRAD: 3, PR.CONV_KXK_WGRAD: 3, PR.F16_WGRAD: 4,
           PR.PW_F16_WGRAD: 5}


def _ws_slot(o):
    return 3 if (o.code == PR.CONV3X3 and o.i[4] == 3) else WS_SLOT.get(o.code)


def _workspaces(obj):
    if hasattr(obj, "wss"):
        return [obj.split_ws] + list(obj.wss.values())
    return [obj.split_ws, obj.wgrad_ws]


@pytest.mark.parametrize("name", ["heads_distill", "heads_f16", "r50_pointwise_train", "f16_r50_train", "r101_frozen"])
def test_every_workspace_slot_points_at_a_large_enough_workspace_of_the_pipeline(build, name):
    obj = build(name)
    ws = {w.data_ptr(): w for w in _workspaces(obj)}
    assert len(ws) == len(_workspaces(obj)) and all(w.dtype == torch.uint8 and w.numel() >= 16 for w in ws.values())
    carried, need, by_stream = 0, {a: 0 for a in ws}, {}
    for k, o in enumerate(obj.prog.ops):
        slot = _ws_slot(o)
        if slot is None:
            continue
        assert o.p[slot], "record %d (code %d): NULL workspace" % (k, o.code)
        assert o.p[slot] in ws, "record %d (code %d): not a workspace of the pipeline" % (k, o.code)
        assert 0 < o.l[0] <= ws[o.p[slot]].numel(), "record %d (code %d): %d bytes" % (k, o.code, o.l[0])
        need[o.p[slot]] = max(need[o.p[slot]], o.l[0])
        by_stream.setdefault(o.stream, set()).add(o.p[slot])
        carried += 1
    assert carried > 0 or name == "r101_frozen"
    # sized for the largest need, and 16 bytes where nobody asked
    assert all(ws[a].numel() == max(need[a], 16) for a in ws)
    # no two records on different streams share one
    assert sum(len(v) for v in by_stream.values()) == len(set().union(*by_stream.values()))
    # the pipeline owns them: in no Program.keep (a fingerprint names them U<n>)
    for attr in ("prog", "prep", "prog_teacher_pack", "prog_distill_only"):
        P = getattr(obj, attr, None)
        assert P is None or not any(v is w for v in P.keep for w in ws.values())
    if hasattr(obj, "wss"):
        if obj.train:                                    # two auxiliary streams, each with its own
            assert sorted(obj.wss) == [1, 2] and obj.ws is obj.wss[1]
            assert all(by_stream[k] == {obj.wss[k].data_ptr()} for k in (1, 2))
            assert by_stream.get(0, set()) <= {obj.split_ws.data_ptr()}
        else:
            assert all(w.numel() == 16 for w in obj.wss.values())


def test_without_auxiliary_streams_the_filter_gradients_share_the_main_streams_workspace(build):
    bb = _backbone(train=True, overlap_wgrad=False)
    assert list(bb.wss) == [0] and bb.ws is bb.wss[0] and bb.ws.data_ptr() != bb.split_ws.data_ptr()
    wg = [o for o in bb.prog.ops if o.code in (PR.CONV3X3_WGRAD, PR.CONV1X1_WGRAD, PR.CONV_KXK_WGRAD)]
    assert wg and {o.stream for o in wg} == {0} and {o.p[3] for o in wg} == {bb.ws.data_ptr()}
    assert max(o.l[0] for o in wg) == bb.ws.numel()


def test_a_workspace_binds_the_records_of_several_programs_and_allocates_16_bytes_unasked():
    assert PR.Workspace().bind("cpu").numel() == 16
    ws, P, Q = PR.Workspace(), PR.Program(), PR.Program()
    x = _t(4)
    P.add(PR.FILL, p=(x,))
    P.add(PR.CONV3X3_WGRAD, l=(100,), p=(x, None, None, ws.need(100)))
    Q.add(PR.GEMM_CONV_SPLIT, l=(40,), p=(x, ws.need(40)))
    Q.build()                                            # (bound after build: the built array follows)
    assert P.ops[1].p[3] is None and Q.ops[0].p[1] is None
    t = ws.bind("cpu")
    assert t.numel() == 100 and t.dtype == torch.uint8
    assert P.ops[1].p[3] == Q.ops[0].p[1] == Q.arr[0].p[1] == t.data_ptr()
    assert P.ops[0].p[0] == x.data_ptr() and P.ops[1].p[1] is None
    assert not any(isinstance(v, PR.Workspace) or v is t for v in P.keep + Q.keep)
