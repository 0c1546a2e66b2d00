"""The grouped 3x3 gradients, the parts that need no device: the new entry points and their refusals through the raw
C ABI, the workspace function, the kernels.py wrappers' errors, and BodyConfig(grouped_engine=...) against the
committed capture of the X-101-64x4d body."""
import ctypes
import json
import os

import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import kernels as K
from ssad_amd.modeling import resnet_fpn as rf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X64 = dict(block_counts=(3, 4, 23, 3), stride_1x1=False, num_groups=64, width_per_group=4)


@pytest.fixture(scope="module")
def L():
    return K.lib()


_BUF = ctypes.create_string_buffer(64)


@pytest.fixture(scope="module")
def p():
    return ctypes.cast(_BUF, ctypes.c_void_p)


def test_symbols_resolve_and_the_abi_number_stays(L):
    for name in ("ssad_grouped_conv3x3_dgrad_filter_floats", "ssad_grouped_conv3x3_pack_filter_dgrad",
                 "ssad_grouped_conv3x3_dgrad", "ssad_grouped_conv3x3_wgrad_workspace_bytes", "ssad_grouped_conv3x3_wgrad"):
        assert getattr(L, name) is not None
    L.ssad_kernels_abi_version.restype = ctypes.c_int
    assert L.ssad_kernels_abi_version() == 3 == K.ABI_VERSION
    for C, G in ((256, 64), (512, 64), (1024, 64), (2048, 64), (2048, 32)):
        assert L.ssad_grouped_conv3x3_dgrad_filter_floats(C, G) == L.ssad_grouped_conv3x3_filter_floats(C, G) > 0


# (N, C, H, W, group, stride) the kernels refuse, and why
REFUSED = [(1, 256, 8, 8, 2, 1, "128 channels per group"), (1, 24, 8, 8, 2, 1, "12 channels per group"),
           (1, 66, 8, 8, 4, 1, "C % group"), (1, 64, 8, 8, 0, 1, "no groups"), (1, 64, 8, 8, 16, 3, "stride 3"),
           (1, 64, 8, 8, 16, 0, "stride 0"), (0, 64, 8, 8, 16, 1, "no images"), (-1, 64, 8, 8, 16, 2, "N < 0"),
           (1, 64, 0, 8, 16, 1, "H = 0"), (1, 64, 8, -3, 16, 2, "W < 0"), (1, 0, 8, 8, 16, 1, "no channels")]


@pytest.mark.parametrize("geo", REFUSED, ids=[g[-1] for g in REFUSED])
def test_refusals_through_the_c_abi(L, p, geo):
    """SSAD_E_BADARG before any launch: the calls below run on a machine without a device"""
    N, C, H, W, G, s = geo[:6]
    big = ctypes.c_size_t(1 << 40)
    assert L.ssad_grouped_conv3x3_dgrad(p, p, None, N, C, H, W, G, s, p, None) == -1
    assert L.ssad_grouped_conv3x3_dgrad(p, p, p, N, C, H, W, G, s, p, None) == -1
    assert L.ssad_grouped_conv3x3_wgrad(p, p, N, C, H, W, G, s, p, p, big, None) == -1
    assert L.ssad_grouped_conv3x3_wgrad_workspace_bytes(N, C, H, W, G, s) == 0
    if geo[-1] in ("128 channels per group", "12 channels per group", "C % group", "no groups", "no channels"):
        assert L.ssad_grouped_conv3x3_dgrad_filter_floats(C, G) == -1
        assert L.ssad_grouped_conv3x3_pack_filter_dgrad(p, C, G, p, None) == -1


def test_null_pointers_a_short_workspace_and_an_oversized_grid_are_refused(L, p):
    geo = (2, 64, 19, 23, 16, 1)
    need = L.ssad_grouped_conv3x3_wgrad_workspace_bytes(*geo)
    assert need > 0
    assert L.ssad_grouped_conv3x3_wgrad(p, p, *geo, p, p, need - 1, None) == -1          # one byte short
    assert L.ssad_grouped_conv3x3_wgrad(p, p, *geo, p, p, 0, None) == -1
    assert L.ssad_grouped_conv3x3_wgrad(None, p, *geo, p, p, need, None) == -1
    assert L.ssad_grouped_conv3x3_wgrad(p, None, *geo, p, p, need, None) == -1
    assert L.ssad_grouped_conv3x3_wgrad(p, p, *geo, None, p, need, None) == -1
    assert L.ssad_grouped_conv3x3_wgrad(p, p, *geo, p, None, need, None) == -1
    assert L.ssad_grouped_conv3x3_dgrad(None, p, None, *geo, p, None) == -1
    assert L.ssad_grouped_conv3x3_dgrad(p, None, None, *geo, p, None) == -1
    assert L.ssad_grouped_conv3x3_dgrad(p, p, None, *geo, None, None) == -1
    assert L.ssad_grouped_conv3x3_pack_filter_dgrad(None, 64, 16, p, None) == -1
    assert L.ssad_grouped_conv3x3_pack_filter_dgrad(p, 64, 16, None, None) == -1
    # more workgroups than a grid holds: refused, not wrapped (2^22 images x 32 groups x 8 x 4 tiles = 2^32)
    assert L.ssad_grouped_conv3x3_dgrad(p, p, None, 1 << 22, 2048, 64, 64, 32, 1, p, None) == -1


def test_workspace_function_follows_its_formula_and_never_shrinks(L):
    f = L.ssad_grouped_conv3x3_wgrad_workspace_bytes

    def formula(N, C, H, W, G, s):
        cg = C // G
        oh, ow = (H - 1) // s + 1, (W - 1) // s + 1
        tr = 8 if s == 1 else 4
        T = N * ((oh + tr - 1) // tr) * ((ow + 15) // 16)
        gpw = {4: 4, 8: 4, 16: 2, 32: 1, 64: 1}[cg]
        B = (G + gpw - 1) // gpw * (4 if cg == 64 else 1)
        return min(T, max(1, 1024 // B)) * C * cg * 9 * 4

    for cg, G in ((4, 64), (8, 64), (16, 64), (32, 64), (64, 32), (4, 3), (64, 1)):
        for s in (1, 2):
            last_n = 0
            for N in (1, 2, 3, 16, 64):
                got = f(N, cg * G, 40, 56, G, s)
                assert got == formula(N, cg * G, 40, 56, G, s) and got >= last_n
                last_n = got
            last_hw = 0
            for H, W in ((1, 1), (5, 7), (8, 16), (9, 17), (20, 28), (40, 56), (160, 224)):
                got = f(2, cg * G, H, W, G, s)
                assert got == formula(2, cg * G, H, W, G, s) and got >= last_hw
                last_hw = got
    # the layers of tools/grouped_grad_bench.py: bs 16 at 640 x 896, res2 and X-101-32x8d's res5
    assert f(16, 256, 160, 224, 64, 1) == 64 * 256 * 4 * 9 * 4
    assert f(16, 2048, 20, 28, 32, 1) == 8 * 2048 * 64 * 9 * 4


def test_wrappers_raise_kernel_error_on_host_tensors_and_bad_widths(monkeypatch):
    w = torch.zeros(64, 4, 3, 3)
    x, dy = torch.zeros(1, 64, 8, 8), torch.zeros(1, 64, 8, 8)
    with pytest.raises(K.KernelError, match="contiguous float32 device tensor"):
        K.grouped_conv3x3_pack_filter_dgrad(w, 16)
    with pytest.raises(K.KernelError, match="contiguous float32 device tensor"):
        K.grouped_conv3x3_dgrad(dy, w, 16, 1, (8, 8))
    with pytest.raises(K.KernelError, match="contiguous float32 device tensor"):
        K.grouped_conv3x3_wgrad(x, dy, 16, 1)
    # past the tensor check (as on a device): the geometry is refused with the geometry in the message
    monkeypatch.setattr(K, "_f32c", lambda t, name: t)
    with pytest.raises(K.KernelError, match=r"24 channels in 2 groups \(4, 8, 16, 32 or 64 per group\)"):
        K.grouped_conv3x3_pack_filter_dgrad(torch.zeros(24, 12, 3, 3), 2)
    with pytest.raises(K.KernelError, match=r"grouped_conv3x3_dgrad: N 1, 24 channels in 2 groups.*8 x 8, stride 1"):
        K.grouped_conv3x3_dgrad(torch.zeros(1, 24, 8, 8), torch.zeros(24, 12, 3, 3), 2, 1, (8, 8))
    with pytest.raises(K.KernelError, match=r"grouped_conv3x3_wgrad: N 1, 24 channels in 2 groups.*8 x 8, stride 1"):
        K.grouped_conv3x3_wgrad(torch.zeros(1, 24, 8, 8), torch.zeros(1, 24, 8, 8), 2, 1)
    with pytest.raises(K.KernelError, match=r"64 channels in 16 groups.*stride 3"):
        K.grouped_conv3x3_dgrad(torch.zeros(1, 64, 3, 3), w, 16, 3, (8, 8))
    with pytest.raises(K.KernelError, match=r"64 channels in 16 groups.*stride 3"):
        K.grouped_conv3x3_wgrad(x, torch.zeros(1, 64, 3, 3), 16, 3)
    with pytest.raises(K.KernelError, match=r"stride 2.*dy is \(1, 64, 8, 8\)"):
        K.grouped_conv3x3_dgrad(dy, w, 16, 2, (8, 8))
    with pytest.raises(K.KernelError, match=r"stride 2.*dy is \(1, 64, 8, 8\)"):
        K.grouped_conv3x3_wgrad(x, dy, 16, 2)


def _ops(grouped_engine):
    model = rf.BodyModel(rf.BodyConfig(grouped_engine=grouped_engine, **X64))
    rf.add_fpn_resnet_conv5_body(model)
    return list(model.net.Proto().op), model.params


def _args(op):
    out = {}
    for a in op.arg:
        if a.HasField("i"):
            out[a.name] = a.i
        elif a.HasField("s"):
            out[a.name] = a.s.decode() if isinstance(a.s, bytes) else a.s
        elif a.HasField("f"):
            out[a.name] = a.f
    return out


def test_builder_switch_against_the_committed_capture():
    g = json.load(open(os.path.join(GOLDEN, "backbone_graph_x101_64x4d_fpn.json")))
    assert rf.BodyConfig().grouped_engine is False
    plain, params = _ops(False)
    tagged, tparams = _ops(True)
    assert len(plain) == len(tagged) == len(g["ops"])
    assert [(n, s) for n, s, _ in params] == [(n, s) for n, s, _ in tparams] == [(q["name"], q["shape"]) for q in g["params"]]
    n_tagged = 0
    for mine, with_algo, ref in zip(plain, tagged, g["ops"]):
        want = {k: (int(v) if isinstance(v, bool) else v) for k, v in ref["args"].items()}
        want.pop("engine", None)                       # a field of OperatorDef, not an argument
        for op in (mine, with_algo):
            assert op.type == ref["type"] and list(op.input) == ref["input"] and list(op.output) == ref["output"]
        assert _args(mine) == want                     # the default: the committed capture, argument for argument
        extra = dict(_args(with_algo))
        if extra.pop("hip_algo", None) is not None:
            n_tagged += 1
            assert _args(with_algo)["hip_algo"] == "grouped"
            assert with_algo.type == "Conv" and want["kernel"] == 3 and want["group"] == 64 and want["pad"] == 1
            assert with_algo.output[0].endswith("_branch2b")
        assert extra == want                           # nothing else differs
    assert n_tagged == 33
    # a plain ResNet has no grouped layer to mark
    model = rf.BodyModel(rf.BodyConfig(grouped_engine=True))
    rf.add_fpn_resnet_conv5_body(model)
    assert not any(a.name == "hip_algo" for o in model.net.Proto().op for a in o.arg)
