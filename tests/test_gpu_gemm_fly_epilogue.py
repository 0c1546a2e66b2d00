"""gemm_fly_kernel's epilogue with its options compiled in (csrc/kernels/gemm_split.hip).

With M a multiple of 8 a call goes to the instance that has residual / mask / accumulation as template constants and
issues its loads two blocks ahead; any other M, and every call under SSAD_GEMM_FLY_GENERIC=1 (read at every launch),
goes to the all-runtime instance.  Every output keeps its sequence -- scale and bias, + residual, ReLU, mask select,
+ old value, |max| fold of what was stored -- so the two must agree BIT FOR BIT, NaN and Inf included, and both stay
within the engine's bar against the oracle (close() / CONV_RTOL / CONV_FLOOR of test_gpu_gemm_conv.py, unwidened).

Shapes are (N, K, M, H, W): K channels in, M channels out, for the forward forms and the data-gradient forms alike.
Beside the seven forms of the wrappers, "res_mask" (a residual under the mask, through the descriptor) runs the sixth
fast instance, which the backbones' backward pass launches.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from oracle import oracle
from guarded import Arena
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, close, dev

pytestmark = pytest.mark.gpu
SWITCH = "SSAD_GEMM_FLY_GENERIC"

SHAPES = [(2, 40, 256, 9, 15),       # K tail; a pixel tile ending inside an image
          (1, 64, 250, 5, 7),        # M & 7 != 0: the generic instance behind the dispatch
          (2, 32, 264, 8, 16),       # M a multiple of 8 but not 32: the wave-uniform skip, an almost empty 2nd block
          (1, 96, 512, 16, 16),      # two full channel blocks
          (3, 256, 256, 4, 11)]      # P = 44: one partial tile per image
RAGGED = [SHAPES[1], SHAPES[2]]
SHAPE_ID = lambda s: "N%d_K%d_M%d_%dx%d" % s
# form -> (forward?, bias, residual, relu, mask, accumulate)
FORMS = {"plain": (True, 0, 0, 0, 0, 0), "bias": (True, 1, 0, 0, 0, 0), "bias_res_relu": (True, 1, 1, 1, 0, 0),
         "relu": (True, 0, 0, 1, 0, 0), "mask": (False, 0, 0, 0, 1, 0), "acc": (False, 0, 0, 0, 0, 1),
         "mask_acc": (False, 0, 0, 0, 1, 1), "res_mask": (False, 0, 1, 0, 1, 0)}


@pytest.fixture(scope="module")
def K():
    from ssad_amd import kernels
    kernels.lib()
    return kernels


_problems = {}


def problem(shape):
    """host inputs and the oracle's results, computed once per shape; the tests copy what they change"""
    if shape not in _problems:
        N, Kc, M, H, W = shape
        rng = np.random.default_rng(7100 + sum(shape))
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        p = dict(X=f(N, Kc, H, W), Wt=f(M, Kc, 1, 1) * np.float32(1.0 / np.sqrt(Kc)), b=f(M), R=f(N, M, H, W),
                 Wd=f(Kc, M, 1, 1) * np.float32(1.0 / np.sqrt(Kc)), mask=np.maximum(f(N, M, H, W), 0), base=f(N, M, H, W))
        p["ref_b"] = oracle.conv_forward(p["X"], p["Wt"], p["b"], kernel=1, stride=1, pad=0)
        p["ref_nb"] = oracle.conv_forward(p["X"], p["Wt"], None, kernel=1, stride=1, pad=0)
        # the data gradient of the K <- M layer Wd: dY has K channels, dX has M
        p["rdX"] = oracle.conv_backward(np.zeros((N, M, H, W), np.float32), p["Wd"], p["X"], kernel=1, stride=1, pad=0,
                                        want_db=False)[2]
        _problems[shape] = p
    return _problems[shape]


def reference(p, form):
    if form == "plain":
        return p["ref_nb"]
    if form == "bias":
        return p["ref_b"]
    if form == "bias_res_relu":
        return np.maximum(p["ref_b"] + p["R"], 0)
    if form == "relu":
        return np.maximum(p["ref_nb"], 0)
    masked = np.where(p["mask"] > 0, p["rdX"], 0)
    return {"mask": masked, "acc": p["base"] + p["rdX"], "mask_acc": p["base"] + masked,
            "res_mask": np.where(p["mask"] > 0, p["rdX"] + p["R"], 0)}[form]


def run(K, shape, form, ops, take=None):
    """One form through the Python wrapper and through ssad_conv1x1_gemm_split_amax (the entry that folds the |max| of
    what was stored into a word).  ops: host arrays X, Wt / Wd, b, R, mask, base.  take(name, array or shape) places an
    operand or an output (the arena of test (d)); by default ordinary allocations.  Returns (y, the entry's y, word)."""
    N, Kc, M, H, W = shape
    fwd, bias, res, relu, mask, acc = FORMS[form]
    inp = take or (lambda name, a: dev(a))
    out = take or (lambda name, shp: torch.empty(shp, dtype=torch.float32, device="cuda"))
    ws = (lambda n: take("workspace", int(n))) if take else None
    x = inp("x", ops["X"])
    word = inp("word", np.zeros(1, np.int32))
    L = K.lib()
    if fwd:
        wt = K.transpose_filter(inp("w", ops["Wt"]), out=out("wt", (Kc, (M + 3) // 4 * 4)))
        b = inp("bias", ops["b"]) if bias else None
        r = inp("residual", ops["R"]) if res else None
        y = K.conv1x1_forward(x, wt, M, b, r, relu=bool(relu), out=out("y", (N, M, H, W)), split=True, workspace=ws)
        y2 = K.conv1x1_forward_split_amax(x, wt, M, b, r, relu=bool(relu), y_amax=word, out=out("y2", (N, M, H, W)),
                                          workspace=ws)
    else:
        w = inp("w", ops["Wd"].reshape(Kc, M))
        m = inp("mask", ops["mask"]) if mask else None
        r = inp("residual", ops["R"]) if res else None

        def entry(yt, word):
            d = K.gemm_conv_desc(w, M, x, yt, Kc, M, None, r, m, False, bool(acc))
            buf = K._own_workspace(ws, L.ssad_conv1x1_gemm_split_workspace_bytes(C.byref(d)))
            K._check(L.ssad_conv1x1_gemm_split_amax(C.byref(d), None, None, K._ptr(word), K._ptr(buf), buf.numel(),
                                                    K._stream()), "conv1x1_gemm_split_amax (dgrad)")
            return yt
        if res:                             # the backbones' shortcut gradient: no wrapper takes a residual and a mask
            y = entry(out("y", (N, M, H, W)), None)
        else:
            y = K.conv1x1_dgrad(x, w, mask=m, accumulate_into=inp("y", ops["base"]) if acc else None,
                                out=None if acc else out("y", (N, M, H, W)), split=True, workspace=ws)
        y2 = entry(inp("y2", ops["base"]) if acc else out("y2", (N, M, H, W)), word)
    return y.cpu().numpy(), y2.cpu().numpy(), int(word.item())


def both(K, monkeypatch, shape, form, ops):
    """run() on the default dispatch and with the all-runtime instance forced"""
    monkeypatch.delenv(SWITCH, raising=False)
    fast = run(K, shape, form, ops)
    monkeypatch.setenv(SWITCH, "1")
    generic = run(K, shape, form, ops)
    monkeypatch.delenv(SWITCH)
    return fast, generic


def same(fast, generic, what):
    for a, b, name in zip(fast[:2], generic[:2], ("wrapper", "entry with the |max| word")):
        assert np.array_equal(a, b, equal_nan=True), "%s, %s: the compiled-in epilogue differs from the generic one" % (what, name)
    assert np.array_equal(fast[0], fast[1], equal_nan=True), "%s: the two entries differ" % what
    assert fast[2] == generic[2], "%s: |max| words %#x / %#x" % (what, fast[2], generic[2])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
def test_compiled_in_epilogue_vs_oracle_and_bit_identical_to_generic(K, monkeypatch, shape, form):
    """(a) both instances against the oracle; (b) bit for bit against each other, the folded |max| word included"""
    p = problem(shape)
    fast, generic = both(K, monkeypatch, shape, form, p)
    ref = reference(p, form)
    close(fast[0], ref, CONV_RTOL, CONV_FLOOR, form)
    close(generic[0], ref, CONV_RTOL, CONV_FLOOR, form + " (generic)")
    same(fast, generic, form)
    assert fast[2] == int(np.abs(fast[0]).max().view(np.int32)), "the word is not the |max| of what was stored"


@pytest.mark.parametrize("form", ["bias_res_relu", "mask", "acc", "mask_acc", "res_mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
def test_planted_nan_and_inf_stay_at_their_elements(K, monkeypatch, shape, form):
    """(c) a NaN and an Inf in the residual, in the old values (for mask + accumulate: the NaN where the mask is zero)
    and, for the mask alone, in the gradient under a zero mask element: the two instances agree bit for bit and the
    NaN reaches only the outputs the operation connects it to."""
    N, Kc, M, H, W = shape
    p = problem(shape)
    ops = {k: p[k].copy() for k in ("X", "Wt", "Wd", "b", "R", "mask", "base")}
    e_nan, e_inf = (N - 1, M - 1, H - 1, W - 1), (0, M // 2, 0, 1)      # the last output of the last tile; another
    if form == "mask":
        # x is the gradient here: its NaN reaches every output channel of its pixel, and no other pixel
        ops["X"][N - 1, Kc - 1, H - 1, W - 1] = np.nan
        ops["X"][0, 0, 0, 1] = np.inf
        ops["mask"][:, :, H - 1, W - 1] = 1.0
        ops["mask"][e_nan] = 0.0
        ops["mask"][e_inf] = 0.0
    else:
        target = ops["R"] if form in ("bias_res_relu", "res_mask") else ops["base"]
        target[e_nan] = np.nan
        target[e_inf] = np.inf
        ops["mask"][e_nan] = 0.0            # the old NaN sits under a zero mask element: 0 + NaN
        ops["mask"][e_inf] = 1.0
    fast, generic = both(K, monkeypatch, shape, form, ops)
    same(fast, generic, form + " with NaN / Inf")
    y = fast[0]
    if form == "mask":
        assert y[e_nan] == 0.0 and y[e_inf] == 0.0, "a zero mask element must select zero, not multiply"
        want = np.zeros(y.shape, bool)
        want[N - 1, :, H - 1, W - 1] = True
        want[e_nan] = False
        bad = np.isnan(y) & ~want
        bad[0, :, 0, 1] = False             # the Inf's pixel: Inf or NaN wherever the mask is positive
        assert np.isnan(y[want]).all() and not bad.any(), "the NaN left its pixel: %s" % (np.argwhere(bad)[:4],)
        assert not np.isfinite(y[0, :, 0, 1][ops["mask"][0, :, 0, 1] > 0]).any()
    else:
        nans = np.argwhere(np.isnan(y))
        if form == "bias_res_relu":         # ReLU is fmaxf(v, 0), which answers a NaN with 0: at its element or nowhere
            assert all(tuple(e) == e_nan for e in nans), "the NaN left its element"
        elif form == "res_mask":            # the residual's NaN sits under a zero mask element: selected away
            assert nans.size == 0 and y[e_nan] == 0.0, "a zero mask element must select zero, not multiply"
        else:
            assert np.array_equal(nans, [e_nan]), "the NaN left its element"
            assert fast[2] > 0x7f800000, "a NaN's word is above Inf's and survives the fold"
        assert np.array_equal(np.argwhere(np.isinf(y)), [e_inf]) and y[e_inf] > 0


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", RAGGED, ids=SHAPE_ID)
def test_nothing_outside_y_is_written_for_ragged_m(K, monkeypatch, shape, form):
    """(d) every operand, output and workspace of the launches inside one arena of sentinel words: no guard byte and no
    operand changes, no output word stays unwritten, and the results are those of ordinary allocations."""
    N, Kc, M, H, W = shape
    p = problem(shape)
    monkeypatch.delenv(SWITCH, raising=False)
    sizes = []

    def plain(name, a):
        if name == "workspace":
            sizes.append(a)
            return torch.empty(a, dtype=torch.uint8, device="cuda")
        t = dev(a) if isinstance(a, np.ndarray) else torch.empty(a, dtype=torch.float32, device="cuda")
        sizes.append(t.numel() * t.element_size())
        return t
    want = run(K, shape, form, p, take=plain)
    arena = Arena(Arena.bytes_for(*sizes))
    n_ws = [0]

    def guarded(name, a):
        if name == "workspace":
            n_ws[0] += 1
            return arena.take_bytes(a, "workspace #%d" % n_ws[0])
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            return arena.take(a.shape, torch.from_numpy(np.empty(0, a.dtype)).dtype, name, data=a)
        return arena.take(a, torch.float32, name)
    got = run(K, shape, form, p, take=guarded)
    accumulates = FORMS[form][5]
    assert arena.check(modified=("word",) + (("y", "y2") if accumulates else ()))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
