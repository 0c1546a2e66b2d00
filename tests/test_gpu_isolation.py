"""Kernel isolation: what a launch touches and uses besides its output (tests/guarded.py).

Part A -- guard bands and frozen operands.  Every operand, output and workspace of a launch is a view of ONE arena
full of a sentinel NaN, with >= 4096 bytes of guard around each view, the workspace exactly *_workspace_bytes long.
After the launch: no guard byte changed, no input changed, no output word left unwritten; the result meets the
family's bar against the oracle and is bit-equal to the same call on ordinary allocations (results do not depend on
placement).  Filter packs are taken as outputs but may keep sentinel words: their padding is never written; since it
then holds NaNs, a kernel that multiplies padding into a result fails the comparison with the oracle.

Part B -- non-finite locality.  One NaN / +Inf planted in an activation or a gradient may reach only the outputs the
operation's definition connects it to: a tail handled by multiplying a neighbour with zero is exact on finite data and
wrong here.

Contracts the launchers state and these tests assert exactly ("Kernel isolation"):
  * ssad_conv1x1_gemm needs P % 4 == 0 and lda % 4 == 0 (the data gradient's lda is the layer's Cin),
    ssad_conv1x1_wgrad P % 16 == 0, ssad_conv1x1_wgrad_split P % 8 == 0, ssad_conv_kxk_dgrad Cin*k*k % 4 == 0:
    refused with SSAD_E_BADARG before any launch;
  * a Winograd engine computes a whole output tile from one transformed input tile, so a non-finite input may reach
    any output of the tiles that read it and no other: 2 x 2 outputs from a 4 x 4 patch for F(2x2) (at most 2 pixels
    away), 2 x 4 outputs from a 4 x 6 patch for F(2x4) (at most 2 rows / 4 columns away).  What comes out finite inside
    those tiles is held to the oracle like everything else.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle  # noqa: E402
from ssad_amd import synth  # noqa: E402
from guarded import Arena  # noqa: E402
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, DX_FLOOR, DX_RTOL, LOSS_RTOL, close  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = torch.float32


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ssad_amd import kernels
    kernels.lib()  # raises if the HIP extension is missing: no fallback
    return kernels


# ---------------------------------------------------------------------------------------------------------------------
# the two allocators a case runs on
# ---------------------------------------------------------------------------------------------------------------------

def _tdtype(a):
    return torch.from_numpy(np.empty(0, a.dtype)).dtype


class Plain:
    """ordinary allocations (and the record of their sizes, from which the arena is sized)"""

    def __init__(self):
        self.sizes, self.n_ws = [], 0

    def _raw(self, shape, dtype, skew):
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        self.sizes.append(n + skew)
        raw = torch.empty(n + skew + 16, dtype=torch.uint8, device="cuda")
        return raw[skew:skew + n].view(dtype).view(tuple(shape))

    def inp(self, name, a, skew=0):
        a = np.ascontiguousarray(a)
        t = self._raw(a.shape, _tdtype(a), skew)
        t.copy_(torch.from_numpy(a))
        return t

    def out(self, name, shape, dtype=F32, skew=0):
        return self._raw(tuple(shape) if isinstance(shape, (tuple, list)) else (shape,), dtype, skew)

    def ws(self, nbytes, tag):
        n = max(int(nbytes), 1)
        self.sizes.append(n)
        self.n_ws += 1
        return torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")        # never zeroed for the launcher


class Guarded:
    """the same calls on views of one arena"""

    def __init__(self, arena):
        self.arena, self.n_ws = arena, 0

    def inp(self, name, a, skew=0):
        a = np.ascontiguousarray(a)
        return self.arena.take(a.shape, _tdtype(a), name, data=a, skew=skew)

    def out(self, name, shape, dtype=F32, skew=0):
        return self.arena.take(shape, dtype, name, skew=skew)

    def ws(self, nbytes, tag):
        self.n_ws += 1
        return self.arena.take_bytes(max(int(nbytes), 1), "workspace %s #%d" % (tag, self.n_ws))


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def isolated(K, monkeypatch, fn, modified=(), nan_ok=None):
    """fn(al) -> {name: result tensor}: once on ordinary allocations, once inside an arena (the launchers' cached
    workspaces included: K._workspace hands out views of exactly the size asked for).  Returns the arena run's results
    as numpy arrays after the guard / frozen-operand / unwritten-output checks and the bit comparison of the two."""
    plain, cached = Plain(), K._workspace
    monkeypatch.setattr(K, "_workspace", plain.ws)
    want = {k: v.detach().cpu().numpy().copy() for k, v in fn(plain).items()}
    arena = Arena(Arena.bytes_for(*plain.sizes))
    g = Guarded(arena)
    monkeypatch.setattr(K, "_workspace", g.ws)
    res = fn(g)
    monkeypatch.setattr(K, "_workspace", cached)
    assert g.n_ws == plain.n_ws, "a launch took its workspace from outside the arena"
    assert arena.check(modified=modified, nan_ok=nan_ok)
    got = {k: v.detach().cpu().numpy().copy() for k, v in res.items()}
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s depends on where its operands are placed" % k
    return got


def randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def refused(K, call):
    """the launcher's SSAD_E_BADARG, raised by the wrapper before any launch"""
    with pytest.raises(K.KernelError, match=r"code -1\b|unsupported geometry"):
        call()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# Part A: 3x3 forward / data gradient
# ---------------------------------------------------------------------------------------------------------------------

def fwd_engine(K, name):
    """(pack(w, (pf, pd)), floats(M, K), run(al, xs, packed, bias, Cout, **kw)) of a 3x3 engine"""
    L = K.lib()
    if name == "direct":
        return (lambda w, out: K.conv_pack_filter(w, out=out), L.ssad_conv_packed_filter_floats,
                lambda al, xs, p, b, M, **kw: K.conv3x3_forward(xs, p, b, M, **kw))
    if name == "wino":
        return (lambda w, out: K.conv_wino_pack_filter(w, out=out), L.ssad_conv_wino_filter_floats,
                lambda al, xs, p, b, M, **kw: K.conv3x3_forward(xs, p, b, M, wino=True, **kw))
    if name == "wino24":
        return (lambda w, out: K.conv_wino24_pack_filter(w, out=out), L.ssad_conv_wino24_filter_floats,
                lambda al, xs, p, b, M, **kw: K.conv3x3_forward_wino24(xs, p, b, M, **kw))
    assert name == "split"
    return (lambda w, out: K.conv_split_pack_filter(w, out=out), L.ssad_conv_split_filter_floats,
            lambda al, xs, p, b, M, **kw: K.conv3x3_forward_split(xs, p, b, M, workspace=lambda n: al.ws(n, "split3x3"),
                                                                  **kw))


ODD = (2, 37, 131, 7, 9)            # odd channel counts, two images, odd map
FWD_CASES = [("direct", (2, 5, 7, 3, 4)), ("direct", (3, 8, 65, 2, 31)), ("direct", ODD),
             ("wino", (3, 8, 65, 2, 31)), ("wino", (1, 24, 130, 17, 33)), ("wino", ODD),
             ("wino24", (3, 40, 129, 2, 31)), ("wino24", (1, 24, 130, 17, 33)), ("wino24", ODD),
             ("split", (3, 40, 129, 2, 31)), ("split", (1, 24, 130, 17, 33)), ("split", ODD)]
SHAPE_ID = "N%d_C%d_M%d_%dx%d"


def sigmoid64(a):
    return 1.0 / (1.0 + np.exp(-a.astype(np.float64)))


@pytest.mark.parametrize("engine,shape", FWD_CASES, ids=[e + "_" + SHAPE_ID % s for e, s in FWD_CASES])
def test_guarded_conv3x3_forward_and_data_gradient(K, monkeypatch, engine, shape):
    """pack (forward + data gradient), bias + ReLU, bias + Sigmoid, masked data gradient"""
    N, Cin, M, H, W = shape
    rng = np.random.default_rng(7000 + sum(shape))
    X, Wt, b = randn(rng, N, Cin, H, W), randn(rng, M, Cin, 3, 3, scale=(9 * Cin) ** -0.5), randn(rng, M)
    dY, mask = randn(rng, N, M, H, W), np.maximum(randn(rng, N, Cin, H, W), 0)
    pack, floats, run = fwd_engine(K, engine)

    def fn(al):
        w = al.inp("w", Wt)
        pf, pd = al.out("packed_fwd", floats(M, Cin)), al.out("packed_dgrad", floats(Cin, M))
        pack(w, (pf, pd))
        x, bias = al.inp("x", X), al.inp("bias", b)
        y, ys = al.out("y", (N, M, H, W)), al.out("y_sigmoid", (N, M, H, W))
        run(al, [x], pf, bias, M, relu=True, out=[y])
        run(al, [x], pf, bias, M, sigmoid=True, out=[ys])
        dy, m, dx = al.inp("dy", dY), al.inp("mask", mask), al.out("dx", (N, Cin, H, W))
        run(al, [dy], pd, None, Cin, mask_by=[m], out=[dx])
        return dict(y=y, ys=ys, dx=dx)

    got = isolated(K, monkeypatch, fn, nan_ok={"packed_fwd": True, "packed_dgrad": True})
    ref = oracle.conv_forward(X, Wt, b)
    close(got["y"], oracle.relu(ref), CONV_RTOL, CONV_FLOOR, "relu(Y)")
    close(got["ys"], sigmoid64(ref), CONV_RTOL, CONV_FLOOR, "sigmoid(Y)")
    rdX = oracle.conv_backward(mask, Wt, dY, want_db=False)[2]
    close(got["dx"], np.where(mask > 0, rdX, 0), CONV_RTOL, CONV_FLOOR, "masked dX")
    assert np.all(got["dx"][mask <= 0] == 0)


LEVELS2 = [(2, 7, 9), (2, 2, 3)]         # two levels in one call, the second 2 x 3


@pytest.mark.parametrize("engine", ["direct", "wino", "wino24", "split"])
def test_guarded_conv3x3_two_levels_in_one_launch(K, monkeypatch, engine):
    """direct / F(2x2): conv3x3_forward_multi, two problems (own filter and bias) x two levels; F(2x4) / split: two
    levels sharing the filter; split: amax_in / amax_out words between guards as well."""
    Cin, M = 24, 40
    rng = np.random.default_rng(7100)
    pack, floats, run = fwd_engine(K, engine)
    nprob = 2 if engine in ("direct", "wino") else 1
    Xs = [[randn(rng, n, Cin, h, w) for n, h, w in LEVELS2] for _ in range(nprob)]
    Ws = [randn(rng, M, Cin, 3, 3, scale=(9 * Cin) ** -0.5) for _ in range(nprob)]
    bs = [randn(rng, M) for _ in range(nprob)]
    words_in = np.array([np.abs(x).max() for x in Xs[0]], np.float32).view(np.int32)

    def fn(al):
        probs, res = [], {}
        for p in range(nprob):
            w, pf = al.inp("w%d" % p, Ws[p]), al.out("packed%d" % p, floats(M, Cin))
            pack(w, (pf, None))
            xs = [al.inp("x%d_%d" % (p, l), x) for l, x in enumerate(Xs[p])]
            ys = [al.out("y%d_%d" % (p, l), (x.shape[0], M) + x.shape[2:]) for l, x in enumerate(Xs[p])]
            probs.append(dict(xs=xs, packed=pf, bias=al.inp("bias%d" % p, bs[p]), out=ys))
            res.update({"y%d_%d" % (p, l): y for l, y in enumerate(ys)})
        if nprob == 2:
            K.conv3x3_forward_multi(probs, M, relu=True, wino=engine == "wino")
        elif engine == "wino24":
            run(al, probs[0]["xs"], probs[0]["packed"], probs[0]["bias"], M, relu=True, out=probs[0]["out"])
        else:
            wi, wo = al.inp("amax_in", words_in), al.inp("amax_out", np.zeros(2, np.int32))
            run(al, probs[0]["xs"], probs[0]["packed"], probs[0]["bias"], M, relu=True, out=probs[0]["out"], amax_in=wi,
                amax_out=wo)
            res["amax_out"] = wo
        return res

    got = isolated(K, monkeypatch, fn, modified=("amax_out",) if engine == "split" else (),
                   nan_ok={"packed%d" % p: True for p in range(nprob)})
    for p in range(nprob):
        for l, x in enumerate(Xs[p]):
            ref = oracle.relu(oracle.conv_forward(x, Ws[p], bs[p]))
            close(got["y%d_%d" % (p, l)], ref, CONV_RTOL, CONV_FLOOR, "problem %d level %d" % (p, l))
    if engine == "split":
        want = np.array([np.abs(got["y0_%d" % l]).max() for l in range(2)], np.float32).view(np.int32)
        assert np.array_equal(got["amax_out"], want)


# ---------------------------------------------------------------------------------------------------------------------
# Part A: 3x3 filter gradient + bias gradient
# ---------------------------------------------------------------------------------------------------------------------

WGRAD_CASES = [(2, 16, 40, 9, 17), (3, 8, 65, 2, 31), ODD]


def wgrad_call(K, monkeypatch, engine):
    if engine != "split":
        monkeypatch.setenv("SSAD_WGRAD_ENGINE", engine)
    return lambda xs, dys, M, **kw: K.conv3x3_wgrad(xs, dys, M, split=engine == "split", **kw)


@pytest.mark.parametrize("shape", WGRAD_CASES, ids=lambda s: SHAPE_ID % s)
@pytest.mark.parametrize("engine", ["direct", "winograd", "split"])
def test_guarded_conv3x3_filter_and_bias_gradient(K, monkeypatch, engine, shape):
    """dW / db written, then accumulated onto; the odd case sums two levels (7 x 9 and 2 x 3)"""
    N, Cin, M, H, W = shape
    rng = np.random.default_rng(7200 + sum(shape))
    maps = [(H, W), (2, 3)] if shape == ODD else [(H, W)]
    Xs, dYs = [randn(rng, N, Cin, h, w) for h, w in maps], [randn(rng, N, M, h, w) for h, w in maps]
    baseW, baseb = randn(rng, M, Cin, 3, 3), randn(rng, M)
    wgrad = wgrad_call(K, monkeypatch, engine)

    def fn(al):
        xs = [al.inp("x%d" % l, x) for l, x in enumerate(Xs)]
        dys = [al.inp("dy%d" % l, d) for l, d in enumerate(dYs)]
        dW, db = al.out("dW", (M, Cin, 3, 3)), al.out("db", (M,))
        wgrad(xs, dys, M, dW=dW, db=db)
        aW, ab = al.inp("dW_acc", baseW), al.inp("db_acc", baseb)
        wgrad(xs, dys, M, dW=aW, db=ab, accumulate=True)
        return dict(dW=dW, db=db, aW=aW, ab=ab)

    got = isolated(K, monkeypatch, fn, modified=("dW_acc", "db_acc"))
    rW, rb = np.zeros((M, Cin, 3, 3), np.float64), np.zeros(M, np.float64)
    for x, d in zip(Xs, dYs):
        w_, b_, _ = oracle.conv_backward(x, np.zeros((M, Cin, 3, 3), np.float32), d)
        rW += w_
        rb += b_
    close(got["dW"], rW, CONV_RTOL, CONV_FLOOR, "dW")
    close(got["db"], rb, CONV_RTOL, CONV_FLOOR, "db")
    close(got["aW"], rW + baseW, CONV_RTOL, CONV_FLOOR, "dW accumulated")
    close(got["ab"], rb + baseb, CONV_RTOL, CONV_FLOOR, "db accumulated")


# ---------------------------------------------------------------------------------------------------------------------
# Part A: pointwise
# ---------------------------------------------------------------------------------------------------------------------

def pointwise_data(shape, seed):
    N, Cin, M, H, W = shape
    rng = np.random.default_rng(seed + sum(shape))
    return dict(X=randn(rng, N, Cin, H, W), Wt=randn(rng, M, Cin, scale=Cin ** -0.5), b=randn(rng, M),
                R=randn(rng, N, M, H, W), dY=randn(rng, N, M, H, W), mask=np.maximum(randn(rng, N, Cin, H, W), 0),
                base=randn(rng, N, Cin, H, W), baseW=randn(rng, M, Cin))


def pointwise_refs(d):
    M, Cin = d["Wt"].shape
    W4 = d["Wt"].reshape(M, Cin, 1, 1)
    ref = oracle.conv_forward(d["X"], W4, d["b"], kernel=1, stride=1, pad=0)
    rdW, _, rdX = oracle.conv_backward(d["X"], W4, d["dY"], kernel=1, stride=1, pad=0)
    return ref, rdW.reshape(M, Cin), rdX


@pytest.mark.parametrize("shape", [(2, 24, 40, 9, 12), (1, 16, 8, 2, 2), (2, 64, 64, 12, 16), (2, 37, 131, 3, 16), ODD],
                         ids=lambda s: SHAPE_ID % s)
def test_guarded_pointwise_exact_engine(K, monkeypatch, shape):
    """transpose_filter, conv1x1_forward (bias, residual, ReLU), conv1x1_dgrad (mask; accumulate_into), conv1x1_wgrad
    (written, accumulated) on the exact-fp32 GEMM.  What the geometry rules of ssad_kernels.h exclude is refused with
    SSAD_E_BADARG before any launch, and asserted so: P % 4 (everything), Cin % 4 (the data gradient's lda), P % 16 (the
    filter gradient)."""
    N, Cin, M, H, W = shape
    P = H * W
    d = pointwise_data(shape, 7300)
    ldm = (M + 3) // 4 * 4
    fwd_ok, dgrad_ok, wgrad_ok = P % 4 == 0, P % 4 == 0 and Cin % 4 == 0, P % 16 == 0

    def fn(al):
        w, wt = al.inp("w", d["Wt"]), al.out("wt", (Cin, ldm))
        K.transpose_filter(w, out=wt)
        res = dict(wt=wt)
        x, dy = al.inp("x", d["X"]), al.inp("dy", d["dY"])
        if fwd_ok:
            res["y"] = K.conv1x1_forward(x, wt, M, al.inp("bias", d["b"]), al.inp("residual", d["R"]), relu=True,
                                         out=al.out("y", (N, M, H, W)))
        if dgrad_ok:
            res["dx"] = K.conv1x1_dgrad(dy, w, mask=al.inp("mask", d["mask"]), out=al.out("dx", (N, Cin, H, W)))
            res["dxa"] = K.conv1x1_dgrad(dy, w, accumulate_into=al.inp("dx_acc", d["base"]))
        if wgrad_ok:
            res["dw"] = K.conv1x1_wgrad(x, dy, out=al.out("dw", (M, Cin)))
            res["dwa"] = K.conv1x1_wgrad(x, dy, out=al.inp("dw_acc", d["baseW"]), accumulate=True)
        return res

    got = isolated(K, monkeypatch, fn, modified=tuple(n for n, ok in (("dx_acc", dgrad_ok), ("dw_acc", wgrad_ok)) if ok))
    ref, rdW, rdX = pointwise_refs(d)
    want_wt = np.zeros((Cin, ldm), np.float32)
    want_wt[:, :M] = d["Wt"].T
    assert np.array_equal(bits(got["wt"]), bits(want_wt))                 # exact, zero padded
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if fwd_ok:
        close(got["y"], np.maximum(ref + d["R"], 0), CONV_RTOL, CONV_FLOOR, "relu(Y + R)")
    else:
        refused(K, lambda: K.conv1x1_forward(dev(d["X"]), dev(want_wt), M))
    if dgrad_ok:
        close(got["dx"], np.where(d["mask"] > 0, rdX, 0), CONV_RTOL, CONV_FLOOR, "masked dX")
        close(got["dxa"], d["base"] + rdX, CONV_RTOL, CONV_FLOOR, "dX accumulated")
    else:
        refused(K, lambda: K.conv1x1_dgrad(dev(d["dY"]), dev(d["Wt"])))
    if wgrad_ok:
        close(got["dw"], rdW, CONV_RTOL, CONV_FLOOR, "dW")
        close(got["dwa"], d["baseW"] + rdW, CONV_RTOL, CONV_FLOOR, "dW accumulated")
    else:
        refused(K, lambda: K.conv1x1_wgrad(dev(d["X"]), dev(d["dY"])))


@pytest.mark.parametrize("shape", [(2, 72, 300, 5, 5), (1, 16, 8, 2, 2), ODD, (1, 64, 72, 4, 6), (2, 37, 131, 3, 16)],
                         ids=lambda s: SHAPE_ID % s)
def test_guarded_pointwise_split_engine(K, monkeypatch, shape):
    """the same on the split-operand engine (any K, M, P for the GEMM; P % 8 for the filter gradient), plus
    gemm_split_pack_filter and the call that takes the pack and the |max| words"""
    N, Cin, M, H, W = shape
    P = H * W
    d = pointwise_data(shape, 7400)
    ldm = (M + 3) // 4 * 4
    wgrad_ok = P % 8 == 0
    x_word = np.array([np.abs(d["X"]).max()], np.float32).view(np.int32)

    def fn(al):
        ws = lambda n: al.ws(n, "gemm_split")
        w, wt = al.inp("w", d["Wt"]), al.out("wt", (Cin, ldm))
        K.transpose_filter(w, out=wt)
        x, dy, bias, r = al.inp("x", d["X"]), al.inp("dy", d["dY"]), al.inp("bias", d["b"]), al.inp("residual", d["R"])
        res = {}
        res["y"] = K.conv1x1_forward(x, wt, M, bias, r, relu=True, out=al.out("y", (N, M, H, W)), split=True, workspace=ws)
        res["dx"] = K.conv1x1_dgrad(dy, w, mask=al.inp("mask", d["mask"]), out=al.out("dx", (N, Cin, H, W)), split=True,
                                    workspace=ws)
        res["dxa"] = K.conv1x1_dgrad(dy, w, accumulate_into=al.inp("dx_acc", d["base"]), split=True, workspace=ws)
        pa = K.gemm_split_pack_filter(wt, ldm, Cin, M, out=al.out("packed_a", K.lib().ssad_gemm_split_filter_floats(Cin, M)))
        yw = al.inp("y_amax", np.zeros(1, np.int32))
        res["y2"] = K.conv1x1_forward_split_amax(x, wt, M, bias, r, relu=True, packed_a=pa, x_amax=al.inp("x_amax", x_word),
                                                 y_amax=yw, out=al.out("y2", (N, M, H, W)), workspace=ws)
        res["y_amax"] = yw
        if wgrad_ok:
            res["dw"] = K.conv1x1_wgrad(x, dy, out=al.out("dw", (M, Cin)), split=True)
            res["dwa"] = K.conv1x1_wgrad(x, dy, out=al.inp("dw_acc", d["baseW"]), accumulate=True, split=True)
        return res

    got = isolated(K, monkeypatch, fn, modified=("dx_acc", "y_amax") + (("dw_acc",) if wgrad_ok else ()),
                   nan_ok={"packed_a": True})
    ref, rdW, rdX = pointwise_refs(d)
    want = np.maximum(ref + d["R"], 0)
    close(got["y"], want, CONV_RTOL, CONV_FLOOR, "relu(Y + R)")
    assert np.array_equal(bits(got["y2"]), bits(got["y"])), "handed-over pack / |max| word changes the result"
    assert got["y_amax"][0] == np.array([np.abs(got["y"]).max()], np.float32).view(np.int32)[0]
    close(got["dx"], np.where(d["mask"] > 0, rdX, 0), CONV_RTOL, CONV_FLOOR, "masked dX")
    close(got["dxa"], d["base"] + rdX, CONV_RTOL, CONV_FLOOR, "dX accumulated")
    if wgrad_ok:
        close(got["dw"], rdW, CONV_RTOL, CONV_FLOOR, "dW")
        close(got["dwa"], d["baseW"] + rdW, CONV_RTOL, CONV_FLOOR, "dW accumulated")
    else:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        refused(K, lambda: K.conv1x1_wgrad(dev(d["X"]), dev(d["dY"]), split=True))


@pytest.mark.parametrize("n", [1, 5, 1023])
def test_guarded_split_absmax(K, monkeypatch, n):
    """element counts that are no multiple of 4; the two-level form measures (n,) and (7,) elements"""
    rng = np.random.default_rng(7500 + n)
    a, b = randn(rng, 1, 1, 1, n), randn(rng, 1, 1, 1, 7, scale=3.0)

    def fn(al):
        x, y = al.inp("a", a), al.inp("b", b)
        one = K.split_absmax(x, al.inp("word", np.zeros(1, np.int32)))
        two = K.split_absmax_levels([x, y], al.inp("words", np.zeros(2, np.int32)))
        return dict(one=one, two=two)

    got = isolated(K, monkeypatch, fn, modified=("word", "words"))
    wa, wb = (np.array([np.abs(t).max()], np.float32).view(np.int32)[0] for t in (a, b))
    assert got["one"][0] == wa and list(got["two"]) == [wa, wb]


# ---------------------------------------------------------------------------------------------------------------------
# Part A: strided / stem / resampling / pooling / grouped
# ---------------------------------------------------------------------------------------------------------------------

GEOM_ID = "N%d_C%d_M%d_%dx%d_k%ds%dp%d"
IMPLICIT = [((2, 16, 24, 12, 16, 3, 2, 1), False), ((1, 16, 24, 9, 11, 3, 2, 1), False), ((2, 37, 131, 7, 9, 3, 2, 1), False),
            ((1, 3, 64, 22, 32, 7, 2, 3), False), ((3, 3, 64, 21, 35, 7, 2, 3), False),
            ((2, 32, 256, 5, 7, 3, 2, 1), True), ((2, 37, 131, 7, 9, 3, 2, 1), True)]


@pytest.mark.parametrize("geom,split_k", IMPLICIT, ids=[GEOM_ID % g + ("_splitk" if s else "") for g, s in IMPLICIT])
def test_guarded_conv_implicit_gemm(K, monkeypatch, geom, split_k):
    """3x3 / 2 with bias + ReLU; the bare 7x7 / 2 stem geometry (3 -> 64, no epilogue term), which routes to stem.hip;
    the split-K plan through its workspace"""
    N, Cin, M, H, W, k, st, pad = geom
    stem = k == 7
    rng = np.random.default_rng(7600 + sum(geom))
    X, Wt, b = randn(rng, N, Cin, H, W), randn(rng, M, Cin, k, k, scale=(Cin * k * k) ** -0.5), randn(rng, M)
    oh, ow = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1

    def fn(al):
        y = K.conv_implicit_gemm(al.inp("x", X), al.inp("w", Wt), None if stem else al.inp("bias", b), stride=st, pad=pad,
                                 relu=not stem, out=al.out("y", (N, M, oh, ow)), split_k=split_k,
                                 wt=al.out("wt", (Cin * k * k, (M + 3) // 4 * 4)))
        return dict(y=y)

    got = isolated(K, monkeypatch, fn)
    ref = oracle.conv_forward(X, Wt, None if stem else b, kernel=k, stride=st, pad=pad)
    close(got["y"], ref if stem else np.maximum(ref, 0), CONV_RTOL, CONV_FLOOR, "Y")


KXK = [(2, 16, 24, 12, 16, 3, 2, 1), (1, 16, 24, 9, 11, 3, 2, 1), (2, 8, 40, 11, 9, 5, 3, 2), (2, 37, 131, 7, 9, 3, 2, 1)]


@pytest.mark.parametrize("geom", KXK, ids=lambda g: GEOM_ID % g)
def test_guarded_conv_kxk_gradients(K, monkeypatch, geom):
    """conv_kxk_wgrad (written, accumulated) and conv_kxk_dgrad (masked; accumulated); Cin*k*k % 4 != 0 is refused by
    the data gradient (its filter is a GEMM operand with 16-byte rows)"""
    N, Cin, M, H, W, k, st, pad = geom
    rng = np.random.default_rng(7700 + sum(geom))
    X, Wt = randn(rng, N, Cin, H, W), randn(rng, M, Cin, k, k, scale=(Cin * k * k) ** -0.5)
    oh, ow = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    dY, mask = randn(rng, N, M, oh, ow), np.maximum(randn(rng, N, Cin, H, W), 0)
    baseW, baseX = randn(rng, M, Cin, k, k), randn(rng, N, Cin, H, W)
    dgrad_ok = (Cin * k * k) % 4 == 0

    def fn(al):
        x, dy, w = al.inp("x", X), al.inp("dy", dY), al.inp("w", Wt)
        res = dict(dw=K.conv_kxk_wgrad(x, dy, k, st, pad, out=al.out("dw", Wt.shape)),
                   dwa=K.conv_kxk_wgrad(x, dy, k, st, pad, out=al.inp("dw_acc", baseW), accumulate=True))
        if dgrad_ok:
            res["dx"] = K.conv_kxk_dgrad(w, dy, H, W, st, pad, mask=al.inp("mask", mask), out=al.out("dx", X.shape))
            res["dxa"] = K.conv_kxk_dgrad(w, dy, H, W, st, pad, out=al.inp("dx_acc", baseX), accumulate=True)
        return res

    got = isolated(K, monkeypatch, fn, modified=("dw_acc",) + (("dx_acc",) if dgrad_ok else ()))
    rdW, _, rdX = oracle.conv_backward(X, Wt, dY, kernel=k, stride=st, pad=pad)
    close(got["dw"], rdW, CONV_RTOL, CONV_FLOOR, "dW")
    close(got["dwa"], baseW + rdW, CONV_RTOL, CONV_FLOOR, "dW accumulated")
    if dgrad_ok:
        close(got["dx"], np.where(mask > 0, rdX, 0), CONV_RTOL, CONV_FLOOR, "masked dX")
        close(got["dxa"], baseX + rdX, CONV_RTOL, CONV_FLOOR, "dX accumulated")
    else:
        dev = lambda a: torch.from_numpy(a).cuda()
        refused(K, lambda: K.conv_kxk_dgrad(dev(Wt), dev(dY), H, W, st, pad))


@pytest.mark.parametrize("shape", [(2, 5, 8, 12), (1, 3, 7, 16), (3, 4, 9, 10), (2, 37, 7, 9)], ids=lambda s: "N%d_C%d_%dx%d" % s)
def test_guarded_subsample_upsample_pool(K, monkeypatch, shape):
    """subsample / subsample_grad (written, accumulated), upsample_nearest (+ addend, in place) and its gradient,
    max_pool3x3s2_bias_relu: all exact (16-byte fast paths and general paths)"""
    N, Cc, H, W = shape
    rng = np.random.default_rng(7800 + sum(shape))
    X, b = randn(rng, N, Cc, H, W), randn(rng, Cc)
    sh, sw = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dS, base = randn(rng, N, Cc, sh, sw), randn(rng, N, Cc, H, W)
    add, dU = randn(rng, N, Cc, 2 * H, 2 * W), randn(rng, N, Cc, 2 * H, 2 * W)

    def fn(al):
        x, ds, du = al.inp("x", X), al.inp("d_sub", dS), al.inp("d_up", dU)
        res = dict(sub=K.subsample(x, 2, out=al.out("sub", dS.shape)),
                   subg=K.subsample_grad(ds, H, W, 2, out=al.out("subg", X.shape)),
                   subga=K.subsample_grad(ds, H, W, 2, accumulate_into=al.inp("subg_acc", base)),
                   up=K.upsample_nearest(x, 2, out=al.out("up", add.shape)),
                   upa=K.upsample_nearest(x, 2, addend=al.inp("addend", add), out=al.out("up_add", add.shape)),
                   upg=K.upsample_nearest_grad(du, 2, out=al.out("upg", X.shape)),
                   pool=K.max_pool3x3s2_bias_relu(x, al.inp("bias", b), relu=True, out=al.out("pool", dS.shape)))
        inplace = al.inp("up_inplace", add)
        res["upi"] = K.upsample_nearest(x, 2, addend=inplace, out=inplace)
        return res

    got = isolated(K, monkeypatch, fn, modified=("subg_acc", "up_inplace"))
    eq = lambda name, want: np.array_equal(bits(got[name]), bits(np.asarray(want, np.float32)))
    assert eq("sub", X[:, :, ::2, ::2])
    scat = np.zeros_like(X)
    scat[:, :, ::2, ::2] = dS
    assert eq("subg", scat) and eq("subga", base + scat)
    up = X.repeat(2, axis=2).repeat(2, axis=3)
    assert eq("up", up) and eq("upa", up + add) and eq("upi", up + add)
    d = dU.reshape(N, Cc, H, 2, W, 2)
    assert eq("upg", ((d[:, :, :, 0, :, 0] + d[:, :, :, 0, :, 1]) + d[:, :, :, 1, :, 0]) + d[:, :, :, 1, :, 1])
    z = torch.from_numpy(X) + torch.from_numpy(b).view(1, -1, 1, 1)
    assert eq("pool", torch.nn.functional.max_pool2d(torch.relu(z), 3, 2, 1).numpy())


@pytest.mark.parametrize("geom", [(2, 4, 16, 19, 23, 1), (2, 8, 4, 9, 17, 2), (3, 4, 5, 7, 9, 1)],
                         ids=lambda g: "N%d_cg%d_G%d_%dx%d_s%d" % g)
def test_guarded_grouped_conv3x3(K, monkeypatch, geom):
    N, cg, G, H, W, s = geom
    Cc = cg * G
    rng = np.random.default_rng(7900 + sum(geom))
    X, Wt, b = randn(rng, N, Cc, H, W), randn(rng, Cc, cg, 3, 3, scale=(9 * cg) ** -0.5), randn(rng, Cc)
    oh, ow = (H - 1) // s + 1, (W - 1) // s + 1
    floats = K.lib().ssad_grouped_conv3x3_filter_floats(Cc, G)

    def fn(al):
        packed = K.grouped_conv3x3_pack_filter(al.inp("w", Wt), G, out=al.out("packed", floats))
        y = K.grouped_conv3x3_forward(al.inp("x", X), None, al.inp("bias", b), group=G, stride=s, relu=True,
                                      out=al.out("y", (N, Cc, oh, ow)), packed=packed)
        return dict(y=y)

    got = isolated(K, monkeypatch, fn, nan_ok={"packed": True})
    ref = np.concatenate([oracle.conv_forward(np.ascontiguousarray(X[:, g * cg:(g + 1) * cg]),
                                              np.ascontiguousarray(Wt[g * cg:(g + 1) * cg]), b[g * cg:(g + 1) * cg],
                                              kernel=3, stride=s, pad=1) for g in range(G)], axis=1)
    close(got["y"], np.maximum(ref, 0), CONV_RTOL, CONV_FLOOR, "relu(Y)")


# ---------------------------------------------------------------------------------------------------------------------
# Part A: losses (guards, frozen operands, placement independence)
# ---------------------------------------------------------------------------------------------------------------------

LOSS_MAPS = [(1, 1, 1, 1366), (1, 1, 1, 11), (2, 2, 5, 7)]      # (N, A, H, W): 4098, 33 and 420 logits at 3 classes


def test_guarded_sigmoid_loss_family(K, monkeypatch):
    """distill_loss_forward / _backward, focal_loss_forward / _backward, cls_losses_fused, pow_sum over three levels"""
    Cn = 3
    rng = np.random.default_rng(8000)
    lv = [synth.distill_inputs(rng, n, a, Cn, h, w) for n, a, h, w in LOSS_MAPS]
    dkw = dict(gamma=2.0, alpha=0.5, beta=0.3, num_classes=Cn, ignored_label=-1, scale=0.5)
    fkw = dict(gamma=2.0, alpha=0.25, num_classes=Cn, scale=0.5)
    one3 = np.array([1.0, 0.5, 2.0], np.float32)

    def fn(al):
        levels = [(al.inp("logits%d" % i, x), al.inp("teacher%d" % i, q), al.inp("labels%d" % i, g))
                  for i, (x, q, g) in enumerate(lv)]
        norm, fg, dl = al.inp("normalizer", np.array([37.5], np.float32)), al.inp("fg", np.array([11.0], np.float32)), \
            al.inp("dloss", one3)
        outs = lambda nm: [al.out("%s%d" % (nm, i), x.shape) for i, (x, _, _) in enumerate(lv)]
        pairs = [(x, g) for x, _, g in levels]
        res = dict(distill=K.distill_loss_forward(levels, norm, out=al.out("distill", 3), **dkw),
                   focal=K.focal_loss_forward(pairs, fg, out=al.out("focal", 3), **fkw),
                   powsum=K.pow_sum([q for _, q, _ in levels], 1.8, out=al.out("powsum", ())))
        res.update({"ddx%d" % i: t for i, t in enumerate(K.distill_loss_backward(levels, norm, dl, out=outs("ddx"), **dkw))})
        res.update({"fdx%d" % i: t for i, t in enumerate(K.focal_loss_backward(pairs, fg, dl, out=outs("fdx"), **fkw))})
        d2, f2, dxs = K.cls_losses_fused(levels, norm, fg, dkw, fkw, out=outs("cdx"),
                                         losses=(al.out("fused_distill", 3), al.out("fused_focal", 3)))
        res.update(fused_distill=d2, fused_focal=f2, **{"cdx%d" % i: t for i, t in enumerate(dxs)})
        return res

    got = isolated(K, monkeypatch, fn)
    for i, (x, q, g) in enumerate(lv):
        _, d64, _ = oracle.distill_loss_forward(x, q, g, 37.5, **dkw)
        _, f64, _ = oracle.focal_loss_forward(x, g, 11.0, **fkw)
        close(got["distill"][i], d64, LOSS_RTOL, 0, "distill loss %d" % i)
        close(got["fused_distill"][i], d64, LOSS_RTOL, 0, "fused distill loss %d" % i)
        close(got["focal"][i], f64, LOSS_RTOL, 0, "focal loss %d" % i)
        close(got["fused_focal"][i], f64, LOSS_RTOL, 0, "fused focal loss %d" % i)
        close(got["ddx%d" % i], oracle.distill_loss_backward(x, q, g, 37.5, float(one3[i]), **dkw), DX_RTOL, DX_FLOOR, "ddx")
        close(got["fdx%d" % i], oracle.focal_loss_backward(x, g, 11.0, float(one3[i]), **fkw), DX_RTOL, DX_FLOOR, "fdx")
        both = oracle.distill_loss_backward(x, q, g, 37.5, 1.0, **dkw) + oracle.focal_loss_backward(x, g, 11.0, 1.0, **fkw)
        close(got["cdx%d" % i], both, DX_RTOL, 2 * DX_FLOOR, "fused dX %d" % i)
    close(got["powsum"], sum(np.sum(q.astype(np.float64) ** 1.8) for _, q, _ in lv), 1e-5, 0, "powsum")


def test_guarded_select_smooth_l1_levels(K, monkeypatch):
    rng = np.random.default_rng(8100)
    A = 2
    maps = [(2, 5, 7), (1, 1, 11), (2, 3, 4)]
    preds = [randn(rng, n, 4 * A, h, w) for n, h, w in maps]
    tg = []
    for l, (n, h, w) in enumerate(maps):
        if l == 2:
            tg.append((np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)))          # no foreground
            continue
        m = 5 + l
        flat = rng.choice(n * A * h * w, size=m, replace=False)
        n_, a_, y_, x_ = np.unravel_index(flat, (n, A, h, w))
        tg.append((randn(rng, m, 4, scale=0.5), np.stack([n_, 4 * a_, y_, x_], 1).astype(np.float32)))

    def fn(al):
        tp = [al.inp("pred%d" % l, p) for l, p in enumerate(preds)]
        tt = [(al.inp("Y%d" % l, y), al.inp("L%d" % l, lc)) if len(y) else (torch.zeros((0, 4), device="cuda"),) * 2
              for l, (y, lc) in enumerate(tg)]
        losses, dps = K.select_smooth_l1_levels(tp, tt, al.inp("S", np.array([41.0], np.float32)),
                                                al.inp("dloss", np.array([1.0], np.float32)), beta=0.11, scale=0.5,
                                                losses=al.out("losses", 3),
                                                d_preds=[al.out("dpred%d" % l, p.shape) for l, p in enumerate(preds)])
        return dict(losses=losses, **{"dp%d" % l: t for l, t in enumerate(dps)})

    got = isolated(K, monkeypatch, fn)
    S = np.array([41.0], np.float32)
    for l, (y, lc) in enumerate(tg):
        _, l64 = oracle.select_smooth_l1_forward(preds[l], y, lc, S, beta=0.11, scale=0.5)
        close(float(got["losses"][l]), l64, LOSS_RTOL, 1e-9, "loss %d" % l)
        close(got["dp%d" % l], oracle.select_smooth_l1_backward(preds[l], y, lc, S, 1.0, beta=0.11, scale=0.5), DX_RTOL,
              DX_FLOOR, "dY_hat %d" % l)


def test_guarded_softmax_family(K, monkeypatch):
    """group_spatial_softmax (+ drop_background, + gradient), softmax_focal_loss_forward / _backward over three levels;
    references in float64 from the operators' definitions"""
    Cn = 3
    rng = np.random.default_rng(8200)
    maps = [(1, 1, 1, 1365), (1, 1, 1, 11), (2, 2, 5, 7)]         # 4095, 33 and 420 logits
    xs = [randn(rng, n, a * Cn, h, w, scale=2.0) for n, a, h, w in maps]
    labs = [rng.integers(-1, Cn, size=(n, a, h, w)).astype(np.int32) for n, a, h, w in maps]
    dps = [randn(rng, *x.shape) for x in xs]
    kw = dict(gamma=2.0, alpha=0.25, num_classes=Cn, scale=0.5)
    dl3 = np.array([1.0, 0.5, 2.0], np.float32)

    def fn(al):
        tx = [al.inp("logits%d" % i, x) for i, x in enumerate(xs)]
        tl = [al.inp("labels%d" % i, g) for i, g in enumerate(labs)]
        fg = al.inp("fg", np.array([11.0], np.float32))
        res = {}
        loss, probs = K.softmax_focal_loss_forward(list(zip(tx, tl)), fg, out=al.out("loss", 3),
                                                   probs=[al.out("prob%d" % i, x.shape) for i, x in enumerate(xs)], **kw)
        dxs = K.softmax_focal_loss_backward([(None, g) for g in tl], probs, fg, al.inp("dloss", dl3),
                                            out=[al.out("dx%d" % i, x.shape) for i, x in enumerate(xs)], **kw)
        res.update(loss=loss, **{"prob%d" % i: t for i, t in enumerate(probs)}, **{"dx%d" % i: t for i, t in enumerate(dxs)})
        n, a, h, w = maps[2]
        res["sm"] = K.group_spatial_softmax(tx[2], Cn, out=al.out("softmax", xs[2].shape))
        res["smd"] = K.group_spatial_softmax(tx[2], Cn, drop_background=True, out=al.out("softmax_fg", (n, a * (Cn - 1), h, w)))
        res["smg"] = K.group_spatial_softmax_grad(res["sm"], al.inp("dprob", dps[2]), Cn, out=al.out("softmax_grad", xs[2].shape))
        return res

    got = isolated(K, monkeypatch, fn)
    for i, ((n, a, h, w), x, g) in enumerate(zip(maps, xs, labs)):
        z = x.astype(np.float64).reshape(n, a, Cn, h, w)
        p = np.exp(z - z.max(2, keepdims=True))
        p /= p.sum(2, keepdims=True)
        close(got["prob%d" % i], p.reshape(x.shape), 1e-5, 1e-7, "probabilities %d" % i)
        # softmax_focal_loss_op.cu: -alpha (1-p_t)^gamma log(p_t) for foreground targets, -(1-alpha) ... for background,
        # nothing for ignored anchors; normalised by fg_num
        t = np.clip(g, 0, None)
        pt = np.take_along_axis(p, t[:, :, None], 2)[:, :, 0]
        wgt = np.where(g > 0, 0.25, 0.75) * (g >= 0)
        ref = float(np.sum(-wgt * (1 - pt) ** 2.0 * np.log(np.maximum(pt, np.finfo(np.float32).tiny)))) * 0.5 / 11.0
        close(float(got["loss"][i]), ref, LOSS_RTOL, 0, "softmax focal loss %d" % i)
        assert np.all(got["dx%d" % i].reshape(n, a, Cn, h, w)[np.broadcast_to((g < 0)[:, :, None], z.shape)] == 0)
    n, a, h, w = maps[2]
    p = got["sm"].astype(np.float64).reshape(n, a, Cn, h, w)
    assert np.array_equal(bits(got["smd"]), bits(got["sm"].reshape(n, a, Cn, h, w)[:, :, 1:].reshape(n, a * (Cn - 1), h, w)))
    dp = dps[2].astype(np.float64).reshape(p.shape)
    close(got["smg"], (p * (dp - (p * dp).sum(2, keepdims=True))).reshape(xs[2].shape), 1e-5, 1e-7, "softmax gradient")


# ---------------------------------------------------------------------------------------------------------------------
# Part A: elementwise
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,skew", [(1, 0), (5, 0), (1023, 0), (1023, 4)], ids=lambda v: str(v))
def test_guarded_elementwise(K, monkeypatch, n, skew):
    """relu, relu_grad, sigmoid, sum_n, scale_, affine_channel_, relu_grad_rowsum; skew 4: every view starts 4 bytes
    into its slot, so aligned16() fails and the scalar paths of elementwise.hip run (these launchers only)"""
    rng = np.random.default_rng(8300 + n + skew)
    x, dy = randn(rng, n), randn(rng, n)
    terms = [randn(rng, n) for _ in range(5)]
    Cc, hw = 3, n if n <= 5 else (n + 3) // 4 * 4          # rows of 1024: the 16-byte path unless skewed; 1, 5: the tail loop
    x4, r4, dy4 = randn(rng, 2, Cc, hw, 1), randn(rng, 2, Cc, hw, 1), randn(rng, 2, Cc, hw, 1)
    sc, b = randn(rng, Cc), randn(rng, Cc)

    def fn(al):
        kw = dict(skew=skew)
        tx, tdy = al.inp("x", x, **kw), al.inp("dy", dy, **kw)
        res = dict(relu=K.relu(tx, out=al.out("relu", n, **kw)), sigmoid=K.sigmoid(tx, out=al.out("sigmoid", n, **kw)),
                   sum=K.sum_n([al.inp("term%d" % i, t, **kw) for i, t in enumerate(terms)], out=al.out("sum", n, **kw)),
                   scaled=K.scale_(al.inp("scaled", x, **kw), 0.37))
        res["relu_grad"] = K.relu_grad(res["relu"], tdy, out=al.out("relu_grad", n, **kw))
        res["affine"] = K.affine_channel_(al.inp("affine", x4, **kw), al.inp("bias", b), al.inp("scale", sc),
                                          al.inp("residual", r4, **kw), relu=True)
        y4 = al.inp("y4", np.maximum(x4, 0), **kw)
        res["rg_dx"], res["rg_sum"] = K.relu_grad_rowsum(y4, al.inp("dy4", dy4, **kw),
                                                         out=(al.out("rg_dx", x4.shape, **kw), al.out("rg_sum", (2, Cc))))
        return res

    got = isolated(K, monkeypatch, fn, modified=("scaled", "affine"))
    assert np.array_equal(got["relu"], oracle.relu(x))
    assert np.array_equal(got["relu_grad"], oracle.relu_grad(oracle.relu(x), dy))
    close(got["sigmoid"], oracle.sigmoid(x), 1e-6, 0, "sigmoid")
    s = terms[0].copy()
    for t in terms[1:]:
        s = s + t
    assert np.array_equal(got["sum"], s)
    assert np.array_equal(got["scaled"], x * np.float32(0.37))
    aff = np.maximum(x4.astype(np.float64) * sc.reshape(1, Cc, 1, 1) + b.reshape(1, Cc, 1, 1) + r4, 0)
    close(got["affine"], aff, 1e-6, 1e-7, "affine_channel")
    gdx = np.where(x4 > 0, dy4, 0).astype(np.float32)
    assert np.array_equal(got["rg_dx"], gdx)
    close(got["rg_sum"], gdx.astype(np.float64).sum((2, 3)), 1e-5, 1e-6, "rowsum")


def test_guarded_upsample_nearest_on_skewed_views(K, monkeypatch):
    """ssad_upsample_nearest / _grad live in elementwise.hip too and choose their 16-byte kernels by aligned16(): an even
    width on views that start 4 bytes into their slots must take the general kernels and give the same bits"""
    N, Cc, H, W = 2, 5, 8, 12
    rng = np.random.default_rng(8350)
    X, add, dU = randn(rng, N, Cc, H, W), randn(rng, N, Cc, 2 * H, 2 * W), randn(rng, N, Cc, 2 * H, 2 * W)

    def fn(al):
        x = al.inp("x", X, skew=4)
        return dict(upa=K.upsample_nearest(x, 2, addend=al.inp("addend", add, skew=4),
                                           out=al.out("up_add", add.shape, skew=4)),
                    upg=K.upsample_nearest_grad(al.inp("d_up", dU, skew=4), 2, out=al.out("upg", X.shape, skew=4)))

    got = isolated(K, monkeypatch, fn)
    assert np.array_equal(bits(got["upa"]), bits(X.repeat(2, axis=2).repeat(2, axis=3) + add))
    d = dU.reshape(N, Cc, H, 2, W, 2)
    want = ((d[:, :, :, 0, :, 0] + d[:, :, :, 0, :, 1]) + d[:, :, :, 1, :, 0]) + d[:, :, :, 1, :, 1]
    assert np.array_equal(bits(got["upg"]), bits(want))


@pytest.mark.parametrize("n", [1, 5, 1023])
def test_guarded_momentum_sgd(K, monkeypatch, n):
    """momentum_sgd_update_ (weight and bias rule) and ssad_momentum_sgd_flat: three segments carved out of flat w / g /
    m buffers back to back with gaps the update must not touch -- a filter of 5 rows x n with a per-row factor
    (row_scale / row_len), a bias of n, a filter of 7 -- against oracle.sgd_update with the row factor applied to the
    gradient first."""
    rng = np.random.default_rng(8400 + n)
    lr, mu, wd = 0.01, 0.9, 1e-4
    w1, g1, m1 = (randn(rng, n) for _ in range(3))
    segs = [(3, 5 * n, False, n), (3 + 5 * n + 2, n, True, 0), (3 + 6 * n + 4, 7, False, 0)]      # (offset, n, is_bias, row_len)
    total = segs[-1][0] + 7 + 5
    fw, fg, fm = (randn(rng, total) for _ in range(3))
    rows = randn(rng, 5) ** 2 + np.float32(0.5)

    def fn(al):
        lrt = al.inp("lr", np.array([lr], np.float32))
        res = {}
        for bias in (False, True):
            t = [al.inp("%s_%d" % (nm, bias), a) for nm, a in (("w", w1), ("g", g1), ("m", m1))]
            K.momentum_sgd_update_(t[0], t[1], t[2], lrt, mu, wd, bias)
            res.update({"w%d" % bias: t[0], "g%d" % bias: t[1], "m%d" % bias: t[2]})
        W, G, M_ = al.inp("flat_w", fw), al.inp("flat_g", fg), al.inp("flat_m", fm)
        rs = al.inp("row_scale", rows)
        tab = (K.SgdSegment * len(segs))()
        for i, (off, cnt, isb, rl) in enumerate(segs):
            tab[i] = K.SgdSegment(off, cnt, int(isb), rl, rs.data_ptr() if rl else None)
        rc = K.lib().ssad_momentum_sgd_flat(W.data_ptr(), G.data_ptr(), M_.data_ptr(), lrt.data_ptr(), mu, wd, tab, len(segs),
                                            None, K._stream())
        assert rc == 0
        res.update(W=W, G=G, M=M_)
        return res

    got = isolated(K, monkeypatch, fn, modified=("w_0", "g_0", "m_0", "w_1", "g_1", "m_1", "flat_w", "flat_g", "flat_m"))
    for bias in (False, True):
        rw, rg, rm = oracle.sgd_update(w1, g1, m1, lr, mu, wd, bias)
        for nm, r in (("w", rw), ("g", rg), ("m", rm)):
            close(got["%s%d" % (nm, bias)], r, 1e-6, 1e-7, "sgd %s" % nm)
    touched = np.zeros(total, bool)
    for off, cnt, isb, rl in segs:
        sl = slice(off, off + cnt)
        touched[sl] = True
        g = fg[sl] * np.repeat(rows, rl) if rl else fg[sl]
        rw, rg, rm = oracle.sgd_update(fw[sl], g.astype(np.float32), fm[sl], lr, mu, wd, isb)
        for nm, src, r in (("W", fw, rw), ("G", fg, rg), ("M", fm, rm)):
            close(got[nm][sl], r, 1e-6, 1e-7, "flat sgd %s, segment at %d" % (nm, off))
    for nm, src in (("W", fw), ("G", fg), ("M", fm)):
        assert np.array_equal(bits(got[nm][~touched]), bits(src[~touched])), "flat sgd wrote between its segments (%s)" % nm


# ---------------------------------------------------------------------------------------------------------------------
# Part B: non-finite locality of the convolutions and GEMMs
#
# Operands are N(0, 1), filters N(0, 1) / sqrt(K): unit scale on purpose -- with a NaN or an Inf in a tensor the split
# engines drop to scale 1 for that tensor, and at unit scale the hi + lo split alone stays at ~1e-7 of the output scale
# (a numpy model of the split at K = 360 gives 9e-8 and no element outside CONV_RTOL / CONV_FLOOR), so the bar below is
# the family's own.  Three images, channel counts that are no multiple of 8, a 7 x 9 map (the exact pointwise GEMM and
# the pointwise filter gradients take the nearest map their P % 4 / P % 16 / P % 8 rules admit, 8 x 10 and 8 x 9; the
# exact data gradient needs Cin % 4 == 0 and runs the 72 -> 300 layer only).
# ---------------------------------------------------------------------------------------------------------------------

VALUES = [("nan", np.float32(np.nan)), ("inf", np.float32(np.inf))]


def plants(shape):
    """the last channel of image 1 at an interior pixel; channel 0 of image 2 at pixel (0, 0); the last pixel of the last
    channel of image 0"""
    N, Cc, H, W = shape
    return [(1, Cc - 1, H // 2, W // 2), (2, 0, 0, 0), (0, Cc - 1, H - 1, W - 1)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def within_bar(got, ref, where, what):
    """the elements `where` of got are finite and within CONV_RTOL / CONV_FLOOR of ref (scale: max |ref| over the tensor)"""
    g, r = got[where].astype(np.float64), ref[where].astype(np.float64)
    assert np.all(np.isfinite(g)), "%s: %d non-finite outputs where none is allowed" % (what, int((~np.isfinite(g)).sum()))
    err, lim = np.abs(g - r), CONV_RTOL * np.abs(r) + CONV_FLOOR * float(np.abs(ref).max())
    assert np.all(err <= lim), "%s: %d outside tol, worst %.3e of the scale" % (what, int((err > lim).sum()),
                                                                                 float(err.max() / np.abs(ref).max()))


def tiles_that_read(shape, at, tile):
    """Winograd reach, exactly: the outputs of the th x tw tiles (aligned to the map's origin) whose (th + 2) x (tw + 2)
    input patch -- the tile and a one-pixel halo -- contains pixel at[2:] of image at[0]; every output channel"""
    (th, tw), (H, W) = tile, shape[2:]
    allowed = np.zeros(shape, bool)
    rows = [r for r in range(H) if r // th * th - 1 <= at[2] <= r // th * th + th]
    cols = [c for c in range(W) if c // tw * tw - 1 <= at[3] <= c // tw * tw + tw]
    allowed[at[0], :, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] = True
    return allowed


def check_locality(got, clean, ref_planted, ref_clean, at, tile, exact, what):
    """got: the run with the value planted in image at[0] at pixel at[2:]; tile: None = the non-finite set equals the
    oracle's, (th, tw) = it may extend to the Winograd tiles that read the pixel (tiles_that_read).  Whatever came out
    finite -- inside those tiles too -- is held to the oracle without the planted value: where the oracle with the value
    is finite it does not depend on it."""
    n0 = at[0]
    nf, nf_ref = ~np.isfinite(got), ~np.isfinite(ref_planted)
    assert nf_ref.any() and not nf_ref[np.arange(len(got)) != n0].any()            # the reference itself is local
    assert not (nf_ref & ~nf).any(), "%s: %d outputs the planted value must reach are finite" % (what, int((nf_ref & ~nf).sum()))
    others = np.arange(len(got)) != n0
    assert not nf[others].any(), "%s: the planted value reached another image (%d outputs)" % (what, int(nf[others].sum()))
    allowed = nf_ref if tile is None else tiles_that_read(got.shape, at, tile)
    leak = nf & ~allowed
    assert not leak.any(), "%s: %d non-finite outputs outside the allowed set, the first at %s" % (
        what, int(leak.sum()), tuple(int(v[0]) for v in np.nonzero(leak)))
    within_bar(got, ref_clean, ~nf, what)
    if exact:
        assert np.array_equal(bits(got[others]), bits(clean[others])), "%s: the other images' bits changed" % what


WINO_TILE = {"wino": (2, 2), "wino24": (2, 4)}        # output tile (rows, columns) of F(2x2) and F(2x4)


def forward_op(K, engine, form, Cin, M, H, W, seed):
    """(run(x numpy) -> y numpy, oracle(x), input shape, Winograd tile or None, exact) of one engine and form; fwd: the layer Cin -> M applied
    to X; dgrad: its data gradient applied to dY"""
    rng = np.random.default_rng(seed)
    k, st, pad = (1, 1, 0) if engine.startswith("pw") else (3, 2, 1) if engine in ("implicit", "kxk") else (3, 1, 1)
    Wt = randn(rng, M, Cin, k, k, scale=(Cin * k * k) ** -0.5)
    oh, ow = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    tw = dev(Wt)
    if form == "fwd":
        shape = (3, Cin, H, W)
        ref = lambda x: oracle.conv_forward(x, Wt, None, kernel=k, stride=st, pad=pad)
    else:
        shape = (3, M, oh, ow)
        X0 = np.zeros((3, Cin, H, W), np.float32)
        ref = lambda dy: oracle.conv_backward(X0, Wt, dy, kernel=k, stride=st, pad=pad)[2]
    if engine in ("direct", "wino", "wino24", "split"):
        pack, floats, run3 = fwd_engine(K, engine)
        pf, pd = dev(np.zeros(floats(M, Cin), np.float32)), dev(np.zeros(floats(Cin, M), np.float32))
        pack(tw, (pf, pd))
        al = Plain()
        run = lambda x: run3(al, [dev(x)], pf if form == "fwd" else pd, None, M if form == "fwd" else Cin)[0].cpu().numpy()
    elif engine in ("pw_exact", "pw_split"):
        split = engine == "pw_split"
        wt = K.transpose_filter(tw)
        if form == "fwd":
            run = lambda x: K.conv1x1_forward(dev(x), wt, M, split=split).cpu().numpy()
        else:
            run = lambda dy: K.conv1x1_dgrad(dev(dy), tw, split=split).cpu().numpy()
    elif engine == "implicit":
        assert form == "fwd"
        run = lambda x: K.conv_implicit_gemm(dev(x), tw, None, stride=st, pad=pad).cpu().numpy()
    else:
        assert engine == "kxk" and form == "dgrad"
        run = lambda dy: K.conv_kxk_dgrad(tw, dev(dy), H, W, st, pad).cpu().numpy()
    return run, ref, shape, WINO_TILE.get(engine), engine not in ("split", "pw_split")


FORWARD_B = [(e, f, 37, 131, 7, 9) for e in ("direct", "wino", "wino24", "split") for f in ("fwd", "dgrad")] + [
    ("pw_exact", "fwd", 72, 300, 8, 10), ("pw_exact", "dgrad", 72, 300, 8, 10), ("pw_exact", "fwd", 37, 131, 8, 10),
    ("pw_split", "fwd", 72, 300, 7, 9), ("pw_split", "dgrad", 72, 300, 7, 9), ("pw_split", "fwd", 37, 131, 7, 9),
    ("pw_split", "dgrad", 37, 131, 7, 9), ("implicit", "fwd", 37, 131, 7, 9), ("kxk", "dgrad", 36, 131, 7, 9)]


@pytest.mark.parametrize("case", FORWARD_B, ids=lambda c: "%s_%s_%dto%d_%dx%d" % c)
def test_nonfinite_locality_forward_and_data_gradient(K, case):
    """The set of non-finite outputs contains the oracle's and stays inside the planted value's image; it equals the
    oracle's for the direct, split and GEMM kernels and stays inside the 2 x 2 (F(2x2)) / 2 x 4 (F(2x4)) output tiles that
    read the pixel for the Winograd engines -- at most 2 pixels away, 4 along a row for F(2x4); every output that is finite,
    inside those tiles too, is within the bar of the oracle WITHOUT the planted value; on the exact-fp32
    engines the other two images keep their bits.  (3x3 / stride 2: conv_implicit_gemm forward; its data gradient,
    conv_kxk_dgrad, needs Cin * 9 % 4 == 0 and runs a 36 -> 131 layer.)"""
    engine, form, Cin, M, H, W = case
    run, ref, shape, tile, exact = forward_op(K, engine, form, Cin, M, H, W, 9000 + Cin + M)
    x0 = randn(np.random.default_rng(9100 + Cin), *shape)
    clean, ref_clean = run(x0), ref(x0)
    within_bar(clean, ref_clean, np.ones(clean.shape, bool), "clean run")
    for at in plants(shape):
        # in output coordinates (stride 2: the forward halves them, the data gradient doubles them)
        sy = (ref_clean.shape[2] / shape[2], ref_clean.shape[3] / shape[3])
        at_out = at[:2] + (int(at[2] * sy[0]), int(at[3] * sy[1]))
        for vname, v in VALUES:
            x = x0.copy()
            x[at] = v
            check_locality(run(x), clean, ref(x), ref_clean, at_out, tile, exact, "%s at %s" % (vname, at))


@pytest.mark.parametrize("engine", ["direct", "wino", "wino24", "split"])
def test_nonfinite_locality_across_the_levels_of_one_launch(K, engine):
    """two levels in one call, the value in level 0: level 1 (2 x 3) keeps its bits on the exact engines and stays within
    the bar on the split engine (each level has its own |max| word)"""
    Cin, M = 37, 131
    rng = np.random.default_rng(9200)
    Wt = randn(rng, M, Cin, 3, 3, scale=(9 * Cin) ** -0.5)
    X0, X1 = randn(rng, 3, Cin, 7, 9), randn(rng, 3, Cin, 2, 3)
    pack, floats, run3 = fwd_engine(K, engine)
    pf = dev(np.zeros(floats(M, Cin), np.float32))
    pack(dev(Wt), (pf, None))
    al = Plain()
    run = lambda a, b: [y.cpu().numpy() for y in run3(al, [dev(a), dev(b)], pf, None, M)]
    c0, c1 = run(X0, X1)
    r0, r1 = oracle.conv_forward(X0, Wt, None), oracle.conv_forward(X1, Wt, None)
    at = plants(X0.shape)[0]
    for vname, v in VALUES:
        x = X0.copy()
        x[at] = v
        g0, g1 = run(x, X1)
        check_locality(g0, c0, oracle.conv_forward(x, Wt, None), r0, at, WINO_TILE.get(engine),
                       engine != "split", "level 0, %s" % vname)
        within_bar(g1, r1, np.ones(g1.shape, bool), "level 1, %s in level 0" % vname)
        if engine != "split":
            assert np.array_equal(bits(g1), bits(c1)), "level 1 changed its bits with a %s in level 0" % vname


WGRAD_B = [("direct", 37, 131, 7, 9), ("winograd", 37, 131, 7, 9), ("split", 37, 131, 7, 9), ("pw_exact", 37, 131, 8, 10),
           ("pw_exact", 72, 300, 8, 10), ("pw_split", 37, 131, 8, 9), ("pw_split", 72, 300, 8, 9), ("kxk", 37, 131, 7, 9)]


@pytest.mark.parametrize("case", WGRAD_B, ids=lambda c: "%s_%dto%d_%dx%d" % c)
def test_nonfinite_locality_filter_gradients(K, monkeypatch, case):
    """A value planted in dY at output channel m0 may make only row m0 of dW (and db[m0]) non-finite; planted in X at
    channel c0, only column c0 (db not at all).  Every other element is finite and within the bar of the oracle without
    the planted value; what the oracle makes non-finite is non-finite."""
    engine, Cin, M, H, W = case
    rng = np.random.default_rng(9300 + Cin + H * W)
    k, st, pad = (1, 1, 0) if engine.startswith("pw") else (3, 2, 1) if engine == "kxk" else (3, 1, 1)
    oh, ow = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    X0, dY0 = randn(rng, 3, Cin, H, W), randn(rng, 3, M, oh, ow)
    W0 = np.zeros((M, Cin, k, k), np.float32)
    has_db = engine in ("direct", "winograd", "split")
    if has_db:
        wgrad = wgrad_call(K, monkeypatch, engine)
        run = lambda x, dy: tuple(t.cpu().numpy() for t in wgrad([dev(x)], [dev(dy)], M))
    elif engine == "kxk":
        run = lambda x, dy: (K.conv_kxk_wgrad(dev(x), dev(dy), k, st, pad).cpu().numpy(), None)
    else:
        run = lambda x, dy: (K.conv1x1_wgrad(dev(x), dev(dy), split=engine == "pw_split").cpu().numpy().reshape(W0.shape), None)
    ref = lambda x, dy: oracle.conv_backward(x, W0, dy, kernel=k, stride=st, pad=pad)[:2]
    rW, rb = ref(X0, dY0)
    cW, cb = run(X0, dY0)
    within_bar(cW, rW, np.ones(cW.shape, bool), "clean dW")
    for which, base in (("dY", dY0), ("X", X0)):
        for at in plants(base.shape):
            for vname, v in VALUES:
                t = base.copy()
                t[at] = v
                x, dy = (X0, t) if which == "dY" else (t, dY0)
                gW, gb = run(x, dy)
                pW, pb = ref(x, dy)
                what = "%s in %s at %s" % (vname, which, at)
                allowed = np.zeros(gW.shape, bool)
                if which == "dY":
                    allowed[at[1]] = True
                else:
                    allowed[:, at[1]] = True
                nf, nf_ref = ~np.isfinite(gW), ~np.isfinite(pW)
                assert nf_ref.any() and not (nf_ref & ~allowed).any()
                assert not (nf_ref & ~nf).any(), "%s: dW elements the value must reach are finite" % what
                leak = nf & ~allowed
                assert not leak.any(), "%s: %d non-finite dW elements outside %s, the first at %s" % (
                    what, int(leak.sum()), "row m0" if which == "dY" else "column c0", tuple(int(i[0]) for i in np.nonzero(leak)))
                within_bar(gW, rW, ~nf, what + ", dW")          # row m0 / column c0 too, wherever they came out finite
                if has_db:
                    ok = np.ones(M, bool)
                    if which == "dY":
                        ok[at[1]] = False
                        assert not np.isfinite(gb[at[1]])
                    within_bar(gb, rb, ok, what + ", db")


MASKED_B = [("direct", 37, 131, 7, 9), ("wino", 37, 131, 7, 9), ("wino24", 37, 131, 7, 9), ("split", 37, 131, 7, 9),
            ("pw_exact", 72, 300, 8, 10), ("pw_split", 37, 131, 7, 9), ("kxk", 36, 131, 7, 9)]


@pytest.mark.parametrize("case", MASKED_B, ids=lambda c: "%s_%dto%d_%dx%d" % c)
def test_nonfinite_data_gradient_under_the_mask_is_exactly_zero(K, case):
    """ReluGradient fused into the data gradient is a select: where mask <= 0 the result is 0 whatever dX would have
    been (a multiplication by the 0 / 1 mask would turn a NaN or an Inf into a NaN)"""
    engine, Cin, M, H, W = case
    rng = np.random.default_rng(9400 + Cin)
    k, st, pad = (1, 1, 0) if engine.startswith("pw") else (3, 2, 1) if engine == "kxk" else (3, 1, 1)
    oh, ow = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    Wt, dY0 = randn(rng, M, Cin, k, k, scale=(Cin * k * k) ** -0.5), randn(rng, 3, M, oh, ow)
    mask = np.maximum(randn(rng, 3, Cin, H, W), 0)
    tw, tm = dev(Wt), dev(mask)
    if engine in ("direct", "wino", "wino24", "split"):
        pack, floats, run3 = fwd_engine(K, engine)
        pf, pd = dev(np.zeros(floats(M, Cin), np.float32)), dev(np.zeros(floats(Cin, M), np.float32))
        pack(tw, (pf, pd))
        al = Plain()
        run = lambda dy: run3(al, [dev(dy)], pd, None, Cin, mask_by=[tm])[0].cpu().numpy()
    elif engine == "kxk":
        run = lambda dy: K.conv_kxk_dgrad(tw, dev(dy), H, W, st, pad, mask=tm).cpu().numpy()
    else:
        run = lambda dy: K.conv1x1_dgrad(dev(dy), tw, mask=tm, split=engine == "pw_split").cpu().numpy()
    X0 = np.zeros((3, Cin, H, W), np.float32)
    for at in plants(dY0.shape):
        for vname, v in VALUES:
            dy = dY0.copy()
            dy[at] = v
            got = run(dy)
            rdX = oracle.conv_backward(X0, Wt, dy, kernel=k, stride=st, pad=pad)[2]
            hit = ~np.isfinite(rdX) & (mask <= 0)
            assert hit.any()                                  # the case exists: a non-finite dX under the mask
            bad = got[mask <= 0] != 0
            assert not bad.any(), "%s at %s: %d masked outputs are not exactly 0 (%d of them non-finite)" % (
                vname, at, int(bad.sum()), int((~np.isfinite(got[mask <= 0])).sum()))
            assert not (~np.isfinite(rdX) & (mask > 0) & np.isfinite(got)).any()
