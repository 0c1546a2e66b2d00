"""The fp16 family at the edges of the fp16 range: loss-scaled gradients sit in and near the subnormal range, and fp16
overflows in normal operation (hence the dynamic loss scale).

  * conversions, exhaustively: all 65 536 fp16 bit patterns upwards; downwards every finite fp16 value, the exact midpoint
    to its successor (ties: inside the subnormal grid, and 65520 above the largest finite value), the fp32 neighbours
    just above and below each midpoint, +-0, +-Inf, NaN -- bit-equal to numpy (round to nearest even, gradual underflow,
    overflow to Inf, a NaN stays a NaN);
  * subnormal operands (k 2^-24, |k| <= 1023) against float64 at each family's bar: a flushed operand gives 0 and fails
    by the whole scale;
  * subnormal results from normal operands: within one step of the subnormal grid (2^-24) of the rounded float64 result
    (the fp32 accumulation error at this scale is ~1e-10);
  * saturation: the blocked fp16 result is +-Inf exactly where float16(float64 result) is, except within the fp32
    accumulation error (2e-5 relative) of the threshold 65520; the NCHW fp32 form of the same launch is finite.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_f16 import _conv64  # noqa: E402
from test_gpu_isolation_f16 import (BLOCKED_TOL, F16, F32_TOL, bar, blk, close_bb, dev, grouped64, ok, p,  # noqa: E402
                                    pack_dev, pw, sp, unblk, wgrad64)

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -24            # one step of the fp16 subnormal grid
MIN_NORMAL = 2.0 ** -14


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ssad_amd import kernels
    kernels.lib()
    return kernels


def same_or_nan(got, want, src=None):
    """bit equality, NaNs compared as NaN; on a mismatch the count and the first few (source, got, want) bit patterns"""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    u = {2: np.uint16, 4: np.uint32}
    gb, wb = got.view(u[got.itemsize]), want.view(u[want.itemsize])
    bad = np.flatnonzero(np.where(np.isnan(want), ~np.isnan(got), gb != wb))
    if bad.size:
        sb = np.ascontiguousarray(src).reshape(-1) if src is not None else None
        print("%d of %d differ; (source, got, want) bits of the first: %s" % (bad.size, got.size, [
            (hex(int(sb.view(u[sb.itemsize])[i])) if sb is not None else None, hex(int(gb[i])), hex(int(wb[i]))) for i in bad[:8]]))
    return bad.size == 0


# ---------------------------------------------------------------------------------------------------------------------
# conversions
# ---------------------------------------------------------------------------------------------------------------------

def test_every_fp16_pattern_widens_exactly(K):
    """cast_f16_to_f32, f16_unpack_activations, unblock: all 65 536 patterns"""
    L = K.lib()
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    t = dev(h)
    y = torch.empty(65536, dtype=torch.float32, device="cuda")
    ok(L.ssad_cast_f16_to_f32(p(t), p(y), C.c_longlong(65536), sp()))
    assert same_or_nan(y.cpu().numpy(), h.astype(np.float32))
    hb = h.reshape(1, 1, 64, 128, 8)                       # blocked [N][C/8][H][W][8]
    want = unblk(hb, 8)
    x = K.f16_unpack_activations(dev(hb), 8).cpu().numpy()
    assert same_or_nan(x, want.astype(np.float32), want)
    u = torch.empty((1, 8, 64, 128), dtype=F16, device="cuda")
    ok(L.ssad_f16_unblock_activations(p(dev(hb)), 1, 8, 64, 128, p(u), sp()))
    assert same_or_nan(u.cpu().numpy(), want, want)


def narrowing_inputs():
    pos = np.arange(0x7C00, dtype=np.uint16).view(np.float16)                   # every finite value >= +0
    succ = np.arange(1, 0x7C01, dtype=np.uint16).view(np.float16).astype(np.float64)
    succ[-1] = 65536.0                                                          # the successor of 65504 on the grid
    mid = ((pos.astype(np.float64) + succ) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (pos.astype(np.float64) + succ) / 2)      # midpoints are exact in fp32
    assert mid[-1] == 65520.0 and mid[0] == np.float32(2.0 ** -25)
    parts = [pos.astype(np.float32), mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(0))]
    a = np.concatenate(parts)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    a = np.concatenate([a, -a, special])
    return np.concatenate([a, np.zeros(-len(a) % 8, np.float32)])


def test_narrowing_rounds_to_nearest_even_with_gradual_underflow(K):
    """cast_f32_to_f16, f16_pack_activations at scale 1 and at a power-of-two scale (4, on inputs divided by 4)"""
    L = K.lib()
    a = narrowing_inputs()
    n = len(a)
    assert n > 250000
    with np.errstate(over="ignore"):
        want = a.astype(np.float16)
    assert np.isinf(want).sum() > 4 and (np.abs(want[np.isfinite(want)]) < MIN_NORMAL).sum() > 4000
    y = torch.empty(n, dtype=F16, device="cuda")
    ok(L.ssad_cast_f32_to_f16(p(dev(a)), p(y), C.c_longlong(n), sp()))
    assert same_or_nan(y.cpu().numpy(), want, a), "cast"
    x = a.reshape(1, 8, 1, n // 8)
    for scale in (1.0, 4.0):
        src = x / np.float32(scale)
        assert same_or_nan(src * np.float32(scale), x)                    # the division is exact: the kernel sees x
        got = unblk(K.f16_pack_activations(dev(src), scale).cpu().numpy(), 8)
        assert same_or_nan(np.ascontiguousarray(got).reshape(-1), want, a), "pack, scale %g" % scale


# ---------------------------------------------------------------------------------------------------------------------
# operands and results in the subnormal range
# ---------------------------------------------------------------------------------------------------------------------

def subnormals(rng, *shape):
    k = rng.integers(1, 1024, size=shape) * rng.choice([-1, 1], size=shape)
    x = (k * TINY).astype(np.float32)
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x) and np.all(np.abs(x) < MIN_NORMAL) and np.all(x != 0)
    return x


def magnitudes(rng, lo, hi, *shape):
    return (rng.uniform(lo, hi, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float16).astype(np.float32)


def conv3(K, x, Wt, nchw=False):
    M, Cc = Wt.shape[:2]
    y = K.conv3x3_forward_f16(dev(blk(x)), pack_dev(K, Wt), None, Cc, M, out_nchw_f32=nchw).cpu().numpy()
    return y if nchw else unblk(y, M)


def conv1(K, x, Wt):
    M, Cc = Wt.shape
    y = torch.empty((x.shape[0], M // 8) + x.shape[2:] + (8,), dtype=F16, device="cuda")
    ok(pw(K, dev(blk(x)), pack_dev(K, Wt, taps=1), y, Cc, M))
    return unblk(y.cpu().numpy(), M)


def grouped(K, x, Wt):
    L = K.lib()
    N, Cc, H, W = x.shape
    G = Cc // Wt.shape[1]
    pf = torch.zeros(L.ssad_grouped_conv3x3_f16_filter_halves(Cc, G), dtype=F16, device="cuda")
    ok(L.ssad_grouped_conv3x3_f16_pack_filter(p(dev(Wt)), Cc, G, p(pf), sp()))
    y = torch.empty((N, Cc // 8, H, W, 8), dtype=F16, device="cuda")
    ok(L.ssad_grouped_conv3x3_f16(p(dev(blk(x))), p(pf), p(None), N, Cc, H, W, G, 0, p(y), sp()))
    return unblk(y.cpu().numpy(), Cc)


def wgrad(K, x, dy, taps):
    L = K.lib()
    N, Cc, H, W = x.shape
    M = dy.shape[1]
    nb = (L.ssad_conv3x3_wgrad_f16_workspace_bytes if taps == 9 else L.ssad_conv1x1_wgrad_f16_workspace_bytes)(N, Cc, H, W, M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dw = torch.empty((M, Cc, 3, 3) if taps == 9 else (M, Cc), device="cuda")
    xb, dyb = dev(blk(x)), dev(blk(dy))
    if taps == 9:
        ok(L.ssad_conv3x3_wgrad_f16(p(xb), p(dyb), N, Cc, H, W, M, 0, 1.0, p(dw), p(None), p(ws), nb, sp()))
    else:
        ok(L.ssad_conv1x1_wgrad_f16(p(xb), p(dyb), N, Cc, H, W, M, 0, 1.0, p(None), p(dw), p(None), p(ws), nb, sp()))
    return dw.cpu().numpy()


def test_subnormal_operands_are_not_flushed(K):
    """x (or dY) holds exact fp16 subnormals k 2^-24, the other operand magnitudes in [16, 64]"""
    N, Cc, M, H, W = 2, 40, 40, 9, 17
    rng = np.random.default_rng(3000)
    X, Wt = subnormals(rng, N, Cc, H, W), magnitudes(rng, 16, 64, M, Cc, 3, 3)
    ref = _conv64(X.astype(np.float64), Wt.astype(np.float64), None)
    share = float((np.abs(ref) >= MIN_NORMAL).mean())
    print("subnormal operands, 3x3: %.1f %% of the float64 outputs in the normal fp16 range" % (100 * share))
    assert share > 0.99
    bar(conv3(K, X, Wt), ref, BLOCKED_TOL, "3x3 blocked")
    bar(conv3(K, X, Wt, nchw=True), ref, F32_TOL, "3x3 NCHW fp32")
    big = magnitudes(rng, 16, 64, N, Cc, H, W)                       # the same recipe transposed: subnormal dY
    dY = subnormals(rng, N, M, H, W)
    bar(wgrad(K, big, dY, 9), wgrad64(big, dY), F32_TOL, "3x3 filter gradient, subnormal dY")
    dYn = magnitudes(rng, 16, 64, N, M, H, W)
    bar(wgrad(K, X, dYn, 9), wgrad64(X, dYn), F32_TOL, "3x3 filter gradient, subnormal X")
    W1 = magnitudes(rng, 16, 64, M, Cc)
    close_bb(conv1(K, X, W1), np.einsum("mc,nchw->nmhw", W1.astype(np.float64), X.astype(np.float64)), "pointwise")
    bar(wgrad(K, big, dY, 1), wgrad64(big, dY, taps=1), F32_TOL, "pointwise filter gradient, subnormal dY")
    Xg, Wg = subnormals(rng, N, 64, H, W), magnitudes(rng, 16, 64, 64, 8, 3, 3)
    close_bb(grouped(K, Xg, Wg), grouped64(Xg, Wg, None, 8), "grouped")


def test_subnormal_results_are_rounded_not_flushed(K):
    """normal operands (|x| in [2^-9, 2^-8], |w| in [2^-10, 2^-9]), results in the subnormal range: within one step of
    the subnormal grid of the rounded float64 result; at least half of the reference outputs are non-zero subnormals"""
    N, H, W = 2, 9, 17
    rng = np.random.default_rng(3100)

    def check(got, ref, what):
        want = ref.astype(np.float16).astype(np.float64)
        sub = (want != 0) & (np.abs(want) < MIN_NORMAL)
        print("%s: %.1f %% of the reference outputs are non-zero fp16 subnormals, %.1f %% round to zero"
              % (what, 100 * sub.mean(), 100 * (want == 0).mean()))
        assert sub.mean() >= 0.5, what
        err = np.abs(got.astype(np.float64) - want)
        assert float(err.max()) <= TINY, "%s: off by %.2f steps of the subnormal grid; %d of %d subnormal results came out 0" % (
            what, float(err.max()) / TINY, int(((got == 0) & sub).sum()), int(sub.sum()))

    X, Wt = magnitudes(rng, 2.0 ** -9, 2.0 ** -8, N, 8, H, W), magnitudes(rng, 2.0 ** -10, 2.0 ** -9, 40, 8, 3, 3)
    check(conv3(K, X, Wt), _conv64(X.astype(np.float64), Wt.astype(np.float64), None), "3x3")
    W1 = magnitudes(rng, 2.0 ** -10, 2.0 ** -9, 40, 8)
    check(conv1(K, X, W1), np.einsum("mc,nchw->nmhw", W1.astype(np.float64), X.astype(np.float64)), "pointwise")
    Xg, Wg = magnitudes(rng, 2.0 ** -9, 2.0 ** -8, N, 64, H, W), magnitudes(rng, 2.0 ** -10, 2.0 ** -9, 64, 8, 3, 3)
    check(grouped(K, Xg, Wg), grouped64(Xg, Wg, None, 8), "grouped")


def test_saturation_to_infinity_where_the_rounded_result_is(K):
    """outputs of standard deviation ~65504: about a third overflow"""
    N, Cc, M, H, W = 2, 40, 40, 9, 17
    rng = np.random.default_rng(3200)
    X = rng.standard_normal((N, Cc, H, W)).astype(np.float16).astype(np.float32)

    def check(got, ref, what):
        with np.errstate(over="ignore"):
            want = ref.astype(np.float16)
        share = float(np.isinf(want).mean())
        print("%s: %.1f %% of the reference outputs exceed the fp16 range" % (what, 100 * share))
        assert 0.1 < share < 0.6, what
        near = np.abs(np.abs(ref) - 65520.0) <= 2e-5 * 65520.0
        wrong = (np.isinf(got) != np.isinf(want)) | (np.isinf(got) & (np.sign(got) != np.sign(ref)))
        assert not np.isnan(got).any() and not (wrong & ~near).any(), "%s: %d outputs saturate differently" % (
            what, int((wrong & ~near).sum()))
        fin = np.isfinite(got) & np.isfinite(want)
        assert float(np.abs(got[fin].astype(np.float64) - ref[fin]).max()) <= BLOCKED_TOL * 65504.0, what

    Wt = (rng.standard_normal((M, Cc, 3, 3)) * 65504.0 / np.sqrt(9 * Cc)).astype(np.float16).astype(np.float32)
    ref = _conv64(X.astype(np.float64), Wt.astype(np.float64), None)
    check(conv3(K, X, Wt), ref, "3x3 blocked")
    yn = conv3(K, X, Wt, nchw=True)
    assert np.all(np.isfinite(yn)), "the NCHW fp32 form of the same launch is finite"
    bar(yn, ref, F32_TOL, "3x3 NCHW fp32")
    W1 = (rng.standard_normal((M, Cc)) * 65504.0 / np.sqrt(Cc)).astype(np.float16).astype(np.float32)
    check(conv1(K, X, W1), np.einsum("mc,nchw->nmhw", W1.astype(np.float64), X.astype(np.float64)), "pointwise")
