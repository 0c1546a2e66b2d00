"""The reference definitions of tests/default_engine_ref.py against each other and against torch, on the geometries
of the default-engine sweep (tests/test_gpu_default_engine.py): a GPU comparison is worth what its reference is."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import default_engine_ref as R  # noqa: E402

CASES = R.CONV_CASES
IDS = [c["name"] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filter_times_im2col_equals_conv2d_f64(case):
    """W.reshape(M, -1) @ im2col(x), per group over contiguous row blocks, equals conv2d_f64 to 1e-12 relative."""
    X, Wt, b, _ = R.conv_inputs(case)
    g = case["geo"]
    G, M = g["group"], case["cout"]
    X, Wt = X.astype(np.float64), Wt.astype(np.float64)
    ref = R.conv2d_f64(X, Wt, None, g)
    assert ref.shape[2:] == R.out_hw(*case["hw"], g)
    for n in range(case["N"]):
        col = R.im2col(X[n], g)
        Kg, Mg = col.shape[0] // G, M // G
        got = np.concatenate([Wt[k * Mg:(k + 1) * Mg].reshape(Mg, -1) @ col[k * Kg:(k + 1) * Kg] for k in range(G)])
        err = np.abs(got.reshape(ref[n].shape) - ref[n]).max()
        assert err <= 1e-12 * np.abs(ref[n]).max(), (case["name"], n, err)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_col2im_is_the_exact_adjoint_of_im2col(case):
    """<im2col(x), c> == <x, col2im(c)> on small integers, bit for bit; and conv2d_grads_f64's dX is col2im(W^T dY)."""
    g = case["geo"]
    C = case["cin"]
    H, W = case["hw"]
    rng = np.random.default_rng(5)
    x = rng.integers(-4, 5, (C, H, W)).astype(np.float64)
    col = R.im2col(x, g)
    c = rng.integers(-4, 5, col.shape).astype(np.float64)
    back = R.col2im(c, C, H, W, g)
    assert back.shape == x.shape
    assert float((col * c).sum()) == float((x * back).sum())
    # every entry of col is an entry of x or a padding zero, and col2im of ones counts the reads of each pixel
    reads = R.col2im(np.ones_like(col), C, H, W, g)
    assert reads.sum() == np.count_nonzero(R.im2col(np.ones_like(x), g))
    if g["group"] == 1:
        X, Wt, _, dY = R.conv_inputs(case)
        _, _, dX = R.conv2d_grads_f64(X, Wt, dY, g)
        M = case["cout"]
        for n in range(case["N"]):
            dcol = Wt.astype(np.float64).reshape(M, -1).T @ dY[n].astype(np.float64).reshape(M, -1)
            got = R.col2im(dcol, C, H, W, g)
            assert np.abs(got - dX[n]).max() <= 1e-12 * np.abs(dX[n]).max()


@pytest.mark.parametrize("case", [c for c in R.POOL_CASES if c["sym"]], ids=lambda c: c["name"])
def test_max_pool_definition_matches_torch_on_tie_free_data(case):
    g = case["geo"]
    rng = np.random.default_rng(9)
    X = rng.standard_normal((2, 3) + case["hw"])
    xt = torch.tensor(X, requires_grad=True)
    yt = torch.nn.functional.max_pool2d(xt, g["kernel"], g["stride"], g["pads"][:2])
    Y = R.max_pool(X, g)
    assert np.array_equal(Y, yt.detach().numpy())
    dY = rng.standard_normal(Y.shape)
    yt.backward(torch.tensor(dY))
    np.testing.assert_allclose(R.max_pool_grad(X, Y, dY, g), xt.grad.numpy(), rtol=1e-12, atol=0)


def test_max_pool_grad_gives_every_tied_maximum_the_gradient():
    """The contract torch does not share: a window of equal values hands its gradient to each of them, and a pixel
    between two windows (stride > kernel) gets exactly 0."""
    g = R.geometry(2, 3, 0)
    X = np.ones((1, 1, 5, 5), np.float32)
    Y = R.max_pool(X, g)
    assert Y.shape == (1, 1, 2, 2) and (Y == 1).all()
    dY = np.arange(1, 5, dtype=np.float32).reshape(1, 1, 2, 2)
    dX = R.max_pool_grad(X, Y, dY, g)
    want = np.zeros((5, 5), np.float32)
    want[0:2, 0:2], want[0:2, 3:5], want[3:5, 0:2], want[3:5, 3:5] = 1, 2, 3, 4
    assert np.array_equal(dX[0, 0], want)
    # a NaN never becomes a maximum and receives nothing
    X[0, 0, 0, 0] = np.nan
    Y = R.max_pool(X, g)
    assert np.isfinite(Y).all() and R.max_pool_grad(X, Y, dY, g)[0, 0, 0, 0] == 0
