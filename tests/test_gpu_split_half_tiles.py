"""conv3x3_split.hip's work items as pairs of 8 x 16 half-tiles.

A level whose rows make an odd number of 8-row bands is cut into half-tiles, numbered flat over the batch and paired
(a pair may span two images; an odd count leaves an empty half).  Every output's sum is formed in the same chunk, tap
and MFMA order as with 16 x 16 tiles, so the results must be BIT-IDENTICAL to the launch that
SSAD_SPLIT_HALF_TILES=0 forces onto 16 x 16 tiles -- and both stay within the engine's bars against the oracle
(close_split of test_gpu_kernels.py, unwidened).  The plan's item count is host arithmetic: its test needs the built
library but no GPU, and carries no gpu mark."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle  # noqa: E402
from test_gpu_kernels import close_split, dev  # noqa: E402

gpu = pytest.mark.gpu
SWITCH = "SSAD_SPLIT_HALF_TILES"


@pytest.fixture(scope="module")
def K():
    from ssad_amd import kernels
    kernels.lib()
    return kernels


def both_modes(monkeypatch, fn):
    """fn() with the default plan and with 16 x 16 tiles forced"""
    monkeypatch.delenv(SWITCH, raising=False)
    a = fn()
    monkeypatch.setenv(SWITCH, "0")
    b = fn()
    monkeypatch.delenv(SWITCH)
    return a, b


# (N, Cin, M, H, W) -> items (default, forced full): what the case exercises
CASES = [((1, 16, 128, 8, 16), (1, 1)),        # single half, empty partner
         ((3, 16, 128, 5, 7), (2, 3)),         # pairs crossing images plus a dangling half
         ((2, 32, 128, 20, 28), (6, 8)),       # 3 bands x 2 column tiles
         ((1, 16, 200, 24, 16), (4, 4)),       # ragged M (two channel blocks)
         ((2, 16, 128, 40, 56), (20, 24)),     # P4-shaped level
         ((2, 24, 130, 9, 17), (8, 8))]        # two bands: stays in full mode, the mode boundary
IDS = ["N%d_C%d_M%d_%dx%d" % s for s, _ in CASES]

_problems = {}


def problem(shape):
    """inputs and the oracle's forward results (with and without bias), computed once per shape"""
    if shape not in _problems:
        N, Cin, M, H, W = shape
        rng = np.random.default_rng(3100 + sum(shape))
        X = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
        Wt = (rng.standard_normal((M, Cin, 3, 3)) * 0.05).astype(np.float32)
        b = rng.standard_normal(M).astype(np.float32)
        _problems[shape] = (X, Wt, b, oracle.conv_forward(X, Wt, b), oracle.conv_forward(X, Wt, None))
    return _problems[shape]


@gpu
@pytest.mark.parametrize("shape,items", CASES, ids=IDS)
def test_half_tiles_vs_oracle_and_bit_identical_to_full_tiles(K, monkeypatch, shape, items):
    N, Cin, M, H, W = shape
    X, Wt, b, ref, ref_nb = problem(shape)
    Xd, bd = dev(X), dev(b)
    pf = K.conv_split_pack_filter(dev(Wt))

    def run():
        return (K.conv3x3_split_items([(N, H, W)], M),
                K.conv3x3_forward_split([Xd], pf, bd, M)[0],
                K.conv3x3_forward_split([Xd], pf, bd, M, relu=True)[0],
                K.conv3x3_forward_split([Xd], pf, None, M)[0])
    got, full = both_modes(monkeypatch, run)
    assert (got[0], full[0]) == items
    for g, f, what in zip(got[1:], full[1:], ("bias", "bias + relu", "no bias")):
        assert torch.equal(g, f), "%s: half-tile result differs from the 16 x 16 result" % what
    close_split(got[1].cpu().numpy(), ref, "half tiles Y")
    close_split(got[2].cpu().numpy(), oracle.relu(ref), "half tiles relu")
    close_split(got[3].cpu().numpy(), ref_nb, "half tiles no bias")


@gpu
@pytest.mark.parametrize("shape", [(3, 16, 128, 5, 7), (2, 32, 128, 20, 28)], ids=lambda s: "N%d_C%d_M%d_%dx%d" % s)
def test_half_tiles_masked_data_gradient(K, monkeypatch, shape):
    """The data-gradient form: flipped / transposed pack, fused ReluGradient mask (conv3x3_split_kernel<true>)."""
    N, Cin, M, H, W = shape
    X, Wt = problem(shape)[:2]
    rng = np.random.default_rng(3150 + sum(shape))
    dY = rng.standard_normal((N, M, H, W)).astype(np.float32)
    dX = oracle.conv_backward(X, Wt, dY, want_db=False)[2]
    _, pd = K.conv_split_pack_filter(dev(Wt), want_dgrad=True)
    dYd, Xd = dev(dY), dev(X)
    assert K.conv3x3_split_items([(N, H, W)], Cin) < N * ((H + 15) // 16) * ((W + 15) // 16)      # half mode is on

    def run():
        return (K.conv3x3_forward_split([dYd], pd, None, Cin)[0],
                K.conv3x3_forward_split([dYd], pd, None, Cin, mask_by=[Xd])[0])
    got, full = both_modes(monkeypatch, run)
    assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])
    close_split(got[0].cpu().numpy(), dX, "half tiles dX")
    close_split(got[1].cpu().numpy(), np.where(X > 0, dX, 0), "half tiles masked dX")


@gpu
def test_half_tiles_multi_level_launch_and_output_max_words(K, monkeypatch):
    """One launch over full-mode and half-mode levels sharing a filter, two channel blocks, ReLU; the |max| words the
    epilogue folds in (amax_out) equal a measurement of the outputs, bit for bit, in both modes."""
    Cin, M = 32, 256
    levels = [(2, 16, 16), (2, 20, 28), (3, 5, 7), (1, 10, 14)]          # full, half, half, full
    rng = np.random.default_rng(3200)
    Xs = [rng.standard_normal((n, Cin, h, w)).astype(np.float32) for n, h, w in levels]
    Wt = (rng.standard_normal((M, Cin, 3, 3)) * 0.05).astype(np.float32)
    b = rng.standard_normal(M).astype(np.float32)
    refs = [oracle.relu(oracle.conv_forward(X, Wt, b)) for X in Xs]
    Xd, bd = [dev(X) for X in Xs], dev(b)
    pf = K.conv_split_pack_filter(dev(Wt))

    def run():
        words = torch.zeros(len(levels), dtype=torch.int32, device="cuda")
        Ys = K.conv3x3_forward_split(Xd, pf, bd, M, relu=True, amax_out=words)
        return K.conv3x3_split_items(levels, M), Ys, words
    got, full = both_modes(monkeypatch, run)
    assert (got[0], full[0]) == (22, 28)
    for items, Ys, words in (got, full):
        for l, Y in enumerate(Ys):
            assert int(words[l].item()) == int(K.split_absmax(Y).item()), "level %d, %d items" % (l, items)
    for l, (g, f) in enumerate(zip(got[1], full[1])):
        assert torch.equal(g, f), "level %d" % l
        close_split(g.cpu().numpy(), refs[l], "multi-level, level %d" % l)


@pytest.mark.parametrize("N,full,default", [(1, 106, 100), (16, 1696, 1584)])
def test_item_counts_of_the_600px_pyramid(K, monkeypatch, N, full, default):
    """Cout 256 over P3-P7 of a 600 px image: 53 tiles of 16 x 16 per image against 99 half-tiles = 49.5 pairs; only
    the levels with an odd number of 8-row bands (P4, P5, P7) change.  Host arithmetic of the built library: no GPU."""
    shapes = [(N, h, w) for h, w in ((80, 112), (40, 56), (20, 28), (10, 14), (5, 7))]
    got, forced = both_modes(monkeypatch, lambda: K.conv3x3_split_items(shapes, 256))
    assert (forced, got) == (full, default)
    per_level = both_modes(monkeypatch, lambda: [K.conv3x3_split_items([s], 128) for s in shapes])
    assert per_level[1] == [35 * N, 12 * N, 4 * N, N, N]
    assert per_level[0] == [35 * N, 10 * N, 3 * N, N, (N + 1) // 2]
