"""tests/guarded.py checked on a CPU arena, no kernel involved: every kind of damage the GPU isolation tests rely on
it to see must be reported (with the view it is next to), and a clean run must pass."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import guarded  # noqa: E402
from guarded import Arena, GUARD, SENTINEL  # noqa: E402


def fresh():
    rng = np.random.default_rng(0)
    a = Arena(Arena.bytes_for(4 * 35, 4 * 35, 100, 4, 40), device="cpu")
    x = a.take((5, 7), torch.float32, "x", data=rng.standard_normal((5, 7)).astype(np.float32))
    y = a.take((5, 7), torch.float32, "y")
    ws = a.take_bytes(100, "ws")
    lab = a.take((1,), torch.int32, "word", data=np.zeros(1, np.int32))
    return a, x, y, ws, lab


def test_layout_alignment_guards_and_sentinel_fill():
    a, x, y, ws, word = fresh()
    assert SENTINEL == 0x7FC0A5A5 and np.isnan(np.array([SENTINEL], np.uint32).view(np.float32)[0])
    prev_end = 0
    for v in a.views:
        assert v.off % 256 == 0 and v.tensor.data_ptr() % 256 == 0
        assert v.off - prev_end >= GUARD
        assert v.tensor.is_contiguous()
        prev_end = v.off + v.nbytes
    assert a.nbytes - prev_end >= GUARD                            # the last view has its guard too
    assert ws.numel() == 100 and ws.dtype == torch.uint8
    assert bool((y.view(torch.int32) == SENTINEL).all())           # outputs start full of sentinel
    assert bool((a.words == SENTINEL).sum() == a.nbytes // 4 - 35 - 1)
    # a skewed view: 4 bytes into its slot
    s = a.take((9,), torch.float32, "skewed", skew=4)
    assert s.data_ptr() % 256 == 4
    with pytest.raises(MemoryError):
        a.take_bytes(a.nbytes, "too much")


def test_clean_run_passes():
    a, x, y, ws, word = fresh()
    y.copy_(x * 2)
    ws[:10] = 1                                                   # a workspace may be written partly
    assert a.check()
    word.fill_(7)
    with pytest.raises(AssertionError, match="frozen operand 'word'"):
        a.check()
    assert a.check(modified=("word",))


def test_write_of_one_word_before_a_view_is_reported():
    a, x, y, ws, word = fresh()
    y.copy_(x)
    off = next(v.off for v in a.views if v.name == "y")
    a.words[off // 4 - 1] = 0
    with pytest.raises(AssertionError, match=r"guard band overwritten: 1 dirty word.*4 bytes before its start of view 'y'"):
        a.check()


def test_write_just_after_a_view_is_reported():
    a, x, y, ws, word = fresh()
    y.copy_(x)
    v = next(v for v in a.views if v.name == "x")
    a.bytes[v.off + v.nbytes:v.off + v.nbytes + 8] = 0
    with pytest.raises(AssertionError, match=r"2 dirty word\(s\).*the first 0 bytes past its end of view 'x'.*"
                                             r"the last 7 bytes past its end of view 'x'"):
        a.check()
    # a workspace whose length is no multiple of 4: the very next byte counts
    a, x, y, ws, word = fresh()
    y.copy_(x)
    v = next(v for v in a.views if v.name == "ws")
    a.bytes[v.off + 100] = 0
    with pytest.raises(AssertionError, match="0 bytes past its end of view 'ws'"):
        a.check()


def test_write_of_the_same_bits_as_a_float_nan_fill_is_still_seen():
    """the payload distinguishes the sentinel from a NaN a kernel could produce"""
    a, x, y, ws, word = fresh()
    y.copy_(x)
    off = next(v.off for v in a.views if v.name == "y")
    a.bytes[off - 64:off].view(torch.float32).fill_(float("nan"))
    with pytest.raises(AssertionError, match="guard band overwritten: 16 dirty"):
        a.check()


def test_write_into_a_frozen_input_is_reported():
    a, x, y, ws, word = fresh()
    y.copy_(x)
    x[2, 3] += 1.0
    with pytest.raises(AssertionError, match=r"frozen operand 'x' modified: 1 dirty word\(s\), the first at byte 68"):
        a.check()
    assert a.check(modified=("x",))
    # the sign of a zero is a modification too (bit identity, not ==)
    a, x, y, ws, word = fresh()
    y.copy_(x)
    word.view(torch.float32).fill_(-0.0)
    with pytest.raises(AssertionError, match="frozen operand 'word'"):
        a.check()


def test_output_left_unwritten_is_reported_unless_the_reference_has_a_nan_there():
    a, x, y, ws, word = fresh()
    y[:4].copy_(x[:4])
    with pytest.raises(AssertionError, match=r"output 'y' not written completely: 7 word\(s\).*byte 112"):
        a.check()
    ok = np.zeros((5, 7), bool)
    ok[4] = True
    assert a.check(nan_ok={"y": ok})
    ok[4, 6] = False
    with pytest.raises(AssertionError, match=r"1 word\(s\)"):
        a.check(nan_ok={"y": ok})
    assert a.check(nan_ok={"y": True})
    with pytest.raises(AssertionError, match="no view named"):
        a.check(modified=("nope",))


def fresh16():
    rng = np.random.default_rng(1)
    a = Arena(Arena.bytes_for(2 * 48, 2 * 48, 2 * 3), device="cpu")
    x = a.take((2, 3, 8), torch.float16, "x", data=rng.standard_normal((2, 3, 8)).astype(np.float16))
    y = a.take((2, 3, 8), torch.float16, "y")
    return a, x, y


def test_sentinel_word_as_two_halves():
    a, x, y = fresh16()
    h = y.reshape(-1).numpy().view(np.uint16)
    assert h[0] == 0xA5A5 and h[1] == 0x7FC0                       # memory order: -0.02205, then a NaN
    v = h[:2].view(np.float16)
    assert abs(float(v[0]) + 0.02205) < 1e-5 and np.isnan(v[1])


def test_unwritten_word_in_an_fp16_output_is_reported():
    a, x, y = fresh16()
    y.copy_(x)
    assert a.check()                                               # fully written: passes
    a, x, y = fresh16()
    y.copy_(x)
    y.reshape(-1).view(torch.int32)[5] = SENTINEL                  # halves 10, 11 left as they were
    with pytest.raises(AssertionError, match=r"output 'y' not written completely: 1 word\(s\).*byte 20"):
        a.check()
    # one written half of a word is enough for the word to count as written
    a, x, y = fresh16()
    y.copy_(x)
    y.reshape(-1).view(torch.int32)[5] = SENTINEL
    y.reshape(-1)[11] = 1.0
    assert a.check()


def test_nan_ok_for_an_fp16_output_is_per_half_reduced_to_words():
    a, x, y = fresh16()
    y.copy_(x)
    y.reshape(-1).view(torch.int32)[5] = SENTINEL
    y.reshape(-1).view(torch.int32)[9] = SENTINEL
    ok = np.zeros((2, 3, 8), bool)
    ok.reshape(-1)[10] = True                                      # the reference is NaN in the even half of word 5
    with pytest.raises(AssertionError, match=r"1 word\(s\).*byte 36"):
        a.check(nan_ok={"y": ok})
    ok.reshape(-1)[19] = True                                      # ... and in the odd half of word 9
    assert a.check(nan_ok={"y": ok})
    ok[:] = False
    ok.reshape(-1)[12] = True                                      # a NaN next door excuses nothing
    with pytest.raises(AssertionError, match=r"2 word\(s\)"):
        a.check(nan_ok={"y": ok})
    assert a.check(nan_ok={"y": True})


def test_fp16_output_of_odd_length_is_not_searched():
    a = Arena(Arena.bytes_for(6), device="cpu")
    a.take((3,), torch.float16, "odd")
    assert a.check()


def fresh64():
    rng = np.random.default_rng(2)
    a = Arena(Arena.bytes_for(8 * 6, 8 * 6, 8 * 3, 5), device="cpu")
    x = a.take((2, 3), torch.float64, "x", data=rng.standard_normal((2, 3)))
    y = a.take((2, 3), torch.float64, "y")
    k = a.take((3,), torch.int64, "k")
    return a, x, y, k


def test_half_written_float64_output_is_reported():
    """an 8-byte element is unwritten when BOTH halves hold the sentinel word; a fully written view passes"""
    a, x, y, k = fresh64()
    y.copy_(x)
    k.fill_(-1)
    assert a.check()                                               # fully written: passes
    a, x, y, k = fresh64()
    y[0].copy_(x[0])
    k.fill_(0)
    with pytest.raises(AssertionError, match=r"output 'y' not written completely: 3 word\(s\).*byte 24 of the view "
                                             r"\(element \(1, 0\)\)"):
        a.check()
    ok = np.zeros((2, 3), bool)
    ok[1] = True
    assert a.check(nan_ok={"y": ok})
    ok[1, 2] = False
    with pytest.raises(AssertionError, match=r"output 'y' not written completely: 1 word"):
        a.check(nan_ok={"y": ok})
    # one written half is a written element: 2^32 * k + sentinel in the low half is a value an int64 may hold
    a, x, y, k = fresh64()
    y.copy_(x)
    k.fill_(0)
    k.view(torch.int32)[2] = SENTINEL
    y.reshape(-1).view(torch.int32)[5] = SENTINEL
    assert a.check()
    k.view(torch.int32)[3] = SENTINEL
    with pytest.raises(AssertionError, match=r"output 'k' not written completely: 1 word\(s\).*byte 8 "):
        a.check()


def test_one_byte_outputs_are_not_searched():
    a = Arena(Arena.bytes_for(8), device="cpu")
    a.take((8,), torch.uint8, "flags")
    assert a.check()                                               # their tests assert the value set themselves
    assert a.untouched("flags").shape == (2,) and a.untouched("flags").all()


def test_untouched_sees_a_one_word_write():
    a, x, y, ws, word = fresh()
    u = a.untouched("y")
    assert u.shape == (5, 7) and u.dtype == bool and u.all()
    y[3, 4] = 0.0
    u = a.untouched("y")
    assert not u[3, 4] and u.sum() == 34
    y.view(torch.int32)[3, 4] = SENTINEL                           # the sentinel's own bits count as untouched
    assert a.untouched("y").all()
    assert not a.untouched("x").any()                              # an input: nothing of it is sentinel
    a, x, y, k = fresh64()
    u = a.untouched("y")
    assert u.shape == (2, 3, 2) and u.all()
    y.reshape(-1).view(torch.int32)[3] = 0                         # the high half of element (0, 1)
    u = a.untouched("y")
    assert not u[0, 1, 1] and u[0, 1, 0] and u.sum() == 11
    a, x, y = fresh16()
    assert a.untouched("y").shape == (24,)                         # 2-byte elements: flat words
    with pytest.raises(AssertionError, match="no view named"):
        a.untouched("nope")


def test_module_is_a_plain_helper():
    assert not hasattr(guarded, "pytest_configure") and not any(n.startswith("pytest_") for n in dir(guarded))
