"""The descriptor-table builders of kernels.py, field by field over small CPU tensors: every launcher trusts the
addresses and sizes of these structs, and every eager wrapper and native program takes its tables from these
builders.  Host work only; nothing is launched."""
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import kernels as K

X = torch.zeros((2, 8, 4, 6), dtype=torch.float32)              # NCHW
XB = torch.zeros((3, 1, 5, 7, 8), dtype=torch.float16)          # blocked [N][C/8][H][W][8]
Y, AUX, PACKED, BIAS = (torch.zeros(4) for _ in range(4))
P = lambda t: t.data_ptr()


def _fields(table):
    return [tuple(getattr(e, name) for name, _ in e._fields_) for e in table]


@pytest.mark.parametrize("build, struct", [(K.conv_levels, K.ConvLevel), (K.f16_levels, K.F16Level)])
def test_level_tables(build, struct):
    tab = build([(X, Y, AUX, PACKED, BIAS), (XB, None, None, None, None), (XB, Y, None, BIAS, None)])
    assert tab._type_ is struct and len(tab) == 3
    assert _fields(tab) == [(P(X), P(Y), P(AUX), 2, 4, 6, P(PACKED), P(BIAS)),     # packed and bias are per row
                            (P(XB), None, None, 3, 5, 7, None, None),              # None is NULL; N, H, W = dims 0, 2, 3
                            (P(XB), P(Y), None, 3, 5, 7, P(BIAS), None)]
    assert len(build([])) == 0


def test_conv_levels_column_adapter():
    cols = K._conv_levels([X, XB], [Y, None], None, [PACKED, AUX], [None, BIAS])
    rows = K.conv_levels([(X, Y, None, PACKED, None), (XB, None, None, AUX, BIAS)])
    assert cols._type_ is K.ConvLevel and bytes(cols) == bytes(rows)
    assert bytes(K._conv_levels([X], None, None)) == bytes(K.conv_levels([(X, None, None, None, None)]))
    assert len(K._conv_levels([], None, None)) == 0
    with pytest.raises(K.KernelError):          # a launch over len(xs) levels would read past a shorter table
        K._conv_levels([X, XB], [Y], None)


def test_f16_wgrad_levels():
    tab = K.f16_wgrad_levels([XB, X], [Y, AUX])
    assert tab._type_ is K.F16WgradLevel
    assert _fields(tab) == [(P(XB), P(Y), 3, 5, 7), (P(X), P(AUX), 2, 4, 6)]
    assert len(K.f16_wgrad_levels([], [])) == 0


def test_f16_pack_entries():
    tab = K.f16_pack_entries([(X, Y, AUX, 64, 256, 9), (XB, Y, None, 36, 20, 1)])
    assert tab._type_ is K.F16PackEntry
    assert _fields(tab) == [(P(X), P(Y), P(AUX), 64, 256, 9, 0), (P(XB), P(Y), None, 36, 20, 1, 0)]
    assert len(K.f16_pack_entries([])) == 0


def test_pack_entries():
    tab = K.pack_entries([(X, 136, 20, Y, None), (X, 36, 20, None, AUX), (XB, 8, 8, Y, AUX)])
    assert tab._type_ is K.PackEntry
    assert _fields(tab) == [(P(X), 136, 20, P(Y), None), (P(X), 36, 20, None, P(AUX)), (P(XB), 8, 8, P(Y), P(AUX))]
    assert len(K.pack_entries([])) == 0


def test_grouped_pack_entries():
    tab = K.grouped_pack_entries([(X, Y, AUX, 256, 64), (X, None, AUX, 512, 32), (X, Y, None, 2048, 32)])
    assert tab._type_ is K.GroupedPackEntry
    assert _fields(tab) == [(P(X), P(Y), P(AUX), 256, 64), (P(X), None, P(AUX), 512, 32),
                            (P(X), P(Y), None, 2048, 32)]
    assert len(K.grouped_pack_entries([])) == 0
    with pytest.raises(K.KernelError, match="an empty table"):      # the eager wrapper refuses before any device work
        K.grouped_conv3x3_pack_filters([])


def test_sgd_segments():
    big = (1 << 33) + 5                                             # offsets and lengths are 64-bit
    tab = K.sgd_segments([(0, 576, False, 0, None), (big, big + 1, 0, 36, Y), (7, 64, True, 0, None),
                          (9, 3, 0, 36, None)])
    assert tab._type_ is K.SgdSegment
    assert _fields(tab) == [(0, 576, 0, 0, None), (big, big + 1, 0, 36, P(Y)), (7, 64, 1, 0, None),
                            (9, 3, 0, 0, None)]                     # no row scale: row_len is not used and stays 0
    assert len(K.sgd_segments([])) == 0


def test_f16_flags():
    assert K.f16_flags() == 0
    assert K.f16_flags(relu=True) == K.CONV_RELU == 1
    assert K.f16_flags(sigmoid=True, out_nchw_f32=True) == K.CONV_SIGMOID | K.F16_OUT_NCHW_F32 == 20
    assert K.f16_flags(True, False, True, False) == K.CONV_RELU | K.CONV_MASK_AUX == 3

