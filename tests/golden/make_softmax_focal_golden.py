#!/usr/bin/env python3
"""Golden vectors for GroupSpatialSoftmax and SoftmaxFocalLoss from the reference's own kernels.

The reference's device code (caffe2/modules/detectron/group_spatial_softmax_op.cu and softmax_focal_loss_op.cu)
is plain C++ inside `__global__` functions whose only CUDA-isms are the grid-stride loop macro and the `max`
overloads.  At generation time this script reads those files where they lie under /root/reference, cuts out the
`__global__` function definitions and the loop macro (caffe2/core/common_gpu.h) into a TEMPORARY directory, and
compiles them with g++ behind the shim below -- `__global__` defined away, a <<<1, 1>>> launch geometry (one
thread walks the whole grid-stride loop) and CUDA's `max(float, float)` / `max(float, double)` overloads.  The
kernels are then called on the inputs and only inputs and outputs are stored: nothing compiled and none of the
reference's text is written into the repository.

What the reference does on the host around the kernels is RESTATED here in numpy (it is three library calls):
  * SoftmaxFocalLoss:          math::Sum over the per-cell losses (accumulated in float64 here, rounded to float32
                               once) and math::Scale by `scale` (one float32 multiply);
  * SoftmaxFocalLossGradient:  math::Scale of dX by `scale` (float32 multiply per element);
  * GroupSpatialSoftmaxGradient: Copy dY -> dX, then after the two kernels math::Mul by Y (float32 multiply).

Logits are drawn, then rounded to the nearest float16 value, so that they can be stored in half the bytes; they are
float32 inputs of exactly those values.  The five-level call alone is 188 082 logits (N*A*C = 1458 channels x 129
positions): its arrays are spread over two more files to keep every file under the repository's size limit.

    softmax_focal_ref.npz            single-level cases: x_<set> / p_<set> (logits, reference probabilities),
                                     case_<k>_{labels,fg,params,loss,dx}, params = gamma, alpha, scale, dloss;
                                     `case_sets` / `case_names` name each case's data set; sg_<set>_{dy,dx}: softmax
                                     gradient cases on the same probabilities
    softmax_focal_ref_levels_a.npz   the five-level call: lv_params (gamma, alpha, scale, dloss, fg_num), lv_maps,
                                     lv_loss and per level lv_<l>_{x,labels,p,dx}
    softmax_focal_ref_levels_b.npz

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_softmax_focal_golden.py
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/caffe2/"
F = np.float32

SHIM = r"""
#include <cfloat>
#include <cmath>
#include <cstddef>
#define __global__
struct Dim3 { unsigned x; };
static const Dim3 blockIdx = {0}, threadIdx = {0}, blockDim = {1}, gridDim = {1};   // <<<1, 1>>>
using std::exp; using std::log; using std::pow;          // the float overloads, as in device code
static inline float max(float a, float b) { return a < b ? b : a; }
static inline double max(float a, double b) { return (double)a < b ? b : (double)a; }
static inline double max(double a, double b) { return a < b ? b : a; }
"""

DRIVER = r"""
extern "C" {
void group_softmax(int N, int A, int H, int W, const float* X, float* P, int C) {
  GroupSpatialSoftmaxKernel(N, A, W, H, X, P, C);
}
void sum_probs(int N, int A, int H, int W, const float* Y, const float* dY, float* s, int C) {
  SumProbsKernel(N, A, W, H, Y, dY, s, C);
}
void sub_sum(int N, int A, int H, int W, const float* s, float* dX, int C) { SubSumKernel(N, A, W, H, s, dX, C); }
void focal_softmax(int N, int A, int H, int W, const float* X, float* P, int C) {
  SpatialSoftmaxKernel(N, A, H, W, X, P, C);
}
void focal_loss(int N, int A, int H, int W, const float* P, const int* T, float* losses, const float* wp,
                float gamma, float alpha, int C) {
  SoftmaxFocalLossKernel(N, A, H, W, P, T, losses, wp, gamma, alpha, C);
}
void focal_weight(int N, int A, int H, int W, const float* P, const int* T, float* buff, const float* wp,
                  float gamma, float alpha, int C) {
  SoftmaxFocalLossGradientWeightKernel(N, A, H, W, P, T, buff, wp, gamma, alpha, C);
}
void focal_grad(int N, int D, int H, int W, const float* P, const int* T, const float* buff, const float* dloss,
                float* dX, int C) {
  SoftmaxFocalLossGradientKernel(N, D, H, W, P, T, buff, dloss, dX, C);
}
}
"""


def global_functions(text):
    """Every `__global__ void f(...) {...}` definition of a .cu file, by brace matching."""
    out = []
    for m in re.finditer(r"__global__\s+void\s+\w+\s*\(", text):
        i = text.index("{", m.end())
        depth, j = 1, i + 1
        while depth:
            depth += {"{": 1, "}": -1}.get(text[j], 0)
            j += 1
        out.append(text[m.start():j])
    return out


def loop_macro():
    src = open(REF + "caffe2/core/common_gpu.h").read().split("\n")
    i = next(k for k, l in enumerate(src) if l.startswith("#define CUDA_1D_KERNEL_LOOP"))
    j = i
    while src[j].rstrip().endswith("\\"):
        j += 1
    return "\n".join(src[i:j + 1])


def build_reference(tmp):
    parts = [SHIM, loop_macro()]
    for name in ("group_spatial_softmax_op.cu", "softmax_focal_loss_op.cu"):
        fns = global_functions(open(REF + "modules/detectron/" + name).read())
        assert fns, name
        parts += fns
    parts.append(DRIVER)
    src = os.path.join(tmp, "ref_kernels.cc")
    with open(src, "w") as f:
        f.write("\n\n".join(parts))
    lib = os.path.join(tmp, "ref_kernels.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", lib])
    return C.CDLL(lib)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Reference(object):
    def __init__(self, lib):
        self.lib = lib

    def softmax(self, x, Cn, fn="focal_softmax"):
        N, D, H, W = x.shape
        p = np.zeros_like(x)
        getattr(self.lib, fn)(N, D // Cn, H, W, ptr(x), ptr(p), Cn)
        return p

    def focal(self, p, labels, fg, gamma, alpha, scale, dloss, Cn):
        N, D, H, W = p.shape
        A = D // Cn
        wp = np.array([fg], F)
        losses = np.zeros(labels.shape, F)
        self.lib.focal_loss(N, A, H, W, ptr(p), ptr(labels), ptr(losses), ptr(wp), C.c_float(gamma),
                            C.c_float(alpha), Cn)
        loss = F(F(losses.astype(np.float64).sum()) * F(scale))            # math::Sum, math::Scale (restated)
        buff = np.zeros(labels.shape, F)
        self.lib.focal_weight(N, A, H, W, ptr(p), ptr(labels), ptr(buff), ptr(wp), C.c_float(gamma),
                              C.c_float(alpha), Cn)
        dx = np.zeros_like(p)
        dl = np.array([dloss], F)
        self.lib.focal_grad(N, D, H, W, ptr(p), ptr(labels), ptr(buff), ptr(dl), ptr(dx), Cn)
        dx = (dx * F(scale)).astype(F)                                     # math::Scale (restated)
        return loss, dx

    def softmax_grad(self, y, dy, Cn):
        N, D, H, W = y.shape
        A = D // Cn
        s = np.zeros((N, A, H, W), F)
        dx = dy.copy()                                                     # Copy (restated)
        self.lib.sum_probs(N, A, H, W, ptr(y), ptr(dy), ptr(s), Cn)
        self.lib.sub_sum(N, A, H, W, ptr(s), ptr(dx), Cn)
        return (dx * y).astype(F)                                          # math::Mul (restated)


def f16_exact(a):
    return a.astype(np.float16).astype(F)


def prior_bias(A, Cn, pi=0.01):
    b = np.zeros((A, Cn), F)
    b[:, 0] = np.log((Cn - 1) * (1 - pi) / pi)
    return b.reshape(1, A * Cn, 1, 1)


def logits(rng, shape, kind):
    N, A, Cn, H, W = shape
    full = (N, A * Cn, H, W)
    if kind == "normal":                      # N(0, 1) + the head's prior bias
        x = rng.standard_normal(full).astype(F) + prior_bias(A, Cn)
    elif kind == "narrow":                    # spread of 8: no labelled p rounds to 1
        x = rng.uniform(-4.0, 4.0, full).astype(F)
    elif kind == "wide":                      # some labelled p underflow to 0: the FLT_MIN clamp
        x = rng.uniform(-60.0, 60.0, full).astype(F)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(f16_exact(x))


def labels(rng, shape, kind):
    N, A, Cn, H, W = shape
    n = N * A * H * W
    if kind == "ignore":
        return np.full((N, A, H, W), -1, np.int32)
    if kind == "background":
        return np.zeros((N, A, H, W), np.int32)
    t = np.zeros(n, np.int32)
    perm = rng.permutation(n)
    nfg = max(1, int(round(0.05 * n)))
    nig = max(1, int(round(0.05 * n))) if n > 2 else 0
    t[perm[:nfg]] = rng.integers(1, Cn, nfg)
    t[perm[0]] = Cn - 1                       # the last class is always present
    t[perm[nfg:nfg + nig]] = -1
    return t.reshape(N, A, H, W)


SHAPES = {"s1": (2, 9, 81, 5, 7), "s2": (1, 9, 81, 1, 1), "s3": (2, 3, 5, 13, 21), "s4": (1, 1, 2, 3, 3)}
# data set -> (shape, logits)
SETS = {"s1_normal": ("s1", "normal"), "s2_normal": ("s2", "normal"), "s2_wide": ("s2", "wide"),
        "s3_normal": ("s3", "normal"), "s3_narrow": ("s3", "narrow"), "s3_wide": ("s3", "wide"),
        "s4_normal": ("s4", "normal"), "s4_narrow": ("s4", "narrow")}
# (name, data set, labels, gamma, alpha, fg_num, scale)
CASES = [
    ("s1_mixed", "s1_normal", "mixed", 2.0, 0.25, 37.5, 0.125),
    ("s2_mixed", "s2_normal", "mixed", 2.0, 0.25, 1.0, 1.0),
    ("s2_mixed_g15", "s2_normal", "mixed", 1.5, 0.5, 0.0, 0.125),
    ("s2_wide", "s2_wide", "mixed", 1.0, 0.25, 37.5, 1.0),
    ("s2_ignore", "s2_normal", "ignore", 2.0, 0.25, 0.0, 1.0),
    ("s3_mixed", "s3_normal", "mixed", 2.0, 0.25, 37.5, 1.0),
    ("s3_mixed_g15", "s3_normal", "mixed", 1.5, 0.5, 1.0, 0.125),
    ("s3_ignore", "s3_normal", "ignore", 2.0, 0.25, 0.0, 1.0),
    ("s3_background", "s3_normal", "background", 1.0, 0.25, 0.0, 1.0),
    ("s3_narrow_g05", "s3_narrow", "mixed", 0.5, 0.25, 37.5, 1.0),
    ("s3_wide", "s3_wide", "mixed", 2.0, 0.25, 1.0, 0.125),
    ("s4_mixed", "s4_normal", "mixed", 1.0, 0.25, 1.0, 1.0),
    ("s4_background", "s4_normal", "background", 2.0, 0.25, 37.5, 0.125),
    ("s4_narrow_g05", "s4_narrow", "mixed", 0.5, 0.25, 0.0, 1.0),
]
LEVEL_MAPS = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
SG_SETS = ("s2_normal", "s3_normal", "s3_wide", "s4_normal")    # softmax gradient cases (81 classes; ragged tail; saturated)
DLOSS = 1.0        # the builder's loss gradient (utils/blob.py:166-172); one case uses another value


def labelled_p(p, t, Cn):
    N, D, H, W = p.shape
    pg = p.reshape(N, D // Cn, Cn, H, W)
    idx = np.clip(t, 0, Cn - 1)[:, :, None]
    return np.take_along_axis(pg, idx, axis=2)[:, :, 0][t >= 0]


def main():
    rng = np.random.default_rng(20260319)
    tmp = tempfile.mkdtemp(prefix="softmax_focal_ref_")
    try:
        ref = Reference(build_reference(tmp))
        out = {}
        data = {}
        for name, (shape_key, kind) in SETS.items():
            shape = SHAPES[shape_key]
            x = logits(rng, shape, kind)
            p = ref.softmax(x, shape[2])
            # GroupSpatialSoftmax and the loss's own softmax kernel are the same arithmetic
            assert np.array_equal(p, ref.softmax(x, shape[2], "group_softmax"))
            data[name] = (shape, x, p)
            out["x_" + name] = x.astype(np.float16)
            out["p_" + name] = p
            out["shape_" + name] = np.array(shape, np.int32)
        for k, (name, dset, lkind, gamma, alpha, fg, scale) in enumerate(CASES):
            shape, x, p = data[dset]
            t = labels(rng, shape, lkind)
            dloss = 0.75 if name == "s3_mixed_g15" else DLOSS
            loss, dx = ref.focal(p, t, fg, gamma, alpha, scale, dloss, shape[2])
            pl = labelled_p(p, t, shape[2])
            if gamma < 1.0:
                assert not np.any(pl == F(1.0)), name        # the reference computes inf * 0 there
            if dset.endswith("wide"):
                assert np.any(pl == 0.0), name               # the FLT_MIN clamp is exercised
            assert np.isfinite(loss) and np.isfinite(dx).all(), name
            out["case_%d_labels" % k] = t.astype(np.int8)
            out["case_%d_fg" % k] = np.array([fg], F)
            out["case_%d_params" % k] = np.array([gamma, alpha, scale, dloss], F)
            out["case_%d_loss" % k] = np.array([loss], F)
            out["case_%d_dx" % k] = dx
        out["case_names"] = np.array([c[0] for c in CASES])
        out["case_sets"] = np.array([c[1] for c in CASES])
        # softmax gradient on four of the probability sets
        for dset in SG_SETS:
            shape, x, p = data[dset]
            dy = f16_exact(rng.standard_normal(p.shape).astype(F))
            out["sg_%s_dy" % dset] = dy.astype(np.float16)
            out["sg_%s_dx" % dset] = ref.softmax_grad(p, dy, shape[2])
        out["sg_sets"] = np.array(SG_SETS)
        np.savez_compressed(os.path.join(HERE, "softmax_focal_ref.npz"), **out)

        # the five-level call: N = 2, A = 9, C = 81, one fg_num / gamma / alpha / scale for all levels
        a, b = {}, {}
        N, A, Cn = 2, 9, 81
        gamma, alpha, fg, scale = 2.0, 0.25, 37.5, 0.125
        a["lv_params"] = np.array([gamma, alpha, scale, DLOSS, fg], F)
        a["lv_maps"] = np.array(LEVEL_MAPS, np.int32)
        losses = []
        for l, (H, W) in enumerate(LEVEL_MAPS):
            shape = (N, A, Cn, H, W)
            x = logits(rng, shape, "normal")
            t = labels(rng, shape, "mixed")
            p = ref.softmax(x, Cn)
            loss, dx = ref.focal(p, t, fg, gamma, alpha, scale, DLOSS, Cn)
            losses.append(loss)
            a["lv_%d_labels" % l] = t.astype(np.int8)
            # level 0 is three quarters of the bytes: its x and p go to file a, its dx to file b
            a["lv_%d_x" % l] = x.astype(np.float16)
            (a if l == 0 else b)["lv_%d_p" % l] = p
            b["lv_%d_dx" % l] = dx
        a["lv_loss"] = np.array(losses, F)
        np.savez_compressed(os.path.join(HERE, "softmax_focal_ref_levels_a.npz"), **a)
        np.savez_compressed(os.path.join(HERE, "softmax_focal_ref_levels_b.npz"), **b)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for n in ("softmax_focal_ref.npz", "softmax_focal_ref_levels_a.npz", "softmax_focal_ref_levels_b.npz"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
