"""Conv / ConvGradient through the operator boundary for the default-engine tests (a plain helper module: no fixture,
no pytest setting): the argument spellings of ConvPoolOpBase, one run of an operator and its registered gradient, and
the comparison with the float64 definitions of default_engine_ref.py at the project's CONV_RTOL / CONV_FLOOR.

Run as a program it is the child process of test_conv1x1_engine_blas_switch: the process-wide switch
SSAD_CONV1X1_ENGINE is read once, so the cases that it reroutes need a process of their own.  It checks itself and
exits non-zero with the failing case's name."""
import os
import sys

if __name__ == "__main__":
    _here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(_here, "golden"), _here, os.path.dirname(_here)):
        if p not in sys.path:
            sys.path.insert(0, p)

import numpy as np

import ssad_amd  # noqa: E402,F401
from ssad_amd.caffe2_hip import caffe2_pb2, core, dyndep, workspace  # noqa: E402
import default_engine_ref as R  # noqa: E402
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, close  # noqa: E402

GPU = core.DeviceOption(caffe2_pb2.CUDA, 0)
SPELLINGS = ("single", "hw", "list")


def feed(name, arr):
    workspace.FeedBlob(name, arr, device_option=GPU)


def geo_args(g, spelling="auto", pool=False):
    """The operator arguments of a geometry.  single: kernel / stride / pad / dilation (needs equal axes);
    hw: kernel_h + kernel_w, stride_h + stride_w, pad_t .. pad_r, dilation_h + dilation_w; list: kernels, strides,
    pads, dilations; auto: single per argument where its axes are equal, hw otherwise."""
    (kh, kw), (sh, sw), pads, (dh, dw) = g["kernel"], g["stride"], g["pads"], g["dilation"]
    kw_ = {}

    def pair(single, h, w, plural, a, b):
        if spelling == "list":
            kw_[plural] = [a, b]
        elif spelling == "single" or (spelling == "auto" and a == b):
            assert a == b, "the single spelling needs equal axes"
            kw_[single] = a
        else:
            kw_[h], kw_[w] = a, b

    pair("kernel", "kernel_h", "kernel_w", "kernels", kh, kw)
    pair("stride", "stride_h", "stride_w", "strides", sh, sw)
    if not pool:
        pair("dilation", "dilation_h", "dilation_w", "dilations", dh, dw)
    if spelling == "list":
        kw_["pads"] = list(pads)
    elif spelling == "single" or (spelling == "auto" and len(set(pads)) == 1):
        assert len(set(pads)) == 1
        kw_["pad"] = pads[0]
    else:
        kw_["pad_t"], kw_["pad_l"], kw_["pad_b"], kw_["pad_r"] = pads
    if g["group"] != 1:
        kw_["group"] = g["group"]
    return kw_


def run_conv(g, X, Wt, b, dY, spelling="auto", want_dx=True, fuse_relu=False, **extra):
    """Conv [X, w, (b)] -> Y, then ConvGradient.  With the dX output the gradient is the registered one
    (GradientRegistry); without it the definition is written out, as a graph whose input needs no gradient has it.
    Returns {Y, dW, (db), (dX)} as numpy."""
    workspace.ResetWorkspace()
    feed("X", X); feed("w", Wt); feed("Y_grad", dY)
    ins = ["X", "w"]
    if b is not None:
        feed("b", b)
        ins.append("b")
    args = geo_args(g, spelling)
    if fuse_relu:
        args["fuse_relu"] = 1
    args.update(extra)
    with core.DeviceScope(GPU):
        conv = core.CreateOperator("Conv", ins, ["Y"], order="NCHW", **args)
    workspace.RunOperatorOnce(conv)
    out = {"Y": workspace.FetchBlob("Y")}
    gops, gin = core.GradientRegistry.GetGradientForOp(conv, ["Y_grad"])
    assert [o.type for o in gops] == ["ConvGradient"]
    names = list(gops[0].output)
    assert names == (["w_grad", "b_grad", "X_grad"] if b is not None else ["w_grad", "X_grad"]), names
    assert all(a.name != "fuse_relu" for a in gops[0].arg)
    if want_dx:
        workspace.RunOperatorsOnce(gops)
    else:
        gargs = dict(geo_args(g, spelling), **extra)
        if b is None:
            gargs["no_bias"] = 1
        with core.DeviceScope(GPU):
            grad = core.CreateOperator("ConvGradient", ["X", "w", "Y_grad"], names[:-1], order="NCHW", **gargs)
        workspace.RunOperatorOnce(grad)
        names = names[:-1]
    for blob, key in (("w_grad", "dW"), ("b_grad", "db"), ("X_grad", "dX")):
        if blob in names:
            out[key] = workspace.FetchBlob(blob)
    return out


def reference(g, X, Wt, b, dY, relu=False):
    """{Y, dW, db, dX} float64.  The gradient does not see fuse_relu: the caller passes the dY it wants."""
    Y = R.conv2d_f64(X, Wt, b, g)
    dW, db, dX = R.conv2d_grads_f64(X, Wt, dY, g)
    return {"Y": np.maximum(Y, 0) if relu else Y, "dW": dW, "db": db, "dX": dX}


def check(got, ref, what):
    for key, val in got.items():
        assert val.dtype == np.float32 and val.shape == ref[key].shape, (what, key, val.shape, ref[key].shape)
        close(val, ref[key], CONV_RTOL, CONV_FLOOR, "%s %s" % (what, key))


# the geometries SSAD_CONV1X1_ENGINE=blas moves from the pointwise / implicit GEMM kernels to im2col + the general GEMM
BLAS_CASES = [
    dict(name="pointwise", route="loop/loop", cin=24, cout=40, hw=(9, 13), N=2, geo=R.geometry(1)),
    dict(name="strided_pointwise", route="im2col/im2col", cin=16, cout=32, hw=(8, 16), N=2, geo=R.geometry(1, 2)),
    dict(name="k7s2", route="im2col/im2col", cin=3, cout=16, hw=(33, 47), N=2, geo=R.geometry(7, 2, 3)),
    dict(name="k3s2", route="im2col/im2col", cin=12, cout=20, hw=(11, 9), N=2, geo=R.geometry(3, 2, 1)),
    dict(name="k5", route="im2col/im2col", cin=6, cout=7, hw=(8, 8), N=2, geo=R.geometry(5, 1, 2)),
]


def main():
    import torch
    if os.environ.get("SSAD_CONV1X1_ENGINE") != "blas":
        print("SSAD_CONV1X1_ENGINE=blas is not set")
        return 2
    assert torch.cuda.is_available()
    dyndep.InitOpsLibrary()
    for case in BLAS_CASES:
        try:
            X, Wt, b, dY = R.conv_inputs(case)
            check(run_conv(case["geo"], X, Wt, b, dY), reference(case["geo"], X, Wt, b, dY), case["name"])
        except Exception as e:          # the parent reports the case by name
            print("FAILED %s: %s" % (case["name"], e))
            return 1
    print("ok %d" % len(BLAS_CASES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
