"""Bit fixture of the convolution operators: tests/golden/conv_operator_bits.json.

Drives Conv / ConvGradient / ConvGroup / ConvGradientGroup through core.CreateOperator, workspace.RunOperatorOnce and
FetchBlob and records the sha256 of the raw words of every output blob, per case, plus the `filter_packs` and
`conv_launch_calls` counts of a created Conv and ConvGradient run twice.  Every case runs twice, each time in a fresh
workspace; an output whose two runs differ is recorded as "unstable" (tests/test_gpu_conv_operator_bits.py then holds
it to the oracle instead of to the hash).

Run on an MI355X from the repository root, at the commit whose bits are to be pinned:

    python tests/golden/make_conv_operator_bits.py

The file names that commit.  The cases and the code that runs them are shared with the test, which imports this module.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "conv_operator_bits.json")

N, HW, HW_SMALL = 2, (9, 13), (5, 7)          # 9x13 is a tile multiple of neither Winograd engine


def pair(name, C, M, **kw):
    """Conv + ConvGradient (dX; relu_grad_on_input 0 and 1 where the engine has it)"""
    d = dict(name=name, kind="pair", C=C, M=M, algo=None, no_bias=False, kernel=3, stride=1, pad=1, group=1,
             dtype="float32", hw=HW, relu_grad=True)
    d.update(kw)
    return d


CASES = [
    pair("auto_16_24", 16, 24),
    pair("auto_32_40", 32, 40),
    pair("direct_32_40", 32, 40, algo="direct"),
    pair("winograd_32_40", 32, 40, algo="winograd"),
    pair("winograd24_128_128", 128, 128, algo="winograd24"),
    pair("split_256_256", 256, 256, algo="split"),
    pair("split_64_128", 64, 128, algo="split"),
    pair("split_48_128", 48, 128, algo="split"),
    pair("split_128_36_no_bias", 128, 36, algo="split", no_bias=True),
    dict(name="split_256_256_fuse_relu", kind="fwd", C=256, M=256, algo="split", fuse="fuse_relu"),
    dict(name="split_256_256_fuse_sigmoid", kind="fwd", C=256, M=256, algo="split", fuse="fuse_sigmoid"),
    dict(name="group_split", kind="group", algo="split"),
    pair("grouped_g32_cg4_s1", 128, 128, algo="grouped", group=32),
    pair("grouped_g32_cg4_s2", 128, 128, algo="grouped", group=32, stride=2),
    pair("f16_3x3_16_24", 16, 24, dtype="float16", relu_grad=False),
    pair("f16_3x3_16_36", 16, 36, dtype="float16", relu_grad=False),
    pair("f16_1x1_s1_16_24", 16, 24, dtype="float16", relu_grad=False, kernel=1, pad=0),
    pair("f16_1x1_s2_16_24", 16, 24, dtype="float16", relu_grad=False, kernel=1, pad=0, stride=2),
    # the default engine: the geometries of test_default_engine_conv_and_gradient (tests/test_gpu_operators.py) -- the
    # gradient's per-image loop (k1s1: 117 pixels a map) and its batched route (the rest) --, a pointwise layer whose
    # gradient takes the GEMM route (128 pixels), and one of test_default_engine_grouped_conv_and_gradient
    pair("default_k1s1", 24, 40, kernel=1, pad=0, relu_grad=False),
    pair("default_k1s1_gemm", 24, 40, kernel=1, pad=0, hw=(8, 16), relu_grad=False),
    pair("default_k1s2", 16, 32, kernel=1, pad=0, stride=2, hw=(10, 14), relu_grad=False),
    pair("default_k7s2", 3, 16, kernel=7, pad=3, stride=2, hw=(33, 47), relu_grad=False),
    pair("default_k3s2", 12, 20, kernel=3, pad=1, stride=2, hw=(11, 9), relu_grad=False),
    pair("default_k5s1", 6, 7, kernel=5, pad=2, hw=(8, 8), relu_grad=False),
    pair("default_k3s1_g4", 16, 24, group=4, hw=(9, 12), relu_grad=False),
]
COUNTER_CASE = "split_256_256"


def seed_of(name):
    return int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)


def sha_words(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def out_size(n, k, st, pad):
    return (n + 2 * pad - k) // st + 1


def pair_inputs(c):
    rng = np.random.default_rng(seed_of(c["name"]))
    H, W = c["hw"]
    k, st, pd = c["kernel"], c["stride"], c["pad"]
    dt = np.dtype(c["dtype"])
    X = rng.standard_normal((N, c["C"], H, W)).astype(dt)
    cin = c["C"] // c["group"]
    Wt = (rng.standard_normal((c["M"], cin, k, k)) / np.sqrt(cin * k * k)).astype(dt)
    b = rng.standard_normal(c["M"]).astype(dt)
    dY = rng.standard_normal((N, c["M"], out_size(H, k, st, pd), out_size(W, k, st, pd))).astype(dt)
    return dict(X=X, w=Wt, b=b, dY=dY)


def group_inputs(c):
    """three problems: two maps of one 256 -> 256 filter and one 256 -> 36 problem"""
    rng = np.random.default_rng(seed_of(c["name"]))
    maps, filt = [HW, HW_SMALL, HW], [0, 0, 1]
    out = {}
    for f, M in enumerate((256, 36)):
        out["w%d" % f] = (rng.standard_normal((M, 256, 3, 3)) / 48.0).astype(np.float32)
        out["b%d" % f] = rng.standard_normal(M).astype(np.float32)
    for i, (hw, f) in enumerate(zip(maps, filt)):
        out["X%d" % i] = rng.standard_normal((N, 256) + hw).astype(np.float32)
        out["dY%d" % i] = rng.standard_normal((N, out["w%d" % f].shape[0]) + hw).astype(np.float32)
    return out, filt


def _api():
    import ssad_amd  # noqa: F401
    from ssad_amd.caffe2_hip import caffe2_pb2, core, dyndep, workspace
    dyndep.InitOpsLibrary()
    return core, workspace, core.DeviceOption(caffe2_pb2.CUDA, 0)


def conv_args(c):
    kw = dict(kernel=c["kernel"], pad=c["pad"], stride=c["stride"], order="NCHW")
    if c["group"] != 1:
        kw["group"] = c["group"]
    if c["algo"]:
        kw["hip_algo"] = c["algo"]
    return kw


def run_pair(c):
    core, workspace, GPU = _api()
    workspace.ResetWorkspace()
    for k, v in pair_inputs(c).items():
        workspace.FeedBlob(k, v, device_option=GPU)
    kw = conv_args(c)
    fwd_in = ["X", "w"] if c["no_bias"] else ["X", "w", "b"]
    with core.DeviceScope(GPU):
        ops = [core.CreateOperator("Conv", fwd_in, ["Y"], **kw)]
        for r in ((0, 1) if c["relu_grad"] else (0,)):
            t = "_relu" if r else ""
            outs = ["dW" + t] + ([] if c["no_bias"] else ["db" + t]) + ["dX" + t]
            gkw = dict(kw, relu_grad_on_input=1) if r else dict(kw)
            if c["no_bias"]:
                gkw["no_bias"] = 1
            ops.append(core.CreateOperator("ConvGradient", ["X", "w", "dY"], outs, **gkw))
    workspace.RunOperatorsOnce(ops)
    names = [o for op in ops for o in op.output]
    got = {n: workspace.FetchBlob(n) for n in names}
    workspace.ResetWorkspace()
    return got


def run_fwd(c):
    core, workspace, GPU = _api()
    workspace.ResetWorkspace()
    p = pair(c["name"], c["C"], c["M"], algo=c["algo"])
    for k, v in pair_inputs(p).items():
        workspace.FeedBlob(k, v, device_option=GPU)
    with core.DeviceScope(GPU):
        op = core.CreateOperator("Conv", ["X", "w", "b"], ["Y"], **dict(conv_args(p), **{c["fuse"]: 1}))
    workspace.RunOperatorOnce(op)
    got = {"Y": workspace.FetchBlob("Y")}
    workspace.ResetWorkspace()
    return got


def run_group(c):
    core, workspace, GPU = _api()
    workspace.ResetWorkspace()
    blobs, filt = group_inputs(c)
    for k, v in blobs.items():
        workspace.FeedBlob(k, v, device_option=GPU)
    k = len(filt)
    kw = dict(kernel=3, pad=1, stride=1, order="NCHW", hip_algo=c["algo"])
    fin = [n for i, f in enumerate(filt) for n in ("X%d" % i, "w%d" % f, "b%d" % f)]
    gin = [n for i, f in enumerate(filt) for n in ("X%d" % i, "w%d" % f, "dY%d" % i)]
    with core.DeviceScope(GPU):
        ops = [core.CreateOperator("ConvGroup", fin, ["Y%d" % i for i in range(k)], **kw)]
        for r in (0, 1):
            t = "_relu" if r else ""
            outs = (["dW%d%s" % (f, t) for f in range(2)] + ["db%d%s" % (f, t) for f in range(2)] +
                    ["dX%d%s" % (i, t) for i in range(k)])
            ops.append(core.CreateOperator("ConvGradientGroup", gin, outs, filter_index=filt, n_filters=2,
                                           relu_grad_on_input=r, **kw))
    workspace.RunOperatorsOnce(ops)
    got = {n: workspace.FetchBlob(n) for op in ops for n in op.output}
    workspace.ResetWorkspace()
    return got


RUNNERS = {"pair": run_pair, "fwd": run_fwd, "group": run_group}


def run_case(c):
    return RUNNERS[c["kind"]](c)


def run_counters():
    """A created Conv and a created ConvGradient (nets as written, no lowering) of COUNTER_CASE, each run twice:
    what `filter_packs` and `conv_launch_calls` rise by per run."""
    core, workspace, GPU = _api()
    workspace.ResetWorkspace()
    c = next(x for x in CASES if x["name"] == COUNTER_CASE)
    for k, v in pair_inputs(c).items():
        workspace.FeedBlob(k, v, device_option=GPU)
    kw = conv_args(c)
    rises = {}
    for op_type, ins, outs in (("Conv", ["X", "w", "b"], ["Y"]), ("ConvGradient", ["X", "w", "dY"], ["dW", "db", "dX"])):
        net = core.Net("conv_operator_bits_" + op_type)
        with core.DeviceScope(GPU):
            getattr(net, op_type)(ins, outs, **kw)
        net.Proto().arg = list(net.Proto().arg) + [core.MakeArgument("hip_lowering", 0)]
        workspace.CreateNet(net, overwrite=True)
        runs = []
        for _ in range(2):
            p0, l0 = workspace.Counter("filter_packs"), workspace.Counter("conv_launch_calls")
            workspace.RunNet(net)
            runs.append({"filter_packs": workspace.Counter("filter_packs") - p0,
                         "conv_launch_calls": workspace.Counter("conv_launch_calls") - l0})
        rises[op_type] = runs
        workspace.DeleteNet(net)
    workspace.ResetWorkspace()
    return rises


def reference(c, name):
    """float64 torch reference of output `name` of a pair / fwd case, for outputs recorded as "unstable" """
    import torch
    p = c if c["kind"] == "pair" else pair(c["name"], c["C"], c["M"], algo=c["algo"])
    v = pair_inputs(p)
    x, w, b = (torch.tensor(v[k].astype(np.float64), requires_grad=True) for k in ("X", "w", "b"))
    y = torch.nn.functional.conv2d(x, w, None if p["no_bias"] else b, p["stride"], p["pad"], 1, p["group"])
    if name == "Y":
        y = y.detach()
        fuse = c.get("fuse")
        return (torch.relu(y) if fuse == "fuse_relu" else torch.sigmoid(y) if fuse == "fuse_sigmoid" else y).numpy()
    y.backward(torch.tensor(v["dY"].astype(np.float64)))
    base = name.replace("_relu", "")
    g = {"dW": w.grad, "db": b.grad, "dX": x.grad}[base].numpy()
    return np.where(v["X"] > 0, g, 0.0) if (name.endswith("_relu") and base == "dX") else g


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
    out = {"commit": commit, "N": N, "sha256": {}, "maps": {}, "counters": run_counters()}
    unstable = []
    for c in CASES:
        a, b = run_case(c), run_case(c)
        rec = {}
        for n in a:
            same = a[n].dtype == b[n].dtype and a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes()
            rec[n] = sha_words(a[n]) if same else "unstable"
            if not same:
                unstable.append(c["name"] + "/" + n)
        out["sha256"][c["name"]] = rec
        out["maps"][c["name"]] = list(c["hw"]) if "hw" in c else [list(HW), list(HW_SMALL), list(HW)]
        print(c["name"], len(rec), "outputs", flush=True)
    out["unstable"] = unstable
    dst = args.out
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst, "unstable:", unstable)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
