"""The grouped 3x3 layer's forward kernel and its two gradient kernels (csrc/kernels/grouped_conv3x3.hip,
grouped_conv3x3_grad.hip) beside the `Conv` / `ConvGradient` operators WITHOUT `hip_algo` -- the default engine, the
only route a gradient had through such a layer before.  Report only: no time is fixed anywhere.  Writes
profiles/grouped_grad.md and prints one JSON line.

Layers: the grouped 3x3 of every stage of X-101-64x4d (res2..res5, both strides where the network has them: res2 has
no stride-2 layer) and X-101-32x8d's res5, at batch 16 and 640 x 896 images.

Each layer is a process of its own (this file with --layer I) under its own `timeout`, and the steps are chained with
`&&`: after a layer that fails or hangs nothing more is started.  Inside a layer everything is timed in ONE process,
every timed call warmed, the alternatives taking turns:
  * the three kernels by device events around blocks of --reps launches (packs and workspace made beforehand);
  * the operators by the host clock around workspace.RunOperatorOnce and a device synchronise (device events cannot
    bracket the operator's own stream; operator construction is included): `Conv`, `ConvGradient` with the filter
    gradient as its only output, `ConvGradient` with both outputs.  The default engine has no separate data-gradient
    call, so its data gradient is (both) - (filter only).
Algorithmic bytes: forward x + y + w, data gradient dy + dx + w, filter gradient x + dy + dw, each once, fp32.

    python tools/grouped_grad_bench.py [--rounds 3] [--reps 5] [--warmup 1] [--out profiles/grouped_grad.md]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 16
HBM_STREAM = 6.3e12               # MI355X: achievable HBM streaming rate (float4 copy), bytes / s
PEAK_F32_MFMA = 157.3e12          # dense fp32 MFMA
# (label, C, group, input H, W, stride)
LAYERS = [("64x4d res2 (stride 1)", 256, 64, 160, 224, 1),
          ("64x4d res3.0 (stride 2)", 512, 64, 160, 224, 2), ("64x4d res3.1+ (stride 1)", 512, 64, 80, 112, 1),
          ("64x4d res4.0 (stride 2)", 1024, 64, 80, 112, 2), ("64x4d res4.1+ (stride 1)", 1024, 64, 40, 56, 1),
          ("64x4d res5.0 (stride 2)", 2048, 64, 40, 56, 2), ("64x4d res5.1+ (stride 1)", 2048, 64, 20, 28, 1),
          ("32x8d res5.0 (stride 2)", 2048, 32, 40, 56, 2), ("32x8d res5.1+ (stride 1)", 2048, 32, 20, 28, 1)]
LAYER_TIMEOUT = 240               # seconds per layer process


def summary(v):
    v = sorted(v)
    return dict(median=float(np.median(v)), min=v[0], max=v[-1])


def run_layer(index, args):
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    from ssad_amd.caffe2_hip import caffe2_pb2, core, dyndep, workspace
    if not torch.cuda.is_available():
        raise SystemExit("grouped_grad_bench needs a GPU: nothing is estimated without one")
    label, C, G, H, W, s = LAYERS[index]
    n, cg = args.batch, C // G
    oh, ow = (H - 1) // s + 1, (W - 1) // s + 1
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(4321 + index)
    x = torch.randn((n, C, H, W), device=dev, generator=gen)
    dy = torch.randn((n, C, oh, ow), device=dev, generator=gen)
    w = torch.randn((C, cg, 3, 3), device=dev, generator=gen) * float((9 * cg) ** -0.5)
    pf, pd = K.grouped_conv3x3_pack_filter(w, G), K.grouped_conv3x3_pack_filter_dgrad(w, G)
    y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
    ws_bytes = int(K.lib().ssad_grouped_conv3x3_wgrad_workspace_bytes(n, C, H, W, G, s))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    kern = dict(fwd=lambda: K.grouped_conv3x3_forward(x, None, None, group=G, stride=s, out=y, packed=pf),
                dgrad=lambda: K.grouped_conv3x3_dgrad(dy, None, G, s, (H, W), out=dx, packed=pd),
                wgrad=lambda: K.grouped_conv3x3_wgrad(x, dy, G, s, out=dw, workspace=ws))

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    dyndep.InitOpsLibrary()
    GPU = core.DeviceOption(caffe2_pb2.CUDA, 0)
    workspace.ResetWorkspace()
    for name, t in (("X", x), ("w", w), ("Y_grad", dy)):
        workspace.FeedBlob(name, t.cpu().numpy(), device_option=GPU)
    geo = dict(kernel=3, pad=1, stride=s, group=G, order="NCHW")
    with core.DeviceScope(GPU):
        ops = dict(fwd=core.CreateOperator("Conv", ["X", "w"], ["Y"], **geo),
                   wgrad=core.CreateOperator("ConvGradient", ["X", "w", "Y_grad"], ["w_grad"], no_bias=1, **geo),
                   both=core.CreateOperator("ConvGradient", ["X", "w", "Y_grad"], ["w_grad", "X_grad"], no_bias=1, **geo))

    def run_op(op):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        workspace.RunOperatorOnce(op)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        for fn in kern.values():
            fn()
        for op in ops.values():
            run_op(op)
    torch.cuda.synchronize()
    # both routes compute the same three tensors: largest difference as a fraction of the largest value
    agree = {}
    for key, mine, blob in (("fwd", y, "Y"), ("dgrad", dx, "X_grad"), ("wgrad", dw, "w_grad")):
        ref = torch.from_numpy(workspace.FetchBlob(blob)).to(dev)
        agree[key] = float((mine - ref).abs().max() / ref.abs().max())
        del ref
    tk, to = {k: [] for k in kern}, {k: [] for k in ops}
    for _ in range(args.rounds):
        for k, fn in kern.items():
            tk[k].append(timed(fn, args.reps))
        for k, op in ops.items():
            to[k].append(run_op(op))
    workspace.ResetWorkspace()
    fl = 4.0
    nbytes = dict(fwd=fl * (x.numel() + y.numel() + w.numel()), dgrad=fl * (dy.numel() + dx.numel() + w.numel()),
                  wgrad=fl * (x.numel() + dy.numel() + dw.numel()))
    flops = 2.0 * 9 * cg * C * n * oh * ow
    e = dict(layer=label, N=n, C=C, group=G, cg=cg, H=H, W=W, stride=s, OH=oh, OW=ow, workspace_bytes=ws_bytes,
             kernel_ms={k: summary(v) for k, v in tk.items()}, operator_ms={k: summary(v) for k, v in to.items()},
             max_abs_diff_vs_operator_of_scale=agree, bytes=nbytes, flops=flops)
    e["operator_ms"]["dgrad"] = summary([b - a for a, b in zip(to["wgrad"], to["both"])])
    e["speedup"] = {k: e["operator_ms"][k]["median"] / e["kernel_ms"][k]["median"] for k in kern}
    e["tb_per_s"] = {k: nbytes[k] / (e["kernel_ms"][k]["median"] * 1e-3) / 1e12 for k in kern}
    e["tflops"] = {k: flops / (e["kernel_ms"][k]["median"] * 1e-3) / 1e12 for k in kern}
    e["dgrad_over_fwd_time"] = e["kernel_ms"]["dgrad"]["median"] / e["kernel_ms"]["fwd"]["median"]
    with open(args.emit, "w") as f:
        json.dump(e, f)


def git_commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, universal_newlines=True).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed block of a kernel")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=N)
    ap.add_argument("--layer", type=int, default=None, help="(internal) time one layer and write --emit")
    ap.add_argument("--emit", default=None)
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse)")
    ap.add_argument("--test-file-seconds", type=float, default=None,
                    help="run time of tests/test_gpu_grouped_grad.py, recorded in the profile")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_grad.md"))
    args = ap.parse_args()
    if args.layer is not None:
        return run_layer(args.layer, args)
    tmp = tempfile.mkdtemp(prefix="grouped_grad_bench_")
    files = [os.path.join(tmp, "layer%d.json" % i) for i in range(len(LAYERS))]
    # one process per layer, each under its own time limit, chained with &&
    steps = ["timeout -k 10 %d %s %s --layer %d --emit %s --rounds %d --reps %d --warmup %d --batch %d" % (
        LAYER_TIMEOUT, sys.executable, os.path.abspath(__file__), i, f, args.rounds, args.reps, args.warmup, args.batch)
        for i, f in enumerate(files)]
    rc = subprocess.call(["bash", "-c", " && ".join(steps)])
    layers = [json.load(open(f)) for f in files if os.path.exists(f)]
    res = {"metric": "grouped_grad_bench", "batch": args.batch, "rounds": args.rounds, "reps_per_block": args.reps,
           "commit": args.commit or git_commit(), "exit_status_of_the_chain": rc, "layers": layers,
           "test_file_seconds": args.test_file_seconds}
    if layers:
        write_profile(res, args)
    print(json.dumps(res))
    return rc


def write_profile(res, args):
    f3 = lambda d: "%.3f (%.3f ... %.3f)" % (d["median"], d["min"], d["max"])
    L = ["# Grouped 3x3 convolution: the data and filter gradient kernels", "",
         "`python tools/grouped_grad_bench.py` on one MI355X, fp32, batch %d, 640 x 896 images, library built from commit "
         "`%s` plus the change that adds the kernels.  One process per layer; every timed call warmed (%d passes); the "
         "alternatives take turns, %d rounds; median (min ... max) over the rounds, ms.  These are figures of one run on "
         "one machine: the columns of a row are comparable with each other, not with a figure taken in another run."
         % (res["batch"], res["commit"], args.warmup, res["rounds"]), "",
         "`kernel`: `ssad_grouped_conv3x3_forward` / `_dgrad` / `_wgrad` (device events around blocks of %d launches; packs "
         "and workspace made beforehand).  `default engine`: the `Conv` / `ConvGradient` operators without `hip_algo` "
         "through `workspace.RunOperatorOnce` -- one im2col and one strided-batched GEMM per image, col2im for the data "
         "gradient -- by the host clock around the call and a device synchronise (operator construction included); its "
         "data gradient is `ConvGradient` with both outputs minus `ConvGradient` with the filter gradient alone." % args.reps,
         ""]
    if res["exit_status_of_the_chain"]:
        L += ["**The chain stopped early (exit status %d): the layers after the last row were not run.**"
              % res["exit_status_of_the_chain"], ""]
    for key, title in (("fwd", "Forward"), ("dgrad", "Data gradient"), ("wgrad", "Filter gradient")):
        L += ["## %s" % title, "",
              "| layer | C / groups | map | kernel ms | default engine ms | default / kernel | algorithmic TB/s | share of "
              "%.1f TB/s | TFLOP/s | share of fp32 MFMA peak |" % (HBM_STREAM / 1e12), "|---|---|---|---|---|---|---|---|---|---|"]
        for e in res["layers"]:
            L.append("| %s | %d / %d (cg %d) | %dx%d -> %dx%d | %s | %s | %.1f x | %.2f | %.0f %% | %.1f | %.0f %% |" % (
                e["layer"], e["C"], e["group"], e["cg"], e["H"], e["W"], e["OH"], e["OW"], f3(e["kernel_ms"][key]),
                f3(e["operator_ms"][key]), e["speedup"][key], e["tb_per_s"][key], 100 * e["tb_per_s"][key] * 1e12 / HBM_STREAM,
                e["tflops"][key], 100 * e["tflops"][key] * 1e12 / PEAK_F32_MFMA))
        L.append("")
    L += ["## Data gradient against the forward kernel", "",
          "At stride 1 the data gradient is the forward product on the transposed, tap-flipped filter; at stride 2 it "
          "multiplies each tap once per 2 x 2 pixels of the larger map (per-parity tap subsets), the same flops as the "
          "forward pass.", "", "| layer | data gradient / forward time |", "|---|---|"]
    L += ["| %s | %.2f |" % (e["layer"], e["dgrad_over_fwd_time"]) for e in res["layers"]]
    L += ["", "## Filter-gradient workspace and agreement with the default engine", "",
          "`ssad_grouped_conv3x3_wgrad_workspace_bytes` (the per-range partial sums) and, per tensor, the largest "
          "difference between the two routes as a fraction of the largest value, taken before timing.", "",
          "| layer | workspace bytes | Y | dX | dW |", "|---|---|---|---|---|"]
    for e in res["layers"]:
        a = e["max_abs_diff_vs_operator_of_scale"]
        L.append("| %s | %d | %.1e | %.1e | %.1e |" % (e["layer"], e["workspace_bytes"], a["fwd"], a["dgrad"], a["wgrad"]))
    if res.get("test_file_seconds") is not None:
        L += ["", "`tests/test_gpu_grouped_grad.py` ran in %.1f s on the same machine (pytest's own total)."
              % res["test_file_seconds"]]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    sys.exit(main() or 0)
