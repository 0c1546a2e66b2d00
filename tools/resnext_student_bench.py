"""A ResNeXt as the student of the native step (NativeResNetFPN(..., grouped_grad=True)), measured in ONE process on
one GPU.  Writes profiles/resnext_student.md and prints one JSON line.

 (a) the pack segment of X-101-64x4d's 30 trained grouped layers, same-call A/B: ONE ssad_grouped_conv3x3_pack_filters
     launch against the chain of 60 per-layer launches (ssad_grouped_conv3x3_pack_filter + _pack_filter_dgrad per
     layer).  Bits are compared first; then the two take turns, HIP events around each block of repetitions.  Both are
     called the same way (ctypes, from this script), so a figure is enqueue + execution of the whole sequence on an
     otherwise idle stream -- what the head of a step pays.  GATE: the one-launch record stays only if it is not slower.
 (b) backbone pack + forward + backward + SGD at batch 16, 640 x 896 for x101-64x4d, x101-32x8d and r101 (taking turns),
     and the per-class event times of instrumented steps.  Report only: the parent refuses the configuration.
 (c) the whole NativeDistillModel step with an x101-64x4d student: teacher-less, and under an x101-32x8d teacher.
     Report only.

    python tools/resnext_student_bench.py [--batch 16] [--steps 5] [--rounds 4] [--warmup 2] [--only abc]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGE_HW = (640, 896)
TESTS_HEADING = "## Gradient errors against float64"      # kept from the file on disk: written from the tests' output


def blocks_of(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 4), min=round(v[0], 4), max=round(v[-1], 4))


def pack_ab(args, dev):
    """(a) -> dict"""
    import torch
    from ssad_amd import kernels as K
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    L = K.lib()
    nat = NativeResNetFPN("x101-64x4d", 1, (128, 128), dev, train=True, grouped_grad=True)
    layers = [l for l in nat._layers.values() if l.group > 1 and l.train]
    assert len(layers) == 30
    outs = {tag: [(torch.empty_like(l.pf), torch.empty_like(l.pd)) for l in layers] for tag in ("one", "chain")}
    tab = (K.GroupedPackEntry * len(layers))()
    for k, (l, (pf, pd)) in enumerate(zip(layers, outs["one"])):
        tab[k] = K.GroupedPackEntry(l.w.data_ptr(), pf.data_ptr(), pd.data_ptr(), l.cout, l.group)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    chain_args = [(C.c_void_p(l.w.data_ptr()), l.cout, l.group, C.c_void_p(pf.data_ptr()), C.c_void_p(pd.data_ptr()))
                  for l, (pf, pd) in zip(layers, outs["chain"])]

    def one():
        rc = L.ssad_grouped_conv3x3_pack_filters(tab, len(layers), st)
        assert rc == 0, rc

    def chain():
        for w, Cc, G, pf, pd in chain_args:
            rc = L.ssad_grouped_conv3x3_pack_filter(w, Cc, G, pf, st) or L.ssad_grouped_conv3x3_pack_filter_dgrad(w, Cc, G, pd, st)
            assert rc == 0, rc

    one()
    chain()
    torch.cuda.synchronize()
    for (a, b), (c, d) in zip(outs["one"], outs["chain"]):
        if not (torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(b.view(torch.int32), d.view(torch.int32))):
            raise SystemExit("pack A/B: the one-launch packs differ from the per-layer launchers' bits")
    for _ in range(args.pack_warmup):
        one()
        chain()
    torch.cuda.synchronize()
    t = {"one": [], "chain": []}
    for _ in range(args.pack_rounds):
        t["one"].append(1e3 * blocks_of(one, args.pack_reps))
        t["chain"].append(1e3 * blocks_of(chain, args.pack_reps))
    moved = 4.0 * sum(l.w.numel() + l.pf.numel() + l.pd.numel() for l in layers)
    return dict(layers=len(layers), bits_equal=True, bytes=moved, reps=args.pack_reps, rounds=args.pack_rounds,
                one_launch_us=stats(t["one"]), chain_us=stats(t["chain"]))


def backbones(args, dev, images):
    """(b) -> dict arch -> figures"""
    import torch
    from ssad_amd import program as PR
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    archs = ("x101-64x4d", "x101-32x8d", "r101")
    # random gradients on random weights train nothing: a rate small enough that ~15 such updates leave the
    # activations where they were (at 1e-5 the |max| of res5 grows by 5 % a step and the run ends non-finite)
    nets = {a: NativeResNetFPN(a, args.batch, IMAGE_HW, dev, train=True, grouped_grad=True, lr=1e-9) for a in archs}
    gen = torch.Generator(device=dev).manual_seed(77)
    for nat in nets.values():
        for d in nat.d_fpn:
            d.copy_(torch.randn(d.shape, device=dev, generator=gen) * 1e-3)

    def step(nat):
        nat.pack()
        nat.forward(images)
        nat.backward()
        nat.sgd_step()

    for nat in nets.values():
        for _ in range(args.warmup):
            step(nat)
    torch.cuda.synchronize()
    blocks = {a: [] for a in archs}
    for _ in range(args.rounds):
        for a in archs:
            blocks[a].append(blocks_of(lambda: step(nets[a]), args.steps))
    out = {}
    for a in archs:
        nat = nets[a]
        t = PR.Timing()
        nat.timing = t
        for _ in range(args.profile_steps):
            step(nat)
        torch.cuda.synchronize()
        nat.timing = None
        cls = {k: round(v["ms"] / args.profile_steps, 3) for k, v in t.collect().items()}
        assert bool(torch.isfinite(nat.params_flat).all()) and bool(torch.isfinite(nat.grads_flat).all()), a
        out[a] = dict(ms_per_step=stats(blocks[a]), classes_ms_per_step=cls,
                      trained_parameters=int(nat.params_flat.numel()), launches=len(nat.prog.ops))
    return out


def model_steps(args, dev, images):
    """(c) -> dict"""
    import torch
    from ssad_amd import synth
    from ssad_amd.backbone_pipeline import NativeDistillModel
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    shapes, n = synth.LEVEL_SHAPES_600, args.batch
    gen = torch.Generator(device=dev).manual_seed(1234)
    labels = []
    for h, w in shapes:                       # bench.py's synthetic labels: 5 % ignored, 2 % foreground
        u = torch.rand((n, 9, h, w), device=dev, generator=gen)
        lab = torch.zeros((n, 9, h, w), dtype=torch.int32, device=dev)
        lab[u < 0.05] = -1
        fg = (u >= 0.05) & (u < 0.07)
        lab[fg] = torch.randint(1, 81, (int(fg.sum()),), device=dev, generator=gen, dtype=torch.int32)
        labels.append(lab)
    targets, n_fg = [], 0
    for lab in labels:
        idx = torch.nonzero(lab > 0)
        Lc = torch.stack([idx[:, 0], 4 * idx[:, 1], idx[:, 2], idx[:, 3]], dim=1).float().contiguous()
        targets.append(((torch.randn((Lc.shape[0], 4), device=dev, generator=gen) * 0.5).contiguous(), Lc))
        n_fg += Lc.shape[0]
    fg_num = torch.tensor([float(max(n_fg, 1))], device=dev)
    models = {}
    for name, teacher in (("teacherless", None), ("x101-32x8d teacher", "x101-32x8d")):
        kw = dict(teacher_init=synth.head_params(np.random.default_rng(2))) if teacher else dict(distill=False)
        heads = DistillHeads(HeadConfig(num_gpus=1), N=n, shapes=shapes, device=dev, lr=1e-6,
                             student_init=synth.head_params(np.random.default_rng(1)), **kw)
        models[name] = NativeDistillModel(heads, "x101-64x4d", teacher, N=n, image_hw=IMAGE_HW, device=dev,
                                          student_grouped_grad=True)
    for m in models.values():
        for _ in range(args.warmup):
            m.step(images, labels, targets, fg_num)
    torch.cuda.synchronize()
    blocks = {k: [] for k in models}
    for _ in range(args.rounds):
        for k, m in models.items():
            blocks[k].append(blocks_of(lambda: m.step(images, labels, targets, fg_num), args.steps))
    for k, m in models.items():
        assert bool(torch.isfinite(m.heads.losses).all()) and bool(torch.isfinite(m.student.params_flat).all()), k
    return {k: dict(ms_per_step=stats(v)) for k, v in blocks.items()}


def report(args, res):
    from ssad_amd import program as PR
    lines = ["# A ResNeXt student in the native step", "",
             "`python tools/resnext_student_bench.py` on one MI355X, one process, fp32.  Figures of one run on one "
             "machine: rows of one table were taken in the same process, taking turns, and compare with each other; "
             "they do not compare with a figure of another run or machine (bench.py's headline, say).  median "
             "(min ... max) over the blocks."]
    a = res.get("pack")
    if a:
        one, ch = a["one_launch_us"], a["chain_us"]
        verdict = ("The one-launch record is not slower: it stays."
                   if one["median"] <= ch["median"] else
                   "The one-launch record LOST this A/B: the step program should emit per-layer records instead.")
        lines += ["", "## (a) The pack segment: one launch against 60", "",
                  "X-101-64x4d's %d trained grouped layers, both packs of each (%.1f MB read + written).  Bits compared "
                  "first: equal.  Then %d rounds of %d repetitions each, the two sequences taking turns after %d warm-up "
                  "repetitions, HIP events around each block; both are called through ctypes from the script, so a "
                  "figure is enqueue + execution of the whole sequence on an otherwise idle stream."
                  % (a["layers"], a["bytes"] / 1e6, a["rounds"], a["reps"], args.pack_warmup), "",
                  "| pack segment | launches | us per segment | min ... max |", "|---|---|---|---|",
                  "| `ssad_grouped_conv3x3_pack_filters` (GROUPED_PACKS) | 1 | %.1f | %.1f ... %.1f |" % (one["median"], one["min"], one["max"]),
                  "| per-layer `_pack_filter` + `_pack_filter_dgrad` | %d | %.1f | %.1f ... %.1f |" % (2 * a["layers"], ch["median"], ch["min"], ch["max"]),
                  "", "%s  (%.1fx)" % (verdict, ch["median"] / max(one["median"], 1e-9))]
    b = res.get("backbones")
    if b:
        archs = list(b)
        lines += ["", "## (b) Backbone pack + forward + backward + SGD", "",
                  "Batch %d, %d x %d, random initialisation, the three networks in one process taking turns: %d rounds of "
                  "%d steps, %d warm-up steps each.  No parent figure exists for the two ResNeXts (the parent refuses "
                  "`train=True` on them); r101 is the plain network of the same depth, next to them for scale.  Report only."
                  % (args.batch, IMAGE_HW[0], IMAGE_HW[1], args.rounds, args.steps, args.warmup), "",
                  "| student backbone | trained parameters | launch records | ms / step | min ... max |", "|---|---|---|---|---|"]
        for k in archs:
            e = b[k]
            lines.append("| %s | %.1f M | %d | %.2f | %.2f ... %.2f |" % (
                k, e["trained_parameters"] / 1e6, e["launches"], e["ms_per_step"]["median"], e["ms_per_step"]["min"],
                e["ms_per_step"]["max"]))
        lines += ["", "Per kernel class, from %d instrumented steps per network after the timed blocks (`program.Timing`: "
                  "events around every launch, so launches that overlap in the timed step run one after the other here and "
                  "a column does not add up to the step time above).  ms per step; classes below 0.05 ms everywhere are "
                  "left out." % args.profile_steps, "",
                  "| class | kernel family | %s |" % " | ".join(archs), "|---|---|%s" % ("---|" * len(archs))]
        keys = sorted(set(k for a_ in archs for k in b[a_]["classes_ms_per_step"]))
        for k in keys:
            row = [b[a_]["classes_ms_per_step"].get(k, 0.0) for a_ in archs]
            if max(row) < 0.05:
                continue
            lines.append("| %d | %s | %s |" % (k, PR.KLASS.get(k, dict(name="class %d" % k))["name"],
                                              " | ".join("%.2f" % v for v in row)))
        lines.append("| | sum of all classes | %s |" % " | ".join(
            "%.2f" % sum(b[a_]["classes_ms_per_step"].values()) for a_ in archs))
    c = res.get("model")
    if c:
        lines += ["", "## (c) The whole step with an x101-64x4d student", "",
                  "`NativeDistillModel(..., student_grouped_grad=True)`, batch %d, %d x %d, synthetic labels as in bench.py, "
                  "the two models in one process taking turns (%d rounds of %d steps, %d warm-up steps).  Report only."
                  % (args.batch, IMAGE_HW[0], IMAGE_HW[1], args.rounds, args.steps, args.warmup), "",
                  "| model | ms / step | min ... max |", "|---|---|---|"]
        for k, e in c.items():
            lines.append("| x101-64x4d student, %s | %.2f | %.2f ... %.2f |" % (
                k, e["ms_per_step"]["median"], e["ms_per_step"]["min"], e["ms_per_step"]["max"]))
    # the tests' section is not measured here: taken over from the file being replaced, else from the committed profile
    kept = []
    for path in (args.out, os.path.join(ROOT, "profiles", "resnext_student.md")):
        if kept or not os.path.exists(path):
            continue
        old = open(path).read().split("\n")
        at = [k for k, l in enumerate(old) if l.startswith(TESTS_HEADING)]
        if at:
            kept = [""] + old[at[0]:]
            while kept and not kept[-1]:
                kept.pop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + kept) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=1)
    ap.add_argument("--pack-reps", type=int, default=50)
    ap.add_argument("--pack-rounds", type=int, default=10)
    ap.add_argument("--pack-warmup", type=int, default=20)
    ap.add_argument("--only", default="abc", help="which parts to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnext_student.md"))
    args = ap.parse_args()
    import torch
    import ssad_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("resnext_student_bench needs a GPU: nothing is estimated without one")
    dev = torch.device("cuda", 0)
    res = {"metric": "resnext_student", "batch": args.batch, "image_hw": list(IMAGE_HW)}
    if "a" in args.only:
        res["pack"] = pack_ab(args, dev)
        torch.cuda.empty_cache()
    images = torch.randn((args.batch, 3) + IMAGE_HW, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    if "b" in args.only:
        res["backbones"] = backbones(args, dev, images)
        torch.cuda.empty_cache()
    if "c" in args.only:
        res["model"] = model_steps(args, dev, images)
    report(args, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
