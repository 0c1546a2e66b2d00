"""Bit fixture of the fp32 3x3 launchers under ssad_amd.kernels: tests/golden/wino_launch_bits.json.

The Winograd F(2x2) and F(2x4) engines on a level table that takes every branch of their pass planner (8 x 16
patches, sub-patch pairs with an absent partner, an empty level, ragged pairs), the F(2x2) engine's split tail where
it replaces the launch and where it follows a full round, and the table form of the three pack launchers -- sha256 of
the raw words of every output.  A split tail sums its partial results in unit order, another order than the unsplit
kernel's, so its hashes pin the launcher's decision as well as the arithmetic.

Run on an MI355X from the repository root, at the commit whose bits are to be pinned:

    python tests/golden/make_wino_launch_bits.py

Every case runs twice, each time in a fresh process; two runs that differ stop the generator (no case is recorded as
unstable).  The file names the commit.  The cases and the code that runs them are shared with the test, which imports
this module.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "wino_launch_bits.json")

MIXED = [(1, 8, 16), (3, 8, 8), (1, 0, 0), (2, 5, 7)]     # patches, pairs with an absent partner, empty, ragged pairs
# an empty tensor has no address, and the masked forms need one per level: there the table goes without its empty level
# (MASKED_REFUSALS pins that the whole table is refused)
NONEMPTY = [s for s in MIXED if s[1] * s[2]]
CHANNELS = [(36, 20), (136, 20)]              # NHALF; two channel blocks; both with a channel-tail chunk


def _engine_cases():
    out = []
    for engine, routes, forms in (("wino", ("levels", "multi"), ("bias_relu", "masked")),
                                  ("wino24", ("levels",), ("bias_relu", "masked", "accum"))):
        for route in routes:
            for cout, cin in CHANNELS:
                for form in forms:
                    out.append(dict(name="%s_%s_%d_%d_%s" % (engine, route, cout, cin, form), kind="engine", engine=engine,
                                    route=route, Cout=cout, Cin=cin, form=form))
    return out


def _tail(name, shape, setting, flag):
    return dict(name=name, kind="tail", shape=shape, Cout=136, Cin=64, setting=setting, flag=flag)


CASES = _engine_cases() + [
    _tail("tail_replaces_launch_1x8x8", (1, 8, 8), 1, False),            # 2 items, no full round
    _tail("tail_behind_round_setting2_1x128x136", (1, 128, 136), 2, False),   # 272 items: a round of 256 + 16
    _tail("tail_behind_round_flag_1x128x136", (1, 128, 136), 1, True),
    _tail("tail_off_1x128x136", (1, 128, 136), 0, False),
] + [dict(name="pack_" + e, kind="pack", engine=e) for e in ("wino", "wino24", "split")]
MASKED_REFUSALS = [("wino", "levels"), ("wino", "multi"), ("wino24", "levels")]


def seed_of(name):
    return int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)


def sha_words(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _api():
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    return torch, K


def _filter(rng, cout, cin):
    return (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)


def _maps(rng, shapes, c):
    return [rng.standard_normal((n, c, h, w)).astype(np.float32) for n, h, w in shapes]


PACKERS = {"wino": "conv_wino_pack_filter", "wino24": "conv_wino24_pack_filter"}


def run_engine(c, shapes=None):
    torch, K = _api()
    dev = lambda a: torch.from_numpy(a).cuda()
    rng = np.random.default_rng(seed_of(c["name"]))
    cout, cin, masked = c["Cout"], c["Cin"], c["form"] != "bias_relu"
    if shapes is None:
        shapes = NONEMPTY if masked else MIXED
    # two filters: `multi` gives the first two levels one and the rest the other; `levels` uses the first only
    ws = [dev(_filter(rng, cout, cin)) for _ in range(2)]
    bs = [dev(rng.standard_normal(cout).astype(np.float32)) for _ in range(2)]
    # forward: x has Cin channels, y Cout; masked (data gradient): dy has Cout channels, dx and the mask Cin
    xs = [dev(a) for a in _maps(rng, shapes, cout if masked else cin)]
    n_out = cin if masked else cout
    masks = [dev(a) for a in _maps(rng, shapes, n_out)] if masked else None
    outs = [dev(a) for a in _maps(rng, shapes, n_out)]        # what `accum` adds to; overwritten otherwise
    pack = getattr(K, PACKERS[c["engine"]])
    packs = [pack(w, want_dgrad=True)[1 if masked else 0] for w in ws]
    kw = dict(relu=not masked)
    if c["engine"] == "wino24":
        K.conv3x3_forward_wino24(xs, packs[0], None if masked else bs[0], n_out, out=outs, mask_by=masks,
                                 accumulate=c["form"] == "accum", **kw)
    elif c["route"] == "levels":
        K.conv3x3_forward(xs, packs[0], None if masked else bs[0], n_out, out=outs, mask_by=masks, wino=True, **kw)
    else:
        cut = [slice(0, 2), slice(2, None)]
        K.conv3x3_forward_multi([dict(xs=xs[s], packed=packs[i], bias=None if masked else bs[i], out=outs[s],
                                      mask_by=masks[s] if masked else None) for i, s in enumerate(cut)],
                                n_out, wino=True, **kw)
    torch.cuda.synchronize()
    return {"y%d" % i: y.cpu().numpy() for i, y in enumerate(outs)}


def masked_table_is_refused(engine, route):
    """the masked form of the whole MIXED table: its empty level has no mask address -> SSAD_E_BADARG; the message"""
    _, K = _api()
    c = dict(name="refused", engine=engine, route=route, Cout=36, Cin=20, form="masked")
    try:
        run_engine(c, MIXED)
    except K.KernelError as e:
        return str(e)
    return None


def run_tail(c):
    torch, K = _api()
    L = K.lib()
    rng = np.random.default_rng(seed_of(c["name"].split("_")[-1]))       # one input per shape: split and unsplit comparable
    cout, cin = c["Cout"], c["Cin"]
    n, h, w = c["shape"]
    wt = torch.from_numpy(_filter(rng, cout, cin)).cuda()
    b = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).cuda()
    x = torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32)).cuda()
    pf, _ = K.conv_wino_pack_filter(wt, want_dgrad=False)
    arr = K._conv_levels([x], None, None)
    prev = L.ssad_conv_wino_split_tail(c["setting"])
    try:
        flags = K.CONV_SPLIT_TAIL if c["flag"] else 0
        launches = L.ssad_conv3x3_forward_wino_launches_for(arr, 1, cout, cin, flags)
        if c["flag"]:       # the per-launch hint has no keyword in kernels.py: the native programs set it
            y = torch.empty((n, cout, h, w), dtype=torch.float32, device="cuda")
            arr = K._conv_levels([x], [y], None)
            rc = L.ssad_conv3x3_forward_wino(arr, 1, K._ptr(pf), K._ptr(b), cout, cin, flags, K._stream())
            assert rc == 0, rc
        else:
            y, = K.conv3x3_forward([x], pf, b, cout, wino=True)
        torch.cuda.synchronize()
    finally:
        L.ssad_conv_wino_split_tail(prev)
    return {"y": y.cpu().numpy(), "launches": launches}


def run_pack(c):
    """one table of three entries: 136 x 20 forward only, 136 x 20 data gradient only, 36 x 20 both"""
    torch, K = _api()
    L = K.lib()
    rng = np.random.default_rng(seed_of(c["name"]))
    e = c["engine"]
    size = getattr(L, "ssad_conv_%s_filter_floats" % e)
    w136 = torch.from_numpy(_filter(rng, 136, 20)).cuda()
    w36 = torch.from_numpy(_filter(rng, 36, 20)).cuda()
    buf = lambda m, k: torch.full((size(m, k),), 7.0, dtype=torch.float32, device="cuda")
    out = {"fwd_136_20": buf(136, 20), "dgrad_136_20": buf(20, 136), "fwd_36_20": buf(36, 20), "dgrad_36_20": buf(20, 36)}
    tab = (K.PackEntry * 3)(K.PackEntry(w136.data_ptr(), 136, 20, out["fwd_136_20"].data_ptr(), 0),
                            K.PackEntry(w136.data_ptr(), 136, 20, 0, out["dgrad_136_20"].data_ptr()),
                            K.PackEntry(w36.data_ptr(), 36, 20, out["fwd_36_20"].data_ptr(), out["dgrad_36_20"].data_ptr()))
    rc = getattr(L, "ssad_conv_%s_pack_filters" % e)(tab, 3, K._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


RUNNERS = {"engine": run_engine, "tail": run_tail, "pack": run_pack}


def run_case(c):
    return RUNNERS[c["kind"]](c)


def hashes():
    """per case: the sha256 of every output array (a split-tail case's launch count as it is)"""
    digest = lambda v: sha_words(v) if isinstance(v, np.ndarray) else v
    return {"sha256": {c["name"]: {k: digest(v) for k, v in run_case(c).items()} for c in CASES},
            "masked_refusals": {"%s_%s" % er: masked_table_is_refused(*er) for er in MASKED_REFUSALS}}


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--emit", action="store_true", help="print one run's hashes as JSON (what the two child runs do)")
    args = ap.parse_args()
    if args.emit:
        print("HASHES " + json.dumps(hashes(), sort_keys=True))
        return
    runs = []
    for _ in range(2):
        text = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--emit"], cwd=ROOT).decode()
        runs.append(json.loads(next(l for l in text.splitlines() if l.startswith("HASHES "))[7:]))
    a, b = runs
    differ = [n + "/" + k for n in a["sha256"] for k in a["sha256"][n] if a["sha256"][n][k] != b["sha256"][n].get(k)]
    if differ or a["masked_refusals"] != b["masked_refusals"]:
        sys.exit("two runs of one library differ, nothing written: %s" % differ)
    t = a["sha256"]
    same = [n for n in ("tail_behind_round_setting2_1x128x136", "tail_behind_round_flag_1x128x136")
            if t[n]["y"] == t["tail_off_1x128x136"]["y"]]
    if same:
        sys.exit("the split tail gives the unsplit launch's words, the hash would not pin the decision: %s" % same)
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
    with open(args.out, "w") as f:
        json.dump(dict(a, commit=commit, levels=[list(s) for s in MIXED]), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, len(t), "cases")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
