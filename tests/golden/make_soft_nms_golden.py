#!/usr/bin/env python3
"""Golden vectors for Soft-NMS and bounding-box voting from the reference's own code.

Like make_nms_golden.py: detectron/lib/utils/cython_nms.pyx (`soft_nms`, lines 98-203) and cython_bbox.pyx
(`bbox_overlaps`, lines 32-72) do not build in this image, so their text is EXECUTED AS PYTHON: this script reads the
files where they lie under /root/reference at generation time (nothing of them is stored in the repository), removes
what only the C compiler needs -- the substitutions in `strip_cython` are the whole transformation -- and runs the
result.  `box_voting` (utils/boxes.py:262-311) is Python already: its text is executed as it stands with that
`bbox_overlaps`.  With numpy >= 2 a float32 scalar that meets a Python number stays float32 (NEP 50), which is what the
typed C variables do; `np.exp` of a float32 is float32 where the compiled module rounds a double exp (one ulp).

Only arrays are stored:
  soft_dets_<d>                      [n][5] float32 input of data set d
  soft_{data,method,nt,sigma,thresh,margin}[v]   one entry per case v (method 0 hard, 1 linear, 2 gaussian, the
                                     reference's numbering); margin = the smallest relative distance of any discrete
                                     decision of the case from flipping (see `order_free`)
  soft_keep_<v>, soft_scores_<v>     what the reference returned: original indices in pick order, decayed scores
  ms_*                               one multi-class array in the layout of detect.hip's class-sorted candidates
  vote_*                             box_voting cases

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_soft_nms_golden.py     -> tests/golden/soft_nms_ref.npz
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/detectron/lib/utils/"
OUT = os.path.join(HERE, "soft_nms_ref.npz")
CAP = 1024                      # soft_nms.hip's kSoftNmsLdsCap: the segment length up to which it works in LDS
F = np.float32
SCORING = ("ID", "TEMP_AVG", "AVG", "IOU_AVG", "GENERALIZED_AVG", "QUASI_SUM")


def strip_cython(lines):
    out = []
    for s in lines:
        if s.strip().startswith(("@cython.", "cimport ", "#")):
            continue
        s = re.sub(r"np\.ndarray\[[^\]]*\] ", "", s)                    # typed array arguments / locals
        s = re.sub(r"^(\s*)(unsigned int|float) (\w+=)", r"\1\3", s)    # typed keyword arguments
        if re.match(r"\s*cdef (unsigned int |int |float |DTYPE_t )?[\w, ]+$", s):
            continue                                                    # bare declarations carry no value
        s = re.sub(r"^(\s*)cdef (unsigned int |int |float |DTYPE_t )?", r"\1", s)   # typed assignments keep their value
        s = re.sub(r"^(\s*)with nogil:", r"\1if True:", s)
        out.append(s)
    return "\n".join(out)


def reference_soft_nms():
    src = open(REF + "cython_nms.pyx").read().split("\n")
    start = next(i for i, l in enumerate(src) if l.startswith("def soft_nms("))
    text = strip_cython(src[start:])
    assert "cdef" not in text and "np.ndarray" not in text and "weight*boxes[pos, 4]" in text
    ns = {"np": np}
    exec(compile(text, "<cython_nms.pyx:soft_nms as python>", "exec"), ns)
    return ns["soft_nms"]


def reference_box_voting():
    src = open(REF + "cython_bbox.pyx").read().split("\n")
    start = next(i for i, l in enumerate(src) if l.startswith("def bbox_overlaps("))
    text = strip_cython(src[start:])
    assert "cdef" not in text and "np.ndarray" not in text and "overlaps[n, k] = iw * ih / ua" in text
    ns = {"np": np, "DTYPE": np.float32}
    exec(compile(text, "<cython_bbox.pyx:bbox_overlaps as python>", "exec"), ns)
    overlaps, memo = ns["bbox_overlaps"], {}

    def bbox_overlaps(a, b):       # the reference's function, called once per distinct (top, all) pair
        key = (a.tobytes(), b.tobytes())
        if key not in memo:
            memo[key] = overlaps(np.ascontiguousarray(a), np.ascontiguousarray(b))
        return memo[key]

    src = open(REF + "boxes.py").read().split("\n")
    start = next(i for i, l in enumerate(src) if l.startswith("def box_voting("))
    end = next(i for i, l in enumerate(src) if l.startswith("def nms("))
    ns2 = {"np": np, "bbox_overlaps": bbox_overlaps}
    exec(compile("\n".join(src[start:end]), "<boxes.py:box_voting>", "exec"), ns2)
    return ns2["box_voting"], bbox_overlaps


def order_free(dets, sigma, nt, thresh, method):
    """The definition soft_nms.hip is written to (no swap bookkeeping), and the margin of every decision it takes:
    (best - second best) / best at each pick, |new - thresh| / thresh after each decay.  Returns keep, scores, margin."""
    b, s = dets[:, :4], dets[:, 4].copy()
    area = (b[:, 2] - b[:, 0] + F(1)) * (b[:, 3] - b[:, 1] + F(1))
    live = np.ones(len(s), bool)
    keep, out, margin = [], [], np.inf
    while live.any():
        idx = np.flatnonzero(live)
        i = idx[np.argmax(s[idx])]
        if idx.size > 1:
            top2 = np.sort(s[idx])[-2:].astype(np.float64)
            margin = min(margin, (top2[1] - top2[0]) / max(top2[1], 1e-30))
        keep.append(i)
        out.append(s[i])
        live[i] = False
        j = np.flatnonzero(live)
        iw = np.minimum(b[i, 2], b[j, 2]) - np.maximum(b[i, 0], b[j, 0]) + F(1)
        ih = np.minimum(b[i, 3], b[j, 3]) - np.maximum(b[i, 1], b[j, 1]) + F(1)
        hit = (iw > 0) & (ih > 0)
        j, iw, ih = j[hit], iw[hit], ih[hit]
        ov = iw * ih / (area[i] + area[j] - iw * ih)
        if method == 1:
            w = np.where(ov > nt, F(1) - ov, F(1))
        elif method == 2:
            w = np.exp(-(ov * ov) / sigma)
        else:
            w = np.where(ov > nt, F(0), F(1))
        s[j] = w * s[j]
        if j.size and thresh > 0:
            margin = min(margin, float(np.min(np.abs(s[j].astype(np.float64) - thresh) / thresh)))
        live[j[s[j] < thresh]] = False
    return np.asarray(keep, np.int32), np.asarray(out, F), margin


def boxes(rng, n, spread, size):
    ctr = rng.uniform(0, spread, size=(n, 2)).astype(F)
    wh = rng.uniform(4, size, size=(n, 2)).astype(F)
    scores = rng.permutation(n).astype(F) / F(n) + F(0.0015)           # distinct, none equal to a score_thresh of 0.001
    return np.concatenate([ctr - wh / 2, ctr + wh / 2, scores[:, None]], axis=1).astype(F)


def soft_cases(soft_nms):
    rng = np.random.default_rng(20261018)
    dsets, cases = [], []                 # cases: (data set, method, nt, sigma, thresh)
    for n, spread, size in ((1, 50, 30), (2, 5, 30), (63, 120, 40), (64, 100, 40), (65, 110, 40), (256, 200, 60),
                            (257, 220, 60), (400, 80, 50), (CAP, 70, 60), (CAP + 1, 70, 60)):
        dsets.append(boxes(rng, n, spread, size))
        for method in (1, 0):
            for nt in ((0.3, 0.5) if n <= 257 else (0.3,)):
                cases.append((len(dsets) - 1, method, nt, 0.5, 0.001))
    # pairwise disjoint boxes, five of them scored below score_thresh: nothing is ever tested against it, all survive
    g = np.arange(40)
    x, y = (g % 8) * 30.0, (g // 8) * 30.0
    sc = rng.permutation(40).astype(F) / F(40) + F(0.002)
    sc[[3, 11, 17, 29, 38]] = F([0.0009, 0.0005, 0.0007, 0.0001, 0.0003])
    dsets.append(np.stack([x, y, x + 20, y + 20, sc], 1).astype(F))
    cases += [(len(dsets) - 1, 1, 0.3, 0.5, 0.001), (len(dsets) - 1, 0, 0.3, 0.5, 0.001)]
    # identical boxes: overlap 1 with the first pick
    dsets.append(np.array([[4, 6, 30, 40, s] for s in (0.3, 0.9, 0.5, 0.7, 0.1, 0.8)], F))
    cases += [(len(dsets) - 1, 1, 0.3, 0.5, 0.001), (len(dsets) - 1, 0, 0.5, 0.5, 0.001)]
    # gaussian: seeds are tried in order until no decision of the case is closer than 1e-3 to flipping
    for n, spread, size in ((2, 5, 30), (30, 80, 40), (64, 100, 40)):
        for sigma in (0.3, 0.5):
            for seed in range(1000):
                d = boxes(np.random.default_rng(7000 + seed), n, spread, size)
                if order_free(d, F(sigma), F(0.3), F(0.001), 2)[2] >= 1e-3:
                    break
            else:
                raise SystemExit("no gaussian seed with margin >= 1e-3 at n = %d" % n)
            dsets.append(d)
            cases.append((len(dsets) - 1, 2, 0.3, sigma, 0.001))
    blobs = {"soft_dets_%d" % d: a for d, a in enumerate(dsets)}
    margins = []
    for v, (d, method, nt, sigma, thresh) in enumerate(cases):
        out, keep = soft_nms(dsets[d].copy(), F(sigma), F(nt), F(thresh), np.uint8(method))
        k2, s2, margin = order_free(dsets[d], F(sigma), F(nt), F(thresh), method)
        assert margin > 0, "exact tie in case %d" % v
        assert margin >= 1e-3 or method != 2
        # the order-free definition is the reference's function whenever no two current scores tie
        assert np.array_equal(k2, keep) and np.array_equal(s2, out[:, 4]), v
        assert np.array_equal(out[:, :4], dsets[d][keep, :4])
        blobs["soft_keep_%d" % v] = np.asarray(keep, np.int32)
        blobs["soft_scores_%d" % v] = np.asarray(out[:, 4], F)
        margins.append(margin)
    for i, name in enumerate(("data", "method")):
        blobs["soft_" + name] = np.array([c[i] for c in cases], np.int32)
    for i, name in ((2, "nt"), (3, "sigma"), (4, "thresh")):
        blobs["soft_" + name] = np.array([c[i] for c in cases], F)
    blobs["soft_margin"] = np.array(margins, np.float64)
    return blobs


def multi_segment(soft_nms):
    """6 classes, classes 0, 3 and 5 empty, four trailing -1 slots; per class what the reference returns."""
    rng = np.random.default_rng(20261019)
    parts, cls = [], []
    for c, n in ((1, 70), (2, 1), (4, 130)):
        d = boxes(rng, n, 90, 40)
        parts.append(d[np.argsort(-d[:, 4], kind="stable")])           # score-descending like the detector's segments
        cls += [c] * n
    dets = np.concatenate(parts + [np.zeros((4, 5), F)])
    cls = np.array(cls + [-1] * 4, np.int32)
    blobs = {"ms_dets": dets, "ms_cls": cls, "ms_classes": np.int32(6)}
    for name, method in (("linear", 1), ("hard", 0)):
        rank = np.full(len(cls), -1, np.int32)
        score = np.zeros(len(cls), F)
        for c in range(6):
            pos = np.flatnonzero(cls == c)
            if pos.size:
                out, keep = soft_nms(dets[pos].copy(), F(0.5), F(0.3), F(0.001), np.uint8(method))
                assert order_free(dets[pos], F(0.5), F(0.3), F(0.001), method)[2] > 0
                rank[pos[keep]] = np.arange(len(keep))
                score[pos[keep]] = out[:, 4]
        blobs["ms_rank_" + name], blobs["ms_score_" + name] = rank, score
    return blobs


def vote_cases(soft_nms, box_voting, bbox_overlaps):
    sys.path.insert(0, HERE)
    from make_nms_golden import reference_nms
    nms = reference_nms()[0]
    variants = [(m, b) for m in SCORING for b in ((1.0, 0.5) if m in ("TEMP_AVG", "GENERALIZED_AVG", "QUASI_SUM")
                                                  else (1.0,))]
    blobs, rows, k, t = {}, [], 0, 0
    for a, (n, spread, size) in enumerate(((1, 50, 30), (65, 60, 40), (400, 120, 50))):
        for seed in range(1000):
            alld = boxes(np.random.default_rng(9000 + 10 * a + seed), n, spread, size)
            tops = [soft_nms(alld.copy(), F(0.5), F(0.3), F(0.001), np.uint8(1))[0],
                    alld[nms(alld.copy(), F(0.5))]]
            # voter sets must not hinge on rounding: every IoU at least 1e-4 away from both thresholds
            if all(np.abs(bbox_overlaps(tp[:, :4], alld[:, :4]).astype(np.float64) - th).min() >= 1e-4
                   for tp in tops for th in (0.5, 0.8)):
                break
        else:
            raise SystemExit("no voting seed with an IoU margin at n = %d" % n)
        blobs["vote_all_%d" % a] = alld
        for i, tp in enumerate(tops):
            blobs["vote_top_%d" % t] = np.ascontiguousarray(tp, F)
            for th in ((0.5, 0.8) if n < 400 else ((0.8,) if i == 0 else (0.5,))):
                for m, beta in variants:
                    blobs["vote_out_%d" % k] = np.asarray(box_voting(tp, alld, th, m, beta), F)
                    rows.append((a, t, SCORING.index(m), th, beta))
                    k += 1
            t += 1
    for i, (name, dt) in enumerate((("all", np.int32), ("top", np.int32), ("scoring", np.int32), ("thresh", F),
                                    ("beta", F))):
        blobs["vote_" + name] = np.array([r[i] for r in rows], dt)
    return blobs


def generate():
    soft_nms = reference_soft_nms()
    box_voting, bbox_overlaps = reference_box_voting()
    blobs = soft_cases(soft_nms)
    blobs.update(multi_segment(soft_nms))
    blobs.update(vote_cases(soft_nms, box_voting, bbox_overlaps))
    blobs["lds_cap"] = np.int32(CAP)
    return blobs


def main():
    blobs = generate()
    np.savez_compressed(OUT, **blobs)
    print("wrote %s: %d soft-NMS cases (smallest gaussian margin %.2e), %d voting cases, %d bytes" % (
        OUT, len(blobs["soft_method"]), blobs["soft_margin"][blobs["soft_method"] == 2].min(), len(blobs["vote_all"]),
        os.path.getsize(OUT)))


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
