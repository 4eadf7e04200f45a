"""The scan input path (csrc/scan.hip, abcnet_amd.augment.ScanBuilder) measured three ways, one process, on the frozen trained
fixture (tests/golden/trained_unet_state.npz) and the drawings of drawn_molecules(64, 512, seed=777):

  cover   the drawings made into scans on the host -- a bilinear grey upscale by 2.5 (even images) and by 3.3 (odd ones), paper
          and ink at grey levels that are not 255 and 0, a white border of unequal width on the four sides -- then
          ScanBuilder(cover=c) -> InferenceRunner(assemble=True, evaluate=True, score_similarity=True) for c in 0, 32, 64, 128:
          the mean environment similarity per cover, beside the baseline of the original 512 x 512 drawings through
          ImageBuilder(mode="test"), under both candidate rules of the extractor (omega_rule "raw", the runner's default, and
          "peaks").  The similarity is free of positions, so every row is graded against the same graph records,
          parsed once in the drawings' own coordinates (drawn_molecules annotates carbons that have no bond and so no ink: the
          crop to the ink moves some of them off the canvas, where parse_graph refuses them).
  kernel  ScanBuilder.run() alone (device events around back-to-back calls of the five launches, so launch gaps count); the time
          of each launch alone comes from `rocprofv3 --kernel-trace --stats -- python profiles/tools/scan_step.py --parts kernel`
  step    `r.step()` with the input resident against `sb.run(); r.step()`, alternating blocks, median per-step device time

It prints what it measures; no target is fixed in advance.  One JSON line per measurement.

    python profiles/tools/scan_step.py [--steps 40] [--warmup 10] [--parts cover,kernel,step]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import ImageBuilder, ScanBuilder  # noqa: E402
from abcnet_amd.infer import InferenceRunner  # noqa: E402
from abcnet_amd.raster import TargetRasterizer, parse_graph, parse_record  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]
B, S = 64, 512
COVERS = (0, 32, 64, 128)
PAPER, INK = 212, 38
MAX_SRC = (1792, 1792)


def model():
    from make_trained_fixture import unpack_state
    m = UNet(1, HEADS, dtype="bf16", dropout_p=0.2)
    m.load_state_dict(unpack_state(os.path.join(ROOT, "tests", "golden", "trained_unet_state.npz")))
    return m.to("cuda").eval()


def make_scans(x):
    """the drawings as grey scans (uint8, mixed sizes)"""
    rs = np.random.RandomState(12)
    scans = []
    for b in range(x.shape[0]):
        f = 2.5 if b % 2 == 0 else 3.3
        n = int(round(S * f))
        grey = PAPER + (INK - PAPER) * x[b:b + 1]                       # f32 [1, 1, S, S]
        up = torch.nn.functional.interpolate(grey, size=(n, n), mode="bilinear", align_corners=False)[0, 0].numpy()
        top, bottom, left, right = (int(v) for v in rs.randint(3, 50, size=4))
        page = np.full((n + top + bottom, n + left + right), 255, dtype=np.uint8)
        page[top:top + n, left:left + n] = np.clip(np.rint(up), 0, 255).astype(np.uint8)
        scans.append(page)
    return scans


def runner(m, rule):
    r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, evaluate=True, score_similarity=True, omega_rule=rule)
    rz = TargetRasterizer(B, S // 4, targets=r.targets, sparse=True)
    r.use_sparse_targets(rz)
    return r, rz


def similarity(r):
    r.reset_evaluation()
    r.step()
    return r.evaluation()["similarity"]


def part_cover(m, x, notes, scans, rule):
    r, rz = runner(m, rule)
    # (the evaluating step wants targets: the drawings' own, rasterised once; its tables are not what this part reports)
    rz.load([parse_record(a, q, h=S // 4) for a, q in notes])
    rz.run()
    r.load_graphs([parse_graph(a, q, h=S // 4) for a, q in notes])
    ib = ImageBuilder(B, S, "test", out=r.input_images)
    ib.load([((1.0 - x[b, 0].numpy()) * 255).astype(np.uint8) for b in range(B)])
    ib.run()
    res = similarity(r)
    base = np.asarray(res["rows"])[:, L.GRAPH_SIM_COLUMNS.index("dice_q20")] / 2.0 ** 20
    print(json.dumps({"part": "cover", "omega_rule": rule, "input": "512 x 512 drawings, mode='test'", "similarity": round(res["similarity"], 6),
                      "per_image_min_max": [round(float(base.min()), 4), round(float(base.max()), 4)],
                      "dice_one": int(res["dice_one"]), "none": int(res["none"]), "counted": int(res["counted"])}), flush=True)
    best = None
    for cover in COVERS:
        sb = ScanBuilder(B, S, out=r.input_images, max_src=MAX_SRC, cover=cover, polarity="dark")
        sb.load(scans)
        sb.run()
        res = similarity(r)
        g = sb.geometry()
        # the white border is a third level: where the ink is sparse the threshold lands between paper and border, and the paper
        # becomes ink; the mean over the other images is printed beside the mean over all
        split = g["thr"] < PAPER
        per_image = np.asarray(res["rows"])[:, L.GRAPH_SIM_COLUMNS.index("dice_q20")] / 2.0 ** 20
        print(json.dumps({"part": "cover", "omega_rule": rule, "input": "scans", "cover_q8": cover, "similarity": round(res["similarity"], 6),
                          "paper_taken_for_ink": int((~split).sum()), "similarity_of_the_others": round(float(per_image[split].mean()), 6),
                          "dice_one": int(res["dice_one"]), "none": int(res["none"]), "counted": int(res["counted"]),
                          "thr_min_max": [int(g["thr"].min()), int(g["thr"].max())], "rows_min_max": [int(g["rows"].min()), int(g["rows"].max())],
                          "ink_on_canvas": int(r.input_images.sum().item())}), flush=True)
        if best is None or res["similarity"] > best[1]:
            best = (cover, res["similarity"])
        del sb
    print(json.dumps({"part": "cover", "omega_rule": rule, "best_cover_q8": best[0], "rule": "the best mean similarity, the smaller cover on a tie"}), flush=True)


def part_kernel(scans, iters=100):
    for cover in (0, 64):
        sb = ScanBuilder(B, S, max_src=MAX_SRC, cover=cover)
        sb.load(scans)
        for _ in range(10):
            sb.run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            sb.run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000 / iters
        src_bytes = sum(int(s.size) for s in scans)
        print(json.dumps({"part": "kernel", "batch": B, "size": S, "cover_q8": cover, "us_per_run": round(us, 2), "source_bytes": src_bytes,
                          "out_bytes": B * S * S * 4,
                          "method": "device events around %d back-to-back runs of the five launches (gaps included; each launch alone: "
                                    "run --parts kernel under rocprofv3 --kernel-trace --stats)" % iters}), flush=True)
        del sb


def part_step(m, scans, steps, warmup):
    r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True)
    sb = ScanBuilder(B, S, out=r.input_images, max_src=MAX_SRC)
    sb.load(scans)
    sb.run()

    def plain():
        r.step()

    def with_scan():
        sb.run()
        r.step()
    forms = {"r.step()": plain, "sb.run(); r.step()": with_scan}
    for f in forms.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for blk in range(4):
        for name, f in (forms.items() if blk % 2 == 0 else reversed(list(forms.items()))):
            ev = []
            for _ in range(steps // 4):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            times[name] += [a.elapsed_time(b) for a, b in ev]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(json.dumps({"part": "step", "form": k, "batch": B, "size": S, "steps": len(v), "ms_per_step_median": round(med[k], 4),
                          "ms_min": round(min(v), 4)}), flush=True)
    print(json.dumps({"part": "step", "scan_minus_plain_ms": round(med["sb.run(); r.step()"] - med["r.step()"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="cover,kernel,step")
    a = ap.parse_args()
    parts = a.parts.split(",")
    x, notes = drawn_molecules(B, S, seed=777)
    scans = make_scans(x)
    m = model() if ("cover" in parts or "step" in parts) else None
    if "cover" in parts:
        for rule in ("raw", "peaks"):      # (raw: the runner's default candidate rule, the one the default cover follows)
            part_cover(m, x, notes, scans, rule)
    if "kernel" in parts:
        part_kernel(scans)
    if "step" in parts:
        part_step(m, scans, a.steps, a.warmup)


if __name__ == "__main__":
    main()
