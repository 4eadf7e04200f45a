"""The stroke normaliser (csrc/stroke.hip, abcnet_amd.ops.StrokeNormalizer, the sixth launch of augment.ScanBuilder) measured three
ways, one process, on the frozen trained fixture and the scans of profiles/tools/scan_step.py (its scan maker is imported, not
copied: the same 64 drawings of drawn_molecules(64, 512, seed=777) made into grey scans on the host):

  similarity  ScanBuilder(thin=t, stroke_radius=r) -> InferenceRunner(assemble=True, evaluate=True, score_similarity=True) for
              t in None, 1, 2, "stable" and r in 0, 1, 2, at the default cover: the mean environment similarity per setting under
              both candidate rules of the extractor, beside the two baselines of profiles/r13_scan.md -- the 512 x 512 drawings
              themselves through ImageBuilder(mode="test"), and the scans with no normalisation (t = None, r = 0 builds no sixth
              launch: it IS that baseline).  The images where Otsu takes the paper for ink (the white border is a third level)
              are reported apart, as r13 does.
  kernel      StrokeNormalizer.run() alone over a scan batch (device events around back-to-back out-of-place calls, so launch
              gaps count); the launch alone comes from
              `rocprofv3 --kernel-trace --stats -- python profiles/tools/stroke_step.py --parts kernel`
  step        `sb.run(); r.step()` without and with the sixth launch, alternating blocks, median per-step device time

It prints what it measures; no target is fixed in advance.  One JSON line per measurement.

    python profiles/tools/stroke_step.py [--steps 40] [--warmup 10] [--parts similarity,kernel,step]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import scan_step as ss  # noqa: E402  (puts the repository root on sys.path)
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import ImageBuilder, ScanBuilder  # noqa: E402
from abcnet_amd.infer import InferenceRunner  # noqa: E402
from abcnet_amd.ops import StrokeNormalizer  # noqa: E402
from abcnet_amd.raster import parse_graph, parse_record  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402

B, S = ss.B, ss.S
THINS = (None, 1, 2, "stable")
RADII = (0, 1, 2)
DICE = L.GRAPH_SIM_COLUMNS.index("dice_q20")


def per_image(res):
    return np.asarray(res["rows"])[:, DICE] / 2.0 ** 20


def part_similarity(m, x, notes, scans, rule):
    r, rz = ss.runner(m, rule)
    rz.load([parse_record(a, q, h=S // 4) for a, q in notes])
    rz.run()
    r.load_graphs([parse_graph(a, q, h=S // 4) for a, q in notes])
    ib = ImageBuilder(B, S, "test", out=r.input_images)
    ib.load([((1.0 - x[b, 0].numpy()) * 255).astype(np.uint8) for b in range(B)])
    ib.run()
    res = ss.similarity(r)
    print(json.dumps({"part": "similarity", "omega_rule": rule, "input": "512 x 512 drawings, mode='test'",
                      "similarity": round(res["similarity"], 6), "ink_on_canvas": int(r.input_images.sum().item())}), flush=True)
    table, base = {}, None
    for thin in THINS:
        for radius in RADII:
            plain = thin is None and radius == 0
            kw = {} if plain else dict(thin=thin, stroke_radius=radius)
            sb = ScanBuilder(B, S, out=r.input_images, max_src=ss.MAX_SRC, polarity="dark", **kw)
            sb.load(scans)
            sb.run()
            res = ss.similarity(r)
            g = sb.geometry()
            split = g["thr"] < ss.PAPER          # (the others: Otsu took the paper for ink)
            dice = per_image(res)
            row = {"part": "similarity", "omega_rule": rule, "input": "scans", "thin": thin, "stroke_radius": radius,
                   "sixth_launch": not plain, "cover_q8": sb.cover, "similarity": round(res["similarity"], 6),
                   "paper_taken_for_ink": int((~split).sum()), "similarity_of_the_others": round(float(dice[split].mean()), 6),
                   "similarity_of_those": round(float(dice[~split].mean()), 6) if (~split).any() else None,
                   "dice_one": int(res["dice_one"]), "none": int(res["none"]), "counted": int(res["counted"]),
                   "ink_on_canvas": int(r.input_images.sum().item())}
            if not plain:
                st = sb.stroke_stats()
                row.update(iterations_min_max=[int(st["iterations"].min()), int(st["iterations"].max())],
                           converged=int(st["converged"].sum()), skipped=int(st["skipped"].sum()))
            print(json.dumps(row), flush=True)
            table[(thin, radius)] = (res["similarity"], float(dice[split].mean()))
            if plain:
                base = table[(thin, radius)]
            del sb
    return base, table


def part_kernel(scans, iters=100):
    sb = ScanBuilder(B, S, max_src=ss.MAX_SRC)
    sb.load(scans)
    src = sb.run().clone()
    dst = torch.empty_like(src)
    for thin, radius in ((None, 0), (1, 1), (2, 1), ("stable", 0), ("stable", 1), ("stable", 3)):
        sn = StrokeNormalizer(src, out=dst, thin=thin, radius=radius)          # (out of place: every call does the same work)
        for _ in range(10):
            sn.run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            sn.run()
        e1.record()
        torch.cuda.synchronize()
        st = sn.stats()
        print(json.dumps({"part": "kernel", "batch": B, "size": S, "thin": thin, "radius": radius,
                          "us_per_run": round(e0.elapsed_time(e1) * 1000 / iters, 2),
                          "iterations_min_max": [int(st["iterations"].min()), int(st["iterations"].max())],
                          "ink_in": int(st["ink_in"].sum()), "ink_out": int(st["ink_out"].sum()), "bytes_moved": 2 * B * S * S * 4,
                          "method": "device events around %d back-to-back launches (gaps included; the launch alone: run --parts kernel "
                                    "under rocprofv3 --kernel-trace --stats)" % iters}), flush=True)


def part_step(m, scans, steps, warmup):
    r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True)
    plain = ScanBuilder(B, S, out=r.input_images, max_src=ss.MAX_SRC)
    peel = ScanBuilder(B, S, out=r.input_images, max_src=ss.MAX_SRC, thin=1, stroke_radius=1)
    sixth = ScanBuilder(B, S, out=r.input_images, max_src=ss.MAX_SRC, thin="stable", stroke_radius=1)
    for sb in (plain, peel, sixth):
        sb.load(scans)

    def step_after(sb):
        def f():
            sb.run()
            r.step()
        return f
    forms = {"five launches; r.step()": step_after(plain), "six launches (thin=1, stroke_radius=1); r.step()": step_after(peel),
             "six launches (thin='stable', stroke_radius=1); r.step()": step_after(sixth)}
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
    a, b, c = list(forms)
    print(json.dumps({"part": "step", "sixth_launch_ms": {"thin=1, stroke_radius=1": round(med[b] - med[a], 4),
                                                          "thin='stable', stroke_radius=1": round(med[c] - med[a], 4)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="similarity,kernel,step")
    a = ap.parse_args()
    parts = a.parts.split(",")
    x, notes = drawn_molecules(B, S, seed=777)
    scans = ss.make_scans(x)
    m = ss.model() if ("similarity" in parts or "step" in parts) else None
    if "similarity" in parts:
        seen = {}
        for rule in ("raw", "peaks"):
            seen[rule] = part_similarity(m, x, notes, scans, rule)
        # a setting is better when it beats the unnormalised scans under BOTH rules (the mean over all 64 images)
        better = [k for k in seen["raw"][1] if k != (None, 0) and all(seen[r][1][k][0] > seen[r][0][0] for r in seen)]
        print(json.dumps({"part": "similarity", "beats_the_unnormalised_scans_under_both_rules":
                          [{"thin": t, "stroke_radius": r, "raw": round(seen["raw"][1][(t, r)][0], 6),
                            "peaks": round(seen["peaks"][1][(t, r)][0], 6)} for t, r in better],
                          "unnormalised": {r: round(seen[r][0][0], 6) for r in seen}}), flush=True)
    if "kernel" in parts:
        part_kernel(scans)
    if "step" in parts:
        part_step(m, scans, a.steps, a.warmup)


if __name__ == "__main__":
    main()
