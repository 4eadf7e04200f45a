"""The cell component filter of the scan path (abc_build_scan_images_clean, ScanBuilder(clean_cell=...)) measured three ways, a
process per part, on the frozen trained fixture and the scans of profiles/tools/scan_step.py (r13), whose conventions it keeps:

  sim     r13's synthetic scans made dirty on the host -- a seeded handful of ink-grey blobs of 2 x 2 .. 5 x 5 inside the white
          border band, and a strip of paper appended below the drawing that carries one row of letter-sized blobs -- through
          ScanBuilder -> InferenceRunner(assemble=True, evaluate=True, score_similarity=True): the mean environment similarity
          of the clean scans, of the dirty scans with the plain builder, and of the dirty scans with clean_cell 8 / 16 / 32 at
          clean_keep=256 and at clean_keep=0, clean_min_ink=64, under both candidate rules; beside each cleaned row the number
          of drawings that lost ink of their own to the filter (ink_dropped above the known added dirt)
  kernel  ScanBuilder.run() on the dirty scans without and with cleaning (cell 16, keep 256), alternating blocks in one process,
          device events around back-to-back calls; each launch alone comes from
          `rocprofv3 --kernel-trace --stats -- python profiles/tools/scan_clean_step.py --parts kernel`
  step    `sb.run(); r.step()` without and with cleaning, alternating blocks, median per-step device time

No real scan was available.  It prints what it measures; no target is fixed in advance.  One JSON line per measurement.

    python profiles/tools/scan_clean_step.py [--steps 40] [--warmup 10] [--parts sim,kernel,step]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scan_step as r13  # noqa: E402  (puts the repository root on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import ScanBuilder  # noqa: E402
from abcnet_amd.infer import InferenceRunner  # noqa: E402
from abcnet_amd.raster import parse_graph, parse_record  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402

B, S = r13.B, r13.S
PAPER, INK = r13.PAPER, r13.INK
STRIP, CAPTION_AT, LETTER, LETTERS = 160, 100, (14, 9), 10      # rows appended; the caption's row in them; a letter; how many
MAX_SRC = (r13.MAX_SRC[0] + STRIP, r13.MAX_SRC[1])
SETTINGS = [(cell, 0, 256) for cell in (8, 16, 32)] + [(cell, 64, 0) for cell in (8, 16, 32)]      # (cell, min_ink, keep)


def make_dirty(scans):
    """(dirty scans, ink pixels added to each): specks inside the white border band, a caption on a strip of paper below"""
    rs = np.random.RandomState(16)
    out, added = [], []
    for page in scans:
        h, w = page.shape
        k = 0
        while (page[h - 1 - k] == 255).all():
            k += 1                                            # the bottom border
        side = page[h - k - 1] == 255                         # the left and right borders, from the last row of paper
        strip = np.where(side, 255, PAPER).astype(np.uint8)[None, :].repeat(STRIP, axis=0)
        left = int(np.argmin(side))
        n = 0
        for i in range(LETTERS):
            x = left + 40 + i * (LETTER[1] + 8)
            strip[CAPTION_AT:CAPTION_AT + LETTER[0], x:x + LETTER[1]] = INK
            n += LETTER[0] * LETTER[1]
        page = np.vstack([page[:h - k], strip, page[h - k:]])
        border = page == 255
        for _ in range(int(rs.randint(3, 7))):
            while True:                                       # a blob that lies in the border band whole
                a = int(rs.randint(2, 6))
                y, x = int(rs.randint(0, page.shape[0] - a + 1)), int(rs.randint(0, w - a + 1))
                if border[y:y + a, x:x + a].all():
                    break
            page[y:y + a, x:x + a] = INK
            border[y:y + a, x:x + a] = False
            n += a * a
        out.append(page)
        added.append(n)
    return out, np.asarray(added)


def part_sim(m, notes, scans, dirty, added, rule):
    r, rz = r13.runner(m, rule)
    rz.load([parse_record(a, q, h=S // 4) for a, q in notes])
    rz.run()
    r.load_graphs([parse_graph(a, q, h=S // 4) for a, q in notes])

    def row(name, srcs, **kw):
        sb = ScanBuilder(B, S, out=r.input_images, max_src=MAX_SRC, polarity="dark", **kw)
        sb.load(srcs)
        sb.run()
        res = r13.similarity(r)
        g = sb.geometry()
        split = g["thr"] < PAPER                               # (r13: on the others the threshold lands on the paper)
        per_image = np.asarray(res["rows"])[:, L.GRAPH_SIM_COLUMNS.index("dice_q20")] / 2.0 ** 20
        rec = {"part": "sim", "omega_rule": rule, "input": name, "similarity": round(res["similarity"], 6),
               "paper_taken_for_ink": int((~split).sum()), "similarity_of_the_others": round(float(per_image[split].mean()), 6),
               "bh_min_max": [int(g["bh"].min()), int(g["bh"].max())], "rows_min_max": [int(g["rows"].min()), int(g["rows"].max())],
               "status_nonzero": int((g["status"] != 0).sum())}
        if kw:
            st = sb.clean_stats()
            lost = (st["ink_dropped"] > added) & split
            kept_dirt = (st["ink_dropped"] < added) & split
            rec.update(clean_cell=kw["clean_cell"], clean_min_ink=kw["clean_min_ink"], clean_keep=kw["clean_keep"],
                       drawings_that_lost_ink=int(lost.sum()), drawings_that_kept_dirt=int(kept_dirt.sum()),
                       components_min_max=[int(st["components"].min()), int(st["components"].max())],
                       kept_min_max=[int(st["kept"].min()), int(st["kept"].max())])
        print(json.dumps(rec), flush=True)
        del sb
    row("clean scans, plain builder", scans)
    row("dirty scans, plain builder", dirty)
    for cell, min_ink, keep in SETTINGS:
        row("dirty scans, cleaned", dirty, clean_cell=cell, clean_min_ink=min_ink, clean_keep=keep)


def _alternate(forms, steps, warmup, part):
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
        print(json.dumps({"part": part, "form": k, "batch": B, "size": S, "calls": len(v), "ms_median": round(med[k], 4),
                          "ms_min": round(min(v), 4)}), flush=True)
    return med


def part_kernel(dirty, iters=100):
    plain = ScanBuilder(B, S, max_src=MAX_SRC)
    clean = ScanBuilder(B, S, max_src=MAX_SRC, clean_cell=16, clean_keep=256)
    for sb in (plain, clean):
        sb.load(dirty)
    res = {}
    for blk in range(4):
        for name, sb in (("plain", plain), ("cleaned", clean)) if blk % 2 == 0 else (("cleaned", clean), ("plain", plain)):
            for _ in range(10):
                sb.run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                sb.run()
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(name, []).append(e0.elapsed_time(e1) * 1000 / iters)
    for name, v in res.items():
        print(json.dumps({"part": "kernel", "form": name, "batch": B, "size": S, "us_per_run_blocks": [round(x, 2) for x in v],
                          "us_per_run_median": round(statistics.median(v), 2), "source_bytes": sum(int(s.size) for s in dirty),
                          "method": "device events around %d back-to-back runs, 4 alternating blocks (gaps included)" % iters}), flush=True)
    print(json.dumps({"part": "kernel", "cleaned_over_plain": round(statistics.median(res["cleaned"]) / statistics.median(res["plain"]), 4)}),
          flush=True)


def part_step(m, dirty, steps, warmup):
    r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True)
    plain = ScanBuilder(B, S, out=r.input_images, max_src=MAX_SRC)
    clean = ScanBuilder(B, S, out=r.input_images, max_src=MAX_SRC, clean_cell=16, clean_keep=256)
    for sb in (plain, clean):
        sb.load(dirty)

    def with_plain():
        plain.run()
        r.step()

    def with_clean():
        clean.run()
        r.step()
    med = _alternate({"sb.run(); r.step()": with_plain, "cleaned sb.run(); r.step()": with_clean}, steps, warmup, "step")
    print(json.dumps({"part": "step", "cleaned_minus_plain_ms": round(med["cleaned sb.run(); r.step()"] - med["sb.run(); r.step()"], 4)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="sim,kernel,step")
    a = ap.parse_args()
    parts = a.parts.split(",")
    x, notes = drawn_molecules(B, S, seed=777)
    scans = r13.make_scans(x)
    dirty, added = make_dirty(scans)
    print(json.dumps({"part": "scans", "dirty_rows_min_max": [min(d.shape[0] for d in dirty), max(d.shape[0] for d in dirty)],
                      "added_ink_min_max": [int(added.min()), int(added.max())], "capacity": list(MAX_SRC)}), flush=True)
    m = r13.model() if ("sim" in parts or "step" in parts) else None
    if "sim" in parts:
        for rule in ("raw", "peaks"):
            part_sim(m, notes, scans, dirty, added, rule)
    if "kernel" in parts:
        part_kernel(dirty)
    if "step" in parts:
        part_step(m, dirty, a.steps, a.warmup)


if __name__ == "__main__":
    main()
