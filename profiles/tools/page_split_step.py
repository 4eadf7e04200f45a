"""The page splitter (abc_split_scan_pages, PageSplitter) measured on composed pages, and the choice of its default cell and reach.

No real page was available.  Pages are composed on the host: P = 6 sheets of 2 x 2 drawings of drawn_molecules(24, 512, seed=777)
at their own size, flat grey ink on flat grey paper, 160 pixels of paper between and around them, and under each drawing a
caption of ten letter-sized blobs (14 x 9, as profiles/tools/scan_clean_step.py draws them), once 96 pixels below the drawing's
frame and once 160 (the gutter's width).  These drawings are sparse at 512: fragments of one drawing lie up to about a hundred
pixels apart, which is what a reach has to bridge.

  groups  for every (cell, reach) tried: PageSplitter over the pages with room for every group; from its cell tables, for each
          of the 24 drawings, the groups that hold its ink.  whole = one group that holds exactly the drawing's ink; split = more
          than one group; merged = a group of it holds other ink too (a caption, a neighbour).  The cell tables are first
          compared with tests/page_split_oracle.py's on the same pages: the oracle decides, the device must agree.
  kernel  PageSplitter.run() against ScanBuilder(clean_cell=cell).run() on the same source bytes at B = P: alternating blocks in
          one process, device events around back-to-back calls; each launch alone comes from
          `rocprofv3 --kernel-trace --stats -- python profiles/tools/page_split_step.py --parts kernel`
  step    `r.step()` of an InferenceRunner(assemble=True) of batch 24 alone and after `sp.run()` into its input_images

It prints what it measures, one JSON line per measurement, and writes the tables to --out; no time is fixed in advance.

    python profiles/tools/page_split_step.py [--steps 40] [--warmup 10] [--parts groups,kernel,step] [--out profiles/r27_page_split.md]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scan_step as r13  # noqa: E402  (puts the repository root on sys.path)

sys.path.insert(0, os.path.join(r13.ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import page_split_oracle as po  # noqa: E402
from abcnet_amd.augment import DEFAULT_SPLIT_CELL, DEFAULT_SPLIT_REACH, PageSplitter, ScanBuilder  # noqa: E402
from abcnet_amd.infer import InferenceRunner  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402

S, P, PER_PAGE = 512, 6, 4
D = P * PER_PAGE
PAPER, INK = r13.PAPER, r13.INK
GUTTER, CAPTIONS_BELOW, LETTER, LETTERS = 160, (96, 160), (14, 9), 10
MAX_SRC = (2 * (S + max(CAPTIONS_BELOW) + LETTER[0]) + 3 * GUTTER, 2 * S + 3 * GUTTER)
SETTINGS = [(8, 4)] + [(cell, reach) for cell in (16, 32, 64) for reach in (1, 2, 3, 4)]


def make_pages(x, caption_below):
    """(pages uint8, per drawing (page, boolean mask of its ink on the page)), the captions caption_below pixels under the frames"""
    pages, truth = [], []
    slot_h = S + caption_below + LETTER[0]                    # a drawing's frame and its caption
    shape = (2 * slot_h + 3 * GUTTER, MAX_SRC[1])
    for p in range(P):
        page = np.full(shape, PAPER, dtype=np.uint8)
        for k in range(PER_PAGE):
            y, x0 = GUTTER + (k // 2) * (slot_h + GUTTER), GUTTER + (k % 2) * (S + GUTTER)
            ink = np.asarray(x[p * PER_PAGE + k, 0]) > 0
            page[y:y + S, x0:x0 + S][ink] = INK
            mask = np.zeros(shape, dtype=bool)
            mask[y:y + S, x0:x0 + S] = ink
            truth.append((p, mask))
            for i in range(LETTERS):
                cx = x0 + 120 + i * (LETTER[1] + 8)
                page[y + S + caption_below:y + slot_h, cx:cx + LETTER[1]] = INK
        pages.append(page)
    return pages, truth


def part_groups(pages, truth, caption_below):
    rows = []
    for cell, reach in SETTINGS:
        sp = PageSplitter(P, 1024, 64, max_src=MAX_SRC, max_per_page=64, cell=cell, reach=reach, debug_cells=True)
        sp.load(pages)
        sp.run()
        labels, _ = sp.cells()
        dr, pg = sp.drawings(), sp.pages()
        weight = {(int(r["page"]), int(r["label"])): int(r["weight"]) for r in dr if r["page"] >= 0}
        agree, truly = True, {}
        for p, page in enumerate(pages):
            _, _, _, _, lab, w = po.analyse(page, 0, cell, reach, (sp.max_h, sp.pitch))
            agree &= bool(np.array_equal(lab, labels[p])) and all(weight.get((p, k), v) == v for k, v in w.items())
            truly.update({(p, k): v for k, v in w.items()})
        agree &= int(sp.total[1]) == len(truly)
        weight = truly
        whole = split = merged = 0
        for p, mask in truth:
            cells = po.co.cell_ink(mask, cell) > 0
            own = set(labels[p][:cells.shape[0], :cells.shape[1]][cells].tolist())
            held = sum(weight[(p, k)] for k in own)
            split += len(own) > 1
            merged += held > int(mask.sum())
            whole += len(own) == 1 and held == int(mask.sum())
        rec = {"part": "groups", "caption_below": caption_below, "cell": cell, "reach": reach, "drawings": len(truth), "whole": int(whole), "split": int(split),
               "merged": int(merged), "groups_kept": int(pg["kept"].sum()), "pages_full": int((pg["status"] != 0).sum()),
               "device_agrees_with_oracle": agree}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del sp
    return rows


def _blocks(forms, iters=50):
    res = {}
    names = list(forms)
    for blk in range(4):
        for name in (names if blk % 2 == 0 else names[::-1]):
            f = forms[name]
            for _ in range(10):
                f()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(name, []).append(e0.elapsed_time(e1) * 1000 / iters)
    return {k: statistics.median(v) for k, v in res.items()}


def part_kernel(pages):
    rows = []
    for cell, reach in ((16, 2), (32, 1), (32, 2), (32, 4), (64, 1)):
        clean = ScanBuilder(P, S, max_src=MAX_SRC, clean_cell=cell)
        sp = PageSplitter(P, D, S, max_src=MAX_SRC, cell=cell, reach=reach)
        for b in (clean, sp):
            b.load(pages)
        med = _blocks({"clean": clean.run, "split": sp.run})
        rec = {"part": "kernel", "cell": cell, "reach": reach, "pages": P, "canvases": D, "size": S,
               "source_bytes": sum(int(p.size) for p in pages), "clean_builder_us": round(med["clean"], 2),
               "splitter_us": round(med["split"], 2), "splitter_over_clean": round(med["split"] / med["clean"], 3),
               "canvases_written": int(sp.total[0]), "method": "device events around 50 back-to-back runs, 4 alternating blocks (gaps included)"}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del clean, sp
    return rows


def part_step(pages, steps, warmup):
    m = r13.model()
    r = InferenceRunner(m, D, S, S, use_graph=True, assemble=True)
    sp = PageSplitter(P, D, S, out=r.input_images, max_src=MAX_SRC)
    sp.load(pages)
    sp.run()

    def both():
        sp.run()
        r.step()
    for f in (r.step, both):
        for _ in range(warmup):
            f()
    med = _blocks({"r.step()": r.step, "sp.run(); r.step()": both}, iters=max(steps // 4, 1))
    rec = {"part": "step", "batch": D, "size": S, "cell": DEFAULT_SPLIT_CELL, "reach": DEFAULT_SPLIT_REACH,
           "runner_step_us": round(med["r.step()"], 1), "with_splitter_us": round(med["sp.run(); r.step()"], 1),
           "added_us": round(med["sp.run(); r.step()"] - med["r.step()"], 1)}
    print(json.dumps(rec), flush=True)
    return rec


def choose(groups):
    """the (cell, reach) with the fewest merged drawings over all the page sets (a caption drawn into a canvas cannot be taken out
    again downstream, while a drawing in pieces shows in the counts), then the most whole, then the smaller cell and reach"""
    keys = sorted({(g["cell"], g["reach"]) for g in groups})
    tot = {k: [sum(g[c] for g in groups if (g["cell"], g["reach"]) == k) for c in ("whole", "merged")] for k in keys}
    return max(keys, key=lambda k: (-tot[k][1], tot[k][0], -k[0], -k[1])), tot


def write_report(path, groups, kernel, step):
    out = ["# r27: a page scan into its drawings (abc_split_scan_pages)", "",
           "Written by `profiles/tools/page_split_step.py`.  No real page was available: %d pages, each a 2 x 2 sheet of" % P,
           "`drawn_molecules(24, 512, seed=777)` drawings, %d pixels of paper between and around them, a caption of %d blobs of"
           % (GUTTER, LETTERS),
           "%d x %d under each, %s pixels below its frame.  These drawings are sparse: fragments of one drawing lie up to about a"
           % (LETTER[0], LETTER[1], " or ".join(str(c) for c in CAPTIONS_BELOW)),
           "hundred pixels apart.  whole: one group holds exactly the drawing's ink; split: its ink lies in more than one group;",
           "merged: a group of it holds other ink too (here always its caption).  The device's cell tables were compared with",
           "`tests/page_split_oracle.py`'s on the same pages before counting.", ""]
    if groups:
        out += ["| caption below | cell | reach | whole | split | merged | groups kept | pages with a status | device = oracle |",
                "|---|---|---|---|---|---|---|---|---|"]
        out += ["| %d | %d | %d | %d / %d | %d | %d | %d | %d | %s |" % (g["caption_below"], g["cell"], g["reach"], g["whole"], g["drawings"],
                                                                        g["split"], g["merged"], g["groups_kept"], g["pages_full"],
                                                                        g["device_agrees_with_oracle"]) for g in groups]
        best, tot = choose(groups)
        out += ["", "Fewest merged drawings over both page sets, then most whole, then the smaller cell and reach: cell %d, reach %d"
                % best, "(%d whole, %d merged of %d).  `augment.DEFAULT_SPLIT_CELL`, `DEFAULT_SPLIT_REACH` at the time of this run: %d, %d."
                % (tot[best][0], tot[best][1], len(CAPTIONS_BELOW) * D, DEFAULT_SPLIT_CELL, DEFAULT_SPLIT_REACH), ""]
    if kernel:
        out += ["The launch sequence alone against `abc_build_scan_images_clean` on the same source bytes (B = P = %d, pages of %d x %d;"
                % (P, MAX_SRC[0], MAX_SRC[1]), "the splitter writes %d canvases of %d x %d, the clean builder %d), microseconds per run:"
                % (D, S, S, P), "", "| cell | reach | clean builder | splitter | ratio | canvases written |", "|---|---|---|---|---|---|"]
        out += ["| %d | %d | %.1f | %.1f | %.2f | %d |" % (k["cell"], k["reach"], k["clean_builder_us"], k["splitter_us"], k["splitter_over_clean"],
                                                        k["canvases_written"]) for k in kernel]
        out += ["", "(%s)" % kernel[0]["method"], ""]
    if step:
        out += ["The runner step (InferenceRunner(assemble=True), batch %d, %d x %d, captured graph) alone and after `sp.run()`:" % (D, S, S),
                "%.1f us and %.1f us: %.1f us added." % (step["runner_step_us"], step["with_splitter_us"], step["added_us"]), ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="groups,kernel,step")
    ap.add_argument("--out", default=os.path.join(r13.ROOT, "profiles", "r27_page_split.md"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    x, _ = drawn_molecules(D, S, seed=777)
    sets = {c: make_pages(x, c) for c in CAPTIONS_BELOW}
    pages = sets[max(CAPTIONS_BELOW)][0]
    print(json.dumps({"part": "pages", "pages": P, "capacity": list(MAX_SRC), "drawings": D}), flush=True)
    groups = kernel = step = None
    if "groups" in parts:
        groups = [r for c, (pg, truth) in sets.items() for r in part_groups(pg, truth, c)]
        print(json.dumps({"part": "groups", "chosen": list(choose(groups)[0])}), flush=True)
    if "kernel" in parts:
        kernel = part_kernel(pages)
    if "step" in parts:
        step = part_step(pages, a.steps, a.warmup)
    if groups and kernel and step:
        write_report(a.out, groups, kernel, step)


if __name__ == "__main__":
    main()
