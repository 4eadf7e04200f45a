"""The evaluation tables (csrc/eval_tables.hip, ops.EvalTables, InferenceRunner(evaluate=True)) measured five ways, one process,
b64 @ 512 x 512 bf16 (128 x 128 maps), synthetic targets of 30 atoms and 32 bonds per image (step, kernel, torch) or the
annotation records of synthetic.drawn_molecules, the repo's molecule generator (sparse, loop):

  step    InferenceRunner.step() with and without evaluate=True (captured graphs, alternating blocks, median per-step device time)
  kernel  the evaluation launch sequence alone (device events around back-to-back launches after a warm-up, so launch gaps count),
          with the bytes of the target planes it has to read over that time
  torch   the oracle's torch restatement of test_accuracy.py:105-269 (tests/evaltab_oracle.py) on the same DEVICE tensors: the
          reference's own way, about 330 reductions each followed by a host read
  sparse  the evaluation launch sequence alone, abc_eval_tables_update against abc_eval_tables_update_sparse on the SAME maps
          (drawn by TargetRasterizer(sparse=True) from the generator's records): a device event pair around every update,
          alternating blocks of the two forms, median; the results are compared bit for bit on the way
  loop    one evaluation batch end to end, wall clock with a device sync per batch, two ways:
            dense    the eight dense maps in pinned host memory -> load_batch(imgs, targets) -> step()   (the host rasteriser that
                     has to build those maps first, utils.py:83-228, is NOT in the figure)
            records  uint8 renders and annotation strings -> SampleBuilder.load() / run() -> step()       (parsing included)

One JSON line per measurement.

    python profiles/tools/evaltab_step.py [--batch 64] [--size 512] [--steps 40] [--warmup 10] [--parts step,kernel,torch,sparse,loop]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.infer import InferenceRunner  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules, synthetic_images, synthetic_targets  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402
import evaltab_oracle as eo  # noqa: E402

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="step,kernel,torch")
    a = ap.parse_args()
    parts = a.parts.split(",")
    B, S = a.batch, a.size
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = UNet(1, HEADS, dtype="bf16").to(dev)
    x = synthetic_images(B, S, seed=7).to(dev)
    # (eight distinct images' targets, repeated: drawing 64 on the host takes longer than everything measured here)
    tg = [t.repeat((B + 7) // 8, *([1] * (t.dim() - 1)))[:B].contiguous().to(dev) for t in synthetic_targets(min(B, 8), S // 4, seed=3)]
    ev = InferenceRunner(m, B, S, S, use_graph=True, evaluate=True)
    ev.load_batch(x, tg)
    if "step" in parts:
        plain = InferenceRunner(m, B, S, S, use_graph=True)
        plain.load_batch(x)
        forms = {"step()": plain.step, "step(), evaluate=True": ev.step}
        for f in forms.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for blk in range(4):
            for name, f in (forms.items() if blk % 2 == 0 else reversed(list(forms.items()))):
                marks = []
                for _ in range(a.steps // 4):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    marks.append((e0, e1))
                torch.cuda.synchronize()
                times[name] += [p.elapsed_time(q) for p, q in marks]
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            print(json.dumps({"part": "step", "form": k, "batch": B, "size": S, "steps": len(v), "ms_per_step_median": round(med[k], 4),
                              "ms_min": round(min(v), 4), "img_per_s": round(B * 1000.0 / med[k], 1)}), flush=True)
        print(json.dumps({"part": "step", "added_ms": round(med["step(), evaluate=True"] - med["step()"], 4),
                          "evaluate_over_plain": round(med["step(), evaluate=True"] / med["step()"], 4)}), flush=True)
        del plain
    else:
        ev.step()
    if "kernel" in parts:
        et = ev.evaluator
        for _ in range(a.warmup):
            et.run()
        torch.cuda.synchronize()
        iters = a.steps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            et.run()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        nbytes = sum(t.numel() * t.element_size() for t in tg) - tg[6].numel() * 8      # (the rho target is read where a bin has mass only)
        print(json.dumps({"part": "kernel", "batch": B, "size": S, "ms_per_update": round(ms, 4), "target_bytes": nbytes,
                          "TB_per_s": round(nbytes / ms / 1e9, 3),
                          "method": "device events around %d back-to-back updates (3 launches each, gaps included)" % iters}), flush=True)
    if "torch" in parts:
        lg = [t for t in ev.logits]
        eo.evaluate(lg, tg, confusion=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            eo.evaluate(lg, tg, confusion=False)
        torch.cuda.synchronize()
        print(json.dumps({"part": "torch", "batch": B, "size": S, "ms_per_batch": round((time.perf_counter() - t0) * 1000 / reps, 2),
                          "method": "wall clock, tests/evaltab_oracle.evaluate on the device tensors, %d repetitions after one warm-up" % reps}),
              flush=True)
    if "sparse" in parts or "loop" in parts:
        records_parts(a, parts, ev, x)


def records_parts(a, parts, ev, x):
    """the `sparse` and `loop` parts: both run on the records of synthetic.drawn_molecules"""
    import numpy as np
    from abcnet_amd.augment import SampleBuilder
    from abcnet_amd.ops import EvalTables
    B, S = a.batch, a.size
    # (eight distinct molecules, repeated: the generator is host code)
    imgs, ann = drawn_molecules(min(B, 8), S, seed=5)
    renders = [np.ascontiguousarray(255 - 255 * imgs[b % len(ann), 0].numpy().astype(np.uint8)) for b in range(B)]
    atoms_s, bonds_s = [ann[b % len(ann)][0] for b in range(B)], [ann[b % len(ann)][1] for b in range(B)]
    n_items = (sum(len(s.split(";")) - 1 for s in atoms_s) / B, sum(len(s.split(";")) - 1 for s in bonds_s) / B)
    sb = SampleBuilder(ev, amount=0.1, max_src=(S, S), sparse=True)      # (registers its rasteriser: ev evaluates sparsely from here on)
    rng = np.random.RandomState(0)
    sb.load(renders, atoms_s, bonds_s, rng)
    sb.run()
    ev.step()
    torch.cuda.synchronize()
    flags = sb.raster.group_flags
    fl = flags.cpu()
    groups = {"groups": fl.numel(), "no_bit": int((fl == 0).sum()), "atom_bits": int(((fl & 0x0F) != 0).sum()), "bond_bits": int(((fl & 0xF0) != 0).sum())}
    if "sparse" in parts:
        old = ev.evaluator
        mk = lambda f: EvalTables(*old.keep[:4], old.keep[4], old.keep[5], btype_idx=old.keep[6], n_valid=old.keep[7], target_flags=f)  # noqa: E731
        forms = {"dense": mk(None), "sparse": mk(flags)}
        for f in forms.values():
            for _ in range(a.warmup):
                f.run()
        torch.cuda.synchronize()
        same = all(torch.equal(getattr(forms["dense"], k), getattr(forms["sparse"], k)) for k in ("counts_last", "meters_last"))
        times = {k: [] for k in forms}
        for blk in range(4):
            for name, f in (forms.items() if blk % 2 == 0 else reversed(list(forms.items()))):
                marks = []
                for _ in range(a.steps // 4):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f.run()
                    e1.record()
                    marks.append((e0, e1))
                torch.cuda.synchronize()
                times[name] += [p.elapsed_time(q) for p, q in marks]
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            print(json.dumps({"part": "sparse", "form": k, "batch": B, "size": S, "updates": len(v), "ms_per_update_median": round(med[k], 4),
                              "ms_min": round(min(v), 4)}), flush=True)
        print(json.dumps(dict({"part": "sparse", "sparse_over_dense": round(med["sparse"] / med["dense"], 4), "bit_identical": same,
                               "atoms_per_image": n_items[0], "bonds_per_image": n_items[1],
                               "method": "device event pair around every update (3 launches), alternating blocks"}, **groups)), flush=True)
    if "loop" in parts:
        reps = max(4, a.steps // 4)

        def wall(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1000)
            return ts

        def records_loop():
            sb.load(renders, atoms_s, bonds_s, rng)
            sb.run()
            ev.step()

        t_rec = wall(records_loop)
        # the parent interface: dense maps (here: the ones the rasteriser just drew, copied out once) in pinned host memory
        h_tg = [t.cpu().pin_memory() for t in ev.targets]
        h_x = x.cpu().pin_memory()
        ev.use_sparse_targets(None)

        def dense_loop():
            ev.load_batch(h_x, h_tg)
            ev.step()

        t_den = wall(dense_loop)
        nbytes = sum(t.numel() * t.element_size() for t in h_tg)
        for name, ts, note in (("dense", t_den, "pinned dense maps -> load_batch -> step; the host rasteriser is not included"),
                               ("records", t_rec, "uint8 renders + annotation strings -> SampleBuilder.load / run -> step; parsing included")):
            print(json.dumps({"part": "loop", "form": name, "batch": B, "size": S, "batches": len(ts), "ms_per_batch_median": round(statistics.median(ts), 3),
                              "ms_min": round(min(ts), 3), "method": "wall clock, device sync per batch; " + note}), flush=True)
        print(json.dumps({"part": "loop", "dense_target_bytes": nbytes, "records_over_dense": round(statistics.median(t_rec) / statistics.median(t_den), 4)}),
              flush=True)


if __name__ == "__main__":
    main()
