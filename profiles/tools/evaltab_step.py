"""The evaluation tables (csrc/eval_tables.hip, ops.EvalTables, InferenceRunner(evaluate=True)) measured three ways, one process,
b64 @ 512 x 512 bf16 (128 x 128 maps), synthetic targets of 30 atoms and 32 bonds per image:

  step    InferenceRunner.step() with and without evaluate=True (captured graphs, alternating blocks, median per-step device time)
  kernel  the evaluation launch sequence alone (device events around back-to-back launches after a warm-up, so launch gaps count),
          with the bytes of the target planes it has to read over that time
  torch   the oracle's torch restatement of test_accuracy.py:105-269 (tests/evaltab_oracle.py) on the same DEVICE tensors: the
          reference's own way, about 330 reductions each followed by a host read

One JSON line per measurement.

    python profiles/tools/evaltab_step.py [--batch 64] [--size 512] [--steps 40] [--warmup 10] [--parts step,kernel,torch]
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
from abcnet_amd.synthetic import synthetic_images, synthetic_targets  # noqa: E402
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


if __name__ == "__main__":
    main()
