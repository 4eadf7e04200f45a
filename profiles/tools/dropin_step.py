"""Time the reference training loop (train.py:94-141) on the drop-in UNet three ways, one process, same box:

  literal  model(imgs) -> oracle.loss_oracle.abc_loss (the repo's restatement of train.py:95-137 as torch ops)
           -> backward -> torch.optim.Adam(lr=2.5e-4, weight_decay=1e-8)
  dropin   model(imgs) -> abcnet_amd.loss.abc_loss -> backward -> abcnet_amd.optim.Adam (same settings)
  trainer  abcnet_amd.train.Trainer.step() (fused heads, hipGraph) -- the path every published number uses

Median and mean of per-step device time (CUDA events around each step; no host sync inside a step) after warm-up, and img/s
from the median.  One JSON line per mode.

    python profiles/tools/dropin_step.py [--batch 16] [--size 384] [--dtype bf16] [--steps 50] [--warmup 10] [--modes literal,dropin,trainer]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.loss import abc_loss  # noqa: E402
from abcnet_amd.optim import Adam  # noqa: E402
from abcnet_amd.synthetic import synthetic_images, synthetic_targets  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402
from oracle import loss_oracle  # noqa: E402

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--modes", default="literal,dropin,trainer")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    x = synthetic_images(a.batch, a.size, seed=7).to(dev)
    tg = [t.to(dev) for t in synthetic_targets(a.batch, a.size // 4, seed=1)]
    for mode in a.modes.split(","):
        torch.manual_seed(0)
        m = UNet(1, HEADS, dtype=a.dtype).to(dev)
        m.train()
        if mode == "trainer":
            from abcnet_amd.train import Trainer
            tr = Trainer(m, a.batch, a.size, a.size, lr=2.5e-4, weight_decay=1e-8)
            tr.load_batch(x, tg)
            step = tr.step
        else:
            opt = (torch.optim.Adam if mode == "literal" else Adam)(m.parameters(), lr=2.5e-4, weight_decay=1e-8)
            lossf = (lambda p: loss_oracle.abc_loss(p, tg, m.s)[0]) if mode == "literal" else (lambda p: abc_loss(p, tg, m.s))

            def step():
                loss = lossf(m(x))
                opt.zero_grad()
                loss.backward()
                opt.step()
        times = []
        for k in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            if k >= a.warmup:
                times.append((e0, e1))
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in times]
        med = statistics.median(ms)
        print(json.dumps({"mode": mode, "batch": a.batch, "size": a.size, "dtype": a.dtype, "steps": a.steps, "warmup": a.warmup,
                          "ms_per_step_median": round(med, 4), "ms_per_step_mean": round(statistics.fmean(ms), 4),
                          "ms_min": round(min(ms), 4), "img_per_s": round(a.batch * 1000.0 / med, 1)}), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
