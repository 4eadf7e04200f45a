"""The input-image builder (csrc/augment.hip, abcnet_amd.augment) measured three ways, one process:

  host    ms per image on one host thread: the numpy restatement of utils.py:42-81's image half (resize when drawn, canvas,
          threshold, the two 512 x 512 np.random noise fields) against what the device path leaves on the host (draw_augment,
          parse_record and the staging memcpy of SampleBuilder.load)
  kernel  abc_build_images alone (device events around back-to-back launches, so launch gaps count) at b16 @ 384^2 and b64 @ 512^2,
          with the bytes it must move (uint8 sources read + f32 batch written) over that time; the kernel's own time comes from
          `rocprofv3 --kernel-trace --stats -- python profiles/tools/augment_step.py --parts kernel`
  step    `rz.run(); tr.step()` (targets rasterised on the device, images resident) against `sb.run(); tr.step()` (targets AND images
          built on the device) at b16 @ 384^2 bf16, alternating blocks, median per-step device time

One JSON line per measurement.

    python profiles/tools/augment_step.py [--steps 40] [--warmup 10] [--parts host,kernel,step]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.augment import ImageBuilder, SampleBuilder, draw_augment  # noqa: E402
from abcnet_amd.raster import parse_record  # noqa: E402
from abcnet_amd.synthetic import random_annotations  # noqa: E402
import augment_oracle as ao  # noqa: E402

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]


def host_numpy_image(src, rs, amount=0.1, S=512):
    """utils.py:42-81's image half restated in numpy (the resize is the oracle's INTER_LINEAR)"""
    img = src.astype(np.float32)
    rows, cols = img.shape
    if rs.rand() < 0.2:
        if rs.rand() < 0.5:
            rows, cols = int(rs.uniform(0.8, 1) * S), S
        else:
            rows, cols = S, int(rs.uniform(0.8, 1) * S)
        img = ao.resize_linear(img, rows, cols)
    canvas = np.full((S, S), 255, dtype=np.float32)
    ddx, ddy = (S - rows) // 2, (S - cols) // 2
    canvas[ddx:ddx + rows, ddy:ddy + cols] = img
    ink = (canvas / 255) < 0.6
    salt = rs.uniform(0, 1, ink.shape) < rs.uniform(0, amount / 100)
    ink = np.logical_or(ink, salt)
    pepper = rs.uniform(0, 1, ink.shape) < rs.uniform(0, amount)
    out = np.zeros([1, S, S], dtype=np.float32)
    out[0] = 1 - np.logical_or(1 - ink, pepper)
    return out


def part_host(n=24):
    torch.set_num_threads(1)
    S = 512
    srcs = [ao.fixture_render(10 + i, S, S) for i in range(4)]
    rs = np.random.RandomState(0)
    host_numpy_image(srcs[0], rs)
    t0 = time.perf_counter()
    for i in range(n):
        host_numpy_image(srcs[i % 4], rs)
    t_np = (time.perf_counter() - t0) * 1000 / n
    ann = [random_annotations(30, 32, 900 + i, size=400) for i in range(16)]
    ib = ImageBuilder(16, S, "train", max_src=(S, S))
    t0 = time.perf_counter()
    reps = 4
    for _ in range(reps):
        draws = [draw_augment(rs, 0.1, srcs[i % 4].shape, S) for i in range(16)]
        [parse_record(a, q, *offs, h=S // 4) for (a, q), (_, offs) in zip(ann, draws)]
        ib.load([srcs[i % 4] for i in range(16)], [d for d, _ in draws])
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) * 1000 / (reps * 16)
    print(json.dumps({"part": "host", "numpy_ms_per_image": round(t_np, 3), "device_path_host_ms_per_image": round(t_dev, 4),
                      "note": "one host thread; device path = draw_augment + parse_record (30 atoms, 32 bonds) + staging memcpy"}), flush=True)


def part_kernel(iters=200):
    for B, S in ((16, 384), (64, 512)):
        rs = np.random.RandomState(1)
        srcs = [ao.fixture_render(20 + i, S, S) for i in range(4)]
        ib = ImageBuilder(B, S, "train", max_src=(S, S))
        draws = [draw_augment(rs, 0.1, (S, S), S)[0] for _ in range(B)]
        ib.load([srcs[i % 4] for i in range(B)], draws)
        for _ in range(20):
            ib.run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            ib.run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000 / iters
        nbytes = B * S * S * (4 + 1)
        print(json.dumps({"part": "kernel", "batch": B, "size": S, "us_per_launch": round(us, 2), "bytes": nbytes,
                          "TB_per_s": round(nbytes / us / 1e6, 3), "resized_images": sum(d.rows != S or d.cols != S for d in draws),
                          "method": "device events around %d back-to-back launches (launch gaps included; kernel time alone: run "
                                    "--parts kernel under rocprofv3 --kernel-trace)" % iters}),
              flush=True)


def part_step(steps, warmup):
    from abcnet_amd.train import Trainer
    from abcnet_amd.unet import UNet
    B, S = 16, 384
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = UNet(1, HEADS, dtype="bf16").to(dev)
    tr = Trainer(m, B, S, S)
    sb = SampleBuilder(tr, amount=0.1, max_src=(S, S), sparse=True, max_atoms=64, max_bonds=64)
    srcs = [ao.fixture_render(30 + i, S, S) for i in range(B)]
    ann = [random_annotations(30, 32, 900 + i, size=300) for i in range(B)]
    sb.load(srcs, [a for a, _ in ann], [q for _, q in ann], np.random.RandomState(2))
    rz = sb.raster

    def with_raster():
        rz.run()
        tr.step()

    def with_sample():
        sb.run()
        tr.step()
    forms = {"rz.run(); tr.step()": with_raster, "sb.run(); tr.step()": with_sample}
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
                          "ms_min": round(min(v), 4), "img_per_s": round(B * 1000.0 / med[k], 1)}), flush=True)
    a, b = med["rz.run(); tr.step()"], med["sb.run(); tr.step()"]
    print(json.dumps({"part": "step", "sample_over_raster": round(b / a, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="host,kernel,step")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if "host" in parts:
        part_host()
    if "kernel" in parts:
        part_kernel()
    if "step" in parts:
        part_step(a.steps, a.warmup)


if __name__ == "__main__":
    main()
