"""The bf16 gradient exchange (csrc/exchange.hip, GradReducer(mode="direct", wire_dtype="bf16")) measured on ONE GPU, one fresh
process: backend nccl, world 1, the exchange forced on (Trainer(force_exchange=True)), as tests/rccl_world1_worker.py does.

  step     ms per step at b16 @ 384^2 bf16 (8 MB buckets) for the plain Trainer, exchange="direct" in f32 and exchange="direct",
           exchange_dtype="bf16": alternating blocks, median per-step device time.  At world 1 nothing crosses a link: this is what
           the three extra launches per bucket and the bf16 collectives cost when there is nothing to exchange.
  kernels  abc_grad_pack_bf16 / abc_grad_reduce_bf16 (W = 1, 2, 4, 8 rows of bucket / W elements) / abc_grad_unpack_bf16 alone at
           every bucket size of that plan: HIP events around back-to-back launches, median of the repeats, the bytes the kernel must
           move and the fraction of the 8.0 TB/s HBM peak that implies.  "hot": the same buffers every launch (a bucket fits the
           last-level cache); "rotated": every launch on another of enough copies to exceed it (> 512 MB): the HBM figure.
           Back-to-back launches from Python come ~5 us apart, which is longer than these kernels run at every bucket size of the
           plan: the event figures are then the launch cadence, an upper bound of the kernel time.  The kernels' own times:
           `rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/tools/exchange_step.py --parts kernels --buffers rotated`,
           then `python profiles/tools/exchange_step.py --trace DIR/.../*_kernel_trace.csv` (no GPU needed): median duration per
           kernel and grid, with the bytes and rates that follow.
  wire     GradReducer.wire_bytes_per_step() of that plan for W = 2, 4, 8, f32 and bf16: ARITHMETIC, not a measurement -- no number
           exists for W > 1.

One JSON line per measurement.  On a tree without the bf16 exchange the forms it lacks are left out (the A/B against an older tree).

    python profiles/tools/exchange_step.py [--steps 60] [--warmup 10] [--parts step,kernels,wire] [--buffers hot,rotated]
    python profiles/tools/exchange_step.py --trace KERNEL_TRACE_CSV
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import distributed as D  # noqa: E402
from abcnet_amd.synthetic import synthetic_images, synthetic_targets  # noqa: E402
from abcnet_amd.train import Trainer  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]
B, S = 16, 384
HBM_PEAK = 8.0e12
HAS_BF16 = hasattr(D.GradReducer, "WIRE_DTYPES")


def make_trainer(dev, x, tg, **kw):
    m = UNet(1, HEADS, dtype="bf16")
    m.reset_parameters(seed=1)
    m = m.to(dev)
    tr = Trainer(m, B, S, S, use_graph=True, bucket_mb=8.0, **kw)
    tr.load_batch(x, tg)
    return tr


def part_step(dev, x, tg, steps, warmup):
    forms = {"plain": {}, "direct f32": {"exchange": "direct", "force_exchange": True}}
    if HAS_BF16:
        forms["direct bf16"] = {"exchange": "direct", "force_exchange": True, "exchange_dtype": "bf16"}
    trs = {k: make_trainer(dev, x, tg, **kw) for k, kw in forms.items()}
    for tr in trs.values():
        for _ in range(warmup):
            tr.step()
    torch.cuda.synchronize()
    times = {k: [] for k in trs}
    for blk in range(4):
        order = list(trs.items()) if blk % 2 == 0 else list(reversed(list(trs.items())))
        for name, tr in order:
            ev = []
            for _ in range(max(steps // 4, 1)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.step()
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            times[name] += [a.elapsed_time(b) for a, b in ev]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, tr in trs.items():
        r = tr.reducer
        print(json.dumps({"part": "step", "form": k, "batch": B, "size": S, "steps": len(times[k]), "ms_per_step_median": round(med[k], 4),
                          "ms_min": round(min(times[k]), 4), "over_plain": round(med[k] / med["plain"], 4), "mode": r.mode if r.active else None,
                          "wire_dtype": getattr(r, "wire_dtype", "f32"), "fallback": r.fallback_reason, "buckets": len(tr.buckets),
                          "segments": len(tr._segments)}), flush=True)
    return trs


def time_launches(launch, nbuf, iters=20, repeats=15):
    """median over `repeats` of the device time per launch of `iters` back-to-back launches; launch(i) uses buffer set i % nbuf"""
    for i in range(max(nbuf, 4)):
        launch(i)
    torch.cuda.synchronize()
    us = []
    k = 0
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            launch(k)
            k += 1
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1000 / iters)
    return statistics.median(us), min(us)


def part_kernels(dev, sizes, buffers=("hot", "rotated")):
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    for total in sizes:
        ncopy = min(4096, max(2, -(-(512 << 20) // (total * 6))))      # rotated: more than 512 MB of f32 + bf16 buffers in all (4096 sets at most)
        f32 = torch.randn(ncopy, total, device=dev)
        h16 = torch.empty(ncopy, total, dtype=torch.bfloat16, device=dev)
        o16 = torch.empty(ncopy, total, dtype=torch.bfloat16, device=dev)
        for i in range(ncopy):
            L.check(lib.abc_grad_pack_bf16(f32[i].data_ptr(), h16[i].data_ptr(), total, st), "pack")
        cases = [("pack", None, 6 * total, lambda i: lib.abc_grad_pack_bf16(f32[i].data_ptr(), h16[i].data_ptr(), total, st)),
                 ("unpack", None, 6 * total, lambda i: lib.abc_grad_unpack_bf16(h16[i].data_ptr(), f32[i].data_ptr(), total, st))]
        for w in (1, 2, 4, 8):
            n = total // w
            cases.append(("reduce", w, 2 * (w + 1) * n, lambda i, w=w, n=n: lib.abc_grad_reduce_bf16(h16[i].data_ptr(), o16[i].data_ptr(), w, n, st)))
        for name, w, nbytes, fn in cases:
            row = {"part": "kernels", "kernel": name, "W": w, "bucket_elems": total, "bytes": nbytes}
            for label, nbuf in (("hot", 1), ("rotated", ncopy)):
                if label not in buffers:
                    continue
                med, best = time_launches(lambda i, fn=fn, nbuf=nbuf: L.check(fn(i % nbuf), name), nbuf)
                row["%s_us" % label] = round(med, 2)
                row["%s_us_min" % label] = round(best, 2)
                row["%s_TB_per_s" % label] = round(nbytes / med / 1e6, 3)
                row["%s_of_hbm_peak" % label] = round(nbytes / (med * 1e-6) / HBM_PEAK, 3)
            row["method"] = "device events around 20 back-to-back launches (launch gaps included), median of 15; rotated over %d buffer sets" % ncopy
            print(json.dumps(row), flush=True)
        del f32, h16, o16
        torch.cuda.empty_cache()


def part_wire(trs):
    for k, tr in trs.items():
        if k == "plain":
            continue
        r = tr.reducer
        print(json.dumps({"part": "wire", "form": k, "store_elems": sum(hi - lo for lo, hi, _ in tr.buckets),
                          "bytes_per_step": {"W=%d" % w: r.wire_bytes_per_step(world=w) for w in (2, 4, 8)},
                          "note": "arithmetic on the plan, (W-1)/W x elements x bytes on each of the two legs; nothing here was measured at W > 1"}),
              flush=True)


def reduce_trace(path):
    """a rocprofv3 kernel-trace csv of `--parts kernels` -> one JSON line per (kernel, grid): launches, median / min duration, and for
    the grids this tool launches (one thread per 8 elements, whole workgroups of 256) the bytes and rate that follow"""
    import csv
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            kind = next((k for k in ("unpack_bf16", "pack_bf16", "reduce_bf16") if k + "_kernel" in name), None)
            if kind is None:
                continue
            rows.setdefault((kind, int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"])), []).append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    for (kind, grid), us in sorted(rows.items()):
        med = statistics.median(us)
        print(json.dumps({"part": "trace", "kernel": kind, "grid_threads": grid, "launches": len(us), "us_median": round(med, 2),
                          "us_min": round(min(us), 2), "elements_at_most": grid * 8}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="step,kernels,wire")
    ap.add_argument("--buffers", default="hot,rotated")
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        return reduce_trace(a.trace)
    parts = a.parts.split(",")
    os.environ.setdefault("MASTER_PORT", str(D.free_port()))
    rank, world = D.init_process_group(backend="nccl")
    assert (rank, world) == (0, 1)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = synthetic_images(B, S, seed=7).to(dev)
    tg = [t.to(dev) for t in synthetic_targets(B, S // 4, seed=1)]
    if "step" in parts:
        trs = part_step(dev, x, tg, a.steps, a.warmup)
    else:
        trs = {"direct f32": make_trainer(dev, x, tg, exchange="direct", force_exchange=True)}
        if HAS_BF16:
            trs["direct bf16"] = make_trainer(dev, x, tg, exchange="direct", force_exchange=True, exchange_dtype="bf16")
    if "wire" in parts and HAS_BF16:
        part_wire(trs)
    if "kernels" in parts and HAS_BF16:
        sizes = sorted(set(hi - lo for lo, hi, _ in trs["direct bf16"].buckets))
        del trs
        torch.cuda.empty_cache()
        part_kernels(dev, sizes, tuple(a.buffers.split(",")))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
