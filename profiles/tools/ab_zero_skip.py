"""A/B of the fused heads pass's zero skip on the step bench.py times, through the Trainer's constructor argument (one process, the
forms alternating; run from the repository root on the GPU box):

    python profiles/tools/ab_zero_skip.py [--forms full,tiles,skip] [--rounds 5] [--steps 30] [--warmup 5] [--raster] [--variant unet2]
                                          [--no-graph] [--only FORM]

  full   Trainer(zero_skip=False): every row tile takes the loss arithmetic and is stored (abc_heads_fused_desc.no_zero_skip = 1)
  tiles  the skip of the arithmetic alone: dl_tiles taken out of the descriptor, so tiles without a target are stored as zeros and the
         conv2 weight gradient reads them all
  skip   the default: with the tile mask, unflagged tiles neither stored nor read

Prints the tile mask's occupancy of the batch and, per form, every round's ms per step.  --only FORM runs that one form alone (the
process to put under `rocprofv3 --kernel-trace --stats` for the per-kernel split: the fused pass carries the tile and the store
skip, head_wgrad_blocked_kernel the reader's)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="full,tiles,skip")
    ap.add_argument("--only", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--variant", default="unet", choices=["unet", "unet2"])
    ap.add_argument("--raster", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    a = ap.parse_args()
    forms = [a.only] if a.only else a.forms.split(",")

    import abcnet_amd  # noqa: F401
    from abcnet_amd.contract import HEADS
    from abcnet_amd.synthetic import synthetic_images, synthetic_targets
    from abcnet_amd.train import Trainer
    if a.variant == "unet2":
        from abcnet_amd.unet2 import UNet
    else:
        from abcnet_amd.unet import UNet
    dev = torch.device("cuda", 0)
    steps = {}
    for form in forms:
        # the workload of bench.py's headline line: same seeds, same batch
        model = UNet(1, list(HEADS), dtype="bf16")
        model.reset_parameters(seed=1234)
        model = model.to(dev)
        tr = Trainer(model, a.batch, a.size, a.size, use_graph=not a.no_graph, zero_skip=form != "full")
        if form == "tiles":
            tr.eng.hf.dl_tiles = None
        tr.load_batch(synthetic_images(a.batch, a.size, seed=7).to(dev), [t.to(dev) for t in synthetic_targets(a.batch, a.size // 4, seed=1)])
        step = tr.step
        if a.raster:
            from abcnet_amd.raster import TargetRasterizer, parse_record
            from abcnet_amd.synthetic import random_annotations
            rz = TargetRasterizer(a.batch, a.size // 4, max_atoms=64, max_bonds=64, targets=tr.targets, sparse=True)
            tr.use_sparse_targets(rz)
            rz.load([parse_record(*random_annotations(30, 32, 900 + i, size=a.size), h=a.size // 4) for i in range(a.batch)])

            def step(rz=rz, tr=tr):
                rz.run()
                tr.step()
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        steps[form] = (step, tr)
    if "skip" in steps:
        words = steps["skip"][1].eng.hf_tiles.cpu().tolist()
        bits = sum(bin(w & ((1 << 64) - 1)).count("1") for w in words)
        waves = sum(1 for w in words for q in range(4) if any((w >> (4 * mt + q)) & 1 for mt in range(15)))
        groups = sum(1 for w in words for mg in range(4) if (w >> (16 * mg)) & 0xFFFF)
        print(json.dumps({"chunks": len(words), "tile_bits_set": round(bits / (60.0 * len(words)), 4), "waves_with_a_tile": round(waves / (4.0 * len(words)), 4),
                          "chunk_mgroups_read": round(groups / (4.0 * len(words)), 4)}), flush=True)
    res = {f: [] for f in forms}
    for _ in range(a.rounds):
        for form in forms:
            step = steps[form][0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            res[form].append(round(1000 * (time.perf_counter() - t0) / a.steps, 3))
    for form in forms:
        print(json.dumps({"form": form, "ms_per_step": res[form], "loss": steps[form][1].loss_value()["total"]}), flush=True)


if __name__ == "__main__":
    main()
