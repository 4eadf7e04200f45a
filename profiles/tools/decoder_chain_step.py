"""The whole decoder chain behind the network, one process, one JSON line: InferenceRunner(assemble=True, molblocks=True,
evaluate=True, score_graphs=True, score_similarity=True) on drawn_molecules(seed 777) fed through SampleBuilder, beside the same
runner with none of those flags on the images the builder made; b64 @ 512 x 512 bf16, the frozen trained fixture.  Graph replay,
device events around each window of --steps steps, the windows of the two runners alternated; ms per step = window / steps.

    python profiles/tools/decoder_chain_step.py [--steps 200] [--windows 4] [--tree DIR]

--tree DIR: import abcnet_amd from DIR (a checkout of another commit, built) instead of this tree: an A/B of two commits runs
this file once per tree in fresh processes, alternated, and compares the medians."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--windows", type=int, default=4)
ap.add_argument("--tree", default=ROOT)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.augment import SampleBuilder  # noqa: E402
from abcnet_amd.infer import InferenceRunner  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402
from make_trained_fixture import unpack_state  # noqa: E402

B, S = 64, 512
m = UNet(1, [1, 14, 3, 2, 1, 360, 60, 60], dtype="bf16", dropout_p=0.2)
m.load_state_dict(unpack_state(os.path.join(ROOT, "tests", "golden", "trained_unet_state.npz")))
m = m.to("cuda").eval()
chain = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, molblocks=True, evaluate=True, score_graphs=True, score_similarity=True)
plain = InferenceRunner(m, B, S, S, use_graph=True)
x, notes = drawn_molecules(B, S, seed=777)
sb = SampleBuilder(chain, amount=0.1, max_src=(S, S), sparse=True)
sb.load([((1.0 - x[b, 0].numpy()) * 255).astype(np.uint8) for b in range(B)], [n[0] for n in notes], [n[1] for n in notes],
        np.random.RandomState(0))
sb.run()
plain.load_batch(chain.input_images)
for r in (chain, plain):
    for _ in range(10):      # (eager, capture, replays)
        r.step()
torch.cuda.synchronize()
assert chain._graph is not None and plain._graph is not None
ms = {"chain": [], "plain": []}
for w in range(a.windows):
    for name, r in ((("chain", chain), ("plain", plain)) if w % 2 == 0 else (("plain", plain), ("chain", chain))):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            r.step()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / a.steps)
ev = chain.evaluation()
med = {k: statistics.median(v) for k, v in ms.items()}
print(json.dumps({"tree": os.path.abspath(a.tree), "lib": abcnet_amd._lib.LIB_PATH, "batch": B, "size": S, "steps_per_window": a.steps,
                  "chain_ms": round(med["chain"], 4), "plain_ms": round(med["plain"], 4), "chain_minus_plain_ms": round(med["chain"] - med["plain"], 4),
                  "chain_windows_ms": [round(v, 4) for v in ms["chain"]], "plain_windows_ms": [round(v, 4) for v in ms["plain"]],
                  "exact": ev["molecules"]["exact"], "counted": ev["molecules"]["counted"], "dice_q20": ev["similarity"]["dice_q20"],
                  "text_bytes": sum(len(t) for t in chain.molblocks() if t is not None)}), flush=True)
