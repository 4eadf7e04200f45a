"""The bf16 gradient exchange inside the training step on a ONE-GPU box (started by tests/test_gpu_00_exchange_bf16_insitu.py as a
fresh process; modelled on rccl_world1_worker.py): backend "nccl" with world size 1 and the exchange forced on, so that every
bucket goes pack -> all_to_all_single -> rank-ordered sum -> all_gather_into_tensor -> unpack on the communication stream between
the hipGraph segments of the backward plan.  At world 1 the sum has one row and rounding to bf16 twice is rounding once: the
padded gradient store after 3 steps (2 of them graph replays, lr = 0) must equal bf16_rne of the plain Trainer's, bit for bit.

    python exchange_bf16_worker.py OUT_FILE
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import distributed as D  # noqa: E402
from abcnet_amd.synthetic import synthetic_images, synthetic_targets  # noqa: E402
from abcnet_amd.train import Trainer  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402

import exchange_oracle as X  # noqa: E402

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]
SIZE, BATCH, STEPS = 64, 2, 3


def main():
    out = sys.argv[1]
    rank, world = D.init_process_group(backend="nccl")
    assert (rank, world) == (0, 1) and dist.get_backend() == "nccl"
    dev = torch.device("cuda", torch.cuda.current_device())
    x = synthetic_images(BATCH, SIZE, seed=7).to(dev)
    tg = [t.to(dev) for t in synthetic_targets(BATCH, SIZE // 4, seed=1)]

    def run(**kw):
        m = UNet(1, HEADS, dtype="bf16")
        m.reset_parameters(seed=1)
        m = m.to(dev)
        tr = Trainer(m, BATCH, SIZE, SIZE, lr=0.0, use_graph=True, bucket_mb=4.0, **kw)
        tr.load_batch(x, tg)
        for _ in range(STEPS):
            tr.step()
        torch.cuda.synchronize()
        return m._grad_store.cpu().numpy().copy(), tr

    def report(tr):
        r = tr.reducer
        return {"mode": r.mode, "wire_dtype": r.wire_dtype, "fallback": r.fallback_reason, "buckets": len(tr.buckets),
                "segments": len(tr._segments), "graphs": tr._graphs is not None, "wire_bytes_per_step": r.wire_bytes_per_step(),
                "wire_bytes_w2": r.wire_bytes_per_step(world=2)}

    g_plain, tr0 = run()
    res = {"backend": dist.get_backend(), "store_elems": int(g_plain.size), "nonzero": int(np.count_nonzero(g_plain)),
           "plain": {"segments": len(tr0._segments)}}
    g_f32, tr1 = run(exchange="direct", force_exchange=True)
    res["direct_f32"] = dict(report(tr1), equals_plain=bool(np.array_equal(g_f32.view(np.uint32), g_plain.view(np.uint32))))
    g_bf16, tr2 = run(exchange="direct", force_exchange=True, exchange_dtype="bf16")
    want = X.round_bf16(g_plain)
    res["direct_bf16"] = dict(report(tr2), equals_rounded_plain=bool(X.same_bits(g_bf16, want)),
                              differing=int((g_bf16.view(np.uint32) != want.view(np.uint32)).sum()),
                              changed_by_rounding=int((want.view(np.uint32) != g_plain.view(np.uint32)).sum()),
                              nan=int(np.isnan(g_plain).sum()))
    with open(out, "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
