#!/usr/bin/env python3
"""Seeded cases of the fused heads pass (abc_heads_fused_fwd_bwd) and every array it writes for them.

    python profiles/tools/heads_small_golden.py --write tests/golden/heads_small.npz      (on the GPU, at the commit to be held to)

The cases are the smallest that reach every branch of the five one-tile heads' path: one chunk, chunks across an image boundary,
many chunks; dropout off and on; dense targets, no target at all (every wave takes the skip path) and a single pixel with targets
(exactly one wave of one chunk fires); logits stored and NULL; no_zero_skip 0 and 1.  Inputs come from numpy's default_rng with a
fixed seed, so tests/test_gpu_heads_small.py regenerates them and the fixture holds outputs only, as raw bytes; an array above
2 KiB is held as its SHA-256.  The pass feeds fixed-order reductions (the loss sums, BatchNorm's backward, the conv2 weight gradient),
so nothing it writes may change by a bit (profiles/r25_heads_small.md).
"""
import ctypes as C
import functools
import hashlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DIGEST_ABOVE = 2048
HEADS = [1, 14, 3, 2, 1, 360, 60, 60]
LD = 128 * len(HEADS)
SHAPES = [(1, 8, 16), (2, 16, 24), (3, 32, 32)]
DROPS = [0.0, 0.2]
TARGETS = ["dense", "zero", "one_wave"]
DROP_SEED = 0x1234567


def cases():
    return [dict(name="b%d_%dx%d.p%d.%s.%s.%s" % (B, h, w, round(10 * p), t, "logits" if lg else "nologits", "noskip" if ns else "skip"),
                 B=B, h=h, w=w, drop_p=p, targets=t, logits=lg, noskip=ns)
            for (B, h, w), p, t, lg, ns in itertools.product(SHAPES, DROPS, TARGETS, (True, False), (0, 1))]


def _imports():
    for p in (os.path.join(ROOT, "tests"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import abcnet_amd  # noqa: F401
    from abcnet_amd import _lib as L
    return torch, L


@functools.lru_cache(maxsize=None)
def inputs(B, h, w, tset):
    """features, BatchNorm coefficients, conv2 weights and the eight target maps of a shape (numpy, as the kernel's types but bf16)"""
    rng = np.random.default_rng(2500 + 100 * B + h + w)
    npix = B * h * w
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    inp = dict(feat=f(npix, LD) * 1.5, scale=rng.uniform(0.4, 1.2, LD).astype(np.float32), shift=f(LD) * 0.3,
               slope=np.full(LD, 0.01, dtype=np.float32), mean=f(LD) * 0.2, invstd=rng.uniform(0.5, 1.5, LD).astype(np.float32))
    inp["w2"] = [f(c, 128) * 0.15 for c in HEADS]
    inp["b2"] = [f(c) * 0.5 for c in HEADS]
    chans = [1, 14, 3, 2, 1, 360, 60, 60]
    dts = [np.float32] * 6 + [np.float64] * 2
    tg = [np.zeros((B, c, h, w), dtype=dt) for c, dt in zip(chans, dts)]
    if tset == "dense":
        for i, t in enumerate(tg):
            v = rng.random(t.shape)
            u = rng.random(t.shape)
            v = np.where(u < 0.4, 0.0, np.where(u < 0.5, 1.0, v))      # exact zeros and exact ones among the values
            tg[i] = (v * 9 + 3).astype(t.dtype) if i == 6 else v.astype(t.dtype)
    elif tset == "one_wave":
        # pixel 40 of image 0: wave 1 of chunk 0, and no other wave of any chunk
        y, x = divmod(40, w)
        tg[0][0, 0, y, x] = 1; tg[1][0, 3, y, x] = 1; tg[2][0, 1, y, x] = 1; tg[3][0, 0, y, x] = 0.5; tg[4][0, 0, y, x] = 1
        tg[5][0, 2 * 60 + 7, y, x] = 1; tg[6][0, 7, y, x] = 5.25; tg[7][0, 7, y, x] = 1
    inp["targets"] = tg
    return inp


def run(lib, c):
    """-> {array name: host tensor}: everything abc_heads_fused_fwd_bwd writes for the case"""
    torch, L = _imports()
    B, h, w = c["B"], c["h"], c["w"]
    inp = inputs(B, h, w, c["targets"])
    npix = B * h * w
    dev = lambda a, t=None: torch.from_numpy(a).to(t or torch.from_numpy(a).dtype).to("cuda").contiguous()
    d = L.HeadsFusedDesc()
    feat = dev(inp["feat"], torch.bfloat16)
    coef = [dev(inp[k]) for k in ("scale", "shift", "slope", "mean", "invstd")]
    d.feat, d.ld = feat.data_ptr(), LD
    d.scale, d.shift, d.slope, d.mean, d.invstd = (t.data_ptr() for t in coef)
    d.drop_p, d.drop_seed, d.drop_salt = c["drop_p"], DROP_SEED, None
    w2, b2 = [dev(t) for t in inp["w2"]], [dev(t) for t in inp["b2"]]
    pack = torch.zeros(lib.abc_heads_fused_pack_bytes(), dtype=torch.uint8, device="cuda")
    logits = [torch.zeros((B, ch, h, w), device="cuda") for ch in HEADS] if c["logits"] else None
    tg = [dev(t) for t in inp["targets"]]
    for i in range(8):
        d.w2[i], d.b2[i] = w2[i].data_ptr(), b2[i].data_ptr()
        d.logits[i] = logits[i].data_ptr() if logits else None
    d.w2_pack = pack.data_ptr()
    (d.t_atom, d.t_types, d.t_charges, d.t_hs, d.t_bond, d.t_btypes, d.t_rho, d.t_omega) = (t.data_ptr() for t in tg)
    d.B, d.h, d.w = B, h, w
    nchunk = lib.abc_heads_fused_chunks(C.byref(d))
    out = dict(dl=torch.zeros(lib.abc_heads_fused_dl_elems(C.byref(d)), dtype=torch.bfloat16, device="cuda"),
               g=torch.zeros((npix, LD), dtype=torch.bfloat16, device="cuda"),
               bnpart=torch.zeros((nchunk, 2, LD), device="cuda"),
               losspart=torch.zeros((lib.abc_heads_fused_loss_blocks(C.byref(d)), 16), dtype=torch.float64, device="cuda"),
               work=torch.zeros(lib.abc_heads_fused_wgrad_floats(C.byref(d)), device="cuda"),
               keep=torch.zeros((3, npix, 2, 8), dtype=torch.uint8, device="cuda"),
               dl_tiles=torch.zeros(nchunk, dtype=torch.int64, device="cuda"))
    d.dl, d.g, d.bn_partial, d.loss_partial = (out[k].data_ptr() for k in ("dl", "g", "bnpart", "losspart"))
    d.wgrad_work, d.keep_mask, d.dl_tiles, d.no_zero_skip = out["work"].data_ptr(), out["keep"].data_ptr(), out["dl_tiles"].data_ptr(), c["noskip"]
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.abc_heads_fused_pack(C.byref(d), st), "heads_fused_pack")
    L.check(lib.abc_heads_fused_fwd_bwd(C.byref(d), st), "heads_fused_fwd_bwd")
    torch.cuda.synchronize()
    if logits:
        out.update(("logits%d" % i, t) for i, t in enumerate(logits))
    del feat, coef, w2, b2, pack, tg
    return {k: v.cpu() for k, v in out.items()}


def as_bytes(t):
    """a host tensor as the bytes it is stored as; above DIGEST_ABOVE its SHA-256"""
    import torch
    raw = t.contiguous().view(torch.uint8).numpy().reshape(-1)
    if raw.size > DIGEST_ABOVE:
        return np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), dtype=np.uint8).copy()
    return raw.copy()


def collect(lib):
    out = {}
    for c in cases():
        for k, v in run(lib, c).items():
            out["%s.%s" % (c["name"], k)] = as_bytes(v)
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="NPZ", required=True)
    a = ap.parse_args()
    _, L = _imports()
    got = collect(L.load())
    os.makedirs(os.path.dirname(os.path.abspath(a.write)), exist_ok=True)
    np.savez_compressed(a.write, **got)
    print("%d arrays, %d bytes -> %s (%d bytes on disk)" % (len(got), sum(v.size for v in got.values()), a.write, os.path.getsize(a.write)))


if __name__ == "__main__":
    main()
