#!/usr/bin/env python3
"""Seeded cases of the step's HBM-bound passes (act_bwd, pool_act, batched weight packing) and what the library answers for them.

    python profiles/tools/hbm_passes_golden.py --write tests/golden/hbm_passes.npz      (on the GPU, at the commit to be held to)

Every case draws its inputs from numpy's default_rng with a fixed seed, so tests/test_gpu_hbm_passes.py regenerates them and the
fixture holds outputs only: per case the output tensor and the partial rows, as raw bytes; an array above 64 KiB is held as its
SHA-256.  The tests import the case tables and the runners from this file and require byte equality with the fixture
(profiles/r20_hbm_passes.md: the kernels changed their load order, address arithmetic and store width, never what they add up).
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DIGEST_ABOVE = 64 * 1024


def _imports():
    for p in (os.path.join(ROOT, "tests"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import abcnet_amd  # noqa: F401
    from abcnet_amd import _lib as L
    return torch, L


# ------------------------------------------------------------------ act_bwd
def _ab(name, dt, B, H, W, Cc, pooled, same, **kw):
    c = dict(name=name, dt=dt, B=B, H=H, W=W, C=Cc, pooled=pooled, same=same, cy_off=0, csame_off=0, cpool_off=0, pad_y=0, pad_same=0,
             pad_pool=0, pad_g=0, drop_p=0.0, drop_seed=0)
    c.update(kw)
    return c


def act_bwd_cases():
    """dt: 0 = f32 (4 channels per vector), 1 = bf16 (8).  pad_*: channels of the row stride beyond what the case reads."""
    BF, F = 1, 0
    return [
        _ab("pool_c16", BF, 2, 6, 10, 16, True, False),
        _ab("pool_c16_same", BF, 2, 6, 10, 16, True, True),
        _ab("pool_c32_same", BF, 2, 6, 10, 32, True, True),
        _ab("pool_c64", BF, 2, 6, 10, 64, True, False),
        _ab("pool_c64_same_f32", F, 2, 6, 10, 64, True, True),
        _ab("pool_c16_f32", F, 2, 6, 10, 16, True, False),
        _ab("pool_odd_7x9", BF, 2, 7, 9, 16, True, False),
        _ab("pool_odd_7x9_same", BF, 2, 7, 9, 32, True, True),
        # channel slices of wider tensors, every row stride different
        _ab("pool_offsets", BF, 2, 6, 10, 32, True, True, cy_off=8, csame_off=16, cpool_off=24, pad_y=16, pad_same=32, pad_pool=40, pad_g=8),
        # 652864 work items on the 2048 x 256 threads of the capped grid: a pair for the first threads, a single item for the rest
        _ab("pool_tail", BF, 2, 808, 808, 16, True, False),
        _ab("pool_tail_same", BF, 2, 808, 808, 16, True, True),
        # the general path: dropout (full resolution: the pooled form has none)
        _ab("drop_c32", BF, 2, 6, 10, 32, False, True, drop_p=0.25, drop_seed=1234, cy_off=8, pad_y=16),
        _ab("plain_c128", BF, 2, 8, 8, 128, False, True, cy_off=32, csame_off=64, pad_y=64, pad_same=96, pad_g=32),
    ]


def act_bwd_inputs(c):
    rng = np.random.default_rng(1000 + sum(map(ord, c["name"])))
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    inp = dict(y=f(B, H, W, c["cy_off"] + Cc + c["pad_y"]) * 1.5 + 0.3)
    if c["same"]:
        inp["d_same"] = f(B, H, W, c["csame_off"] + Cc + c["pad_same"])
    if c["pooled"]:
        inp["d_pool"] = f(B, H // 2, W // 2, c["cpool_off"] + Cc + c["pad_pool"])
    inp["scale"] = rng.uniform(-0.6, 1.4, Cc).astype(np.float32)
    inp["shift"] = f(Cc) * 0.3
    inp["slope"] = rng.choice(np.array([0.0, 0.01, 1.0], dtype=np.float32), Cc)
    inp["mean"] = f(Cc) * 0.2
    inp["invstd"] = rng.uniform(0.5, 1.5, Cc).astype(np.float32)
    return inp


def run_act_bwd(lib, c, inp=None):
    """-> dict(g=[B,H,W,ld_g] tensor as stored, partial=[nblk,2,C] f32), both on the host"""
    torch, L = _imports()
    inp = act_bwd_inputs(c) if inp is None else inp
    tdt = torch.bfloat16 if c["dt"] == L.BF16 else torch.float32
    dev = lambda a, t=None: torch.from_numpy(a).to(t or torch.float32).to("cuda")
    y = dev(inp["y"], tdt)
    coef = [dev(inp[k]) for k in ("scale", "shift", "slope", "mean", "invstd")]
    ld_g = c["C"] + c["pad_g"]
    g = torch.zeros((c["B"], c["H"], c["W"], ld_g), dtype=tdt, device="cuda")
    a = L.ActBwdDesc()
    a.y_raw, a.ld_y, a.g, a.ld_g = y.data_ptr(), y.shape[-1], g.data_ptr(), ld_g
    keep = [y, g] + coef
    if c["same"]:
        ds = dev(inp["d_same"], tdt); keep.append(ds)
        a.dA_same, a.ld_same = ds.data_ptr(), ds.shape[-1]
    if c["pooled"]:
        dp = dev(inp["d_pool"], tdt); keep.append(dp)
        a.dA_pool, a.ld_pool = dp.data_ptr(), dp.shape[-1]
    a.scale, a.shift, a.slope, a.mean, a.invstd = (t.data_ptr() for t in coef)
    a.dtype, a.B, a.H, a.W, a.C = c["dt"], c["B"], c["H"], c["W"], c["C"]
    a.cy_off, a.csame_off, a.cpool_off = c["cy_off"], c["csame_off"], c["cpool_off"]
    a.drop_p, a.drop_seed, a.drop_ld = c["drop_p"], c["drop_seed"], y.shape[-1]
    nblk = lib.abc_act_bwd_blocks(C.byref(a))
    part = torch.zeros((nblk, 2, c["C"]), dtype=torch.float32, device="cuda")
    a.partial = part.data_ptr()
    L.check(lib.abc_act_bwd(C.byref(a), torch.cuda.current_stream().cuda_stream), "act_bwd")
    torch.cuda.synchronize()
    return dict(g=g.cpu(), partial=part.cpu())


# ------------------------------------------------------------------ pool_act
def pool_act_cases():
    return [dict(name="pa_%dx%d_c%d" % (H, W, Cc), B=2, H=H, W=W, C=Cc, c_off=8, pad=8) for H, W in ((6, 10), (7, 9)) for Cc in (16, 64)]


def pool_act_inputs(c):
    rng = np.random.default_rng(2000 + sum(map(ord, c["name"])))
    ct = c["c_off"] + c["C"] + c["pad"]
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    return dict(x=f(c["B"], c["H"], c["W"], ct), scale=rng.uniform(-0.6, 1.4, ct).astype(np.float32), shift=f(ct) * 0.3,
                slope=rng.choice(np.array([0.0, 0.01, 1.0], dtype=np.float32), ct))


def run_pool_act(lib, c, inp=None):
    torch, L = _imports()
    inp = pool_act_inputs(c) if inp is None else inp
    x = torch.from_numpy(inp["x"]).to(torch.bfloat16).to("cuda")
    coef = [torch.from_numpy(inp[k]).to("cuda") for k in ("scale", "shift", "slope")]
    out = torch.zeros((c["B"], c["H"] // 2, c["W"] // 2, c["C"]), dtype=torch.bfloat16, device="cuda")
    a = L.ActSrc()
    a.x, a.Hx, a.Wx, a.ldx = x.data_ptr(), c["H"], c["W"], x.shape[-1]
    a.scale, a.shift, a.slope = (t.data_ptr() for t in coef)
    L.check(lib.abc_pool_act(C.byref(a), L.BF16, c["c_off"], c["C"], c["B"], out.data_ptr(), L.BF16, c["C"],
                             torch.cuda.current_stream().cuda_stream), "pool_act")
    torch.cuda.synchronize()
    return dict(out=out.cpu())


# ------------------------------------------------------------------ batched weight packing
def _pk(name, mode, dt, Cout, Cin, k, rows_pad, **kw):
    c = dict(name=name, mode=mode, dt=dt, Cout=Cout, Cin=Cin, k=k, rows_pad=rows_pad, py=0, px=0, red_total=None, red_off=0, rows_total=0,
             rows_off=0, layout=0, row_scale=False, w_off=0)
    c.update(kw)
    return c


def pack_items():
    """a plan-shaped table: every mode, both layouts, the three destination types, items the tile form takes among them.  The 16-channel
    items cover 4608 destination elements each, so the 2048-element blocks of the dest-major kernel straddle their borders."""
    F, BF, F8 = 0, 1, 2
    return [
        _pk("c16_fwd", 0, BF, 16, 16, 3, 32),
        _pk("c16_dgrad", 1, BF, 16, 16, 3, 32),
        _pk("c16_to_32_odd_offset", 0, BF, 32, 16, 3, 32, w_off=3),          # source not 16-byte aligned
        _pk("tile_64", 0, BF, 64, 64, 3, 64, layout=1),                        # (pack_tiles_kernel's)
        _pk("tile_64_odd_offset", 1, BF, 64, 64, 3, 64, w_off=5),
        _pk("head_1x1", 0, BF, 14, 128, 1, 32),
        _pk("head_1x1_scaled", 0, BF, 14, 128, 1, 32, row_scale=True, layout=1),
        _pk("convt_phase_11", 2, BF, 32, 64, 3, 32, py=1, px=1),
        _pk("convt_phase_01", 2, BF, 32, 64, 3, 32, py=0, px=1, row_scale=True, layout=1),
        _pk("convt_phase_00", 2, BF, 16, 32, 3, 32),
        _pk("convt_dgrad", 3, BF, 32, 64, 3, 64),
        _pk("convt_dgrad_l1", 3, BF, 64, 32, 3, 32, layout=1),
        _pk("rows_off", 0, BF, 16, 48, 3, 32, rows_total=64, rows_off=32),
        _pk("red_off", 1, BF, 48, 16, 3, 32, red_total=96, red_off=32),
        _pk("c16_f32", 0, F, 16, 16, 3, 32),
        _pk("convt_f32", 3, F, 16, 32, 3, 32),
        _pk("c64_e4m3", 0, F8, 64, 64, 3, 64, layout=1),
        _pk("c64_e4m3_dgrad", 1, F8, 64, 64, 1, 64),
    ]


def pack_geometry(lib, c):
    red = {0: c["Cin"], 1: c["Cout"], 2: c["Cin"], 3: c["Cout"]}[c["mode"]]
    rt = red if c["red_total"] is None else c["red_total"]
    ck = lib.abc_conv_chunk(c["dt"], rt)
    red_pad = -(-red // ck) * ck
    ntaps = {0: c["k"] ** 2, 1: c["k"] ** 2, 2: (2 if c["py"] else 1) * (2 if c["px"] else 1), 3: 9}[c["mode"]]
    nch_total = -(-rt // ck)
    rtot = c["rows_total"] or c["rows_pad"]
    return dict(red=red, rt=rt, ck=ck, red_pad=red_pad, ntaps=ntaps, nch_total=nch_total, rtot=rtot, n=ntaps * nch_total * ck * rtot)


def pack_inputs(c):
    rng = np.random.default_rng(3000 + sum(map(ord, c["name"])))
    nw = c["Cout"] * c["Cin"] * (c["k"] ** 2 if c["mode"] < 2 else 9)
    return dict(arena=rng.standard_normal(c["w_off"] + nw, dtype=np.float32), row_scale=rng.uniform(0.5, 1.5, c["Cout"]).astype(np.float32))


def run_pack(lib, items=None):
    """the whole table through ONE abc_pack_batch -> {item name: destination as stored (host tensor)}"""
    torch, L = _imports()
    items = pack_items() if items is None else items
    tdt = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.FP8: torch.uint8}
    isz = lib.abc_pack_item_bytes()
    host = (C.c_char * (isz * len(items)))()
    keep, dsts, first = [], [], 0
    for i, c in enumerate(items):
        inp, geo = pack_inputs(c), pack_geometry(lib, c)
        arena = torch.from_numpy(inp["arena"]).to("cuda")
        rs = torch.from_numpy(inp["row_scale"]).to("cuda")
        dst = torch.zeros(geo["n"], dtype=tdt[c["dt"]], device="cuda")
        keep += [arena, rs]
        dsts.append(dst)
        d = L.PackDesc()
        d.w, d.dst, d.mode, d.dtype_c = arena.data_ptr() + 4 * c["w_off"], dst.data_ptr(), c["mode"], c["dt"]
        d.Cout, d.Cin, d.kh, d.kw, d.py, d.px = c["Cout"], c["Cin"], c["k"], c["k"], c["py"], c["px"]
        d.rows_pad, d.red_pad, d.red_total, d.red_off, d.ck = c["rows_pad"], geo["red_pad"], geo["rt"], c["red_off"], geo["ck"]
        d.rows_total, d.rows_off, d.layout = c["rows_total"], c["rows_off"], c["layout"]
        d.row_scale = rs.data_ptr() if c["row_scale"] else None
        n = lib.abc_pack_item_fill(C.addressof(host) + i * isz, C.byref(d), first)
        if n < 0:
            raise RuntimeError("abc_pack_item_fill refused %s: %s" % (c["name"], lib.abc_last_error().decode()))
        first += n
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to("cuda")
    L.check(lib.abc_pack_batch(table.data_ptr(), len(items), first, torch.cuda.current_stream().cuda_stream), "pack_batch")
    torch.cuda.synchronize()
    return {c["name"]: t.cpu() for c, t in zip(items, dsts)}


# ------------------------------------------------------------------ the fixture
def as_bytes(t):
    """a host tensor as the bytes it is stored as; above DIGEST_ABOVE its SHA-256"""
    import torch
    raw = t.contiguous().view(torch.uint8).numpy().reshape(-1)
    if raw.size > DIGEST_ABOVE:
        return np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), dtype=np.uint8).copy()
    return raw.copy()


def collect(lib):
    out = {}
    for c in act_bwd_cases():
        for k, v in run_act_bwd(lib, c).items():
            out["act_bwd.%s.%s" % (c["name"], k)] = as_bytes(v)
    for c in pool_act_cases():
        for k, v in run_pool_act(lib, c).items():
            out["pool_act.%s.%s" % (c["name"], k)] = as_bytes(v)
    for name, v in run_pack(lib).items():
        out["pack.%s" % name] = as_bytes(v)
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
