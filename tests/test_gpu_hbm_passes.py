"""The step's HBM-bound passes -- act_bwd (pooled, full-resolution, dropout), pool_act, the batched weight packing -- held to two things:

  * byte equality with tests/golden/hbm_passes.npz: what the library answered for the same seeded inputs BEFORE these kernels were
    given more loads in flight, 32-bit index arithmetic and 16-byte stores (profiles/r20_hbm_passes.md).  They feed fixed-order
    reductions, so g, the partial rows and the packed weights may not change by a bit.  Cases, inputs and runners live in
    profiles/tools/hbm_passes_golden.py (which also wrote the fixture); an array above 64 KiB is compared by its SHA-256.
  * a plain torch / numpy restatement on the CPU, so that a regenerated fixture cannot hide a wrong kernel: 1e-4 (f32) / 3e-2 (bf16)
    relative to the largest value, as tests/test_gpu_kernels.py; the packing is a permutation and a rounding, so it is exact.

The vector count per pixel C / 8 (bf16) or C / 4 (f32) has to divide 256, so it is always a power of two: a count that is not is
refused by abc_act_bwd, and test_act_bwd_refuses_a_vector_count_that_is_no_power_of_two holds that instead of a general-path case.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402

import hiputil as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hbm_passes_golden", os.path.join(ROOT, "profiles", "tools", "hbm_passes_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return L.load()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "hbm_passes.npz")) as z:
        return {k: z[k] for k in z.files}


def same_bytes(golden, key, t):
    got = G.as_bytes(t)
    want = golden[key]
    assert got.shape == want.shape and np.array_equal(got, want), "%s differs from the fixture (%d bytes%s)" % (
        key, t.numel() * t.element_size(), ", compared by SHA-256" if t.numel() * t.element_size() > G.DIGEST_ABOVE else "")


def drop_keep(idx, seed, p):
    """abc_drop_keep (common.hpp) on a numpy array of element indices"""
    m = np.uint64(0xFFFFFFFF)
    h = ((idx.astype(np.uint64) * np.uint64(0x9E3779B1)) & m) ^ np.uint64(seed)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return (h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) >= np.float32(p)


def act_bwd_reference(c, inp):
    """g [B,H,W,C] and the two per-channel sums (f64) of [BN -> act -> dropout -> maxpool]'s backward, from the inputs as stored"""
    tdt = U.tdt(c["dt"])
    q = lambda a: torch.from_numpy(a).to(tdt).float()
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    x = q(inp["y"])[..., c["cy_off"]:c["cy_off"] + Cc]
    sc, sh, sl, mu, istd = (torch.from_numpy(inp[k]) for k in ("scale", "shift", "slope", "mean", "invstd"))
    y = x.double() * sc.double() + sh.double()      # (f64: the sign of the kernel's fused multiply-add, exactly)
    up = torch.zeros_like(x)
    if c["pooled"]:
        z = torch.maximum(y, sl.double() * y).float().permute(0, 3, 1, 2)
        _, idx = F.max_pool2d(z, 2, return_indices=True)
        dp = q(inp["d_pool"])[..., c["cpool_off"]:c["cpool_off"] + Cc].permute(0, 3, 1, 2).contiguous()
        up = F.max_unpool2d(dp, idx, 2, output_size=(H, W)).permute(0, 2, 3, 1)
    if c["same"]:
        up = up + q(inp["d_same"])[..., c["csame_off"]:c["csame_off"] + Cc]
    g = up * torch.where(y > 0, torch.ones_like(sl), sl)
    if c["drop_p"] > 0:
        ld = inp["y"].shape[-1]
        pix = np.arange(B * H * W, dtype=np.uint64).reshape(B, H, W, 1)
        idx = pix * np.uint64(ld) + np.uint64(c["cy_off"]) + np.arange(Cc, dtype=np.uint64)
        keep = torch.from_numpy(drop_keep(idx, c["drop_seed"], c["drop_p"]))
        g = torch.where(keep, g * (1.0 / (1.0 - c["drop_p"])), torch.zeros_like(g))
    xh = (x - mu) * istd
    return g, g.double().sum((0, 1, 2)), (g.double() * xh.double()).sum((0, 1, 2))


@pytest.mark.parametrize("case", G.act_bwd_cases(), ids=lambda c: c["name"])
def test_act_bwd(lib, golden, case):
    inp = G.act_bwd_inputs(case)
    got = G.run_act_bwd(lib, case, inp)
    same_bytes(golden, "act_bwd.%s.g" % case["name"], got["g"])
    same_bytes(golden, "act_bwd.%s.partial" % case["name"], got["partial"])
    g_ref, s1, s2 = act_bwd_reference(case, inp)
    t = U.tol(case["dt"], 1e-4, 3e-2)
    Cc = case["C"]
    assert U.relerr(got["g"][..., :Cc].float(), g_ref) < t
    assert got["g"][..., Cc:].float().abs().max().item() == 0 if case["pad_g"] else True      # (nothing past the channels of the row)
    assert U.relerr(got["partial"][:, 0].double().sum(0), s1) < t
    assert U.relerr(got["partial"][:, 1].double().sum(0), s2) < t


def test_act_bwd_refuses_a_vector_count_that_is_no_power_of_two(lib):
    c = G._ab("c24", L.BF16, 2, 6, 10, 24, True, False)
    with pytest.raises(L.AbcNetHipError):
        G.run_act_bwd(lib, c)


@pytest.mark.parametrize("case", G.pool_act_cases(), ids=lambda c: c["name"])
def test_pool_act(lib, golden, case):
    inp = G.pool_act_inputs(case)
    got = G.run_pool_act(lib, case, inp)["out"]
    same_bytes(golden, "pool_act.%s.out" % case["name"], got)
    lo, hi = case["c_off"], case["c_off"] + case["C"]
    x = torch.from_numpy(inp["x"]).to(torch.bfloat16).float()[..., lo:hi]
    sc, sh, sl = (torch.from_numpy(inp[k])[lo:hi] for k in ("scale", "shift", "slope"))
    y = x * sc + sh
    ref = F.max_pool2d(torch.maximum(y, sl * y).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert U.relerr(got.float(), ref) < 3e-2


def pack_reference(lib, c, inp):
    """the packed weight [tap][chunk][row][k] (layout 1: 32-row blocks as [kk][h][row][8]) in f32, from the weight in the reference layout"""
    geo = G.pack_geometry(lib, c)
    w = inp["arena"][c["w_off"]:]
    Cout, Cin, mode, nt = c["Cout"], c["Cin"], c["mode"], geo["ntaps"]
    if mode == 0:
        src = w.reshape(Cout, Cin, nt)                              # [row = cout][red = cin][tap]
    elif mode == 1:
        src = w.reshape(Cout, Cin, nt).transpose(1, 0, 2)          # [row = cin][red = cout][tap]
    elif mode == 2:
        w4 = w.reshape(Cin, Cout, 3, 3)
        nx = 2 if c["px"] else 1
        taps = []
        for t in range(nt):
            iy, ix = t // nx, t % nx
            ky = (0 if iy == 0 else 2) if c["py"] else 1
            kx = (0 if ix == 0 else 2) if c["px"] else 1
            taps.append(w4[:, :, ky, kx].T)                         # [cout][cin]
        src = np.stack(taps, axis=2)
    else:
        src = w.reshape(Cin, Cout, 9)                               # [row = cin][red = cout][tap]
    src = src.astype(np.float32)
    if c["row_scale"] and mode in (0, 2):
        src = src * inp["row_scale"][:, None, None]
    ck = geo["ck"]
    out = np.zeros((nt, geo["nch_total"], geo["rtot"], ck), dtype=np.float32)
    blk = np.zeros((c["rows_pad"], geo["red_pad"], nt), dtype=np.float32)
    blk[:src.shape[0], :src.shape[1]] = src
    ch0 = c["red_off"] // ck
    for ch in range(geo["red_pad"] // ck):
        out[:, ch0 + ch, c["rows_off"]:c["rows_off"] + c["rows_pad"], :] = blk[:, ch * ck:(ch + 1) * ck, :].transpose(2, 0, 1)
    if c["layout"] == 1:
        e = ck // 4                                                  # elements per 16 bytes: k = h * 2e + kk * e + e'
        out = out.reshape(nt, geo["nch_total"], geo["rtot"] // 32, 32, 2, 2, e).transpose(0, 1, 2, 5, 4, 3, 6)
    return np.ascontiguousarray(out).reshape(-1)


def test_pack_batch(lib, golden):
    items = G.pack_items()
    got = G.run_pack(lib, items)
    assert {c["mode"] for c in items} == {0, 1, 2, 3}
    for c in items:
        t = got[c["name"]]
        same_bytes(golden, "pack.%s" % c["name"], t)
        ref = torch.from_numpy(pack_reference(lib, c, G.pack_inputs(c)))
        assert ref.abs().sum().item() > 0
        if c["dt"] == L.FP8:
            dec = t.view(torch.float8_e4m3fn).float()
            assert U.relerr(dec, ref) < 2.0 ** -4, c["name"]      # (e4m3: three mantissa bits)
        else:
            want = ref.to(U.tdt(c["dt"]))
            assert torch.equal(t.view(torch.uint8), want.view(torch.uint8)), c["name"]
