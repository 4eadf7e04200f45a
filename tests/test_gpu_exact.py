"""GPU tests that hold the trunk kernels -- forward convolution, data gradient, transposed convolution, weight gradient -- to EXACT sums.

Operands come from the dyadic lattice of tests/lattice.py: every value, every on-load transform of it and every product is exact, and
each case asserts that the sum of its terms' magnitudes stays below half of 2^24 lattice units, so that f32 sums are exact in any
order, through any K-split and any MFMA shape.  There is no tolerance: f32 outputs (weight gradients after the slab reduction, f32
convolution outputs, the per-channel sum row of the BatchNorm statistics) equal the f64 reference bit for bit, bf16 outputs equal its
round-to-nearest-even.  (One exception: the sum-of-squares row of the statistics, whose terms are off the lattice, keeps the f32-mode
bound of tests/test_gpu_kernels.py, rtol 1e-4.)  One lost, doubled or misplaced term is an inequality, and the failure message says in
which taps, channel tiles, tile rows and columns.

The weight-gradient slabs are filled with NaN before abc_wgrad, as the engine's workspace holds stale data and nothing clears it: a
slab element that its workgroup never writes surfaces in the reduction.  Each case reduces once with accumulate = 0 into a
sentinel-filled dW and once with accumulate = 1 onto a lattice-valued one; cases with the BatchNorm-backward correction on load
(`dual`) also hold the corrected tensor that the kernel writes out to the exact value.

Every case asserts its route first (abc_wgrad_route_info; abc_conv_variant and abc_conv_weight_layout); tests/test_lattice_host.py
proves without a GPU that the tables reach every route.  The weight-gradient table (B = 2 unless said; `tab`: Q's segment table in LDS):

    case                    shape                         K-splits  family    tile  pm  ts  fast  k3  tab
    2x2-tab                 64 x 64, 3x3, 1 x 24 x 48     2, 3, 9   general   2x2   1   0   1     1   1
    2x2-tab-dual            the same, correction on load  3         general   2x2   1   0   1     1   1
    2x2-ragged              64 x 64, 3x3, 20 x 40         3, 7      general   2x2   1   0   1     1   0
    2x2-slices              the same, P 16..80 of 96,     3         general   2x2   1   0   1     1   0
                            Q 32..96 of 128
    4x2-tab (-dual)         512 x 256, 3x3, 1 x 64 x 192  5         general   4x2   1   0   1     1   1
    4x2-ragged              512 x 256, 3x3, 1 x 60 x 184  5         general   4x2   1   0   1     1   0
    1x4                     32 x 128, 1x1, 24 x 40        3         general   1x4   1   0   1     0   0
    1x4-ragged-channels     21 x 128, 1x1, 24 x 40        3         general   1x4   1   0   0     0   0
    2x1-convT-12            64 x 32 stride 2, 12 x 12     3         general   2x1   1   0   1     1   0
    2x1-convT-20x24         64 x 32 stride 2, 3 x 20 x 24 3         general   2x1   1   0   1     1   0
    1x1-convT               32 x 16 stride 2, 12 x 12     3         general   1x1   1   0   1     1   0
    pm4-32x32 (-dual)       32 x 32, 3x3, 64 x 48 (32x48) 3         general   1x1   4   0   1     1   0
    pm4-ragged-width        32 x 32, 3x3, 32 x 40         3         general   1x1   4   0   1     1   0
    pm4-16to32, pm4-32to16  32 x 16 / 16 x 32, 32 x 48    3         general   1x1   4   0   1     1   0
    pm1-prefetch            32 x 32, 3x3, 24 x 40         3         general   1x1   1   0   1     1   0
    ts-pm1 (-dual)          32 x 32, 5x5, 24 x 40         3         general   1x1   1   1   1     0   0
    ts-pm2 (-dual)          32 x 32, 5x5, 32 x 40         3         general   1x1   2   1   1     0   0
    n32r2 (-dual, -qcoef)   32 x 32, 5x5, 32 x 48         3         5x5 32-channel (wgrad_narrow.hip)
    narrow16 (-dual,        16 x 16, 3x3, 3 x 40 x 48     3         16-channel (wgrad_narrow.hip)
      -slices, -slices-dual)
    c1-16-*, c1-32-*        16 / 32 x 1 f32 image, 3x3    5, 7      one-channel (wgrad_c1.hip): W = 72 four pixels per thread,
      (-dual on 16, 3x3)    and 5x5, 40 x 72 / 40 x 70              W = 70 the scalar form
    pooled-q                64 x 32, 3x3, Q pooled on load 3        general   1x1   1   0   0     0   0
    f32-p                   32 x 32, 3x3, f32 P, bf16 Q   3         general   1x1   1   0   1     1   0
    head-1, -21, -90        planar f32 P x 128, 128 k px  1, 5      head (wgrad_heads.hip)
    f32-2x2, f32-1x1        f32 compute mode, 20x40/24x40 3         general   2x2 / 1x1, 1, 0, 1, 1, 0  (k3: bf16 kernels only)

The convolution table (abc_conv_variant in f32 / bf16 mode: 0 conv_igemm.hip, 1 conv_fast.hip, 2 stem.hip, 5 conv_narrow.hip;
`wd`: the weights-direct loop, abc_conv_weight_layout = 1; sums: the statistics' sum row is checked):

    fast-128-coef           128 -> 128, 24 x 40, BatchNorm + LeakyReLU on load    1 / 1 wd    sums
    fast-64to128            64 -> 128, 16 x 16, on-load transform                 1 / 1 wd    sums
    igemm-pooled            32 -> 64, 44 x 72 pooled on load to 22 x 36           0 / 0       sums
    fast-256to96            256 -> 96, 8 x 8                                      1 / 1       sums
    fast-5x5                32 -> 32 5x5, 24 x 24, on-load transform              1 / 1       sums
    narrow-16to16, -16to32, -32to16      20 x 40 (ragged in both directions)      1 / 5       sums
    narrow-mirror           32 -> 16, mirrored taps, no bias (a data gradient)    1 / 5
    narrow-slices           16 of 48 -> 16 of 40 channels, sentinel around        - / 5
    narrow-pool-out         16 -> 32, 22 x 42, second pooled output (odd width)   - / 5
    narrow-stem             the first convolution computed in the halo staging    - / 5
    narrow-5x5              32 -> 32 5x5, 40 x 48                                 1 / 5       sums
    img-w30, -w42-5x5, -w40, -smallest   one-channel f32 image, whole 8-row bands 2 / 2       sums
    img-igemm-w30, -w42-5x5, -w40        the same at 20 rows                      0 / 0       sums
    dgrad-32from64, -64from8-1x1, -32from32-5x5   mode-1 packing, 20 x 24         1 / 1, 0 / 0, 1 / 5
    ConvTranspose: stride-2 data gradient at 12 x 12 and 10 x 20 (1 / 1 wd); abc_convt_fused_fwd at 9 x 11 and 3 x 10 x 20
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.engine import TAPS_CONVT_DGRAD, convT_pack_parity, convT_phase_taps, taps_mirror, taps_square  # noqa: E402

import hiputil as U  # noqa: E402
import lattice as T  # noqa: E402

SENT = -1234.5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return L.load()


def _dev(ts):
    return tuple(t.contiguous().to(U.DEV) for t in ts)


def _ptrs(ts):
    return tuple(t.data_ptr() for t in ts)


@pytest.mark.parametrize("cid,nsplit", [(c["id"], ns) for c in T.WG_CASES for ns in c["nsplit"]])
def test_wgrad_exact(lib, cid, nsplit):
    c = next(k for k in T.WG_CASES if k["id"] == cid)
    o = T.wg_data(c)          # (asserts the budget and that P and Q are exact in bf16)
    assert o["budget"] < 0.5
    B, Ca, Cb, H, W, kind = c["B"], c["Ca"], c["Cb"], c["H"], c["W"], c["kind"]
    ntaps = len(T.wg_taps(c))
    keep, ptr = [], {}
    p = o["p"].contiguous().to(U.DEV) if kind == "head" else U.nhwc(o["p"], c["dtp"])
    q = o["q"].permute(0, 2, 3, 1).contiguous().to(U.DEV) if kind == "c1" else U.nhwc(o["q"], c["dtq"])
    ptr["p"], ptr["q"] = p.data_ptr(), q.data_ptr()
    for name in ("pcoef", "qcoef"):
        if name in o:
            keep.append(_dev(o[name]))
            ptr[name] = _ptrs(keep[-1])
    p_out = None
    if c["dual"]:
        p2 = U.nhwc(o["p2"], T.BF16)
        p_out = torch.full((B, H, W, Ca), float("nan"), dtype=torch.bfloat16, device=U.DEV)
        ptr["p2"], ptr["p_out"] = p2.data_ptr(), p_out.data_ptr()
    d = T.wg_desc(c, nsplit, ptr)
    assert T.wg_route(lib, d) == c["route"]
    if c["dual"]:
        assert lib.abc_wgrad_fuses_apply(C.byref(d)) == 1
    ca, cb = L.i32(), L.i32()
    L.check(lib.abc_wgrad_pads(C.byref(d), C.byref(ca), C.byref(cb)), "pads")
    # the engine's contract: the slabs hold stale data, every element the reduction reads is written by the launch
    part = torch.full((nsplit * ntaps * ca.value * cb.value,), float("nan"), dtype=torch.float32, device=U.DEV)
    d.partial = part.data_ptr()
    L.check(lib.abc_wgrad(C.byref(d), U.stream()), "wgrad")
    dw = torch.full((Ca, Cb, ntaps), SENT, dtype=torch.float32, device=U.DEV)
    acc = o["dw0"].clone().to(U.DEV)
    for out, accumulate in ((dw, 0), (acc, 1)):
        r = L.WgradReduceDesc()
        r.partial, r.nsplit, r.ntaps, r.Ca, r.Cb, r.Ca_pad, r.Cb_pad = part.data_ptr(), nsplit, ntaps, Ca, Cb, ca.value, cb.value
        r.dw, r.accumulate = out.data_ptr(), accumulate
        L.check(lib.abc_wgrad_reduce(C.byref(r), U.stream()), "wgrad_reduce")
    torch.cuda.synchronize()
    what = "%s nsplit=%d" % (cid, nsplit)
    T.assert_wgrad_equal(dw, T.expect(o["ref"], T.F32), what)
    T.assert_wgrad_equal(acc, T.expect(o["ref"] + o["dw0"].double(), T.F32), what + " (accumulate)")
    if c["dual"]:
        T.assert_conv_equal(U.to_nchw(p_out), T.expect(o["P"].double(), T.BF16), what + " p_out")


def _run_conv(lib, c, dt, x, Hx, Wx, wp, bias, taps, **kw):
    """U.conv with the launch kept back, so that the descriptor's routing answers can be asserted before it runs"""
    items = []
    y, st = U.conv(lib, x, T.F32 if c["img"] else dt, dt, c["B"], Hx, Wx, c["ld"], c["coff"], c["Cin"], wp, bias, c["Cout"], taps, c["H"], c["W"],
                   defer=items, **kw)
    d = items[0][0]
    i = 0 if dt == T.F32 else 1
    assert (lib.abc_conv_variant(C.byref(d)), lib.abc_conv_weight_layout(C.byref(d))) == (c["variant"][i], c["layout"][i]), c["id"]
    L.check(lib.abc_conv_fwd(C.byref(d), U.stream()), "conv_fwd")
    torch.cuda.synchronize()
    return y, st, items


def _check_stats(st, ref, what):
    """the per-channel sum row exactly (the rows summed in f64; its budget is asserted with the case), the sum of squares within the
    f32-mode bound of tests/test_gpu_kernels.py"""
    s = st.double().sum(0).cpu()
    n = ref.shape[0] * ref.shape[2] * ref.shape[3]
    want = ref.sum((0, 2, 3))
    assert torch.equal(s[0], want), "%s: sum row differs in channels %s" % (what, (s[0] != want).nonzero().view(-1).tolist()[:16])
    torch.testing.assert_close(s[1] / n, (ref ** 2).mean((0, 2, 3)), rtol=1e-4, atol=1e-4)


# (variant None: a form that only the bf16 kernel has -- the second, pooled output, the fused stem -- or channel slices)
@pytest.mark.parametrize("cid,dt", [(c["id"], dt) for c in T.CONV_CASES for i, dt in enumerate((T.F32, T.BF16)) if c["variant"][i] is not None],
                         ids=lambda v: v if isinstance(v, str) else ("f32" if v == T.F32 else "bf16"))
def test_conv_exact(lib, cid, dt):
    c = next(k for k in T.CONV_CASES if k["id"] == cid)
    o = T.conv_data(c)
    assert o["budget"] < 0.5
    B, Cin, Cout, k, H, W = c["B"], c["Cin"], c["Cout"], c["k"], c["H"], c["W"]
    Hx, Wx = (2 * H, 2 * W) if c["pool"] else (H, W)
    x = o["x"].permute(0, 2, 3, 1).contiguous().to(U.DEV) if c["img"] else U.nhwc(o["x"], dt)
    coef = _dev(o["coef"]) if "coef" in o else None
    if c["mode"] == 1:
        wp = U.pack(lib, o["w"].to(U.DEV), 1, dt, Cin, Cout, k, -(-Cout // 32) * 32, Cin)
    else:
        wp = U.pack(lib, o["w"].to(U.DEV), 0, dt, Cout, Cin, k, -(-Cout // 32) * 32, Cin)
    bias = None if o["bias"] is None else o["bias"].to(U.DEV)
    taps = taps_mirror(taps_square(k)) if c["mirror"] else taps_square(k)
    out = torch.full((B, H, W, c["ldy"]), 7.0, dtype=U.tdt(dt), device=U.DEV)
    pooled = torch.full((B, H // 2, W // 2, Cout), 7.0, dtype=U.tdt(dt), device=U.DEV) if c["pool_out"] else None
    stem = None
    if c["stem"]:
        img, w0, sc0, b0 = o["stem"]
        stem = (img.reshape(B, H, W).contiguous().to(U.DEV), w0.contiguous().to(U.DEV), sc0.to(U.DEV), b0.to(U.DEV), 0.0)
    y, st, _keep = _run_conv(lib, c, dt, x, Hx, Wx, wp, bias, taps, ldy=c["ldy"], cout_off=c["ycoff"], out=out, out_slope=c["out_slope"], coef=coef,
                             pool=c["pool"], stats=c["stats"], pool_out=pooled, stem=stem)
    what = "%s %s" % (cid, "f32" if dt == T.F32 else "bf16")
    want = T.expect(o["out"], dt)
    T.assert_conv_equal(U.to_nchw(y[..., c["ycoff"]:c["ycoff"] + Cout]), want, what)
    if c["ldy"] > Cout:
        rest = torch.cat([y[..., :c["ycoff"]], y[..., c["ycoff"] + Cout:]], dim=-1)
        assert bool((rest == 7.0).all()), "%s: a store outside the descriptor's channels" % what
    if c["pool_out"]:
        T.assert_conv_equal(U.to_nchw(pooled), F.max_pool2d(want, 2), what + " pooled output")
    if c["stats"]:
        assert o["stats_budget"] < 0.5
        _check_stats(st, o["ref"], what)


@pytest.mark.parametrize("dt", [T.F32, T.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,n,m,Cin", T.CONVT_DGRAD_CASES)
def test_conv_transpose_dgrad_exact(lib, dt, B, n, m, Cin):
    """the stride-2 data gradient of ConvTranspose2d(k3, s2) + crop, the incoming gradient read at channel offset `half` of a concat
    buffer whose other half holds lattice values that must not leak in; against autograd in f64"""
    g = T.gen(3000 + n)
    half = Cin // 2
    x = T.draw_data(g, (B, Cin, n, m)).double().requires_grad_(True)
    w = T.draw_weight(g, (Cin, half, 3, 3))
    cat = T.draw_data(g, (B, Cin, 2 * n, 2 * m))
    dout = cat[:, half:]
    F.conv_transpose2d(x, w.double(), None, stride=2)[:, :, 1:, 1:].backward(dout.double())
    xa = torch.ones_like(x).requires_grad_(True)       # sum of |terms|: the same operator over magnitudes
    F.conv_transpose2d(xa, w.double().abs(), None, stride=2)[:, :, 1:, 1:].backward(dout.double().abs())
    assert T.assert_budget(xa.grad, "convT dgrad") < 0.5
    wd = U.pack(lib, w.to(U.DEV), 3, dt, half, Cin, 3, Cin, half)
    dx, _ = U.conv(lib, U.nhwc(cat, dt), dt, dt, B, 2 * n, 2 * m, Cin, half, half, wd, None, Cin, TAPS_CONVT_DGRAD, n, m, stride=2)
    torch.cuda.synchronize()
    assert U.conv.last_variant == 1
    T.assert_conv_equal(U.to_nchw(dx), T.expect(x.grad, dt), "convT dgrad %dx%d" % (n, m))


@pytest.mark.parametrize("B,H,W,Cin,Chalf", T.CONVT_FUSED_CASES)
def test_conv_transpose_fused_exact(lib, B, H, W, Cin, Chalf):
    """abc_convt_fused_fwd (all four output parities in one pass, BatchNorm + LeakyReLU on load) against
    F.conv_transpose2d(...)[:, :, 1:, 1:] in f64, written into the upper half of a concat buffer whose skip half stays untouched.
    (The kernel writes no BatchNorm statistics: abc_convt_desc has no such field.)"""
    dt = T.BF16
    g = T.gen(4000 + H)
    x = T.draw_data(g, (B, Cin, H, W))
    coef = T.draw_coef(g, Cin)
    xa = T.act(x, *coef)
    T.assert_bf16_exact(xa, "convT input")
    w = T.draw_weight(g, (Cin, Chalf, 3, 3))
    bias = T.draw_weight(g, (Chalf,))
    ref = F.conv_transpose2d(xa.double(), w.double(), bias.double(), stride=2)[:, :, 1:, 1:]
    assert T.assert_budget(F.conv_transpose2d(xa.double().abs(), w.double().abs(), bias.double().abs(), stride=2), "convT fused") < 0.5
    Hs, Ws, Ctot = 2 * H, 2 * W, 2 * Chalf
    rows_pad = -(-Chalf // 64) * 64
    ck = lib.abc_conv_chunk(dt, Cin)
    assert ck == 32
    # nine weight slices in one buffer, fragment-contiguous (abc_pack_desc.layout 1), grouped by output parity
    slice_elems = (Cin // ck) * rows_pad * ck
    wall = torch.zeros(9 * slice_elems, dtype=torch.bfloat16, device=U.DEV)
    wdev = w.to(U.DEV)
    first = {(0, 0): 0, (0, 1): 1, (1, 0): 3, (1, 1): 5}
    for py in (0, 1):
        for px in (0, 1):
            n = len(convT_phase_taps(py, px, True, True))
            dst = wall[first[(py, px)] * slice_elems:(first[(py, px)] + n) * slice_elems]
            pd = L.PackDesc()
            pd.w, pd.dst, pd.mode, pd.dtype_c = wdev.data_ptr(), dst.data_ptr(), 2, dt
            pd.Cout, pd.Cin, pd.kh, pd.kw, pd.py, pd.px = Chalf, Cin, 3, 3, convT_pack_parity(py, True), convT_pack_parity(px, True)
            pd.rows_pad, pd.red_pad, pd.red_total, pd.red_off, pd.ck, pd.layout = rows_pad, Cin, Cin, 0, ck, 1
            L.check(lib.abc_pack_conv_weights(C.byref(pd), U.stream()), "pack")
    xd, cf, bd = U.nhwc(x, dt), _dev(coef), bias.to(U.DEV)
    cat = torch.full((B, Hs, Ws, Ctot), 7.0, dtype=torch.bfloat16, device=U.DEV)
    d = L.ConvTDesc()
    U.fill_src(d.src, xd, H, W, Cin, cf)
    d.w, d.bias, d.y, d.dtype = wall.data_ptr(), bd.data_ptr(), cat.data_ptr(), dt
    d.B, d.Hin, d.Win, d.cin_off, d.Cin = B, H, W, 0, Cin
    d.Hout, d.Wout, d.ldy, d.cout_off, d.Cout, d.Cout_pad = Hs, Ws, Ctot, Chalf, Chalf, rows_pad
    assert lib.abc_convt_fused_ok(C.byref(d)) == 1
    L.check(lib.abc_convt_fused_fwd(C.byref(d), U.stream()), "convt_fused")
    torch.cuda.synchronize()
    T.assert_conv_equal(U.to_nchw(cat[..., Chalf:]), T.expect(ref, dt), "convT fused %dx%d" % (H, W))
    assert bool((cat[..., :Chalf] == 7.0).all()), "the skip half of the concat buffer was written"
