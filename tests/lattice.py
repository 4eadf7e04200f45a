"""Operands on a dyadic lattice, so that a convolution or a weight gradient has ONE right answer, bit for bit.

Every value drawn here is exact in bf16, every on-load transform of it (BatchNorm + LeakyReLU, the BatchNorm-backward correction
P = ca * g + cb * y_raw + cc) is exact in bf16, every product is exact in f32 and -- as long as the sum of the terms' magnitudes stays
below 2^24 lattice units (one unit = 1 / 256) -- every sum is exact in f32 in any order, through any split and any MFMA shape.  So an
f32 output equals the f64 reference bit for bit and a bf16 output equals its round-to-nearest-even; one lost, doubled or misplaced term,
a wrong halo, a wrong split boundary or an unwritten slab element is an inequality.  The budget is a condition each case asserts
(budget() < 0.5), never a reason to skip one.

The lattices (UNIT = 1 / 256 is the finest product of two of them):
    x, g, y_raw      k / 4,  |k| <= 8          (coarse: k / 2, |k| <= 2, for cases above ~4000 pixels per output element)
    scale            {1, -1, 0.5, -0.5, 2}
    shift            k / 4,  |k| <= 4          (coarse: k / 2, |k| <= 2)
    slope            {0, 0.25, 0.5, 1}
    weights, bias    k / 8,  |k| <= 8
    ca {+-1, +-0.5, 2}, cb {+-1, +-0.5}, cc k / 4 with |k| <= 4

This module also holds the case tables of tests/test_gpu_exact.py with the route each case is held to, so that
tests/test_lattice_host.py can settle -- without a GPU -- that the tables reach every kernel family and form."""
import ctypes as C
import zlib

import torch
import torch.nn.functional as F

import abcnet_amd  # noqa: F401
from abcnet_amd import _lib as L
from abcnet_amd.engine import TAPS_CONVT_DGRAD, taps_mirror, taps_square

UNIT = 1.0 / 256
F32, BF16 = L.F32, L.BF16
HEAD, C1, NARROW16, N32R2, GENERAL = range(5)       # abc_wgrad_route_info: info[0]


# ---------------------------------------------------------------------------------------------------------------- draws
def gen(seed):
    return torch.Generator().manual_seed(seed)


def draw(g, shape, den, kmax):
    """k / den with integer |k| <= kmax, f32"""
    return torch.randint(-kmax, kmax + 1, tuple(shape), generator=g).float() / den


def pick(g, n, values):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def draw_data(g, shape, coarse=False):
    return draw(g, shape, 2, 2) if coarse else draw(g, shape, 4, 8)


def draw_coef(g, n, coarse=False):
    """(scale, shift, slope) of a BatchNorm + LeakyReLU applied on load"""
    return (pick(g, n, [1.0, -1.0, 0.5, -0.5, 2.0]), draw(g, (n,), 2, 2) if coarse else draw(g, (n,), 4, 4), pick(g, n, [0.0, 0.25, 0.5, 1.0]))


def draw_dual(g, n):
    """(ca, cb, cc) of P = ca * g + cb * y_raw + cc"""
    return pick(g, n, [1.0, -1.0, 0.5, -0.5, 2.0]), pick(g, n, [1.0, -1.0, 0.5, -0.5]), draw(g, (n,), 4, 4)


def draw_weight(g, shape):
    return draw(g, shape, 8, 8)


def act(x, sc, sh, sl):
    """BatchNorm + LeakyReLU as the kernels apply it on load (NCHW, per-channel coefficients)"""
    y = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    return torch.maximum(y, sl.view(1, -1, 1, 1) * y)


def dual(gq, yq, ca, cb, cc):
    return ca.view(1, -1, 1, 1) * gq + cb.view(1, -1, 1, 1) * yq + cc.view(1, -1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- checks
def assert_bf16_exact(t, what=""):
    assert torch.equal(t.float(), t.float().bfloat16().float()), "%s: a value that bf16 does not hold exactly" % what
    assert bool(((t.double() / UNIT) == (t.double() / UNIT).round()).all()), "%s: a value off the 1/256 lattice" % what


def budget(abs_terms):
    """share of the 2^24 lattice units that the largest sum of |terms| uses (abs_terms: op(|p|, |q|) in value units)"""
    return float(abs_terms.double().abs().max()) / UNIT / 2.0 ** 24


def assert_budget(abs_terms, what=""):
    b = budget(abs_terms)
    assert b < 0.5, "%s: the case is wrong for its lattice: sum of |terms| uses %.3f of 2^24 units (must stay below 0.5)" % (what, b)
    return b


def expect(ref64, dt):
    """the tensor a kernel must equal: f32 outputs the f64 reference itself, bf16 outputs its round-to-nearest-even"""
    r = ref64.float()
    assert torch.equal(r.double(), ref64.double()), "the reference is not exact in f32"
    return r.bfloat16().float() if dt == BF16 else r


def _hist(idx, n):
    return torch.bincount(idx.reshape(-1), minlength=n).tolist()


def _first(bad, got, want, n=6):
    ix = bad.nonzero()[:n]
    return "; ".join("%s got %r want %r" % (tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in ix)


def assert_wgrad_equal(got, want, what=""):
    """got, want: [Ca][Cb][ntaps] f32.  The message names what a kernel hunt needs: how many, the first few, and their taps and
    32-channel tiles of either operand"""
    got, want = got.detach().float().cpu(), want.float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~((got == want) & torch.isfinite(got))
    if not bool(bad.any()):
        return
    a, b, t = bad.nonzero(as_tuple=True)
    msg = ("%s: %d of %d weight-gradient elements differ (%d not finite).  first: %s.  by tap: %s.  by 32-channel tile of P: %s, of Q: %s"
           % (what, int(bad.sum()), bad.numel(), int((~torch.isfinite(got)).sum()), _first(bad, got, want), _hist(t, got.shape[2]),
              _hist(a // 32, -(-got.shape[0] // 32)), _hist(b // 32, -(-got.shape[1] // 32))))
    raise AssertionError(msg)


def assert_conv_equal(got, want, what=""):
    """got, want: [B][C][H][W] f32.  Unequal elements by tile-relative row and column (8 x 16 tiles), by channel and by image"""
    got, want = got.detach().float().cpu(), want.float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~((got == want) & torch.isfinite(got))
    if not bool(bad.any()):
        return
    n, c, y, x = bad.nonzero(as_tuple=True)
    H, W = got.shape[2:]
    edge = int(((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).sum())
    msg = ("%s: %d of %d outputs differ (%d on the image border).  first: %s.  by row %% 8: %s.  by column %% 16: %s.  by channel: %s.  by image: %s"
           % (what, int(bad.sum()), bad.numel(), edge, _first(bad, got, want), _hist(y % 8, 8), _hist(x % 16, 16), _hist(c, got.shape[1]),
              _hist(n, got.shape[0])))
    raise AssertionError(msg)


# ---------------------------------------------------------------------------------------------------------------- references
def wgrad_ref(P, Q, taps, stride=1, dtype=torch.float64):
    """dW[a][b][t] = sum over images and pixels p of P[p][a] * Q[stride * p + d_t][b] (zero outside Q): include/abcnet_hip.h's own
    statement of abc_wgrad, one einsum per tap over the pixels whose shifted partner exists"""
    P, Q = P.to(dtype), Q.to(dtype)
    B, Ca, Hg, Wg = P.shape
    Hq, Wq = Q.shape[2:]
    out = torch.zeros((Ca, Q.shape[1], len(taps)), dtype=dtype)
    for t, (dy, dx) in enumerate(taps):
        y0, x0 = max(0, -(dy // stride)), max(0, -(dx // stride))       # the first pixel whose partner stride * p + d is inside Q
        y1 = min(Hg, (Hq - 1 - dy) // stride + 1)
        x1 = min(Wg, (Wq - 1 - dx) // stride + 1)
        if y1 <= y0 or x1 <= x0:
            continue
        p = P[:, :, y0:y1, x0:x1]
        q = Q[:, :, stride * y0 + dy:stride * (y1 - 1) + dy + 1:stride, stride * x0 + dx:stride * (x1 - 1) + dx + 1:stride]
        out[:, :, t] = torch.einsum("nahw,nbhw->ab", p, q)
    return out


# ---------------------------------------------------------------------------------------------------------------- weight-gradient cases
# route = (family, at, bt, pm, ts, fast, k3, table): what abc_wgrad_route_info must answer for the case
def _wg(id, Ca, Cb, H, W, route, **kw):
    c = dict(id=id, Ca=Ca, Cb=Cb, H=H, W=W, route=route, kind="conv", k=3, B=2, nsplit=(3,), dual=False, qcoef=True, qpool=False, dt=BF16,
             coarse=False, ref32=False, cp_off=0, cq_off=0)
    c.update(kw)
    c.setdefault("ldp", c["Ca"])
    c.setdefault("ldq", c["Cb"])
    c.setdefault("dtp", c["dt"])
    c.setdefault("dtq", c["dt"])
    return c


G = GENERAL
WG_CASES = [
    # 2 x 2 pairs, Q's segment table in LDS: 3 x 3 patches (the interior one and every border kind); nsplit 9 = the patch count
    _wg("2x2-tab", 64, 64, 24, 48, (G, 2, 2, 1, 0, 1, 1, 1), B=1, nsplit=(2, 3, 9)),
    _wg("2x2-tab-dual", 64, 64, 24, 48, (G, 2, 2, 1, 0, 1, 1, 1), B=1, nsplit=(3,), dual=True),
    # the same layer ragged in both directions: the table is ineligible; 7 does not divide the 2 * 3 * 3 = 18 patches
    _wg("2x2-ragged", 64, 64, 20, 40, (G, 2, 2, 1, 0, 1, 1, 0), nsplit=(3, 7)),
    _wg("2x2-slices", 64, 64, 20, 40, (G, 2, 2, 1, 0, 1, 1, 0), ldp=96, cp_off=16, ldq=128, cq_off=32),
    # 4 x 2 pairs: the smallest map wgeom gives them (96 patches), coarse lattice, reference in f32 (exact under the asserted budget)
    _wg("4x2-tab", 512, 256, 64, 192, (G, 4, 2, 1, 0, 1, 1, 1), B=1, nsplit=(5,), coarse=True, ref32=True),
    _wg("4x2-tab-dual", 512, 256, 64, 192, (G, 4, 2, 1, 0, 1, 1, 1), B=1, nsplit=(5,), coarse=True, ref32=True, dual=True),
    _wg("4x2-ragged", 512, 256, 60, 184, (G, 4, 2, 1, 0, 1, 1, 0), B=1, nsplit=(5,), coarse=True, ref32=True),
    # 1 x 4 pairs (one tile of P against four of Q), one tap; 21 channels: a ragged tail, the non-prefetch loader
    _wg("1x4", 32, 128, 24, 40, (G, 1, 4, 1, 0, 1, 0, 0), k=1),
    _wg("1x4-ragged-channels", 21, 128, 24, 40, (G, 1, 4, 1, 0, 0, 0, 0), k=1),
    # ConvTranspose (stride 2): P = x at n x m, Q = the gradient at 2n x 2m read at channel offset `half` of a concat buffer
    _wg("2x1-convT-12", 64, 32, 12, 12, (G, 2, 1, 1, 0, 1, 1, 0), kind="convT", qcoef=False, ldq=64, cq_off=32),
    _wg("2x1-convT-20x24", 64, 32, 20, 24, (G, 2, 1, 1, 0, 1, 1, 0), kind="convT", qcoef=False, ldq=64, cq_off=32, B=3),
    _wg("1x1-convT", 32, 16, 12, 12, (G, 1, 1, 1, 0, 1, 1, 0), kind="convT", qcoef=False, ldq=32, cq_off=16),
    # 1 x 1 pair on 32-row patches (PM = 4): unet.py's 192- and 384-pixel levels
    _wg("pm4-32x32", 32, 32, 64, 48, (G, 1, 1, 4, 0, 1, 1, 0)),
    _wg("pm4-ragged-width", 32, 32, 32, 40, (G, 1, 1, 4, 0, 1, 1, 0)),
    _wg("pm4-16to32", 32, 16, 32, 48, (G, 1, 1, 4, 0, 1, 1, 0)),
    _wg("pm4-32to16", 16, 32, 32, 48, (G, 1, 1, 4, 0, 1, 1, 0)),
    _wg("pm4-dual", 32, 32, 32, 48, (G, 1, 1, 4, 0, 1, 1, 0), dual=True),
    # 1 x 1 pair, 8-row patches, both operands prefetched
    _wg("pm1-prefetch", 32, 32, 24, 40, (G, 1, 1, 1, 0, 1, 1, 0)),
    # the tap-split 5 x 5
    _wg("ts-pm1", 32, 32, 24, 40, (G, 1, 1, 1, 1, 1, 0, 0), k=5),
    _wg("ts-pm1-dual", 32, 32, 24, 40, (G, 1, 1, 1, 1, 1, 0, 0), k=5, dual=True),
    _wg("ts-pm2", 32, 32, 32, 40, (G, 1, 1, 2, 1, 1, 0, 0), k=5),
    _wg("ts-pm2-dual", 32, 32, 32, 40, (G, 1, 1, 2, 1, 1, 0, 0), k=5, dual=True),
    # wgrad_narrow.hip: the 5 x 5 32 x 32 kernel and the 16 x 16 one
    _wg("n32r2", 32, 32, 32, 48, (N32R2, 0, 3, 0, 0, 0, 0, 0), k=5, qcoef=False),
    _wg("n32r2-dual", 32, 32, 32, 48, (N32R2, 0, 3, 0, 0, 0, 0, 0), k=5, qcoef=False, dual=True),
    _wg("n32r2-qcoef", 32, 32, 32, 48, (N32R2, 0, 3, 0, 0, 0, 0, 0), k=5),
    _wg("narrow16", 16, 16, 40, 48, (NARROW16, 0, 2, 0, 0, 0, 0, 0), B=3),
    _wg("narrow16-dual", 16, 16, 40, 48, (NARROW16, 0, 2, 0, 0, 0, 0, 0), B=3, dual=True),
    _wg("narrow16-slices", 16, 16, 40, 48, (NARROW16, 0, 2, 0, 0, 0, 0, 0), B=3, ldp=48, cp_off=16, ldq=48, cq_off=16),
    _wg("narrow16-slices-dual", 16, 16, 40, 48, (NARROW16, 0, 2, 0, 0, 0, 0, 0), B=3, ldp=48, cp_off=16, dual=True),
    # wgrad_c1.hip: the one-channel f32 image; W = 72 the four-pixel form, W = 70 the scalar one
    _wg("c1-16-w72", 16, 1, 40, 72, (C1, 0, 1, 0, 0, 0, 0, 0), kind="c1", nsplit=(7,)),
    _wg("c1-32-w70", 32, 1, 40, 70, (C1, 0, 1, 0, 0, 0, 0, 0), kind="c1", nsplit=(5,)),
    _wg("c1-32-w72", 32, 1, 40, 72, (C1, 0, 1, 0, 0, 0, 0, 0), kind="c1", nsplit=(7,)),
    _wg("c1-16-w70", 16, 1, 40, 70, (C1, 0, 1, 0, 0, 0, 0, 0), kind="c1", nsplit=(5,)),
    _wg("c1-32-5x5", 32, 1, 40, 72, (C1, 0, 1, 0, 0, 0, 0, 0), kind="c1", k=5, nsplit=(7,)),
    _wg("c1-16-w72-dual", 16, 1, 40, 72, (C1, 0, 1, 0, 0, 0, 0, 0), kind="c1", nsplit=(7,), dual=True),
    _wg("c1-16-w70-dual", 16, 1, 40, 70, (C1, 0, 1, 0, 0, 0, 0, 0), kind="c1", nsplit=(5,), dual=True),
    # a pooled Q (the general, non-prefetch loader) and an f32 P against a bf16 Q (prefetched and converted on the way to LDS)
    _wg("pooled-q", 64, 32, 24, 40, (G, 1, 1, 1, 0, 0, 0, 0), qpool=True),
    _wg("f32-p", 32, 32, 24, 40, (G, 1, 1, 1, 0, 1, 1, 0), dtp=F32),
    # wgrad_heads.hip: planar f32 P with a per-channel scale, 128 feature channels at an offset of a wider map, 128 * k pixels
    _wg("head-1", 1, 128, 8, 16, (HEAD, 0, 0, 0, 0, 0, 0, 0), kind="head", k=1, nsplit=(1, 5), ldq=256, cq_off=128),
    _wg("head-21", 21, 128, 16, 24, (HEAD, 0, 0, 0, 0, 0, 0, 0), kind="head", k=1, nsplit=(1, 5), ldq=256, cq_off=128),
    _wg("head-90", 90, 128, 16, 24, (HEAD, 0, 0, 0, 0, 0, 0, 0), kind="head", k=1, nsplit=(1, 5), ldq=256, cq_off=128),
    # f32 compute mode
    _wg("f32-2x2", 64, 64, 20, 40, (G, 2, 2, 1, 0, 1, 1, 0), dt=F32),
    _wg("f32-1x1", 32, 32, 24, 40, (G, 1, 1, 1, 0, 1, 1, 0), dt=F32),
]


def wg_taps(c):
    return TAPS_CONVT_DGRAD if c["kind"] == "convT" else taps_square(c["k"])


def wg_dims(c):
    """(Hp, Wp, stride, Hq, Wq as the taps index them, Hx, Wx of Q's tensor)"""
    H, W = c["H"], c["W"]
    if c["kind"] == "convT":
        return H, W, 2, 2 * H, 2 * W, 2 * H, 2 * W
    return H, W, 1, H, W, (2 * H if c["qpool"] else H), (2 * W if c["qpool"] else W)


DUMMY = 0x1000      # a non-null pointer for the host-side queries, which read through none


def wg_desc(c, nsplit, ptr=None):
    """the abc_wgrad_desc of a case.  ptr: name -> device address (p, q, p2, p_out, and the coefficient triples pcoef / qcoef); None:
    placeholders, for the routing queries"""
    ptr = ptr or {}
    get = lambda n: ptr.get(n, DUMMY)
    H, W, stride, Hq, Wq, Hx, Wx = wg_dims(c)
    d = L.WgradDesc()
    d.p.x, d.p.Hx, d.p.Wx, d.p.ldx = get("p"), H, W, c["ldp"]
    d.q.x, d.q.Hx, d.q.Wx, d.q.ldx, d.q.pool = get("q"), Hx, Wx, c["ldq"], int(c["qpool"])
    if c["kind"] == "head":
        d.p.planar, d.p.ctot, d.p.ldx = 1, c["Ca"], 0
    if c["dual"] or c["kind"] == "head":
        d.p.scale, d.p.shift, d.p.slope = ptr.get("pcoef", (DUMMY,) * 3)
    if c["qcoef"] and c["kind"] != "c1":
        d.q.scale, d.q.shift, d.q.slope = ptr.get("qcoef", (DUMMY,) * 3)
    d.dtype_p, d.dtype_q, d.dtype_c = (F32 if c["kind"] == "head" else c["dtp"]), (F32 if c["kind"] == "c1" else c["dtq"]), c["dt"]
    d.B, d.Hg, d.Wg, d.Hq, d.Wq = c["B"], H, W, Hq, Wq
    d.cp_off, d.Ca, d.cq_off, d.Cb, d.stride, d.nsplit = c["cp_off"], c["Ca"], c["cq_off"], c["Cb"], stride, nsplit
    L.set_taps(d, wg_taps(c))
    if c["dual"]:
        d.p2, d.ld_p2, d.cp2_off, d.p_dual, d.p_out, d.ld_pout = get("p2"), c["Ca"] + 32, 16, 1, get("p_out"), c["Ca"]
    return d


def wg_route(lib, d):
    info = (C.c_int32 * 8)()
    L.check(lib.abc_wgrad_route_info(C.byref(d), info), "route_info")
    return tuple(info)


_WG_DATA = {}


def wg_data(c):
    """the operands of a case and its f64 reference, computed once per case (the K-split counts share them):
    P (what the kernel multiplies, NCHW f32), Q likewise, ref [Ca][Cb][ntaps], and the raw tensors the device reads"""
    if c["id"] in _WG_DATA:
        return _WG_DATA[c["id"]]
    g = gen(zlib.crc32(c["id"].encode()))        # (a seed of the case alone: adding a case moves no other)
    B, Ca, Cb, coarse = c["B"], c["Ca"], c["Cb"], c["coarse"]
    H, W, stride, Hq, Wq, Hx, Wx = wg_dims(c)
    o = dict()
    # P
    pfull = draw_data(g, (B, c["ldp"], H, W), coarse)
    o["p"] = pfull
    if c["dual"]:
        cf = draw_dual(g, c["ldp"])
        o["pcoef"] = (cf[0], cf[2], cf[1])       # (scale, shift, slope) = (ca, cc, cb)
        y2 = draw_data(g, (B, Ca + 32, H, W), coarse)
        o["p2"] = y2
        s = slice(c["cp_off"], c["cp_off"] + Ca)
        P = dual(pfull[:, s], y2[:, 16:16 + Ca], cf[0][s], cf[1][s], cf[2][s])
    elif c["kind"] == "head":
        sc = pick(g, Ca, [1.0, -1.0, 0.5, -0.5, 2.0])
        o["pcoef"] = (sc, torch.zeros(Ca), torch.ones(Ca))
        P = pfull * sc.view(1, -1, 1, 1)
    else:
        P = pfull[:, c["cp_off"]:c["cp_off"] + Ca]
    # Q
    qfull = draw_data(g, (B, c["ldq"], Hx, Wx), coarse)
    o["q"] = qfull
    Q = qfull
    if c["qcoef"] and c["kind"] != "c1":
        o["qcoef"] = draw_coef(g, c["ldq"], coarse)
        Q = act(qfull, *o["qcoef"])
    if c["qpool"]:
        Q = F.max_pool2d(Q, 2)
    Q = Q[:, c["cq_off"]:c["cq_off"] + Cb]
    assert_bf16_exact(P, c["id"] + " P")
    assert_bf16_exact(Q, c["id"] + " Q")
    taps = wg_taps(c)
    o["budget"] = assert_budget(wgrad_ref(P.abs(), Q.abs(), taps, stride, torch.float32 if c["ref32"] else torch.float64), c["id"])
    ref = wgrad_ref(P, Q, taps, stride, torch.float32 if c["ref32"] else torch.float64)
    o["P"], o["Q"], o["ref"] = P, Q, ref.double()
    o["dw0"] = draw(g, ref.shape, 4, 8)          # what the accumulating reduction adds onto
    _WG_DATA[c["id"]] = o
    return o


# ---------------------------------------------------------------------------------------------------------------- convolution cases
# variant / layout: what abc_conv_variant / abc_conv_weight_layout must answer, per compute dtype (f32, bf16); None: the case does
# not run in that dtype
def _cv(id, Cin, Cout, H, W, variant, layout=(0, 0), **kw):
    c = dict(id=id, Cin=Cin, Cout=Cout, H=H, W=W, variant=variant, layout=layout, k=3, B=2, coef=False, pool=False, mirror=False,
             bias=True, img=False, stem=False, pool_out=False, out_slope=None, stats=True, mode=0, wmax=8)
    c.update(kw)
    c.setdefault("ld", c["Cin"])
    c.setdefault("coff", 0)
    c.setdefault("ldy", c["Cout"])
    c.setdefault("ycoff", 0)
    return c


CONV_CASES = [
    # conv_fast.hip (bf16); the same cases in f32 mode run conv_igemm.hip
    _cv("fast-128-coef", 128, 128, 24, 40, (1, 1), (0, 1), coef=True, wmax=2),
    _cv("fast-64to128", 64, 128, 16, 16, (1, 1), (0, 1), coef=True),
    _cv("igemm-pooled", 32, 64, 22, 36, (0, 0), (0, 0), pool=True, wmax=2),
    _cv("fast-256to96", 256, 96, 8, 8, (1, 1), (0, 0)),
    _cv("fast-5x5", 32, 32, 24, 24, (1, 1), (0, 0), k=5, coef=True, wmax=4),
    # conv_narrow.hip (bf16): ragged in both directions (20 = 2 x 8 + 4 rows, 40 = 2 x 16 + 8 columns)
    _cv("narrow-16to16", 16, 16, 20, 40, (1, 5)),
    _cv("narrow-16to32", 16, 32, 20, 40, (1, 5)),
    _cv("narrow-32to16", 32, 16, 20, 40, (1, 5)),
    _cv("narrow-mirror", 32, 16, 20, 40, (1, 5), mirror=True, bias=False, stats=False),
    _cv("narrow-slices", 16, 16, 20, 40, (None, 5), ld=48, coff=16, ldy=40, ycoff=8, stats=False),
    _cv("narrow-pool-out", 16, 32, 22, 42, (None, 5), pool_out=True, out_slope=0.25, stats=False),
    _cv("narrow-stem", 16, 16, 24, 40, (None, 5), stem=True, out_slope=0.0, stats=False),
    _cv("narrow-5x5", 32, 32, 40, 48, (1, 5), k=5, wmax=2),
    # one-channel f32 images: stem.hip where the rows are whole 8-row bands (W = 30, 42: its scalar form; 40: four pixels per thread;
    # 8 x 4 with 8 output channels: the smallest shape it accepts), conv_igemm.hip otherwise (20 rows: no whole bands)
    _cv("img-w30", 1, 16, 24, 30, (2, 2), img=True),
    _cv("img-w42-5x5", 1, 32, 16, 42, (2, 2), img=True, k=5),
    _cv("img-w40", 1, 16, 24, 40, (2, 2), img=True),
    _cv("img-smallest", 1, 8, 8, 4, (2, 2), img=True),
    _cv("img-igemm-w30", 1, 16, 20, 30, (0, 0), img=True),
    _cv("img-igemm-w42-5x5", 1, 32, 20, 42, (0, 0), img=True, k=5),
    _cv("img-igemm-w40", 1, 16, 20, 40, (0, 0), img=True),
    # data gradients: mode-1 packing, mirrored taps, no bias; 20 x 24 is ragged where 16 x 24 is not
    _cv("dgrad-32from64", 64, 32, 20, 24, (1, 1), (0, 0), mode=1, mirror=True, bias=False, stats=False),
    _cv("dgrad-64from8-1x1", 8, 64, 20, 24, (0, 0), (0, 0), mode=1, mirror=True, bias=False, stats=False, k=1),
    _cv("dgrad-32from32-5x5", 32, 32, 20, 24, (1, 5), (0, 0), mode=1, mirror=True, bias=False, stats=False, k=5),
]


def conv_desc_host(c, dt):
    """the abc_conv_desc of a case with placeholder pointers: what the routing queries of the host test read"""
    d = L.ConvDesc()
    pool = c["pool"]
    Hx, Wx = (2 * c["H"], 2 * c["W"]) if pool else (c["H"], c["W"])
    d.src.x, d.src.Hx, d.src.Wx, d.src.ldx, d.src.pool = DUMMY, Hx, Wx, c["ld"], int(pool)
    if c["coef"] or pool:
        d.src.scale = d.src.shift = d.src.slope = DUMMY
    d.w, d.bias, d.y = DUMMY, (DUMMY if c["bias"] else None), DUMMY
    d.dtype_in, d.dtype_c, d.dtype_out = (F32 if c["img"] else dt), dt, dt
    d.B, d.Hin, d.Win, d.cin_off, d.Cin = c["B"], c["H"], c["W"], c["coff"], c["Cin"]
    d.Hg, d.Wg, d.Hout, d.Wout, d.ldy, d.cout_off, d.Cout, d.Cout_pad = c["H"], c["W"], c["H"], c["W"], c["ldy"], c["ycoff"], c["Cout"], -(-c["Cout"] // 32) * 32
    d.stride, d.om = 1, 1
    if c["out_slope"] is not None:
        d.out_act, d.out_slope = 1, c["out_slope"]
    if c["pool_out"]:
        d.pool_y, d.ld_pool = DUMMY, c["Cout"]
    if c["stem"]:
        d.stem_x = d.stem_w = d.stem_scale = d.stem_bias = DUMMY
    taps = taps_square(c["k"])
    L.set_taps(d, taps_mirror(taps) if c["mirror"] else taps)
    if c["stats"]:
        d.stats_rows, d.stats = 2, DUMMY
    return d


# ConvTranspose2d(k3, s2) + the crop of the first row and column, all four output parities in one pass (convt_fused.hip):
# (B, H, W, Cin, Chalf)
CONVT_FUSED_CASES = [(1, 9, 11, 64, 32), (3, 10, 20, 64, 64)]
# the stride-2 data gradient of the same layer: (B, n rows, m columns, Cin)
CONVT_DGRAD_CASES = [(2, 12, 12, 64), (2, 10, 20, 64)]


def convt_desc_host(B, H, W, Cin, Chalf):
    d = L.ConvTDesc()
    d.src.x, d.src.Hx, d.src.Wx, d.src.ldx = DUMMY, H, W, Cin
    d.src.scale = d.src.shift = d.src.slope = DUMMY
    d.w, d.bias, d.y, d.dtype = DUMMY, DUMMY, DUMMY, BF16
    d.B, d.Hin, d.Win, d.cin_off, d.Cin = B, H, W, 0, Cin
    d.Hout, d.Wout, d.ldy, d.cout_off, d.Cout, d.Cout_pad = 2 * H, 2 * W, 2 * Chalf, Chalf, Chalf, -(-Chalf // 64) * 64
    return d


_CONV_DATA = {}


def conv_data(c):
    """the operands of a convolution case and its f64 reference, computed once per case (both compute dtypes share them; every value
    is exact in bf16, so the two see the same numbers): x as the device reads it (NCHW here), xin = what is convolved, w in the
    reference layout, ref = convolution + bias [B][Cout][H][W], out = ref after the output activation"""
    if c["id"] in _CONV_DATA:
        return _CONV_DATA[c["id"]]
    g = gen(zlib.crc32(c["id"].encode()))
    B, Cin, Cout, k, H, W = c["B"], c["Cin"], c["Cout"], c["k"], c["H"], c["W"]
    Hx, Wx = (2 * H, 2 * W) if c["pool"] else (H, W)
    o = dict()
    if c["stem"]:
        # the network's first convolution computed inside the halo staging: image in {0, 0.5, 1}, first-layer weights k / 2, folded
        # BatchNorm scale in {1, 0.5, 2} and bias k / 4: relu(conv * scale + bias) is a multiple of 1 / 8 below 32, exact in bf16
        img = draw(g, (B, 1, H, W), 2, 2).abs()
        w0, sc0, b0 = draw(g, (Cin, 1, 3, 3), 2, 2), pick(g, Cin, [1.0, 0.5, 2.0]), draw(g, (Cin,), 4, 4)
        o["stem"] = (img, w0, sc0, b0)
        x = torch.relu(F.conv2d(img.double(), w0.double(), None, padding=1) * sc0.double().view(1, -1, 1, 1) + b0.double().view(1, -1, 1, 1)).float()
    else:
        x = draw_data(g, (B, c["ld"], Hx, Wx))
    o["x"] = x
    xin = x
    if c["coef"] or c["pool"]:
        o["coef"] = draw_coef(g, c["ld"])
        xin = act(x, *o["coef"])
    if c["pool"]:
        xin = F.max_pool2d(xin, 2)
    xin = xin[:, c["coff"]:c["coff"] + Cin]
    assert_bf16_exact(xin, c["id"] + " input")
    # the weight in the reference layout: Conv2d's [Cout][Cin][k][k]; a data gradient (mode 1) reads the forward layer's weight,
    # whose output channels are this convolution's input channels
    w = draw(g, (Cin, Cout, k, k) if c["mode"] == 1 else (Cout, Cin, k, k), 8, c["wmax"])      # (wmax < 8: a subset of the weight lattice)
    bias = draw_weight(g, (Cout,)) if c["bias"] else None
    o["w"], o["bias"] = w, bias
    p = k // 2
    b64 = None if bias is None else bias.double()

    def op(xx, ww, bb):
        if c["mode"] == 1:
            return F.conv_transpose2d(xx, ww, bb, padding=p)
        return F.conv2d(xx, ww.flip(2, 3) if c["mirror"] else ww, bb, padding=p)

    ref = op(xin.double(), w.double(), b64)
    o["budget"] = assert_budget(op(xin.double().abs(), w.double().abs(), None if b64 is None else b64.abs()), c["id"])
    o["xin"], o["ref"] = xin, ref
    o["out"] = ref if c["out_slope"] is None else torch.maximum(ref, c["out_slope"] * ref)
    if c["stats"]:
        # the per-channel sum row: whatever pixels a row of the statistics buffer covers, its f32 sum is exact when even the sum
        # over ALL pixels of |output| stays inside the budget
        o["stats_budget"] = assert_budget(ref.abs().sum((0, 2, 3)), c["id"] + " statistics")
    _CONV_DATA[c["id"]] = o
    return o
