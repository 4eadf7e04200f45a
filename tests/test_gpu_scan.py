"""The scan input path on the device (csrc/scan.hip through abcnet_amd.augment.ScanBuilder) against the numpy transcription of
its contract (tests/scan_oracle.py), bit for bit: the f32 batch with assert_array_equal, the geometry rows as integers; two
identities that need no oracle; graph capture; the parameter guards; and an InferenceRunner fed in place."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import ImageBuilder, ScanBuilder  # noqa: E402
import scan_oracle as so  # noqa: E402

DEV = "cuda"
POL = {"dark": so.DARK, "light": so.LIGHT, "auto": so.AUTO}
# source rows per workgroup of the histogram and box passes (SCAN_ROWS in csrc/scan.hip)
SCAN_ROWS = 64


def _grey(seed, h, w, paper=200, ink=50, strokes=4, light=False):
    """a grey scan: noisy paper, a few noisy strokes (straight runs of ink pixels, 1 or 2 wide)"""
    rs = np.random.RandomState(seed)
    mask = np.zeros((h, w), dtype=bool)
    for _ in range(strokes):
        y, x = rs.randint(0, h), rs.randint(0, w)
        dy, dx = rs.choice([-1, 0, 1]), rs.choice([-1, 0, 1])
        if dy == 0 and dx == 0:
            dx = 1
        for _ in range(rs.randint(3, max(4, max(h, w) // 2))):
            if 0 <= y < h and 0 <= x < w:
                mask[y, x] = True
                if rs.rand() < 0.5 and x + 1 < w:
                    mask[y, x + 1] = True
            y, x = y + dy, x + dx
    img = np.where(mask, rs.normal(ink, 8, (h, w)), rs.normal(paper, 6, (h, w)))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return (255 - img) if light else img


def _mixed_sources():
    """the batch of the parity test; max_src = (320, 112)"""
    one = np.array([[77]], dtype=np.uint8)                                   # 1 x 1 (a single value: CONSTANT)
    odd = _grey(1, 17, 23)                                                   # width no multiple of 16
    down = _grey(2, 100, 37, strokes=6)                                      # downscales at a non-integer ratio
    down[1, 2] = 10
    down[98, 35] = 10                                                        # (a box of 98 x 34 at least: 28 / 98)
    # 300 rows = 4 * SCAN_ROWS + 44: five workgroups per image in the histogram and box passes, the last one partial; ink in the
    # first, the third and the last of them, so the box needs all of them
    tall = _grey(3, 4 * SCAN_ROWS + 44, 100, strokes=5)
    tall[2, 50] = 5
    tall[2 * SCAN_ROWS + 7, 3] = 5
    tall[4 * SCAN_ROWS + 41, 97] = 5
    single = np.full((40, 50), 220, dtype=np.uint8)                          # a single ink pixel
    single[13, 31] = 30
    corners = _grey(4, 50, 60, strokes=0)                                    # ink in all four corners
    for y, x in ((0, 0), (0, 59), (49, 0), (49, 59)):
        corners[y, x] = 20
    const = np.full((20, 20), 128, dtype=np.uint8)                           # a constant image
    light = _grey(5, 60, 90, strokes=6, light=True)                          # light ink on a dark ground
    return [one, odd, down, tall, single, corners, const, light]


def _check(sb, srcs, cover, polarity, what=""):
    out = sb.out.cpu().numpy()
    geom = sb.geometry()
    for b, src in enumerate(srcs):
        want, g = so.build(src, sb.S, sb.margin, cover, POL[polarity])
        assert [int(geom[b][c]) for c in L.SCAN_GEOM_COLUMNS] == so.geom_row(g), (what, b, geom[b], g)
        np.testing.assert_array_equal(out[b, 0], want, err_msg="%s image %d" % (what, b))
    return geom


@pytest.mark.parametrize("polarity", ["dark", "light", "auto"])
def test_matches_the_oracle_on_mixed_sources(polarity):
    srcs = _mixed_sources()
    assert srcs[3].shape[0] == 300 and -(-300 // SCAN_ROWS) >= 3 and 300 % SCAN_ROWS
    stale = [np.zeros((320, 112), dtype=np.uint8)] * len(srcs)               # larger, dark: what lies beyond src_w / src_h afterwards
    for cover in (0, 64, 256):
        sb = ScanBuilder(len(srcs), 32, max_src=(320, 112), margin=2, cover=cover, polarity=polarity)
        sb.load(stale)
        sb.run()
        sb.load(srcs)
        sb.out.fill_(-1.0)
        sb.run()
        geom = _check(sb, srcs, cover, polarity, "cover %d %s" % (cover, polarity))
        assert geom["status"].tolist() == [so.CONSTANT, 0, 0, 0, 0, 0, so.CONSTANT, 0]
        if polarity == "auto":
            assert geom["inverted"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
        if polarity == "dark":
            assert geom["bh"][3] >= 4 * SCAN_ROWS + 40 and geom["ink"][4] == 1
            assert [int(geom[5][c]) for c in ("y0", "x0", "bh", "bw")] == [0, 0, 50, 60]
            assert geom["rows"][2] == 28 and geom["cols"][2] < 28


def test_hand_made_histograms_as_images():
    two = np.full((16, 16), 200, dtype=np.uint8)
    two[3:9, 4:6] = 60
    tie = np.zeros((9, 10), dtype=np.uint8)
    tie[3:6] = 100
    tie[6:] = 200
    const = np.full((5, 7), 93, dtype=np.uint8)
    srcs = [two, tie, const]
    sb = ScanBuilder(3, 32, max_src=(16, 16), margin=2, cover=0)
    sb.load(srcs)
    sb.run()
    geom = _check(sb, srcs, 0, "dark")
    assert geom["thr"].tolist() == [60, 0, -1] and geom["status"].tolist() == [0, 0, so.CONSTANT]
    assert geom["ink"].tolist() == [12, 30, 0] and not sb.out[2].any()


def test_sums_near_their_top_on_a_4096_square():
    """4096 x 4096, all 255 but five pixels of 254: N = 2^24, S = 255 N - 5; thr and the ink count are exact, and the last row and
    column of the capacity are read"""
    img = np.full((4096, 4096), 255, dtype=np.uint8)
    for y, x in ((4095, 4095), (3500, 3000), (3700, 3500), (4000, 4090), (3600, 3100)):
        img[y, x] = 254
    sb = ScanBuilder(1, 32, max_src=(4096, 4096), margin=2, cover=0)
    sb.load([img])
    sb.run()
    geom = _check(sb, [img], 0, "dark")
    g = geom[0]
    assert (g["thr"], g["ink"], g["status"], g["inverted"]) == (254, 5, 0, 0)
    assert (g["y0"], g["x0"], g["bh"], g["bw"]) == (3500, 3000, 596, 1096)


def _bordered(seed, S):
    rs = np.random.RandomState(seed)
    ink = rs.rand(S, S) < 0.15
    ink[0, 5] = ink[S - 1, 9] = ink[7, 0] = ink[11, S - 1] = True            # touches all four borders
    return np.where(ink, 0, 255).astype(np.uint8)


def test_identity_with_test_mode():
    """an S x S source of bytes 0 and 255 whose ink touches all four borders, margin 0, DARK: the box is the image, nothing is
    resized, and the output is ImageBuilder(mode="test")'s for every cover in 1 .. 256"""
    S, B = 32, 2
    srcs = [_bordered(31 + b, S) for b in range(B)]
    ib = ImageBuilder(B, S, "test")
    ib.load(srcs)
    want = ib.run().clone()
    assert 0 < float(want.sum()) < B * S * S
    sb = ScanBuilder(B, S, max_src=(S, S), margin=0, cover=1, polarity="dark")
    sb.load(srcs)
    for cover in range(1, 257):
        sb.d.cover_q8 = cover
        sb.out.fill_(-1.0)
        assert torch.equal(sb.run(), want), cover
    g = sb.geometry()
    assert g["thr"].tolist() == [0, 0] and g["bh"].tolist() == [S, S] and g["bw"].tolist() == [S, S] and g["ddx"].tolist() == [0, 0]


def test_identity_under_pixel_replication():
    """a binary drawing whose box has a larger side of exactly S - 2 margin, upscaled k-fold by pixel replication and coloured with
    two grey levels, comes back as the drawing's box contents at (ddx, ddy), whatever the coverage"""
    S, margin = 32, 2
    lim = S - 2 * margin
    rs = np.random.RandomState(8)
    boxes = []
    for bh, bw in ((lim, 19), (11, lim), (lim, lim)):
        d = rs.rand(bh, bw) < 0.3
        d[0, 3] = d[bh - 1, 1] = d[2, 0] = d[4, bw - 1] = True                # the box is the whole array
        boxes.append(d)
    for k in (2, 3, 5):
        srcs = []
        for i, d in enumerate(boxes):
            big = np.kron(d.astype(np.uint8), np.ones((k, k), dtype=np.uint8)).astype(bool)
            page = np.full((big.shape[0] + 3 + i, big.shape[1] + 9), 190, dtype=np.uint8)      # paper around it, unequal
            page[2:2 + big.shape[0], 4:4 + big.shape[1]][big] = 70
            srcs.append(page)
        for cover in (0, 64, 256):
            sb = ScanBuilder(len(srcs), S, max_src=(5 * lim + 8, 5 * lim + 9), margin=margin, cover=cover)
            sb.load(srcs)
            out = sb.run().cpu().numpy()
            geom = sb.geometry()
            for i, d in enumerate(boxes):
                bh, bw = d.shape
                want = np.zeros((S, S), dtype=np.float32)
                ddx, ddy = (S - bh) // 2, (S - bw) // 2
                want[ddx:ddx + bh, ddy:ddy + bw] = d
                np.testing.assert_array_equal(out[i, 0], want, err_msg="k %d cover %d drawing %d" % (k, cover, i))
                assert (geom[i]["y0"], geom[i]["x0"], geom[i]["bh"], geom[i]["bw"]) == (2, 4, k * bh, k * bw)
                assert (geom[i]["rows"], geom[i]["cols"], geom[i]["ddx"], geom[i]["ddy"]) == (bh, bw, ddx, ddy)


def test_run_replays_from_a_captured_graph():
    """ScanBuilder.run() captured once; a later load of other sizes replays it (the sequence zeroes its own scratch)"""
    S, B = 32, 3
    sb = ScanBuilder(B, S, max_src=(150, 96), margin=2, cover=64, polarity="auto")

    def batch(seed):
        rs = np.random.RandomState(seed)
        return [_grey(seed + b, int(rs.randint(9, 151)), int(rs.randint(9, 97)), light=(b == 1)) for b in range(B)]
    srcs = batch(100)
    sb.load(srcs)
    sb.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sb.run()
    for seed in (200, 300):
        srcs = batch(seed)
        sb.load(srcs)
        sb.out.fill_(-1.0)
        sb.geom.fill_(-7)
        g.replay()
        _check(sb, srcs, 64, "auto", "seed %d" % seed)


def test_bad_parameter_rows_are_refused_not_read():
    """a row whose src_h is above the slot: NaN and BAD_PARAMS for that image only when only the device holds the table, ABC_EINVAL
    at call time when the host copy is given; the output lies between sentinel bands that do not change"""
    S, B, pad = 32, 3, 1024
    big = torch.full((2 * pad + B * S * S,), 7.25, dtype=torch.float32, device=DEV)
    out = big[pad:pad + B * S * S].view(B, 1, S, S)
    sb = ScanBuilder(B, S, out=out, max_src=(70, 40), margin=2, cover=0)
    srcs = [_grey(50 + b, 70 - 9 * b, 40 - 7 * b) for b in range(B)]
    sb.load(srcs)
    sb.run()
    _check(sb, srcs, 0, "dark")
    host_table = sb.d.params_host
    sb.d.params_host = None                                  # the device table alone
    torch.cuda.synchronize()
    sb.d_par[1, 0] = 71
    sb.run()
    torch.cuda.synchronize()
    got, geom = out.cpu().numpy(), sb.geometry()
    assert np.isnan(got[1]).all() and geom[1]["status"] == so.BAD_PARAMS and geom[1]["thr"] == -1
    for b in (0, 2):
        want, g = so.build(srcs[b], S, 2, 0, so.DARK)
        np.testing.assert_array_equal(got[b, 0], want)
        assert [int(geom[b][c]) for c in L.SCAN_GEOM_COLUMNS] == so.geom_row(g)
    assert bool((big[:pad] == 7.25).all()) and bool((big[pad + B * S * S:] == 7.25).all())
    for bad in ((71, 40), (0, 40), (70, 49), (70, -3)):      # above the slot (rows; columns past the pitch of 48), below 1
        sb.d.params_host = host_table
        sb._np_par[1] = bad
        with pytest.raises(L.AbcNetHipError, match=r"\(-1\).*src_h"):
            sb.run()
    with pytest.raises(ValueError):
        sb.load([np.zeros((71, 40), np.uint8)] * B)
    with pytest.raises(ValueError):
        sb.load([np.zeros((4, 4), np.float32)] * B)
    with pytest.raises(ValueError):
        ScanBuilder(1, 32, margin=16)
    with pytest.raises(ValueError):
        ScanBuilder(1, 32, cover=257)
    with pytest.raises(ValueError):
        ScanBuilder(1, 32, polarity="negative")
    with pytest.raises(ValueError):
        ScanBuilder(1, 32, max_src=(4097, 16))
    with pytest.raises(L.AbcNetHipError):
        ScanBuilder(2, 64, out=torch.zeros((2, 3, 64, 64), device=DEV))


def test_inference_runner_fed_in_place():
    """a ScanBuilder over InferenceRunner.input_images: the buffer equals the oracle, step() runs, and the candidates are those of
    the same runner fed the oracle's image through load_batch"""
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.unet import UNet
    from oracle import unet_oracle as uo
    B, S = 2, 64
    m = UNet(1, uo.HEADS, dtype="bf16")
    m.load_state_dict(uo.filled_state("unet", 1, uo.HEADS, seed=0))
    m = m.to(DEV)
    ir = InferenceRunner(m, B, S, S, use_graph=False, extract=True)
    sb = ScanBuilder(B, S, out=ir.input_images, max_src=(200, 180), cover=64, polarity="auto")
    assert sb.margin == 64 * 20 // 512
    srcs = [_grey(900, 200, 150, strokes=9), _grey(901, 90, 180, strokes=7, light=True)]
    sb.load(srcs)
    sb.run()
    ir.step()
    torch.cuda.synchronize()
    want = np.stack([so.build(s, S, sb.margin, 64, so.AUTO)[0] for s in srcs])[:, None]
    np.testing.assert_array_equal(ir.input_images.cpu().numpy(), want)
    assert 0 < want.sum()
    got = ir.candidates()
    masks = [t.clone() for t in (ir.atom_mask, ir.bond_mask)]
    ir.load_batch(torch.from_numpy(want).to(DEV))
    ir.step()
    torch.cuda.synchronize()
    again = ir.candidates()
    for a, b in zip(masks, (ir.atom_mask, ir.bond_mask)):
        assert torch.equal(a, b)
    for a, b in zip(got, again):
        assert a["counts"] == b["counts"] and a["truncated"] == b["truncated"]
        for k in ("atoms", "bonds", "rho"):
            assert torch.equal(a[k], b[k]), k
    # the affine map of record_offsets carries the source's box corner onto the placed drawing
    g = sb.geometry()[0]
    sx, sy, ox, oy = sb.record_offsets(0)
    assert abs(g["y0"] * sx + ox - g["ddx"]) < 1e-9 and abs(g["x0"] * sy + oy - g["ddy"]) < 1e-9
