"""The cell component filter on the device (abc_build_scan_images_clean through abcnet_amd.augment.ScanBuilder(clean_cell=...))
against the transcription of its contract (tests/scan_clean_oracle.py).  Everything is integers and compared exactly: the f32
batch, the geometry rows, the stats rows, the labels and the keep bits of every cell of the capacity grid."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import ScanBuilder  # noqa: E402
from abcnet_amd.ops import StrokeNormalizer  # noqa: E402
import scan_clean_oracle as co  # noqa: E402
import scan_oracle as so  # noqa: E402

POL = {"dark": so.DARK, "light": so.LIGHT, "auto": so.AUTO}
PAPER, INK = 220, 40


def _page(h, w):
    return np.full((h, w), PAPER, dtype=np.uint8)


def _grey(seed, h, w, strokes=4, light=False):
    """a noisy grey scan with a few straight strokes, as the plain path's tests draw them (built afresh here)"""
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
    img = np.where(mask, rs.normal(50, 8, (h, w)), rs.normal(200, 6, (h, w)))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return (255 - img) if light else img


def _blobs(seed, h, w, n, lo=2, hi=9):
    """n ink rectangles of lo .. hi pixels a side at seeded places on a two-valued page"""
    rs = np.random.RandomState(seed)
    img = _page(h, w)
    for _ in range(n):
        bh, bw = int(rs.randint(lo, hi + 1)), int(rs.randint(lo, hi + 1))
        y, x = int(rs.randint(0, h - bh + 1)), int(rs.randint(0, w - bw + 1))
        img[y:y + bh, x:x + bw] = INK
    return img


def _from_cells(occ, cell, h=None, w=None):
    """a page with one ink pixel in the middle of every occupied cell of the boolean grid `occ`"""
    occ = np.asarray(occ, dtype=bool)
    img = _page(h or occ.shape[0] * cell, w or occ.shape[1] * cell)
    ys, xs = np.nonzero(occ)
    img[ys * cell + cell // 2, xs * cell + cell // 2] = INK
    return img


def _builder(srcs, S, max_src, cell, min_ink=0, keep=0, polarity="dark", cover=0, margin=2, **kw):
    sb = ScanBuilder(len(srcs), S, max_src=max_src, margin=margin, cover=cover, polarity=polarity, clean_cell=cell,
                     clean_min_ink=min_ink, clean_keep=keep, debug_cells=True, **kw)
    sb.load(srcs)
    sb.out.fill_(-1.0)
    sb.run()
    return sb


def _check(sb, srcs, what=""):
    """out, geometry, stats, labels and keep of every image against the oracle; returns (geometry, stats, labels, keep)"""
    q = sb.clean
    out = sb.out.cpu().numpy()
    geom, stats = sb.geometry(), sb.clean_stats()
    labels, keep = sb.clean_cells()
    assert labels.shape == keep.shape == (sb.B,) + sb.cap_cells and labels.dtype == np.int32 and keep.dtype == np.uint8
    for b, src in enumerate(srcs):
        want, g, st, lab, kp = co.build(src, sb.S, sb.margin, sb.cover, POL[sb.polarity], q.cell, q.min_ink, q.keep_q8,
                                        (sb.max_h, sb.pitch))
        assert [int(geom[b][c]) for c in L.SCAN_GEOM_COLUMNS] == so.geom_row(g), (what, b, geom[b], g)
        assert [int(stats[b][c]) for c in L.SCAN_CLEAN_COLUMNS] == co.stats_row(st), (what, b, stats[b], st)
        assert np.array_equal(labels[b], lab), (what, b)
        assert np.array_equal(keep[b], kp), (what, b)
        assert np.array_equal(out[b, 0], want), (what, b)
    return geom, stats, labels, keep


def _drawing(img, y, x, h, w):
    """a rectangle outline with both diagonals, two pixels thick: one connected drawing of h x w at (y, x)"""
    img[y:y + 2, x:x + w] = INK
    img[y + h - 2:y + h, x:x + w] = INK
    img[y:y + h, x:x + 2] = INK
    img[y:y + h, x + w - 2:x + w] = INK
    for i in range(min(h, w)):
        img[y + i * (h - 1) // (min(h, w) - 1), x + i * (w - 1) // (min(h, w) - 1)] = INK
    return img


def test_a_speck_in_the_corner_no_longer_sets_the_box():
    """what the filter is for: 200 x 264, a drawing of 80 x 100 and one 3 x 3 speck in the far corner"""
    src = _drawing(_page(200, 264), 60, 80, 80, 100)
    src[196:199, 260:263] = INK
    plain = ScanBuilder(1, 64, max_src=(200, 264), margin=2, cover=0)
    plain.load([src])
    plain.run()
    want, g = so.build(src, 64, 2, 0, so.DARK)
    pg = plain.geometry()[0]
    assert [int(pg[c]) for c in L.SCAN_GEOM_COLUMNS] == so.geom_row(g) and np.array_equal(plain.out[0, 0].cpu().numpy(), want)
    assert (pg["y0"], pg["x0"], pg["bh"], pg["bw"]) == (60, 80, 139, 183)              # the page, as far as the speck
    sb = _builder([src], 64, (200, 264), 8, keep=256)
    geom, stats, _, _ = _check(sb, [src])
    assert (geom[0]["y0"], geom[0]["x0"], geom[0]["bh"], geom[0]["bw"]) == (60, 80, 80, 100)     # the drawing's
    assert geom[0]["ink"] == pg["ink"] and (stats[0]["components"], stats[0]["kept"], stats[0]["ink_dropped"]) == (2, 1, 9)


def _mixed_sources():
    """max_src = (320, 112): ragged sizes, a CONSTANT image, a tall one of five 64-row chunks, light ink on a dark ground"""
    one = np.array([[77]], dtype=np.uint8)
    ragged = _grey(11, 37, 53)
    narrow = _grey(12, 130, 17, strokes=3)
    tall = _grey(13, 300, 100, strokes=5)
    tall[2, 50] = tall[135, 3] = tall[297, 97] = 5
    single = _page(40, 50)
    single[13, 31] = 30
    const = np.full((20, 20), 128, dtype=np.uint8)
    light = _grey(15, 60, 90, strokes=6, light=True)
    return [one, ragged, narrow, tall, single, const, light]


@pytest.mark.parametrize("polarity", ["dark", "light", "auto"])
def test_keeping_everything_is_the_plain_builder(polarity):
    srcs = _mixed_sources()
    for cover, cell in ((0, 8), (64, 16), (256, 64)):
        plain = ScanBuilder(len(srcs), 32, max_src=(320, 112), margin=2, cover=cover, polarity=polarity)
        plain.load(srcs)
        plain.run()
        sb = _builder(srcs, 32, (320, 112), cell, min_ink=0, keep=0, polarity=polarity, cover=cover)
        assert torch.equal(sb.out, plain.out), (cover, cell)
        assert torch.equal(sb.geom, plain.geom), (cover, cell)
        geom, stats = sb.geometry(), sb.clean_stats()
        assert geom["status"].tolist() == [so.CONSTANT, 0, 0, 0, 0, so.CONSTANT, 0]
        assert (stats["ink_kept"] == geom["ink"]).all() and not stats["ink_dropped"].any()
        assert (stats["kept"] == stats["components"]).all() and (stats["components"] > 0).tolist() == [False, True, True, True, True, False, True]
    _check(sb, srcs, polarity)


def test_ragged_edges_under_light_polarity():
    """polarity light: the staging fill 255 right of src_w and below src_h would be ink; src_w is no multiple of 16 or of a cell"""
    rs = np.random.RandomState(3)
    srcs = []
    for h, w in ((45, 37), (64, 50), (9, 21)):
        img = np.full((h, w), 30, dtype=np.uint8)
        img[rs.rand(h, w) < 0.02] = 230
        img[h - 1, w - 1] = 230                               # ink in the last row and column
        srcs.append(img)
    for cell in (8, 16, 32):
        sb = _builder(srcs, 32, (70, 60), cell, min_ink=2, keep=16, polarity="light")
        assert (sb.d_src[0, 45:, :] == 255).all() and (sb.d_src[0, :, 37:] == 255).all()     # the fill is there
        geom, stats, labels, _ = _check(sb, srcs, "cell %d" % cell)
        for b, img in enumerate(srcs):
            ch, cw = co.cdiv(img.shape[0], cell), co.cdiv(img.shape[1], cell)
            assert (labels[b, ch:] == -1).all() and (labels[b, :, cw:] == -1).all()
            assert geom[b]["ink"] == int((img == 230).sum())
            assert stats[b]["ink_kept"] + stats[b]["ink_dropped"] == geom[b]["ink"]


def test_diagonal_cells_join_and_a_gap_separates():
    occ = np.zeros((16, 24), dtype=bool)
    for i in range(5):
        occ[6 - i, 1 + i] = True                             # a NE staircase: cells that touch only by their corners
        occ[9 + i, 1 + i] = True                             # a NW staircase
    occ[3, 12] = occ[3, 14] = True                           # one empty cell between them: two components
    occ[10, 12] = occ[12, 12] = True                         # and vertically
    src = _from_cells(occ, 8)
    sb = _builder([src], 32, (128, 192), 8)
    _, stats, labels, _ = _check(sb, [src])
    assert stats[0]["components"] == 6 and stats[0]["occupied_cells"] == 14
    assert len(set(labels[0][2:7, 1:6][occ[2:7, 1:6]])) == 1 and labels[0, 6, 1] == 2 * 24 + 5
    assert len(set(labels[0][9:14, 1:6][occ[9:14, 1:6]])) == 1 and labels[0, 13, 5] == 9 * 24 + 1
    assert labels[0, 3, 12] != labels[0, 3, 14] and labels[0, 10, 12] != labels[0, 12, 12]


def test_a_comb_merges_late_into_the_first_tooth():
    """vertical teeth joined only along the bottom row: every tooth is a component of its own until the last row of cells"""
    occ = np.zeros((70, 142), dtype=bool)
    occ[:, 2::2] = True
    occ[:3, 2] = False                                        # the first tooth is not the tallest: its first cell is (0, 4)
    occ[69, 2:] = True
    src = _from_cells(occ, 8)
    sb = _builder([src], 32, (560, 1136), 8, keep=256)
    _, stats, labels, keep = _check(sb, [src])
    assert stats[0]["components"] == 1 and (labels[0][occ] == 4).all() and keep[0][occ].all()


def test_a_serpentine_over_the_whole_grid_is_one_component():
    """a path one cell wide that fills a 128 x 130 grid of cells (1024 x 1040 at cell 8): far beyond any tile, both ways"""
    occ = np.zeros((128, 130), dtype=bool)
    occ[0::2] = True
    for r in range(1, 128, 2):
        occ[r, 129 if (r // 2) % 2 == 0 else 0] = True
    src = _from_cells(occ, 8)
    sb = _builder([src], 32, (1024, 1040), 8, keep=256)
    _, stats, labels, _ = _check(sb, [src])
    assert (stats[0]["components"], stats[0]["kept"], stats[0]["occupied_cells"]) == (1, 1, 64 * 130 + 64)
    assert (labels[0][occ] == 0).all() and (labels[0][~occ] == -1).all()


def test_a_solid_page_is_one_component_of_every_cell():
    """2048 x 2048 of ink at cell 8: 65536 occupied cells uniting at once.  (A page of one value alone is CONSTANT, so the source
    carries 16 columns of paper to the right: two columns of empty cells.)"""
    src = _page(2048, 2064)
    src[:, :2048] = INK
    sb = _builder([src], 32, (2048, 2064), 8, keep=256)
    _, stats, labels, keep = _check(sb, [src])
    assert [int(stats[0][c]) for c in L.SCAN_CLEAN_COLUMNS] == [1, 1, 2 ** 22, 0, 2 ** 22, 65536]
    assert (labels[0][:, :256] == 0).all() and keep[0][:, :256].all() and not keep[0][:, 256:].any()


def test_the_boundaries_of_the_keep_rule():
    # weights 100, 12 and 11, far apart: min_ink = 12 keeps the first two
    src = _page(96, 160)
    src[8:18, 8:18] = INK
    src[40:43, 64:68] = INK
    src[72:73, 120:131] = INK
    sb = _builder([src], 32, (96, 160), 8, min_ink=12)
    _, stats, _, _ = _check(sb, [src], "min_ink")
    assert [int(stats[0][c]) for c in L.SCAN_CLEAN_COLUMNS] == [3, 2, 112, 11, 100, 7]
    # H = 128, weights 64 and 63: 256 * 64 == 128 * 128 is kept, one pixel less is not
    src = _page(96, 160)
    src[8:16, 16:32] = INK
    src[48:56, 64:72] = INK
    src[80:88, 128:136] = INK
    src[80, 128] = PAPER
    sb = _builder([src], 32, (96, 160), 8, keep=128)
    _, stats, _, _ = _check(sb, [src], "keep_q8")
    assert [int(stats[0][c]) for c in L.SCAN_CLEAN_COLUMNS] == [3, 2, 192, 63, 128, 4]
    sb = _builder([src], 32, (96, 160), 8, keep=129)
    _, stats, _, _ = _check(sb, [src], "keep_q8 + 1")
    assert (stats[0]["kept"], stats[0]["ink_kept"]) == (1, 128)
    # two equal heaviest components at keep = 256: both are kept, the lighter one is not
    src = _page(96, 160)
    src[8:14, 8:14] = INK
    src[70:76, 130:136] = INK
    src[40:45, 70:77] = INK
    sb = _builder([src], 32, (96, 160), 8, keep=256)
    geom, stats, _, _ = _check(sb, [src], "tie")
    assert [int(stats[0][c]) for c in L.SCAN_CLEAN_COLUMNS] == [3, 2, 72, 35, 36, 5]
    assert (geom[0]["y0"], geom[0]["x0"], geom[0]["bh"], geom[0]["bw"]) == (8, 8, 68, 128)


def test_a_speck_inside_the_kept_box_leaves_the_resample():
    """a ring with a speck at its centre, more than a cell away from the ring: dropped, though it lies inside the kept box"""
    src = _page(120, 120)
    src[10:110, 10:14] = src[10:110, 106:110] = INK
    src[10:14, 10:110] = src[106:110, 10:110] = INK
    clean = src.copy()
    src[58:61, 58:61] = INK
    for S in (32, 128):                                       # downscaled, and copied pixel for pixel
        sb = _builder([src, clean], S, (120, 120), 8, keep=256, cover=0)
        geom, stats, _, _ = _check(sb, [src, clean], "S %d" % S)
        assert torch.equal(sb.out[0], sb.out[1]) and stats[0]["ink_dropped"] == 9 and stats[1]["ink_dropped"] == 0
        assert geom[0]["ink"] == geom[1]["ink"] + 9 and [geom[0][c] for c in ("y0", "x0", "bh", "bw")] == [10, 10, 100, 100]
        plain = ScanBuilder(2, S, max_src=(120, 120), margin=2, cover=0)
        plain.load([src, clean])
        plain.run()
        assert not torch.equal(plain.out[0], plain.out[1])


def test_statuses_in_one_batch_and_the_stroke_stage_after_them():
    normal = _drawing(_page(90, 70), 10, 10, 60, 40)
    const = np.full((30, 30), 99, dtype=np.uint8)
    faint = _page(50, 60)
    faint[20:22, 33:36] = INK                                 # H = 6, below min_ink
    tiny = _page(5, 5)
    tiny[1:4, 0:4] = INK                                      # one cell of 5 x 5, 12 ink pixels
    srcs = [normal, const, faint, tiny]
    sb = _builder(srcs, 32, (96, 80), 8, min_ink=10)
    geom, stats, labels, keep = _check(sb, srcs)
    assert geom["status"].tolist() == [0, so.CONSTANT, L.SCAN_NO_COMPONENT, 0]
    assert not sb.out[1].any() and not sb.out[2].any() and sb.out[0].any() and sb.out[3].any()
    assert [int(geom[2][c]) for c in L.SCAN_GEOM_COLUMNS] == [INK, 0, L.SCAN_NO_COMPONENT, 0, 0, 0, 0, 0, 0, 0, 0, 6]
    assert [int(stats[2][c]) for c in L.SCAN_CLEAN_COLUMNS] == [1, 0, 0, 6, 6, 1] and not any(stats[1].tolist())
    assert (labels[1] == -1).all() and not keep[1].any() and not keep[2].any() and (labels[2] >= 0).sum() == 1
    assert [int(stats[3][c]) for c in L.SCAN_CLEAN_COLUMNS] == [1, 1, 12, 0, 12, 1] and labels[3, 0, 0] == 0
    with pytest.raises(ValueError):
        sb.record_offsets(2)
    # with the stroke options on: the blank images stay blank, the others are the normaliser's over the filter's output
    want = StrokeNormalizer(sb.out.clone(), thin=1, radius=1, drop_isolated=True, skip=sb.geom[:, 2].clone()).run().clone()
    st = _builder(srcs, 32, (96, 80), 8, min_ink=10, thin=1, stroke_radius=1, drop_isolated=True)
    assert torch.equal(st.geom, sb.geom) and torch.equal(st.clean_rows, sb.clean_rows)
    assert torch.equal(st.out, want) and not st.out[1].any() and not st.out[2].any() and st.out[0].any()
    assert st.stroke_stats()["skipped"].tolist() == [0, 1, 1, 0]


def test_nothing_stale_after_a_larger_round():
    """one builder, two rounds: the first fills the capacity grid, the second is small; labels outside the small grids are -1"""
    B = 3
    sb = ScanBuilder(B, 32, max_src=(128, 128), margin=2, cover=0, clean_cell=8, clean_min_ink=5, clean_keep=32, debug_cells=True)
    first = [_blobs(70 + b, 128, 128, 60) for b in range(B)]
    for b in range(B):
        first[b][0, 0] = first[b][127, 127] = first[b][0, 127] = first[b][127, 0] = INK
    sb.load(first)
    sb.run()
    _, stats, _, _ = _check(sb, first, "first")
    assert (stats["occupied_cells"] > 40).all()
    second = [_blobs(80, 37, 53, 5), _blobs(81, 9, 100, 3, hi=6), _blobs(82, 64, 16, 4)]
    sb.load(second)
    sb.out.fill_(-1.0)
    sb.run()
    _, _, labels, keep = _check(sb, second, "second")
    assert (labels[0, 5:] == -1).all() and (labels[0, :, 7:] == -1).all() and not keep[0, 5:].any()


@pytest.fixture(scope="module")
def dozen_blobs():
    img = _blobs(300, 300, 400, 12, lo=4, hi=30)
    return img


@pytest.mark.parametrize("cell", [8, 16, 32, 64])
def test_every_cell_size(dozen_blobs, cell):
    sb = _builder([dozen_blobs], 64, (300, 400), cell, min_ink=40, keep=64, cover=32)
    _, stats, _, _ = _check(sb, [dozen_blobs], "cell %d" % cell)
    assert 0 < stats[0]["kept"] <= stats[0]["components"] <= 12


def test_run_replays_from_a_captured_graph():
    """run() with cleaning captured once; later loads of other sizes replay it (the sequence resets its own scratch)"""
    S, B = 32, 3
    sb = ScanBuilder(B, S, max_src=(150, 96), margin=2, cover=64, polarity="auto", clean_cell=16, clean_min_ink=3, clean_keep=64,
                     debug_cells=True)

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
        sb.clean_rows.fill_(-7)
        sb.cell_labels.fill_(-7)
        g.replay()
        _check(sb, srcs, "seed %d" % seed)


def test_the_accessors_refuse_what_was_not_asked_for():
    plain = ScanBuilder(1, 32)
    with pytest.raises(ValueError):
        plain.clean_stats()
    with pytest.raises(ValueError):
        plain.clean_cells()
    with pytest.raises(ValueError):
        ScanBuilder(1, 32, clean_cell=8).clean_cells()
    assert ScanBuilder(1, 32, clean_cell=8).clean_stats().dtype.names == L.SCAN_CLEAN_COLUMNS
