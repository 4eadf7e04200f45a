"""The page splitter on the device (abc_split_scan_pages through abcnet_amd.augment.PageSplitter) against the transcription of
its contract (tests/page_split_oracle.py).  Everything is integers and compared exactly: the f32 canvases, the geometry rows, the
page and drawing tables, the totals, and the label and the canvas of every cell of the capacity grid.  Pages are two-valued
(0 / 255), so that Otsu gives the same ink whatever is erased from them."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import DEFAULT_SPLIT_CELL, DEFAULT_SPLIT_REACH, PageSplitter, ScanBuilder  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402
import page_split_oracle as po  # noqa: E402
import scan_clean_oracle as co  # noqa: E402
import scan_oracle as so  # noqa: E402

POL = {"dark": so.DARK, "light": so.LIGHT, "auto": so.AUTO}
PAPER, INK = 255, 0


def _page(h, w, paper=PAPER):
    return np.full((h, w), paper, dtype=np.uint8)


def _from_cells(occ, cell, h=None, w=None, n=1):
    """a page with n ink pixels (a short horizontal run) in the middle of every occupied cell of the boolean grid `occ`"""
    occ = np.asarray(occ, dtype=bool)
    img = _page(h or occ.shape[0] * cell, w or occ.shape[1] * cell)
    ys, xs = np.nonzero(occ)
    for k in range(n):
        img[ys * cell + cell // 2, xs * cell + 1 + k] = INK
    return img


def _splitter(pages, D, S, max_src, cell, reach, K=16, min_ink=0, keep=0, polarity="dark", cover=0, margin=2, out=None):
    sp = PageSplitter(len(pages), D, S, out=out, max_src=max_src, max_per_page=K, cell=cell, reach=reach, min_ink=min_ink, keep=keep,
                      margin=margin, cover=cover, polarity=polarity, debug_cells=True)
    sp.load(pages)
    sp.out.fill_(-1.0)
    sp.run()
    return sp


def _check(sp, pages, what=""):
    """everything the last run() wrote against the oracle; returns the oracle's dict"""
    q = sp.q
    want = po.split(pages, sp.D, q.max_per_page, sp.S, sp.margin, sp.cover, POL[sp.polarity], q.cell, q.reach, q.min_ink, q.keep_q8,
                    (sp.max_h, sp.pitch))
    labels, canvas = sp.cells()
    assert sp.total.cpu().tolist() == want["total"].tolist(), (what, sp.total, want["total"])
    assert np.array_equal(sp.page_rows.cpu().numpy(), want["pages"]), (what, sp.pages(), want["pages"])
    assert np.array_equal(sp.drawing_rows.cpu().numpy(), want["drawings"]), (what, sp.drawings(), want["drawings"])
    assert np.array_equal(labels, want["labels"]), what
    assert np.array_equal(canvas, want["canvas"]), what
    assert np.array_equal(sp.geom.cpu().numpy(), want["geom"]), (what, sp.geometry(), want["geom"])
    out = sp.out.cpu().numpy()
    for j in range(sp.D):
        assert np.array_equal(out[j, 0], want["out"][j]), (what, j)
    return want


def _four_blobs():
    """200 x 256: four blobs of different shapes, far apart; one of them is two rectangles a few pixels apart"""
    img = _page(200, 256)
    img[10:40, 20:70] = INK
    img[20:30, 30:50] = PAPER                                 # a ring
    img[15:60, 180:200] = INK
    img[120:150, 30:40] = INK
    img[125:135, 48:90] = INK                                 # close to the one before: the same group
    for i in range(50):
        img[130 + i, 170 + i:173 + i] = INK                   # a diagonal stroke
    return img


# ---- 1. against the plain builder
@pytest.mark.parametrize("S", [32, 128])
@pytest.mark.parametrize("cover", [0, 128])
def test_a_canvas_is_the_plain_builder_on_the_page_with_the_rest_erased(S, cover):
    page = _four_blobs()
    cell, reach = 16, 1
    sp = _splitter([page], 6, S, (200, 256), cell, reach, cover=cover)
    want = _check(sp, [page])
    assert sp.total.cpu().tolist() == [4, 4] and sp.pages()[0]["taken"] == 4
    _, canvas = sp.cells()
    alone = [po.erase_outside(page, canvas[0] == j, cell, PAPER) for j in range(4)]
    assert all((a == INK).any() for a in alone) and sum(int((a == INK).sum()) for a in alone) == int((page == INK).sum())
    plain = ScanBuilder(4, S, max_src=(200, 256), margin=2, cover=cover)
    plain.load(alone)
    plain.run()
    assert torch.equal(sp.out[:4], plain.out)
    ink = L.SCAN_GEOM_COLUMNS.index("ink")
    cols = [c for c in range(len(L.SCAN_GEOM_COLUMNS)) if c != ink]
    assert torch.equal(sp.geom[:4][:, cols], plain.geom[:, cols])
    assert sp.geom[:4, ink].cpu().tolist() == [int((a == INK).sum()) for a in alone] == want["drawings"][:4, 2].tolist()
    assert not sp.out[4:].any() and sp.geometry()["status"][4:].tolist() == [L.SCAN_NO_COMPONENT] * 2


# ---- 2. against the clean builder
@pytest.mark.parametrize("cell", [8, 16, 32, 64])
def test_one_kept_group_at_reach_one_is_the_clean_builder(cell):
    page = _page(230, 250)
    page[10:100, 10:14] = page[10:100, 96:100] = INK
    page[10:14, 10:100] = page[96:100, 10:100] = INK
    page[220:223, 240:243] = INK                              # a speck in the corner, dropped by keep = 256
    sp = _splitter([page], 2, 32, (230, 250), cell, 1, keep=256, cover=64)
    _check(sp, [page], "cell %d" % cell)
    sb = ScanBuilder(1, 32, max_src=(230, 250), margin=2, cover=64, clean_cell=cell, clean_keep=256)
    sb.load([page])
    sb.run()
    assert torch.equal(sp.out[:1], sb.out) and sb.out.any()
    g, c = sp.geometry()[0], sb.geometry()[0]
    assert all(g[k] == c[k] for k in L.SCAN_GEOM_COLUMNS if k != "ink") and g["ink"] == c["ink"] - 9
    assert sp.total.cpu().tolist() == [1, 1] and sp.pages()[0]["groups"] == 2


# ---- 3. the reach rule
@pytest.mark.parametrize("reach", [1, 2, 3, 4])
def test_blocks_join_iff_their_gap_is_below_the_reach(reach):
    """pairs of 2 x 2 blocks of cells with gap empty cells between them, side by side, one above the other and diagonal, for
    gap = reach - 1 (one group) and gap = reach (two); the pairs themselves are more than four cells apart"""
    cell, pages, groups = 8, [], []
    for gap in (reach - 1, reach):
        step = 2 + gap
        for dy, dx in ((0, step), (step, 0), (step, step), (step, -step)):
            occ = np.zeros((20, 24), dtype=bool)
            y, x = 3, 9
            occ[y:y + 2, x:x + 2] = True
            occ[y + dy:y + dy + 2, x + dx:x + dx + 2] = True
            pages.append(_from_cells(occ, cell))
            groups.append(1 if gap < reach else 2)
    sp = _splitter(pages, 2 * len(pages), 32, (160, 192), cell, reach)
    _check(sp, pages, "reach %d" % reach)
    assert sp.pages()["groups"].tolist() == groups and sp.pages()["taken"].tolist() == groups


def test_a_chain_of_links_within_reach_is_one_group():
    occ = np.zeros((30, 30), dtype=bool)
    for i in range(8):
        occ[1 + 3 * i, 1 + 2 * i] = True                      # every link two empty cells from the next: within reach 3
    occ[28, 2] = True                                         # and one cell far from the chain
    page = _from_cells(occ, 8)
    sp = _splitter([page], 4, 32, (240, 240), 8, 3)
    _check(sp, [page])
    labels, _ = sp.cells()
    assert sp.pages()[0]["groups"] == 2 and len(set(labels[0][occ][:-1].tolist())) == 1 and labels[0, 1, 1] == 1 * 30 + 1
    sp = _splitter([page], 12, 32, (240, 240), 8, 2)
    _check(sp, [page])
    assert sp.pages()[0]["groups"] == 9


# ---- 4. the order
def test_the_order_is_that_of_the_first_cells():
    occ = np.zeros((16, 20), dtype=bool)
    occ[2:6, 17:19] = True                                    # starts top-right
    occ[3:5, 0:2] = True                                      # starts a row lower at the far left
    occ[10, 5:9] = True
    page = _from_cells(occ, 8, n=3)
    sp = _splitter([page], 4, 32, (128, 160), 8, 1)
    _check(sp, [page])
    assert sp.drawings()["label"].tolist() == [2 * 20 + 17, 3 * 20, 10 * 20 + 5, -1]
    assert sp.drawings()["rank_in_page"].tolist() == [0, 1, 2, -1]
    assert (sp.geometry()["x0"][:3] > np.array([130, -1, 30])).all() and sp.geometry()["x0"][1] < 16


def test_a_comb_keeps_the_label_of_its_first_cell():
    """vertical teeth joined only along the bottom row (the comb of the cleaning tests), and a block left of it that starts on a
    lower row: the comb's label is its first cell's, though its teeth are separate groups until the last row of cells"""
    occ = np.zeros((30, 32), dtype=bool)
    occ[:24, 8::2] = True
    occ[:3, 8] = False                                        # the first tooth is not the tallest: the first cell is (0, 10)
    occ[23, 8:] = True
    occ[5:7, 0:2] = True
    page = _from_cells(occ, 8)
    sp = _splitter([page], 3, 32, (240, 256), 8, 1)
    _check(sp, [page])
    assert sp.drawings()["label"].tolist() == [10, 5 * 32, -1] and sp.pages()[0]["groups"] == 2


# ---- 5. overflow
def _dots(n, per_row=6, cell=8):
    """n single-cell groups four cells apart, on a page of 256 x 256"""
    occ = np.zeros((32, 32), dtype=bool)
    for i in range(n):
        occ[1 + 5 * (i // per_row), 1 + 5 * (i % per_row)] = True
    return _from_cells(occ, cell)


def test_a_page_takes_at_most_its_share():
    K = 5
    pages = [_dots(K + 1), _dots(K), _dots(2)]
    S, D = 32, 16
    big = torch.full((D + 1, 1, S, S), 7.25, dtype=torch.float32, device="cuda")
    sp = _splitter(pages, D, S, (256, 256), 8, 1, K=K, out=big[:D])
    _check(sp, pages)
    assert sp.pages()["status"].tolist() == [L.SCAN_SPLIT_PAGE_FULL, 0, 0] and sp.pages()["taken"].tolist() == [K, K, 2]
    assert sp.pages()["kept"].tolist() == [K + 1, K, 2] and sp.total.cpu().tolist() == [2 * K + 2, 2 * K + 3]
    assert bool((big[D] == 7.25).all())


def test_canvases_that_do_not_fit_are_dropped_and_said_so():
    pages = [_dots(3), _dots(4), _page(40, 40, 77), _dots(2), _dots(1)]
    S, D = 32, 5
    big = torch.full((D + 1, 1, S, S), 7.25, dtype=torch.float32, device="cuda")
    sp = _splitter(pages, D, S, (256, 256), 8, 1, out=big[:D])
    _check(sp, pages)
    full = L.SCAN_SPLIT_BATCH_FULL
    assert sp.pages()["status"].tolist() == [0, full, so.CONSTANT, full, full]
    assert sp.pages()["first"].tolist() == [0, 3, 5, 5, 5] and sp.pages()["taken"].tolist() == [3, 2, 0, 0, 0]
    assert sp.total.cpu().tolist() == [D, 10] and (sp.drawings()["page"] == [0, 0, 0, 1, 1]).all()
    assert bool((big[D] == 7.25).all()) and bool((big[:D] >= 0).all())
    # and both at once: K cuts the second page to two, D the fourth to none
    sp = _splitter(pages, D, S, (256, 256), 8, 1, K=2, out=big[:D])
    _check(sp, pages)
    page_full = L.SCAN_SPLIT_PAGE_FULL
    assert sp.pages()["status"].tolist() == [page_full, page_full, so.CONSTANT, full, full]
    assert sp.pages()["taken"].tolist() == [2, 2, 0, 1, 0] and sp.total.cpu().tolist() == [D, 10]
    assert bool((big[D] == 7.25).all())


# ---- 6. ragged sizes and statuses in one batch
def _ragged():
    rs = np.random.RandomState(3)
    pages = []
    for h, w in ((45, 37), (64, 50), (9, 21), (256, 200)):
        img = _page(h, w, 0)                                  # light ink on a dark ground
        for _ in range(max(2, h * w // 600)):                 # dots of 2 x 2, and single pixels that min_ink = 2 drops
            y, x = int(rs.randint(0, h - 1)), int(rs.randint(0, w - 1))
            img[y:y + 2, x:x + 2] = 255
            img[int(rs.randint(0, h)), int(rs.randint(0, w))] = 255
        img[h - 2:, w - 2:] = 255                             # ink in the last row and column
        pages.append(img)
    return pages


@pytest.mark.parametrize("cell,reach", [(8, 2), (16, 1), (32, 3)])
def test_ragged_pages_and_statuses_in_one_batch(cell, reach):
    good = _ragged()
    const = _page(30, 30, 99)
    pages = [good[0], const, good[1], good[2], good[3]]
    sp = _splitter(pages, 64, 32, (256, 208), cell, reach, polarity="light", min_ink=2, cover=32)
    assert (sp.d_src[0, 45:, :] == 255).all() and (sp.d_src[0, :, 37:] == 255).all()     # the fill would be ink
    want = _check(sp, pages, "cell %d" % cell)
    assert sp.pages()["status"][1] == so.CONSTANT and want["total"][0] >= 4
    # a BAD_PARAMS page between good ones, the device table alone
    sp.d.params_host = None
    torch.cuda.synchronize()
    sp.d_par[2, 1] = 209                                      # src_w past the pitch
    sp.out.fill_(-1.0)
    sp.run()
    torch.cuda.synchronize()
    bad = [good[0], const, po.BAD, good[2], good[3]]
    _check(sp, bad, "bad, cell %d" % cell)
    assert sp.pages()["status"][2] == so.BAD_PARAMS and not torch.isnan(sp.out).any()
    # the good pages' canvases are what they are alone
    dr, out = sp.drawings(), sp.out.clone()
    for p in (0, 3, 4):
        one = _splitter([pages[p]], 64, 32, (256, 208), cell, reach, polarity="light", min_ink=2, cover=32)
        n = int(one.total[0])
        mine = np.nonzero(dr["page"] == p)[0]
        assert n == len(mine) > 0 and torch.equal(one.out[:n], out[mine[0]:mine[0] + n])
        assert torch.equal(one.geom[:n], sp.geom[mine[0]:mine[0] + n])


def test_a_bad_page_is_refused_at_call_time_when_the_host_table_is_given():
    pages = [_dots(2), _dots(1)]
    sp = _splitter(pages, 4, 32, (256, 256), 8, 1)
    sp._np_par[1] = (257, 256)
    with pytest.raises(L.AbcNetHipError, match=r"\(-1\).*src_h"):
        sp.run()


# ---- 7. the edges of the keep rule, per page
def test_the_boundaries_of_the_keep_rule_per_page():
    # page 0: weights 100, 12 and 11 (min_ink = 12 keeps two); page 1: H = 128, weights 64 and 63: 256 * 64 == 128 * 128 is kept
    a = _page(96, 160)
    a[8:18, 8:18] = INK
    a[40:43, 64:68] = INK
    a[72:73, 120:131] = INK
    b = _page(96, 160)
    b[8:16, 16:32] = INK
    b[48:56, 64:72] = INK
    b[80:88, 128:136] = INK
    b[80, 128] = PAPER
    sp = _splitter([a, b], 8, 32, (96, 160), 8, 1, min_ink=12)
    _check(sp, [a, b], "min_ink")
    assert sp.pages()["kept"].tolist() == [2, 3] and sp.pages()["ink_dropped"].tolist() == [11, 0]
    sp = _splitter([a, b], 8, 32, (96, 160), 8, 1, keep=128)
    _check(sp, [a, b], "keep 128")                            # H differs: 100 on page 0 (50 needed), 128 on page 1 (64 needed)
    assert sp.pages()["kept"].tolist() == [1, 2] and sp.pages()["ink_kept"].tolist() == [100, 192]
    sp = _splitter([a, b], 8, 32, (96, 160), 8, 1, keep=129)
    _check(sp, [a, b], "keep 129")
    assert sp.pages()["kept"].tolist() == [1, 1] and sp.drawings()["weight"][:3].tolist() == [100, 128, 0]
    sp = _splitter([a, b], 8, 32, (96, 160), 8, 1, keep=31)   # 256 * 12 = 3072 < 31 * 100; 256 * 12 >= 30 * 100
    _check(sp, [a, b], "keep 31")
    assert sp.pages()["kept"].tolist() == [1, 3]
    sp = _splitter([a, b], 8, 32, (96, 160), 8, 1, keep=30)
    _check(sp, [a, b], "keep 30")
    assert sp.pages()["kept"].tolist() == [2, 3]
    sp = _splitter([a, b], 8, 32, (96, 160), 8, 1, min_ink=101)
    _check(sp, [a, b], "nothing kept on page 0")
    assert sp.pages()["status"].tolist() == [L.SCAN_NO_COMPONENT, 0] and sp.drawings()["page"][0] == 1


# ---- 8. nothing stale
def test_nothing_stale_after_a_round_with_many_drawings():
    rs = np.random.RandomState(5)
    many = []
    for _ in range(2):
        occ = rs.rand(16, 16) < 0.12
        occ[0, 0] = occ[15, 15] = True
        many.append(_from_cells(occ, 8, n=2))
    few = [_dots(1)[:40, :56], _page(20, 20, 5)]
    sp = PageSplitter(2, 24, 32, max_src=(128, 128), cell=8, reach=1, margin=2, cover=0, debug_cells=True)
    sp.load(many)
    sp.run()
    want = _check(sp, many, "first")
    assert want["total"][0] > 8
    sp.load(few)
    sp.run()
    _check(sp, few, "second")
    fresh = _splitter(few, 24, 32, (128, 128), 8, 1)
    for a, b in ((sp.out, fresh.out), (sp.geom, fresh.geom), (sp.page_rows, fresh.page_rows), (sp.drawing_rows, fresh.drawing_rows),
                 (sp.total, fresh.total), (sp.cell_labels, fresh.cell_labels), (sp.cell_canvas, fresh.cell_canvas)):
        assert torch.equal(a, b)
    assert sp.total.cpu().tolist() == [1, 1]


# ---- 9. a serpentine over the whole grid
@pytest.mark.parametrize("reach", [1, 3])
def test_a_serpentine_over_the_whole_grid_is_one_group(reach):
    occ = np.zeros((128, 128), dtype=bool)
    occ[0::2] = True
    for r in range(1, 128, 2):
        occ[r, 127 if (r // 2) % 2 == 0 else 0] = True
    page = _from_cells(occ, 8)
    sp = _splitter([page], 2, 32, (1024, 1024), 8, reach)
    _check(sp, [page])
    labels, canvas = sp.cells()
    assert [int(v) for v in sp.pages()[0]] == [0, 1, 1, 0, 1, 64 * 128 + 64, 0, 64 * 128 + 64]
    assert (labels[0][occ] == 0).all() and (canvas[0][occ] == 0).all() and (labels[0][~occ] == -1).all()


# ---- 10. a captured graph
def test_run_replays_from_a_captured_graph():
    P, D, S = 2, 12, 32
    sp = PageSplitter(P, D, S, max_src=(150, 96), cell=16, reach=2, min_ink=3, margin=2, cover=64, debug_cells=True)

    def batch(seed):
        rs = np.random.RandomState(seed)
        pages = []
        for _ in range(P):
            h, w = int(rs.randint(40, 151)), int(rs.randint(40, 97))
            img = _page(h, w)
            for _ in range(int(rs.randint(2, 7))):
                y, x = int(rs.randint(0, h - 8)), int(rs.randint(0, w - 8))
                img[y:y + int(rs.randint(2, 9)), x:x + int(rs.randint(2, 9))] = INK
            pages.append(img)
        return pages
    sp.load(batch(100))
    sp.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.run()
    for seed in (200, 300):
        pages = batch(seed)
        sp.load(pages)
        sp.out.fill_(-1.0)
        for t in (sp.geom, sp.page_rows, sp.drawing_rows, sp.total, sp.cell_labels, sp.cell_canvas):
            t.fill_(-7)
        g.replay()
        _check(sp, pages, "seed %d" % seed)


# ---- 11. the use case
SHEET_SEED, SHEET_CELL, SHEET_REACH = 7, DEFAULT_SPLIT_CELL, DEFAULT_SPLIT_REACH     # the chosen cell and reach


def _sheet(seed):
    """a 2 x 2 sheet of four drawings of 128 x 128 with 96 pixels of white between and around them; their places"""
    imgs, _ = drawn_molecules(4, 128, seed)
    page = _page(544, 544)
    alone, places = [], []
    for k in range(4):
        y, x = 96 + 224 * (k // 2), 96 + 224 * (k % 2)
        one = np.where(imgs[k, 0] > 0, INK, PAPER).astype(np.uint8)
        page[y:y + 128, x:x + 128] = one
        alone.append(one)
        places.append((y, x))
    return page, alone, places


def test_a_sheet_of_four_drawings_comes_out_as_the_four_drawings():
    page, alone, places = _sheet(SHEET_SEED)
    # the condition on the input: each drawing is one group and no two are joined at the chosen cell and reach
    thr, inv, ink, cells, lab, weight = po.analyse(page, so.DARK, SHEET_CELL, SHEET_REACH, (544, 544))
    assert len(weight) == 4
    for k, (y, x) in enumerate(places):
        inside = np.zeros_like(ink)
        inside[y:y + 128, x:x + 128] = True
        own = set(lab[co.cell_ink(ink & inside, SHEET_CELL) > 0].tolist())
        assert len(own) == 1 and weight[own.pop()] == int((alone[k] == INK).sum()), k
    S = 64
    sp = _splitter([page], 4, S, (544, 544), None, None, cover=128, margin=S * 20 // 512)       # (None: the defaults)
    assert (sp.q.cell, sp.q.reach) == (SHEET_CELL, SHEET_REACH)
    _check(sp, [page])
    sb = ScanBuilder(4, S, max_src=(128, 128), cover=128)
    sb.load(alone)
    sb.run()
    assert torch.equal(sp.out, sb.out) and sp.total.cpu().tolist() == [4, 4]
    g = sb.geometry()
    for j, (y, x) in enumerate(places):                       # reading order is the order of the places
        rows, cols = int(g[j]["rows"]), int(g[j]["cols"])
        corners = np.array([[g[j]["ddx"], g[j]["ddy"]], [g[j]["ddx"] + rows, g[j]["ddy"] + cols]], dtype=np.float64)
        back = sp.page_positions(j, corners)
        want = np.array([[y + g[j]["y0"], x + g[j]["x0"]], [y + g[j]["y0"] + g[j]["bh"], x + g[j]["x0"] + g[j]["bw"]]], dtype=np.float64)
        np.testing.assert_allclose(back, want, rtol=0, atol=1e-9)
        assert sp.record_offsets(j)[:2] == sb.record_offsets(j)[:2]


# ---- 12. the accessors
def test_the_accessors_refuse_what_was_not_asked_for():
    sp = PageSplitter(1, 2, 32, max_src=(64, 64), cell=8, reach=1)
    with pytest.raises(ValueError):
        sp.cells()
    sp.load([_dots(1)[:64, :64]])
    sp.run()
    assert sp.pages().dtype.names == L.SCAN_PAGE_COLUMNS and sp.drawings().dtype.names == L.SCAN_DRAWING_COLUMNS
    assert sp.geometry().dtype.names == L.SCAN_GEOM_COLUMNS and sp.n_canvases.data_ptr() == sp.total.data_ptr()
    assert sp.n_canvases.dtype == torch.int32 and tuple(sp.n_canvases.shape) == (1,) and int(sp.n_canvases) == 1
    with pytest.raises(ValueError):
        sp.record_offsets(1)                                  # an unused canvas
    with pytest.raises(ValueError):
        sp.page_positions(1, [[0.0, 0.0]])
    with pytest.raises(ValueError):
        sp.load([_dots(1)])                                   # 256 x 256 exceeds the staging capacity
