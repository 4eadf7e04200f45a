"""The page splitter's host side, no GPU: the oracle's partition against a brute-force closure and against the cleaning oracle's at
reach 1, page_positions as the inverse of the record offsets, PageSplitter's argument checks (they run before the device), and
the new symbols with the size of their descriptor."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import (DEFAULT_SPLIT_CELL, DEFAULT_SPLIT_REACH, PageSplitter, fit_scan, scan_page_positions,  # noqa: E402
                                scan_record_offsets)
import page_split_oracle as po  # noqa: E402
import scan_clean_oracle as co  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("reach", [1, 2, 3, 4])
def test_the_flood_fill_is_the_closure_of_the_reach_rule(reach):
    rs = np.random.RandomState(10 + reach)
    seen = 0
    for _ in range(40):
        h, w = int(rs.randint(1, 13)), int(rs.randint(1, 13))
        occ = rs.rand(h, w) < rs.choice([0.05, 0.15, 0.3, 0.6])
        lab = po.partition(occ, reach)
        assert np.array_equal(lab, po.brute_partition(occ, reach)), (h, w, occ)
        assert ((lab >= 0) == occ).all()
        seen += len(set(lab[occ].tolist()))
        if reach == 1:
            assert np.array_equal(lab, co.partition(occ))
    assert seen > 20                                          # (the grids were not all empty or all one group)


def test_a_wider_reach_only_joins():
    rs = np.random.RandomState(2)
    occ = rs.rand(12, 12) < 0.12
    groups = [len(set(po.partition(occ, r)[occ].tolist())) for r in (1, 2, 3, 4)]
    assert groups == sorted(groups, reverse=True) and groups[0] > groups[-1]
    # two cells two apart: separate at reach 1, one group (under the smaller index) from reach 2
    occ = np.zeros((3, 5), dtype=bool)
    occ[0, 4] = occ[2, 2] = True
    assert po.partition(occ, 1)[2, 2] == 12 and po.partition(occ, 2)[2, 2] == 4


def test_the_packing_of_the_oracle_on_a_hand_case():
    """three pages of 3, 0 and 2 single-pixel groups into four canvases, two a page at most"""
    def page(cells):
        img = np.full((64, 64), 255, dtype=np.uint8)
        for cy, cx in cells:
            img[8 * cy + 4, 8 * cx + 4] = 0
        return img
    pages = [page([(0, 5), (3, 0), (6, 6)]), np.full((10, 10), 9, dtype=np.uint8), page([(1, 1), (5, 5)]), po.BAD]
    w = po.split(pages, 3, 2, 16, 1, 0, 0, 8, 1, 0, 0, (64, 64))
    assert w["total"].tolist() == [3, 5]
    assert w["pages"].tolist() == [[po.PAGE_FULL, 3, 3, 0, 2, 3, 0, 3], [1, 0, 0, 2, 0, 0, 0, 0],
                                   [po.BATCH_FULL, 2, 2, 2, 1, 2, 0, 2], [2, 0, 0, 3, 0, 0, 0, 0]]
    assert w["drawings"].tolist() == [[0, 5, 1, 0], [0, 24, 1, 1], [2, 9, 1, 0]]
    assert w["canvas"][0, 0, 5] == 0 and w["canvas"][0, 3, 0] == 1 and w["canvas"][0, 6, 6] == -1 and w["canvas"][2, 5, 5] == -1
    assert w["geom"][1].tolist() == [0, 0, 0, 28, 4, 1, 1, 1, 1, 7, 7, 1] and w["out"][1, 7, 7] == 1.0 and w["out"][1].sum() == 1.0


def test_page_positions_inverts_the_record_offsets():
    # hand rows (y0, x0, bh, bw) at size 64, margin 2: a downscaled fit, and a copied one (the box is smaller than the canvas)
    for y0, x0, bh, bw in ((100, 300, 240, 120), (7, 9, 31, 50), (0, 0, 60, 60), (411, 5, 1, 333)):
        rows, cols, ddx, ddy = fit_scan(bh, bw, 64, 2)
        offs = scan_record_offsets(y0, x0, bh, bw, rows, cols, ddx, ddy)
        copied = (rows, cols) == (bh, bw)
        assert copied == (max(bh, bw) <= 60)
        src = np.array([[y0, x0], [y0 + bh, x0 + bw], [y0 + bh / 2, x0 + bw / 3], [y0 + 0.25, x0 + 7.5]], dtype=np.float64)
        on_canvas = src * np.array(offs[:2]) + np.array(offs[2:])
        np.testing.assert_allclose(on_canvas[0], [ddx, ddy], rtol=0, atol=1e-9)
        np.testing.assert_allclose(on_canvas[1], [ddx + rows, ddy + cols], rtol=0, atol=1e-9)
        back = scan_page_positions(offs, on_canvas)
        np.testing.assert_allclose(back, src, rtol=0, atol=1e-9)
        if copied:                                            # a pure shift: exact
            assert offs[:2] == (1.0, 1.0) and np.array_equal(back, src)
    assert scan_page_positions((0.5, 0.25, 3.0, -1.0), np.zeros((2, 3, 2))).shape == (2, 3, 2)
    with pytest.raises(ValueError):
        scan_page_positions((1.0, 1.0, 0.0, 0.0), np.zeros((4, 3)))


@pytest.mark.parametrize("kw", [
    dict(polarity="grey"), dict(cell=12), dict(cell=True), dict(reach=0), dict(reach=5), dict(reach=1.5), dict(max_per_page=0),
    dict(max_per_page=65), dict(min_ink=-1), dict(min_ink=2 ** 31), dict(keep=257), dict(keep=-1), dict(keep=0.5), dict(size=20),
    dict(size=8200), dict(max_src=(4097, 64)), dict(max_src=(64, 0)), dict(pages=0), dict(pages=65536), dict(canvases=0),
    dict(canvases=65536), dict(margin=16), dict(margin=-1), dict(cover=257)])
def test_the_arguments_are_refused_before_the_device(kw):
    args = dict(pages=2, canvases=8, size=32)
    args.update(kw)
    with pytest.raises(ValueError, match="PageSplitter"):
        PageSplitter(**args)


def test_the_defaults_are_in_range():
    assert DEFAULT_SPLIT_CELL in L.SCAN_CLEAN_CELLS and 1 <= DEFAULT_SPLIT_REACH <= L.SCAN_SPLIT_MAX_REACH


def test_the_symbols_are_declared_and_the_descriptor_is_sized():
    header = open(os.path.join(ROOT, "include", "abcnet_hip.h")).read()
    for name in ("abc_split_scan_pages", "abc_scan_split_desc_size", "abc_scan_split_scratch_bytes"):
        assert name in L.SYMBOLS and (name + "(") in header
    assert "ABC_SCAN_SPLIT_PAGE_FULL = 16" in header and "ABC_SCAN_SPLIT_BATCH_FULL = 32" in header
    assert (L.SCAN_SPLIT_PAGE_FULL, L.SCAN_SPLIT_BATCH_FULL) == (16, 32) == (po.PAGE_FULL, po.BATCH_FULL)
    assert L.SCAN_PAGE_COLUMNS == po.PAGE and L.SCAN_DRAWING_COLUMNS == po.DRAWING
    assert (L.ScanSplitDesc, "abc_scan_split_desc_size") in L.SELF_SIZED_SINCE
    # six pointers, six int32: no padding on any LP64 ABI
    assert C.sizeof(L.ScanSplitDesc) == 6 * C.sizeof(C.c_void_p) + 6 * 4
    lib = L.load()
    assert lib.abc_scan_split_desc_size() == C.sizeof(L.ScanSplitDesc)
    cells = (2048 // 32) * (2048 // 32)
    assert lib.abc_scan_split_scratch_bytes(4, 2048, 2048, 32, 16) >= 4 * 4 * (4 * cells + L.SCAN_NBOX)
    assert lib.abc_scan_split_scratch_bytes(4, 2048, 2048, 32, 16) % 16 == 0
    for bad in ((0, 64, 64, 8, 1), (1, 64, 64, 12, 1), (1, 64, 60, 8, 1), (1, 64, 64, 8, 0), (1, 64, 64, 8, 65536), (1, 4097, 64, 8, 1)):
        assert lib.abc_scan_split_scratch_bytes(*bad) < 0
