"""The host side of the scan input path (abcnet_amd.augment: otsu_threshold, fit_scan, scan_record_offsets; the binding of
abc_build_scan_images) and the numpy oracle of its contract (tests/scan_oracle.py).  No kernel is launched here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import ScanBuilder, fit_scan, otsu_threshold, scan_record_offsets  # noqa: E402
import scan_oracle as so  # noqa: E402


def _hist(**bins):
    h = np.zeros(256, dtype=np.int64)
    for v, n in bins.items():
        h[int(v[1:])] = n
    return h


def test_two_values_give_the_lower_one():
    for a, b, na, nb in ((0, 255, 10, 90), (17, 18, 1, 1), (60, 200, 1000, 3), (254, 255, 5, 5)):
        h = _hist(**{"v%d" % a: na, "v%d" % b: nb})
        assert otsu_threshold(h) == a and so.threshold(h) == a


def test_an_exact_tie_goes_to_the_smallest_threshold():
    """equal counts at 0, 100 and 200: sigma is the same (bit for bit) on t in [0, 99] and t in [100, 199]"""
    h = _hist(v0=7, v100=7, v200=7)
    s, _ = so.sigmas(h)
    assert s[0] == s[99] == s[100] == s[199] and s[0] == s.max() and s[200] == -1.0
    assert otsu_threshold(h) == 0 and so.threshold(h) == 0


def test_a_single_value_has_no_threshold():
    for v in (0, 93, 255):
        h = _hist(**{"v%d" % v: 1234})
        assert otsu_threshold(h) is None and so.threshold(h) is None


def test_sums_stay_exact_at_the_capacity():
    """4096 * 4096 - 5 pixels at 255 and 5 at 254: S = 255 N - 5 is near 2^32 and d near 2^56; the only admissible t is 254"""
    N = 4096 * 4096
    h = _hist(v255=N - 5, v254=5)
    assert otsu_threshold(h) == 254 and so.threshold(h) == 254
    s, w0 = so.sigmas(h)
    S = 255 * (N - 5) + 254 * 5
    d = S * 5 - N * (254 * 5)
    assert w0[254] == 5 and w0[255] == N and d == 5 * (N - 5) and d < 2 ** 56
    assert s[254] == (float(d) * float(d)) / (5.0 * float(N - 5)) and (s[:254] == -1).all() and s[255] == -1
    # all the weight at the top value of every sum: S = 255 * 2^24 - 255 < 2^32, |d| < 2^56
    h = _hist(v255=N - 1, v0=1)
    assert otsu_threshold(h) == 0
    s, _ = so.sigmas(h)
    assert (s[:255] == s[0]).all()      # the same two classes for every t in 0 .. 254


def test_argmax_agrees_with_the_textbook_between_class_variance():
    """300 seeded random histograms: the rule's arg-max is an arg-max of w0 w1 (mu0 - mu1)^2 / N^2 evaluated in floats (the
    two forms differ by rounding only, so the textbook value at the rule's threshold is within a relative 1e-9 of its maximum),
    and the host mirror and the oracle agree bit for bit"""
    rs = np.random.RandomState(2024)
    for k in range(300):
        kind = k % 3
        if kind == 0:
            h = rs.randint(0, 1000, size=256)
        elif kind == 1:      # two bumps on an empty ground
            h = np.zeros(256, dtype=np.int64)
            for c, wd, n in ((rs.randint(20, 100), rs.randint(2, 20), rs.randint(50, 5000)), (rs.randint(140, 240), rs.randint(2, 15), rs.randint(50, 50000))):
                h[max(0, c - wd):c + wd] += rs.randint(1, n, size=len(h[max(0, c - wd):c + wd]))
        else:                # sparse
            h = rs.randint(0, 50, size=256) * (rs.rand(256) < 0.1)
            h[rs.randint(0, 128)] += 3
            h[rs.randint(128, 256)] += 5
        h = h.astype(np.int64)
        thr = otsu_threshold(h)
        assert thr == so.threshold(h)
        N = float(h.sum())
        v = np.arange(256, dtype=np.float64)
        w0 = np.cumsum(h).astype(np.float64)
        w1 = N - w0
        ok = (w0 > 0) & (w1 > 0)
        s0 = np.cumsum(h * v)
        text = np.full(256, -1.0)
        mu0, mu1 = s0[ok] / w0[ok], (s0[-1] - s0[ok]) / w1[ok]
        text[ok] = (w0[ok] / N) * (w1[ok] / N) * (mu0 - mu1) ** 2
        assert ok[thr] and text[thr] >= text.max() * (1 - 1e-9), (k, thr, int(np.argmax(text)))
        assert int(np.argmax(text)) == thr, (k, thr, int(np.argmax(text)))
        # and nothing before thr reaches the maximum in the exact form: the smallest one
        s, _ = so.sigmas(h)
        assert (s[:thr] < s[thr]).all() and (s <= s[thr]).all()


def test_fit_scan():
    # m <= L: copied, centred
    assert fit_scan(10, 20, 32, 2) == (10, 20, 11, 6)
    assert fit_scan(28, 28, 32, 2) == (28, 28, 2, 2)
    assert fit_scan(32, 5, 32, 0) == (32, 5, 0, 13)
    # floor division: 100 x 37 into L = 28 -> 28, 37 * 28 // 100 = 10 (10.36)
    assert fit_scan(100, 37, 32, 2) == (28, 10, 2, 11)
    assert fit_scan(37, 100, 32, 2) == (10, 28, 11, 2)
    assert fit_scan(29, 29, 32, 2) == (28, 28, 2, 2)
    assert fit_scan(300, 299, 64, 3) == (58, 57, 3, 3)          # 299 * 58 // 300 = 57 (57.8)
    # rows, cols >= 1
    assert fit_scan(4096, 1, 32, 2) == (28, 1, 2, 15)
    assert fit_scan(1, 4096, 512, 20) == (1, 472, 255, 20)
    for bh, bw, S, m in ((4096, 1, 32, 2), (100, 37, 32, 2), (7, 9, 64, 0), (4096, 4096, 8, 3)):
        assert fit_scan(bh, bw, S, m) == so.fit(bh, bw, S, m)
    with pytest.raises(ValueError):
        fit_scan(10, 10, 32, 16)
    with pytest.raises(ValueError):
        fit_scan(0, 10, 32, 2)


def test_record_offsets_map_the_box_corner_onto_the_canvas():
    for (y0, x0, bh, bw, S, m) in ((5, 9, 20, 10, 32, 2), (40, 3, 100, 37, 32, 2), (0, 0, 300, 299, 64, 3), (1000, 2000, 3000, 64, 512, 20)):
        rows, cols, ddx, ddy = fit_scan(bh, bw, S, m)
        sx, sy, ox, oy = scan_record_offsets(y0, x0, bh, bw, rows, cols, ddx, ddy)
        assert sx == rows / bh and sy == cols / bw
        assert abs(y0 * sx + ox - ddx) < 1e-9 and abs(x0 * sy + oy - ddy) < 1e-9
        # the far corner of the box lands on the far corner of the placed drawing
        assert abs((y0 + bh) * sx + ox - (ddx + rows)) < 1e-9 and abs((x0 + bw) * sy + oy - (ddy + cols)) < 1e-9
    # not resized: the map is a pure shift, exactly
    assert scan_record_offsets(5, 9, 20, 10, 20, 10, 6, 11) == (1.0, 1.0, 1.0, 2.0)


def test_binding_covers_the_scan_entry():
    lib = L.load()
    assert "abc_build_scan_images" in L.SYMBOLS and "abc_scan_desc_size" in L.SYMBOLS
    assert lib.abc_scan_desc_size() == C.sizeof(L.ScanDesc)
    assert len(L.SCAN_GEOM_COLUMNS) == len(so.GEOM) == 12 and tuple(so.GEOM) == L.SCAN_GEOM_COLUMNS
    assert (so.DARK, so.LIGHT, so.AUTO, so.CONSTANT, so.BAD_PARAMS) == (L.SCAN_DARK, L.SCAN_LIGHT, L.SCAN_AUTO, L.SCAN_CONSTANT,
                                                                       L.SCAN_BAD_PARAMS)
    # refused on the host, nothing launched
    d = L.ScanDesc()
    assert lib.abc_build_scan_images(C.byref(d), None) == -1 and b"null" in lib.abc_last_error()


def test_oracle_on_a_tiny_scan():
    """the oracle itself, by hand: a 6 x 8 grey image whose ink is a 2 x 4 block, S = 8, margin = 1"""
    img = np.full((6, 8), 200, dtype=np.uint8)
    img[2:4, 3:7] = 40
    out, g = so.build(img, 8, 1, 0, so.DARK)
    assert so.geom_row(g) == [40, 0, 0, 2, 3, 2, 4, 2, 4, 3, 2, 8]
    want = np.zeros((8, 8), np.float32)
    want[3:5, 2:6] = 1
    np.testing.assert_array_equal(out, want)
    out, g = so.build(img, 8, 1, 0, so.AUTO)      # the dark side is the minority: still DARK
    assert g["inverted"] == 0
    out, g = so.build(255 - img, 8, 1, 0, so.AUTO)
    assert g["inverted"] == 1 and g["thr"] == 55
    np.testing.assert_array_equal(out, want)
    out, g = so.build(np.full((3, 3), 9, np.uint8), 8, 1, 0, so.DARK)
    assert g["status"] == so.CONSTANT and g["thr"] == -1 and not out.any()


def test_scan_builder_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        assert tuple(ScanBuilder(1, 32).out.shape) == (1, 1, 32, 32)
        return
    with pytest.raises(L.AbcNetHipError, match="no CPU fallback"):
        ScanBuilder(1, 32)
