"""The host side of the cell component filter (the binding of abc_build_scan_images_clean, its guards, ScanBuilder's argument
checks) and the oracle of its contract (tests/scan_clean_oracle.py).  No kernel is launched here: every guard answers before a
launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import ScanBuilder  # noqa: E402
import scan_clean_oracle as co  # noqa: E402
import scan_oracle as so  # noqa: E402


def test_partition_equals_scipy_label_on_random_grids():
    ndi = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(16)
    for k in range(300):
        h, w = int(rs.randint(1, 24)), int(rs.randint(1, 24))
        occ = rs.rand(h, w) < rs.choice([0.1, 0.3, 0.5, 0.7])
        lab = co.partition(occ)
        want, n = ndi.label(occ, structure=np.ones((3, 3)))
        assert ((lab >= 0) == occ).all()
        # the same partition: a bijection between the two labellings, and each label the smallest index of its set
        pairs = {(int(a), int(b)) for a, b in zip(lab[occ], want[occ])}
        assert len(pairs) == n == len({a for a, _ in pairs}) == len({b for _, b in pairs}), k
        idx = np.arange(h * w).reshape(h, w)
        for a, b in pairs:
            assert a == int(idx[want == b].min())


def test_oracle_by_hand():
    """a 20 x 40 page, cell 8: a 6 x 6 block (36 ink pixels) at the top left, a 2 x 2 speck (4) two cells to the right of it
    and a 3 x 1 mark (3) in the last, partial row of cells"""
    img = np.full((20, 40), 200, dtype=np.uint8)
    img[1:7, 1:7] = 40
    img[2:4, 25:27] = 40
    img[17:20, 38] = 40
    cap = (24, 48)
    out, g, st, lab, keep = co.build(img, 16, 1, 0, so.DARK, 8, 0, 0, cap)
    assert co.stats_row(st) == [3, 3, 43, 0, 36, 3] and lab.shape == (3, 6)
    assert lab[0, 0] == 0 and lab[0, 3] == 3 and lab[2, 4] == 16 and (lab >= 0).sum() == 3 and keep.sum() == 3
    plain, pg = so.build(img, 16, 1, 0, so.DARK)
    assert so.geom_row(g) == so.geom_row(pg) and np.array_equal(out, plain)      # keep-all is the plain builder
    out, g, st, lab, keep = co.build(img, 16, 1, 0, so.DARK, 8, 0, 256, cap)
    assert co.stats_row(st) == [3, 1, 36, 7, 36, 3] and keep.sum() == 1 and keep[0, 0] == 1
    assert (g["y0"], g["x0"], g["bh"], g["bw"], g["ink"], g["status"]) == (1, 1, 6, 6, 43, 0)
    out, g, st, lab, keep = co.build(img, 16, 1, 0, so.DARK, 8, 4, 0, cap)       # weight == min_ink is kept, one less is not
    assert co.stats_row(st) == [3, 2, 40, 3, 36, 3]
    out, g, st, lab, keep = co.build(img, 16, 1, 0, so.DARK, 8, 37, 0, cap)
    assert g["status"] == co.NO_COMPONENT and not out.any() and keep.sum() == 0
    assert so.geom_row(g) == [40, 0, co.NO_COMPONENT, 0, 0, 0, 0, 0, 0, 0, 0, 43] and co.stats_row(st) == [3, 0, 0, 43, 36, 3]
    out, g, st, lab, keep = co.build(np.full((5, 5), 9, np.uint8), 16, 1, 0, so.DARK, 8, 0, 0, cap)
    assert g["status"] == so.CONSTANT and co.stats_row(st) == [0] * 6 and (lab == -1).all() and not keep.any()


def test_binding_covers_the_clean_entry():
    lib = L.load()
    for name in ("abc_build_scan_images_clean", "abc_scan_clean_desc_size", "abc_scan_clean_scratch_bytes"):
        assert name in L.SYMBOLS
    assert lib.abc_scan_clean_desc_size() == C.sizeof(L.ScanCleanDesc)
    assert (L.ScanCleanDesc, "abc_scan_clean_desc_size") in L.SELF_SIZED_SINCE and L.ScanCleanDesc not in L._STRUCTS
    assert L.SCAN_CLEAN_COLUMNS == co.STATS and len(co.STATS) == 6
    assert (L.SCAN_NO_COMPONENT, L.SCAN_CLEAN_FAILED) == (co.NO_COMPONENT, co.CLEAN_FAILED) == (4, 8)
    assert L.SCAN_CLEAN_CELLS == co.CELLS


def test_scratch_bytes():
    lib = L.load()
    for B, mh, pitch, cell in ((1, 1, 16, 8), (3, 200, 272, 8), (2, 4096, 4096, 8), (5, 300, 400, 64), (7, 1024, 1024, 16)):
        ncap = co.cdiv(mh, cell) * co.cdiv(pitch, cell)
        # ink, parent and weight words per cell, a keep byte per cell, four meta words, rounded up to 16 bytes per image
        words = (3 * ncap + (ncap + 3) // 4 + 4 + 3) // 4 * 4
        assert lib.abc_scan_clean_scratch_bytes(B, mh, pitch, cell) == B * words * 4
    for bad in ((0, 10, 16, 8), (1, 0, 16, 8), (1, 4097, 16, 8), (1, 10, 24, 8), (1, 10, 4112, 8), (1, 10, 16, 12), (1, 10, 16, 0),
                (65536, 10, 16, 8)):
        assert lib.abc_scan_clean_scratch_bytes(*bad) == -1 and b"scan_clean_scratch_bytes" in lib.abc_last_error()


def _descs():
    """a pair of descriptors that passes every guard: host memory stands in for the device's, nothing is launched by a refusal"""
    B, S, mh, pitch = 2, 32, 40, 48
    keepalive = {
        "out": (C.c_float * (B * S * S + 4))(), "src": (C.c_uint8 * (B * mh * pitch + 16))(), "par": (C.c_int32 * (2 * B))(),
        "hist": (C.c_uint32 * (256 * B))(), "box": (C.c_int32 * (8 * B))(), "geom": (C.c_int32 * (12 * B))(),
        "scratch": (C.c_int32 * 4096)(), "stats": (C.c_int32 * (6 * B))(), "labels": (C.c_int32 * 64)(), "keep": (C.c_uint8 * 64)()}
    al16 = lambda a: (C.addressof(a) + 15) // 16 * 16      # noqa: E731
    d = L.ScanDesc()
    d.out, d.src, d.params = al16(keepalive["out"]), al16(keepalive["src"]), C.addressof(keepalive["par"])
    d.src_stride, d.src_pitch, d.src_max_h = mh * pitch, pitch, mh
    d.B, d.S, d.margin, d.cover_q8, d.polarity = B, S, 2, 0, L.SCAN_DARK
    d.hist, d.box, d.geom = (C.addressof(keepalive[k]) for k in ("hist", "box", "geom"))
    q = L.ScanCleanDesc()
    q.scratch, q.stats = al16(keepalive["scratch"]), C.addressof(keepalive["stats"])
    q.labels_out, q.keep_out = C.addressof(keepalive["labels"]), C.addressof(keepalive["keep"])
    q.cell, q.min_ink, q.keep_q8 = 8, 0, 0
    return d, q, keepalive


def _refused(lib, d, q, code, text):
    rc = lib.abc_build_scan_images_clean(C.byref(d) if d is not None else None, C.byref(q) if q is not None else None, None)
    assert rc == code, (rc, code, text, lib.abc_last_error())
    assert text in lib.abc_last_error(), (text, lib.abc_last_error())


EINVAL, EUNSUPPORTED = -1, -2


def test_every_guard_of_the_clean_entry():
    lib = L.load()
    d, q, _k = _descs()
    _refused(lib, None, q, EINVAL, b"null descriptor")
    _refused(lib, d, None, EINVAL, b"null cleaning descriptor")
    for cell in (0, 4, 7, 12, 24, 128, -8):
        d, q, _k = _descs()
        q.cell = cell
        _refused(lib, d, q, EUNSUPPORTED, b"cell must be 8, 16, 32 or 64")
    for field, bad, text in (("min_ink", -1, b"min_ink"), ("keep_q8", -1, b"keep_q8"), ("keep_q8", 257, b"keep_q8"),
                             ("scratch", None, b"null pointer"), ("stats", None, b"null pointer")):
        d, q, _k = _descs()
        setattr(q, field, bad)
        _refused(lib, d, q, EINVAL, text)
    d, q, _k = _descs()
    q.scratch += 4
    _refused(lib, d, q, EINVAL, b"scratch must be 16-byte aligned")
    for field in ("stats", "labels_out"):
        d, q, _k = _descs()
        setattr(q, field, getattr(q, field) + 2)
        _refused(lib, d, q, EINVAL, b"4-byte aligned")


def test_every_guard_of_the_plain_entry_applies():
    """the guards of abc_build_scan_images, one by one, through both entries: the same code and the same text"""
    lib = L.load()
    cases = [("out", None, EINVAL, b"null pointer"), ("src", None, EINVAL, b"null pointer"), ("params", None, EINVAL, b"null pointer"),
             ("hist", None, EINVAL, b"null pointer"), ("box", None, EINVAL, b"null pointer"), ("geom", None, EINVAL, b"null pointer"),
             ("B", 0, EINVAL, b"B must be"), ("B", 65536, EINVAL, b"B must be"),
             ("S", 0, EUNSUPPORTED, b"S must be"), ("S", 36, EUNSUPPORTED, b"S must be"), ("S", 8200, EUNSUPPORTED, b"S must be"),
             ("src_pitch", 40, EUNSUPPORTED, b"src_pitch"), ("src_pitch", 4112, EUNSUPPORTED, b"src_pitch"),
             ("src_max_h", 0, EUNSUPPORTED, b"src_max_h"), ("src_max_h", 4097, EUNSUPPORTED, b"src_max_h"),
             ("src_stride", 40 * 48 - 16, EINVAL, b"src_stride"), ("src_stride", 40 * 48 + 8, EINVAL, b"src_stride"),
             ("margin", -1, EINVAL, b"margin"), ("margin", 16, EINVAL, b"margin"),
             ("cover_q8", -1, EINVAL, b"cover_q8"), ("cover_q8", 257, EINVAL, b"cover_q8"), ("polarity", 3, EINVAL, b"polarity")]
    for field, bad, code, text in cases:
        d, q, _k = _descs()
        setattr(d, field, bad)
        _refused(lib, d, q, code, text)
        rc = lib.abc_build_scan_images(C.byref(d), None)
        assert rc == code and text in lib.abc_last_error(), (field, bad)
    for field, text in (("src", b"16-byte aligned"), ("out", b"16-byte aligned"), ("hist", b"4-byte aligned"), ("params", b"4-byte aligned")):
        d, q, _k = _descs()
        setattr(d, field, getattr(d, field) + 2)
        _refused(lib, d, q, EINVAL, text)
    # the host copy of the parameter table is checked at call time
    d, q, k = _descs()
    host = (C.c_int32 * 4)(10, 10, 41, 10)
    d.params_host = C.addressof(host)
    _refused(lib, d, q, EINVAL, b"src_h / src_w")


def test_scan_builder_argument_errors_come_before_the_device():
    """ValueError for every bad cleaning argument, with or without a GPU (a machine without one would raise AbcNetHipError next)"""
    for kw in (dict(clean_cell=12), dict(clean_cell=0), dict(clean_cell=128), dict(clean_cell="8"), dict(clean_cell=True),
               dict(clean_cell=8.5), dict(clean_cell=8, clean_min_ink=-1), dict(clean_cell=8, clean_min_ink=1.5),
               dict(clean_cell=8, clean_min_ink=2 ** 31), dict(clean_cell=16, clean_keep=-1), dict(clean_cell=16, clean_keep=257),
               dict(clean_cell=16, clean_keep=0.5), dict(clean_min_ink=3), dict(clean_keep=256), dict(debug_cells=True)):
        with pytest.raises(ValueError, match="clean_"):
            ScanBuilder(1, 32, **kw)
