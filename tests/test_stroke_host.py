"""The host side of the stroke normaliser: the numpy oracle of its contract (tests/stroke_oracle.py) holds the invariants a
thinning must hold, and the binding of abc_normalize_strokes matches the header.  No kernel is launched here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
import stroke_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGHT = np.ones((3, 3), dtype=int)


def _components(a):
    return ndimage.label(a, structure=EIGHT)[1]


def _cases():
    """200 stroke drawings of 64 x 64 and 200 noise images of 32 x 32, seeded"""
    for k in range(200):
        yield "drawing %d" % k, so.drawing(1000 + k, 64, strokes=1 + k % 6, forced=(k % 4 == 0))
    rs = np.random.RandomState(5)
    for k in range(200):
        yield "noise %d" % k, rs.rand(32, 32) < (0.1 + 0.8 * k / 200)


def test_thinning_keeps_the_subset_the_components_and_is_idempotent():
    most = 0
    for name, a in _cases():
        t, it, conv = so.thin(a, so.UNTIL_STABLE)
        assert conv == 1 and it >= 1, name
        assert not (t & ~a).any(), name
        assert _components(t) == _components(a), name
        again, it2, conv2 = so.thin(t, so.UNTIL_STABLE)
        assert (again == t).all() and it2 == 1 and conv2 == 1, name
        most = max(most, it)
    assert most >= 4          # (strokes up to 7 wide: several peels are exercised)


def test_bounded_thinning_is_a_prefix_of_the_stable_one():
    a = so.drawing(77, 64, strokes=6)
    full, n, _ = so.thin(a, so.UNTIL_STABLE)
    assert n >= 3
    prev = a
    for k in range(1, n + 1):
        t, it, conv = so.thin(a, k)
        assert it == k and conv == (1 if k == n else 0)
        assert not (t & ~prev).any()
        prev = t
    assert (prev == full).all()
    t, it, conv = so.thin(a, 0)
    assert (t == a).all() and (it, conv) == (0, 0)
    # past the stable count the bound is not reached
    t, it, conv = so.thin(a, n + 5)
    assert (t == full).all() and (it, conv) == (n, 1)


def test_small_shapes_by_hand():
    lone = np.zeros((8, 8), dtype=bool)
    lone[3, 4] = True
    t, it, conv = so.thin(lone, so.UNTIL_STABLE)
    assert (t == lone).all() and (it, conv) == (1, 1)
    sq = np.zeros((8, 8), dtype=bool)
    sq[2:4, 5:7] = True
    t, it, conv = so.thin(sq, so.UNTIL_STABLE)
    assert t.sum() == 1 and not (t & ~sq).any() and conv == 1
    full = np.ones((8, 8), dtype=bool)
    t, it, conv = so.thin(full, so.UNTIL_STABLE)
    assert t.sum() == 1 and (it, conv) == (5, 1)
    empty = np.zeros((8, 8), dtype=bool)
    t, it, conv = so.thin(empty, so.UNTIL_STABLE)
    assert not t.any() and (it, conv) == (1, 1)


def test_dilate_footprints():
    for r, n in ((0, 1), (1, 5), (2, 13), (3, 29)):
        assert len(so.disk(r)) == n
        a = np.zeros((9, 9), dtype=bool)
        a[4, 4] = True
        d = so.dilate(a, r)
        assert d.sum() == n and d[4, 4] and d[4 - r, 4] and d[4, 4 + r] and (d == d.T).all() and (d == d[::-1, ::-1]).all()
        # clipped at the canvas: a corner pixel keeps the quadrant
        c = np.zeros((9, 9), dtype=bool)
        c[0, 8] = True
        assert so.dilate(c, r).sum() == sum(1 for dy, dx in so.disk(r) if dy >= 0 and dx <= 0)
    # a one-pixel line dilated by disk(1) is the 3-pixel line synthetic._line stamps, away from its ends
    line = np.zeros((9, 16), dtype=bool)
    line[4, :] = True
    assert (so.dilate(line, 1)[:, 3:13] == np.repeat(np.array([0, 0, 0, 1, 1, 1, 0, 0, 0], bool)[:, None], 10, 1)).all()


def test_drop_isolated_removes_exactly_the_pixels_without_a_neighbour():
    rs = np.random.RandomState(9)
    for k in range(50):
        a = rs.rand(24, 24) < 0.08 + 0.01 * k
        a[0, 0] = True
        a[0, 1] = a[1, 1] = False
        a[1, 0] = k % 2 == 0                       # a corner pixel, isolated in the odd cases
        want = a.copy()
        for y, x in zip(*np.nonzero(a)):
            if a[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].sum() == 1:
                want[y, x] = False
        assert (so.despeckle(a) == want).all()
        assert want[0, 0] == (k % 2 == 0)


def test_normalize_composes_the_stages_in_order():
    a = so.drawing(3, 40, strokes=4).astype(np.float32)
    a[5, 30] = 1.0                                 # (may or may not be isolated: the stages decide)
    a[7, 7] = np.nan                               # a NaN is paper
    a[8, 8] = 0.5                                  # not above 0.5: paper
    ink = np.nan_to_num(a, nan=0.0) > 0.5
    out, s = so.normalize(a, "stable", 1, True)
    t, it, conv = so.thin(so.despeckle(ink), so.UNTIL_STABLE)
    want = so.dilate(t, 1)
    assert (out == want).all() and out.dtype == np.float32 and set(np.unique(out)) <= {0.0, 1.0}
    assert so.stats_row(s) == [it, conv, int(ink.sum()), int(want.sum()), 0]
    out, s = so.normalize(a)
    assert (out == ink).all() and so.stats_row(s) == [0, 0, int(ink.sum()), int(ink.sum()), 0]


def _header():
    with open(os.path.join(ROOT, "include", "abcnet_hip.h")) as f:
        return f.read()


def test_mirror_matches_the_header_text():
    text = _header()
    body = re.search(r"typedef struct abc_stroke_desc \{(.*?)\} abc_stroke_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        ctype = "ptr" if pointer else re.match(r"(?:const\s+)?(\w+)", decl).group(1)
        names = re.sub(r"^(?:const\s+)?\w+\s*\**", "", decl)
        for name in names.split(","):
            fields.append((name.strip().lstrip("*").strip(), ctype))
    kinds = {"ptr": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, kinds[t]) for n, t in fields] == [(n, t) for n, t in L.StrokeDesc._fields_]
    # natural alignment, no hidden padding but what C adds: two pointers, six int32, two pointers
    assert C.sizeof(L.StrokeDesc) == 56
    stat = re.search(r"enum abc_stroke_stat \{(.*?)\}", text, re.S).group(1)
    names = [s.strip().split("=")[0].strip() for s in stat.split(",") if s.strip()]
    assert names[-1] == "ABC_STROKE_NSTAT"
    assert tuple(n[len("ABC_STROKE_"):].lower() for n in names[:-1]) == L.STROKE_STAT_COLUMNS == so.STATS
    consts = dict(re.findall(r"(ABC_STROKE_UNTIL_STABLE|ABC_STROKE_MAX_SIZE) = (-?\d+)", text))
    assert int(consts["ABC_STROKE_UNTIL_STABLE"]) == L.STROKE_UNTIL_STABLE == so.UNTIL_STABLE == -1
    assert int(consts["ABC_STROKE_MAX_SIZE"]) == L.STROKE_MAX_SIZE and L.STROKE_MAX_SIZE >= 1024


def test_library_exports_the_entry_and_refuses_on_the_host():
    lib = L.load()
    assert "abc_normalize_strokes" in L.SYMBOLS and "abc_stroke_desc_size" in L.SYMBOLS
    assert lib.abc_stroke_desc_size() == C.sizeof(L.StrokeDesc)
    assert (L.StrokeDesc, "abc_stroke_desc_size") in L.SELF_SIZED_SINCE      # (what load() checks beside SELF_SIZED)
    d = L.StrokeDesc()
    assert lib.abc_normalize_strokes(C.byref(d), None) == -1 and b"null" in lib.abc_last_error()
    assert lib.abc_normalize_strokes(None, None) == -1
    # every parameter is refused before anything is launched (the pointers are never followed: no device is needed)
    buf = (C.c_float * 64)()
    base = (C.addressof(buf) + 15) // 16 * 16

    def desc(**kw):
        d = L.StrokeDesc()
        d.src = d.dst = base
        d.stats = base
        d.B, d.S = 1, 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for kw, word in ((dict(radius=4), b"radius"), (dict(radius=-1), b"radius"), (dict(max_iter=-2), b"max_iter"), (dict(S=12), b"S must"),
                     (dict(S=0), b"S must"), (dict(S=L.STROKE_MAX_SIZE + 8), b"S must"), (dict(B=0), b"B must"),
                     (dict(drop_isolated=2), b"drop_isolated"), (dict(src=base + 4), b"aligned"), (dict(dst=base + 16), b"overlap"),
                     (dict(skip=base, skip_stride=0), b"skip_stride")):
        assert lib.abc_normalize_strokes(C.byref(desc(**kw)), None) == -1, kw
        assert word in lib.abc_last_error(), (kw, lib.abc_last_error())


def test_thin_argument_of_the_python_surface():
    from abcnet_amd.ops import stroke_max_iter
    assert [stroke_max_iter(t) for t in (None, 0, 1, 7, "stable")] == [0, 0, 1, 7, L.STROKE_UNTIL_STABLE]
    for bad in (-1, -2, "forever", 1.5, True):
        with pytest.raises(ValueError):
            stroke_max_iter(bad)


def test_stroke_normalizer_has_no_cpu_fallback():
    import torch
    from abcnet_amd.augment import ScanBuilder
    from abcnet_amd.ops import StrokeNormalizer
    with pytest.raises(ValueError):
        StrokeNormalizer(torch.zeros((1, 1, 8, 8)), radius=4)
    with pytest.raises(ValueError):
        ScanBuilder(1, L.STROKE_MAX_SIZE + 8, thin=1)
    if torch.cuda.is_available():
        return
    with pytest.raises(L.AbcNetHipError, match="no CPU fallback"):
        StrokeNormalizer(torch.zeros((1, 1, 8, 8)))
    with pytest.raises(L.AbcNetHipError, match="no CPU fallback"):
        ScanBuilder(1, 32, thin="stable")
