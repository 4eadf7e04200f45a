"""The stroke normaliser on the device (csrc/stroke.hip through abcnet_amd.ops.StrokeNormalizer and augment.ScanBuilder) against
the numpy transcription of its contract (tests/stroke_oracle.py), bit for bit: the f32 batch with assert_array_equal, the stats
rows as integers.  Then the bound, the independence of the images of a batch, three identities that need no oracle at the real
size, the skip words, the guards, the sixth launch of ScanBuilder, graph capture, and an InferenceRunner fed in place."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import ScanBuilder  # noqa: E402
from abcnet_amd.ops import StrokeNormalizer  # noqa: E402
import scan_oracle as sco  # noqa: E402
import stroke_oracle as so  # noqa: E402

DEV = "cuda"
EIGHT = np.ones((3, 3), dtype=int)
THINS = (None, 1, 2, "stable")


def _rows(sn):
    return [[int(r[c]) for c in L.STROKE_STAT_COLUMNS] for r in sn.stats()]


def _batch(S):
    """three seeded drawings (strokes forced over the word seams and along the four borders; at S = 8, where that fills the canvas,
    two free strokes at most 2 wide), an empty image, a full one, a lone pixel in the last column"""
    imgs = [so.drawing(100 * S + b, S, strokes=4) if S > 8 else so.drawing(100 * S + b, S, strokes=2, forced=False, widest=2) for b in range(3)]
    lone = np.zeros((S, S), dtype=bool)
    lone[S // 2, S - 1] = True
    imgs += [np.zeros((S, S), dtype=bool), np.ones((S, S), dtype=bool), lone]
    return np.stack(imgs).astype(np.float32)[:, None]


@pytest.mark.parametrize("S", [8, 72, 136])
def test_matches_the_oracle(S):
    """S = 8: a fraction of one word; 72: two words and a ragged one; 136: four words and a ragged one"""
    x = _batch(S)
    B = x.shape[0]
    if S > 64:
        assert x[:3, 0, :, 31:33].all(axis=2).any() and x[:3, 0, :, 63:65].all(axis=2).any()      # ink on both sides of a seam
        assert x[:3, 0, 0].any() and x[:3, 0, -1].any() and x[:3, 0, :, 0].any() and x[:3, 0, :, -1].any()
    assert 0 < x[:3].sum() < 3 * S * S * 0.6
    src = torch.from_numpy(x).to(DEV)
    for thin, radius, drop in itertools.product(THINS, (0, 1, 3), (False, True)):
        want = [so.normalize(x[b, 0], thin, radius, drop) for b in range(B)]
        what = "S %d thin %r radius %d drop %d" % (S, thin, radius, drop)
        # out of place: the source is not touched
        dst = torch.full_like(src, -1.0)
        sn = StrokeNormalizer(src, out=dst, thin=thin, radius=radius, drop_isolated=drop)
        assert sn.run() is dst
        got = dst.cpu().numpy()
        for b in range(B):
            np.testing.assert_array_equal(got[b, 0], want[b][0], err_msg="%s image %d" % (what, b))
        assert _rows(sn) == [so.stats_row(w[1]) for w in want], what
        assert torch.equal(src.cpu(), torch.from_numpy(x)), what
        # in place
        buf = src.clone()
        sn = StrokeNormalizer(buf, thin=thin, radius=radius, drop_isolated=drop)
        assert sn.run() is buf
        np.testing.assert_array_equal(buf.cpu().numpy(), got, err_msg=what + " in place")
        assert _rows(sn) == [so.stats_row(w[1]) for w in want], what


def test_values_are_cut_at_one_half():
    """ink iff > 0.5: 0.5 itself, negatives, NaN and -inf are paper; 0.500001, 7 and +inf are ink; the output is 0.0 / 1.0"""
    x = np.zeros((1, 1, 8, 8), dtype=np.float32)
    x[0, 0, 1, :7] = [0.5, np.nextafter(np.float32(0.5), np.float32(1)), 7.0, np.inf, -3.0, np.nan, -np.inf]
    buf = torch.from_numpy(x).to(DEV)
    sn = StrokeNormalizer(buf)
    sn.run()
    want, s = so.normalize(x[0, 0])
    assert want[1, :7].tolist() == [0, 1, 1, 1, 0, 0, 0]
    np.testing.assert_array_equal(buf.cpu().numpy()[0, 0], want)
    assert _rows(sn) == [[0, 0, 3, 3, 0]]


def _bar(S, width):
    a = np.zeros((S, S), dtype=np.float32)
    a[6:S - 6, 10:10 + width] = 1.0
    return a


def test_the_bound_is_kept_and_reported():
    S = 40
    a = _bar(S, 9)
    x = torch.from_numpy(a[None, None]).to(DEV)
    out = torch.zeros_like(x)
    sn = StrokeNormalizer(x, out=out, thin=2)
    sn.run()
    want, s = so.normalize(a, 2)
    assert (s["iterations"], s["converged"]) == (2, 0)
    assert _rows(sn) == [so.stats_row(s)]
    np.testing.assert_array_equal(out.cpu().numpy()[0, 0], want)
    sn = StrokeNormalizer(x, out=out, thin="stable")
    sn.run()
    want, s = so.normalize(a, "stable")
    assert s["converged"] == 1 and s["iterations"] > 3
    assert _rows(sn) == [so.stats_row(s)]
    np.testing.assert_array_equal(out.cpu().numpy()[0, 0], want)
    # a bound past the stable count is not reached
    sn = StrokeNormalizer(x, out=out, thin=s["iterations"] + 4)
    sn.run()
    assert _rows(sn) == [so.stats_row(s)]


def test_images_of_a_batch_do_not_see_each_other():
    """a block that needs more than 10 iterations beside an empty image, a drawing and a full image: every image equals the same
    image run alone, twice over a dst filled with -1 (nothing is left of an earlier image or launch)"""
    S = 72
    imgs = [_bar(S, 25), np.zeros((S, S), np.float32), so.drawing(5, S).astype(np.float32), np.ones((S, S), np.float32),
            np.zeros((S, S), np.float32), _bar(S, 25).T.copy()]
    x = torch.from_numpy(np.stack(imgs)[:, None]).to(DEV)
    alone, alone_rows = [], []
    for b in range(len(imgs)):
        one = x[b:b + 1].clone()
        sn = StrokeNormalizer(one, thin="stable", radius=1, drop_isolated=True)
        sn.run()
        alone.append(one.cpu().numpy()[0])
        alone_rows += _rows(sn)
    assert alone_rows[0][0] > 10 and alone_rows[1][:2] == [1, 1] and alone_rows[1][3] == 0
    dst = torch.empty_like(x)
    sn = StrokeNormalizer(x, out=dst, thin="stable", radius=1, drop_isolated=True)
    for _ in range(2):
        dst.fill_(-1.0)
        sn.stat.fill_(-7)
        sn.run()
        np.testing.assert_array_equal(dst.cpu().numpy(), np.stack(alone))
        assert _rows(sn) == alone_rows


def test_identities_at_the_real_size():
    """S = 512, B = 8, no oracle: the skeleton is a subset of its drawing with the same 8-connected components, and thinning it
    again changes nothing and takes one iteration"""
    S, B = 512, 8
    a = np.stack([so.drawing(900 + b, S, strokes=14) for b in range(B)])
    x = torch.from_numpy(a.astype(np.float32)[:, None]).to(DEV)
    out = torch.full_like(x, -1.0)
    sn = StrokeNormalizer(x, out=out, thin="stable")
    sn.run()
    t = out.cpu().numpy()[:, 0]
    st = sn.stats()
    assert set(np.unique(t)) <= {0.0, 1.0}
    t = t > 0.5
    assert not (t & ~a).any()
    for b in range(B):
        assert ndimage.label(t[b], structure=EIGHT)[1] == ndimage.label(a[b], structure=EIGHT)[1], b
    assert (st["converged"] == 1).all() and (st["iterations"] >= 3).all() and (st["skipped"] == 0).all()
    assert st["ink_in"].tolist() == a.sum(axis=(1, 2)).tolist() and st["ink_out"].tolist() == t.sum(axis=(1, 2)).tolist()
    assert (st["ink_out"] < st["ink_in"]).all()
    again = StrokeNormalizer(out, thin="stable")
    again.run()
    np.testing.assert_array_equal(out.cpu().numpy()[:, 0] > 0.5, t)
    st2 = again.stats()
    assert (st2["iterations"] == 1).all() and (st2["converged"] == 1).all() and st2["ink_out"].tolist() == st["ink_out"].tolist()
    # grown back by disk(1): every pixel of the result lies within one step of the skeleton, and the skeleton is inside it
    wide = torch.empty_like(x)
    StrokeNormalizer(out, out=wide, radius=1).run()
    w = wide.cpu().numpy()[:, 0] > 0.5
    assert (w >= t).all() and (w == np.stack([so.dilate(t[b], 1) for b in range(B)])).all()


def test_the_largest_size_runs():
    """S = ABC_STROKE_MAX_SIZE: the third LDS size; a drawing against the oracle, one launch"""
    S = L.STROKE_MAX_SIZE
    a = so.drawing(4, S, strokes=10).astype(np.float32)
    x = torch.from_numpy(a[None, None]).to(DEV)
    sn = StrokeNormalizer(x, thin="stable", radius=3, drop_isolated=True)
    sn.run()
    want, s = so.normalize(a, "stable", 3, True)
    np.testing.assert_array_equal(x.cpu().numpy()[0, 0], want)
    assert _rows(sn) == [so.stats_row(s)]


def test_skip_words_leave_an_image_alone():
    S, B = 40, 4
    a = np.stack([so.drawing(60 + b, S).astype(np.float32) for b in range(B)])[:, None]
    a[1] = np.nan
    a[1, 0, 3, 4] = np.float32(np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0])      # a NaN with a payload
    a[3, 0, 2, 2] = 0.75                                                  # a skipped image need not be {0, 1}
    table = torch.zeros((B, 5), dtype=torch.int32, device=DEV)           # the skip words are a column of a table
    table[1, 2] = 2
    table[3, 2] = -1
    x = torch.from_numpy(a).to(DEV)
    want = [so.normalize(a[b, 0], "stable", 1, True) for b in range(B)]
    for out in (None, torch.full_like(x, -1.0)):
        buf = x.clone()
        sn = StrokeNormalizer(buf, out=out, thin="stable", radius=1, drop_isolated=True, skip=table[:, 2])
        got = sn.run().cpu().numpy()
        rows = _rows(sn)
        for b in (1, 3):
            assert got[b].view(np.int32).tolist() == a[b].view(np.int32).tolist()      # bit for bit, NaN payload included
            assert rows[b] == [0, 0, 0, 0, 1]
        for b in (0, 2):
            np.testing.assert_array_equal(got[b, 0], want[b][0])
            assert rows[b] == so.stats_row(want[b][1])
    with pytest.raises(L.AbcNetHipError):
        StrokeNormalizer(x, skip=table[:3, 2])
    with pytest.raises(L.AbcNetHipError):
        StrokeNormalizer(x, skip=table[:, 2].long())
    with pytest.raises(L.AbcNetHipError):
        StrokeNormalizer(x, skip=table[:, 2].cpu())


def test_guards_refuse_and_launch_nothing():
    x = torch.full((2, 1, 16, 16), 0.25, dtype=torch.float32, device=DEV)
    for kw in (dict(radius=4), dict(radius=-1), dict(radius=1.0), dict(thin=-2), dict(thin="twice"), dict(thin=1.5)):
        with pytest.raises(ValueError):
            StrokeNormalizer(x, **kw)
    for shape in ((1, 1, 12, 12), (1, 1, L.STROKE_MAX_SIZE + 8, L.STROKE_MAX_SIZE + 8)):
        with pytest.raises(ValueError, match="multiple of 8"):
            StrokeNormalizer(torch.zeros(shape, dtype=torch.float32, device=DEV))
    for bad in (x.half(), x.double(), x.cpu(), x[:, :, :, ::2], torch.zeros((2, 3, 16, 16), device=DEV), torch.zeros((2, 1, 16, 8), device=DEV)):
        with pytest.raises(L.AbcNetHipError):
            StrokeNormalizer(bad)
    for bad in (x.cpu(), x.half(), torch.zeros((1, 1, 16, 16), device=DEV)):
        with pytest.raises(L.AbcNetHipError):
            StrokeNormalizer(x, out=bad)
    # the descriptor-level call: ABC_EINVAL (-1), nothing written
    sn = StrokeNormalizer(x, out=torch.full_like(x, -1.0), thin=1, radius=1)
    for field, value, word in (("radius", 4, b"radius"), ("max_iter", -2, b"max_iter"), ("S", 12, b"S must"),
                               ("S", L.STROKE_MAX_SIZE + 8, b"S must"), ("B", 0, b"B must"), ("drop_isolated", 3, b"drop_isolated"),
                               ("dst", x.data_ptr() + 16, b"overlap"), ("src", x.data_ptr() + 4, b"aligned")):
        keep = getattr(sn.d, field)
        setattr(sn.d, field, value)
        assert sn.lib.abc_normalize_strokes(C.byref(sn.d), None) == -1 and word in sn.lib.abc_last_error(), field
        with pytest.raises(L.AbcNetHipError, match=r"\(-1\)"):
            sn.run()
        setattr(sn.d, field, keep)
    torch.cuda.synchronize()
    assert bool((sn.out == -1.0).all()) and bool((x == 0.25).all()) and not sn.stat.any()
    sn.run()                                                  # (the descriptor is whole again)
    assert not sn.out.any() and _rows(sn) == [[1, 1, 0, 0, 0]] * 2
    with pytest.raises(ValueError, match="STROKE|size <="):
        ScanBuilder(1, L.STROKE_MAX_SIZE + 8, stroke_radius=1)
    with pytest.raises(ValueError):
        ScanBuilder(1, 32, stroke_radius=4)
    with pytest.raises(ValueError):
        ScanBuilder(1, 32, thin=-1)
    with pytest.raises(ValueError):
        ScanBuilder(1, 32).stroke_stats()


# ------------------------------------------------------------------------------------------------------------------ ScanBuilder
def _grey(seed, h, w, paper=200, ink=50, strokes=4, light=False):
    """a grey scan: noisy paper, a few noisy strokes (straight runs of ink pixels, 1 to 3 wide)"""
    rs = np.random.RandomState(seed)
    mask = np.zeros((h, w), dtype=bool)
    for _ in range(strokes):
        y0, x0, y1, x1 = int(rs.randint(0, h)), int(rs.randint(0, w)), int(rs.randint(0, h)), int(rs.randint(0, w))
        so.stroke(mask, y0, x0, y1, x1, int(rs.randint(1, 4)))
    img = np.where(mask, rs.normal(ink, 8, (h, w)), rs.normal(paper, 6, (h, w)))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return (255 - img) if light else img


def _mixed_sources():
    """a batch of the kinds test_gpu_scan.py's parity test mixes; max_src = (320, 112)"""
    one = np.array([[77]], dtype=np.uint8)                                   # 1 x 1 (a single value: CONSTANT)
    odd = _grey(1, 17, 23)                                                   # width no multiple of 16
    down = _grey(2, 100, 37, strokes=6)                                      # downscales at a non-integer ratio
    tall = _grey(3, 300, 100, strokes=5)                                     # five workgroups per image in the scan's row passes
    single = np.full((40, 50), 220, dtype=np.uint8)                          # a single ink pixel: isolated
    single[13, 31] = 30
    blob = np.full((90, 90), 210, dtype=np.uint8)                            # a thick blob: many iterations
    blob[20:70, 25:60] = 40
    const = np.full((20, 20), 128, dtype=np.uint8)                           # a constant image
    light = _grey(5, 60, 90, strokes=6, light=True)                          # light ink on a dark ground
    return [one, odd, down, tall, single, blob, const, light]


def _geom_rows(sb):
    g = sb.geometry()
    return [[int(g[b][c]) for c in L.SCAN_GEOM_COLUMNS] for b in range(sb.B)]


def test_scan_builder_defaults_are_what_they_were():
    srcs = _mixed_sources()
    kw = dict(max_src=(320, 112), margin=2, cover=64, polarity="auto")
    plain = ScanBuilder(len(srcs), 32, **kw)
    same = ScanBuilder(len(srcs), 32, thin=None, stroke_radius=None, drop_isolated=False, **kw)
    also = ScanBuilder(len(srcs), 32, thin=0, **kw)
    assert same.strokes is None and also.strokes is None and plain.strokes is None
    for f, _ in L.ScanDesc._fields_:      # (the pointers differ; the scalar fields do not)
        if f in ("src_stride", "src_pitch", "src_max_h", "B", "S", "margin", "cover_q8", "polarity"):
            assert getattr(plain.d, f) == getattr(same.d, f), f
    for sb in (plain, same):
        sb.load(srcs)
        sb.out.fill_(-1.0)
        sb.run()
    assert torch.equal(plain.out, same.out) and _geom_rows(plain) == _geom_rows(same)
    for b, src in enumerate(srcs):
        want, g = sco.build(src, 32, 2, 64, sco.AUTO)
        np.testing.assert_array_equal(same.out.cpu().numpy()[b, 0], want)


def test_scan_builder_appends_the_normaliser():
    srcs = _mixed_sources()
    S, kw = 32, dict(max_src=(320, 112), margin=2, cover=64, polarity="auto")
    plain = ScanBuilder(len(srcs), S, **kw)
    sb = ScanBuilder(len(srcs), S, thin="stable", stroke_radius=1, drop_isolated=True, **kw)
    for b_ in (plain, sb):
        b_.load(srcs)
        b_.out.fill_(-1.0)
        b_.run()
    got, rows, geom = sb.out.cpu().numpy(), sb.stroke_stats(), sb.geometry()
    assert _geom_rows(sb) == _geom_rows(plain)                                   # `ink` stays the source's count
    assert geom["status"].tolist() == [sco.CONSTANT, 0, 0, 0, 0, 0, sco.CONSTANT, 0]
    for b, src in enumerate(srcs):
        scan, g = sco.build(src, S, 2, 64, sco.AUTO)
        assert [int(geom[b][c]) for c in L.SCAN_GEOM_COLUMNS] == sco.geom_row(g)
        if g["status"]:
            assert not got[b].any() and [int(rows[b][c]) for c in L.STROKE_STAT_COLUMNS] == [0, 0, 0, 0, 1]      # stays blank
            continue
        want, s = so.normalize(scan, "stable", 1, True)
        np.testing.assert_array_equal(got[b, 0], want, err_msg="image %d" % b)
        assert [int(rows[b][c]) for c in L.STROKE_STAT_COLUMNS] == so.stats_row(s), b
    assert not got[4].any() and rows[4]["ink_in"] == 1                            # the single pixel was a speckle
    assert rows[5]["iterations"] > 3
    assert sb.record_offsets(2) == plain.record_offsets(2)
    # a BAD_PARAMS image keeps its NaN, its neighbours their drawings (the device table alone: the host copy would refuse the call)
    for b_ in (plain, sb):
        b_.d.params_host = None
        torch.cuda.synchronize()
        b_.d_par[3, 0] = 321
        b_.run()
    got2, rows2 = sb.out.cpu().numpy(), sb.stroke_stats()
    assert np.isnan(got2[3]).all() and sb.geometry()[3]["status"] == sco.BAD_PARAMS
    assert [int(rows2[3][c]) for c in L.STROKE_STAT_COLUMNS] == [0, 0, 0, 0, 1]
    assert _geom_rows(sb) == _geom_rows(plain)
    keep = [b for b in range(len(srcs)) if b != 3]
    np.testing.assert_array_equal(got2[keep], got[keep])


def test_sixth_launch_replays_from_a_captured_graph():
    S, B = 32, 3
    sb = ScanBuilder(B, S, max_src=(150, 96), margin=2, cover=64, polarity="auto", thin="stable", stroke_radius=1, drop_isolated=True)

    def batch(seed):
        rs = np.random.RandomState(seed)
        return [_grey(seed + b, int(rs.randint(20, 151)), int(rs.randint(20, 97)), light=(b == 1)) for b in range(B)]
    sb.load(batch(100))
    sb.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sb.run()
    for seed in (200, 300):
        srcs = batch(seed)
        sb.load(srcs)
        sb.run()
        eager, eager_rows = sb.out.clone(), sb.stroke_stats().copy()
        sb.out.fill_(-1.0)
        sb.geom.fill_(-7)
        sb.strokes.stat.fill_(-7)
        g.replay()
        assert torch.equal(sb.out, eager) and (sb.stroke_stats() == eager_rows).all()
        for b, src in enumerate(srcs):
            want, s = so.normalize(sco.build(src, S, 2, 64, sco.AUTO)[0], "stable", 1, True)
            np.testing.assert_array_equal(eager.cpu().numpy()[b, 0], want, err_msg="seed %d image %d" % (seed, b))
            assert [int(eager_rows[b][c]) for c in L.STROKE_STAT_COLUMNS] == so.stats_row(s)


def test_inference_runner_fed_in_place():
    """a normalising ScanBuilder over InferenceRunner(assemble=True).input_images: the buffer equals the oracles composed, step()
    runs, and the molecule rows pass the contract's checker"""
    from abcnet_amd.contract import MoleculeRows
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.unet import UNet
    from oracle import unet_oracle as uo
    B, S = 2, 64
    m = UNet(1, uo.HEADS, dtype="bf16")
    m.load_state_dict(uo.filled_state("unet", 1, uo.HEADS, seed=0))
    m = m.to(DEV)
    ir = InferenceRunner(m, B, S, S, use_graph=False, assemble=True)
    sb = ScanBuilder(B, S, out=ir.input_images, max_src=(200, 180), cover=64, polarity="auto", thin="stable", stroke_radius=1)
    srcs = [_grey(900, 200, 150, strokes=9), _grey(901, 90, 180, strokes=7, light=True)]
    sb.load(srcs)
    sb.run()
    ir.step()
    torch.cuda.synchronize()
    want = np.stack([so.normalize(sco.build(s, S, sb.margin, 64, sco.AUTO)[0], "stable", 1)[0] for s in srcs])[:, None]
    np.testing.assert_array_equal(ir.input_images.cpu().numpy(), want)
    assert 0 < want.sum()
    rows = MoleculeRows.checked("test", ir.assembler.rows, need_implh=True)
    counts = rows.tensors[0].cpu().numpy()
    assert rows.B == B and (counts[:, 0] >= 0).all() and (counts[:, 0] <= rows.cap_atoms).all()
    assert (counts[:, 1] >= 0).all() and (counts[:, 1] <= rows.cap_mol_bonds).all()
    assert len(ir.molecules()) == B
