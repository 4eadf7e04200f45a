"""CPU side of the device input-image builder (abcnet_amd.augment, csrc/augment.hip): the oracle against the reference's
goldens, the host draws, the hash mirror, the threshold arithmetic and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import augment as A  # noqa: E402
import augment_oracle as ao  # noqa: E402


def _train(golden_dir):
    return np.load(os.path.join(golden_dir, "augment_512.npz"))


def _bits(a, S=512):
    return np.unpackbits(a)[:S * S].reshape(S, S).astype(bool)


def test_oracle_reproduces_train_golden_with_recorded_fields(golden_dir):
    g = _train(golden_dir)
    tags = set()
    for ci in range(int(g["n"])):
        p = "c%d_" % ci
        rows, cols, ddx, ddy = (int(v) for v in g[p + "geom"])
        ink = ao.ink_train(g[p + "src"], 512, rows, cols, ddx, ddy)
        got = ao.compose(ink, _bits(g[p + "salt"]), _bits(g[p + "pepper"]))
        np.testing.assert_array_equal(got.astype(bool), _bits(g[p + "out"]), err_msg="case %d (%s)" % (ci, g[p + "tag"]))
        tags.add(str(g[p + "tag"]))
        if float(g[p + "amount"]) == 0:
            assert not _bits(g[p + "salt"]).any() and not _bits(g[p + "pepper"]).any()
    assert tags == {"row", "col", "none", "small", "small_row"}


def test_oracle_reproduces_test_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "augment_test_512.npz"))
    c = A.test_ink_max()
    for ci in range(int(g["n"])):
        src = g["c%d_src" % ci]
        want = _bits(g["c%d_out" % ci])
        np.testing.assert_array_equal(ao.build_test(src).astype(bool), want)
        np.testing.assert_array_equal(src <= c, want)        # the kernel's byte compare


def test_byte_cuts():
    """test mode: u8 <= 51 (test_ink_max, passed in the descriptor); train mode where neither axis is resized: u8 <= 152, the cut
    abc_build_images derives from the same float32 division -- the reference's verdicts on every byte"""
    assert A.test_ink_max() == 51
    u8 = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(u8 <= 152, ao.threshold(u8.astype(np.float32)))


class _Replay:
    """an rng that hands out recorded scalar draws in order (the fields are not drawn by draw_augment)"""

    def __init__(self, scalars):
        self.v = list(scalars)

    def rand(self):
        return self.v.pop(0)

    def uniform(self, lo, hi):
        return self.v.pop(0)

    def randint(self, lo, hi):
        return 12345


def test_draw_augment_maps_recorded_draws(golden_dir):
    g = _train(golden_dir)
    for ci in range(int(g["n"])):
        p = "c%d_" % ci
        sc = g[p + "scalars"]
        dr, offs = A.draw_augment(_Replay(sc), float(g[p + "amount"]), g[p + "src"].shape, 512)
        rows, cols, ddx, ddy = (int(v) for v in g[p + "geom"])
        assert (dr.rows, dr.cols, dr.ddx, dr.ddy) == (rows, cols, ddx, ddy), ci
        assert offs == (dr.scale_x, dr.scale_y, ddx, ddy)
        assert (dr.scale_x, dr.scale_y) == tuple(g[p + "scale"])
        assert dr.salt == sc[-2] and dr.pepper == sc[-1]
        assert dr.key == 12345 | (12345 << 32)
        if sc[0] >= 0.2:
            assert type(dr.scale_x) is int and type(dr.scale_y) is int and dr.scale_x == 1   # parse_record's un-augmented scale


def test_draw_augment_follows_the_reference_stream():
    """the same RandomState gives the reference's scalars in the reference's order (first draws identical)"""
    rs, ref = np.random.RandomState(7), np.random.RandomState(7)
    for _ in range(50):
        dr, _ = A.draw_augment(rs, 0.1, (512, 512))
        r1 = ref.rand()
        if r1 < 0.2:
            r2, s = ref.rand(), ref.uniform(0.8, 1)
            assert (dr.rows, dr.cols) == ((int(s * 512), 512) if r2 < 0.5 else (512, int(s * 512)))
        else:
            assert (dr.rows, dr.cols, dr.scale_x, dr.scale_y) == (512, 512, 1, 1)
        assert dr.salt == ref.uniform(0, 0.1 / 100) and dr.pepper == ref.uniform(0, 0.1)
        ref.randint(0, 1 << 32), ref.randint(0, 1 << 32)


def test_noise_hash_known_answers():
    idx = np.array([0, 1, 2, 3, 1000, 524287, 524288, 0xFFFFFFFF], dtype=np.uint64)
    got = A.noise_hash(idx, 0x0123456789ABCDEF)
    want = np.array(KNOWN_HASH, dtype=np.uint32)
    np.testing.assert_array_equal(got, want)
    # the key's both halves matter
    assert (A.noise_hash(idx, 1) != A.noise_hash(idx, 1 << 32)).all()


# abc_noise_hash(idx, abc_noise_seed(key_lo = 0x89ABCDEF, key_hi = 0x01234567)) for the indices above, evaluated by the C function (common.hpp) on the host
KNOWN_HASH = [0xE0CACB04, 0xA22085C3, 0x47D8DD19, 0x1C738A9A, 0x395F469C, 0x7F847063, 0x760DD2EA, 0xB7EF9D96]


def test_noise_threshold_is_the_uniform_compare():
    assert A.noise_threshold(0.0) == 0
    assert A.noise_threshold(1.0) == 0xFFFFFFFF
    for r in (1e-9, 0.001, 0.05, 0.1999, 0.5):
        t = A.noise_threshold(r)
        assert (t - 1) / 2.0 ** 32 < r <= t / 2.0 ** 32


def test_threshold_sweep_matches_float32_division():
    """every float32 in [152.99, 153.01]: the oracle's decision (canvas / 255 < 0.6 in float32) equals np.float32(v) / 255 < 0.6
    (the kernel divides with IEEE float32 division and compares against 0.6f the same way)"""
    lo, hi = np.float32(152.99).view(np.uint32), np.float32(153.01).view(np.uint32)
    v = np.arange(lo, hi + 1, dtype=np.uint32).view(np.float32)
    got = ao.threshold(v)
    want = np.array([np.float32(x) / np.float32(255) < np.float32(0.6) for x in v])
    np.testing.assert_array_equal(got, want)
    assert want.any() and not want.all()


def test_resize_identity_axis_copies_and_edges_clamp():
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, size=(37, 53)).astype(np.float32)
    np.testing.assert_array_equal(ao.resize_linear(img, 37, 53), img)
    r = ao.resize_linear(img, 30, 53)
    assert r.shape == (30, 53) and r.dtype == np.float32
    up = ao.resize_linear(img, 37, 80)       # upscale: the first and last columns clamp to weight (1, 0)
    np.testing.assert_array_equal(up[:, 0], img[:, 0])
    np.testing.assert_array_equal(up[:, -1], img[:, -1])


def _fused_resize(img, rows, cols):
    """resize_linear with each pass's second product added by a fused multiply-add (what contraction would compile)"""
    img = np.asarray(img, dtype=np.float32)
    H, W = img.shape
    one = np.float32(1)
    s0, s1, fx = ao._taps(cols, W)
    r = (img[:, s0].astype(np.float64) * (one - fx) + (img[:, s1] * fx).astype(np.float64)).astype(np.float32)
    t0, t1, fy = ao._taps(rows, H)
    fy = fy[:, None]
    return (r[t0].astype(np.float64) * (one - fy) + (r[t1] * fy).astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("rows, cols", [(512, 450), (450, 512)])
def test_uniform_153_resize_separates_rounding_from_fma(rows, cols):
    """the GPU case test_resizes_round_every_multiply_and_add: a uniform 153 source is ink along a whole column / row when every
    multiply and add is rounded on its own (the reference's arithmetic) and nowhere when the multiply-add is fused"""
    src = np.full((512, 512), 153, np.float32)
    sep = ao.threshold(ao.resize_linear(src, rows, cols))
    fused = ao.threshold(_fused_resize(src, rows, cols))
    assert sep.sum() == 512 and fused.sum() == 0


def test_param_row_layout():
    dr = A.AugmentDraw(430, 512, 41, 0, 0.84, 1, 0.0005, 0.05, 0xFEDCBA9876543210)
    row = A.param_row((512, 512), dr, 512).view(np.uint32)
    assert list(row[:6]) == [512, 512, 430, 512, 41, 0]
    assert row[6] == A.noise_threshold(0.0005) and row[7] == A.noise_threshold(0.05)
    assert (row[8], row[9]) == (0x76543210, 0xFEDCBA98)
    assert list(A.param_row((384, 384), None, 384).view(np.uint32)) == [384, 384, 384, 384, 0, 0, 0, 0, 0, 0]


def test_image_desc_declared_in_binding():
    assert "abc_build_images" in L.SYMBOLS
    assert L.ImageDesc in L._STRUCTS and L._STRUCTS.index(L.ImageDesc) == 26
    lib = L.load()
    assert lib.abc_sizeof(26) == C.sizeof(L.ImageDesc)


def test_draw_augment_rejects_what_does_not_fit():
    class NoResize:
        def rand(self):
            return 0.9

        def uniform(self, lo, hi):
            return lo

        def randint(self, lo, hi):
            return 0
    with pytest.raises(ValueError):
        A.draw_augment(NoResize(), 0.1, (600, 500), 512)      # an oversized source without a resize
    with pytest.raises(ValueError):
        A.draw_augment(NoResize(), 0.1, (512, 512), 384)
    dr, _ = A.draw_augment(NoResize(), 0.1, (300, 450), 512)
    assert (dr.rows, dr.cols, dr.ddx, dr.ddy) == (300, 450, 106, 31)


def _desc(S=512, mode=L.IMG_TRAIN, params_host=None, B=1):
    d = L.ImageDesc()
    d.out, d.src, d.params = 256, 512, 768          # never dereferenced: the refusals come first
    d.src_stride, d.src_pitch, d.src_max_h = 512 * 512, 512, 512
    d.B, d.S, d.mode = B, S, mode
    d.params_host = params_host
    d.test_max_ink = 51
    return d


def test_launcher_refuses_bad_descriptors_on_the_host():
    lib = L.load()
    bad = [dict(S=500), dict(S=4)]
    for kw in bad:
        assert lib.abc_build_images(C.byref(_desc(**kw)), None) == L_EUNSUP
    d = _desc()
    d.src_pitch = 520
    assert lib.abc_build_images(C.byref(d), None) < 0
    d = _desc()
    d.out = 260                                         # not 16-byte aligned
    assert lib.abc_build_images(C.byref(d), None) < 0 and b"aligned" in lib.abc_last_error()
    d = _desc(mode=7)
    assert lib.abc_build_images(C.byref(d), None) < 0

    def with_row(vals, mode=L.IMG_TRAIN, S=512):
        row = np.array(vals, dtype=np.int64).astype(np.int32)
        d = _desc(S=S, mode=mode, params_host=row.ctypes.data)
        rc = lib.abc_build_images(C.byref(d), None)
        return rc, lib.abc_last_error()
    assert with_row([512, 512, 513, 512, 0, 0, 0, 0, 0, 0])[0] == -1             # rows > S
    assert with_row([512, 512, 512, 600, 0, 0, 0, 0, 0, 0])[0] == -1             # cols > S
    assert with_row([512, 512, 400, 512, -1, 0, 0, 0, 0, 0])[0] == -1            # negative offset
    assert with_row([512, 512, 400, 512, 200, 0, 0, 0, 0, 0])[0] == -1           # leaves the canvas
    assert with_row([600, 512, 512, 512, 0, 0, 0, 0, 0, 0])[0] == -1             # source taller than its slot
    rc, msg = with_row([384, 384, 512, 512, 0, 0, 0, 0, 0, 0], mode=L.IMG_TEST)
    assert rc == -1 and b"test mode" in msg


L_EUNSUP = -2
