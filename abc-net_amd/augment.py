"""Input images on the device: the image half of the reference's src/utils.py:42-81 (MolecularImageDataset.__getitem__) and
utils_for_test.py:21-27, split into a tiny host half and one kernel.

    host   draw_augment(): the reference's scalar draws (utils.py:44-58, 73, 76) in its order and arithmetic -- resize branch,
           scale, centring offsets, salt and pepper amounts -- plus a 64-bit noise key;
    device ImageBuilder: the raw uint8 renders and ten int32 per image go over PCIe; csrc/augment.hip resizes (OpenCV
           INTER_LINEAR on float32), centres on the white canvas, thresholds and noises them straight into the network's f32 input.

The salt and pepper fields come from a counter hash of (key, pixel) on the device (abc_noise_hash, mirrored by noise_hash
below), not from np.random's per-pixel stream: per pixel they follow the reference's distribution -- Bernoulli with the drawn
amounts -- not its bits.  That is the position the dropout mask takes (dropout.py, K7).  No CPU fallback.

A third way to build the input, "scan": ScanBuilder takes raw grey scans of any size and background level (what binarize.py's
offline Otsu step and utils_for_test.py's loader do between them, plus the crop and the fit a scan needs) and csrc/scan.hip
thresholds, crops, fits and writes them; otsu_threshold and fit_scan below are the pure host mirrors of its rules.  On request it
appends ops.StrokeNormalizer (csrc/stroke.hip) as a sixth launch: speckles dropped, strokes thinned and grown back to one width.
With clean_cell set it drops dirt and text far from the drawing before the crop (abc_build_scan_images_clean: connected components
over a coarse grid of cells, weighed by their ink).
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from .contract import PinnedStaging, require_device_tensor, stream_or_current
from .ops import StrokeNormalizer, stroke_max_iter

MODES = {"train": L.IMG_TRAIN, "test": L.IMG_TEST}

# one image's draws: the resized size (rows x cols) it takes on the S x S canvas at (ddx, ddy), the reference's scale factors
# (int 1 when not resized), its salt / pepper amounts and the 64-bit key of its noise fields
AugmentDraw = namedtuple("AugmentDraw", "rows cols ddx ddy scale_x scale_y salt pepper key")

_M32 = 0xFFFFFFFF


def _fmix32(h):
    m = np.uint64(_M32)
    h = np.asarray(h, dtype=np.uint64) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def noise_seed(key):
    """abc_noise_seed (csrc/common.hpp): the per-image 32-bit premix of a 64-bit key"""
    lo, hi = key & _M32, (key >> 32) & _M32
    return int(_fmix32(np.uint64(lo ^ 0x5A17F00D) ^ _fmix32(np.uint64((hi * 0x9E3779B1 + 0x7F4A7C15) & _M32))))


def noise_hash(idx, key):
    """numpy mirror of abc_noise_hash(idx, abc_noise_seed(key)) (csrc/common.hpp): uint32 per element index for a 64-bit key"""
    m = np.uint64(_M32)
    h = (np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B1)) & m
    return _fmix32(h ^ np.uint64(noise_seed(key))).astype(np.uint32)


def noise_threshold(rate):
    """uint32 t with  h < t  <=>  h * 2^-32 < rate  (the reference's uniform(0, 1) < amount on a 32-bit uniform); rate >= 1
    saturates at 2^32 - 1"""
    t = math.ceil(float(rate) * 4294967296.0)      # (exact: a power-of-two scaling of a double)
    return max(0, min(t, _M32))


def test_ink_max():
    """the largest byte that utils_for_test.py:22-24, 1 - ((u8 / 255).astype(f32) > 0.2), maps to 1 (checked monotone)"""
    u8 = np.arange(256, dtype=np.uint8)
    ink = (1 - ((u8 / 255).astype("float32") > 0.2)).astype(bool)
    c = int(np.flatnonzero(ink).max())
    if not (ink[:c + 1].all() and not ink[c + 1:].any()):
        raise AssertionError("the test-mode threshold is not a byte cut")
    return c


def draw_augment(rng, amount, src_shape, size=512):
    """utils.py:44-58, 73, 76 for one image of shape src_shape = (rows, cols) with 512 generalised to `size`: the same draws
    in the same order (rand() < 0.2, rand() < 0.5, uniform(0.8, 1), then uniform(0, amount / 100) and uniform(0, amount)) from
    `rng` (np.random itself, or a RandomState), then two randint(0, 2^32) for the noise key.  Returns (AugmentDraw,
    (scale_x, scale_y, ddx, ddy)) -- the second what raster.parse_record takes.  Raises when the image would not fit the canvas."""
    S = int(size)
    rows, cols = int(src_shape[0]), int(src_shape[1])
    scale_x = 1
    scale_y = 1
    if rng.rand() < 0.2:
        if rng.rand() < 0.5:
            scale_x = rng.uniform(0.8, 1)
            rows, cols = int(scale_x * S), S          # cv2.resize(img, (S, int(scale_x * S))): dsize is (width, height)
        else:
            scale_y = rng.uniform(0.8, 1)
            rows, cols = S, int(scale_y * S)
    if not (1 <= rows <= S and 1 <= cols <= S):
        raise ValueError("draw_augment: a %s source does not fit the %d x %d canvas without a resize" % (tuple(src_shape), S, S))
    ddx = (S - rows) // 2
    ddy = (S - cols) // 2
    salt = rng.uniform(0, amount / 100)
    pepper = rng.uniform(0, amount)
    key = int(rng.randint(0, 1 << 32)) | (int(rng.randint(0, 1 << 32)) << 32)
    return AugmentDraw(rows, cols, ddx, ddy, scale_x, scale_y, float(salt), float(pepper), key), (scale_x, scale_y, ddx, ddy)


def param_row(src_shape, draw=None, size=512):
    """the kernel's int32 parameter row (abc_image_param order); draw=None: the test mode's (no resize, pad or noise)"""
    sh, sw = int(src_shape[0]), int(src_shape[1])
    if draw is None:
        vals = [sh, sw, size, size, 0, 0, 0, 0, 0, 0]
    else:
        vals = [sh, sw, draw.rows, draw.cols, draw.ddx, draw.ddy, noise_threshold(draw.salt), noise_threshold(draw.pepper),
                draw.key & _M32, (draw.key >> 32) & _M32]
    return np.array(vals, dtype=np.uint64).astype(np.uint32).view(np.int32)


class ImageBuilder:
    """device-side utils.py:42-81 (mode "train") or utils_for_test.py:21-27 (mode "test") for a batch of `batch` uint8 renders
    into f32 [batch, 1, size, size] -- `out` may be a Trainer's or InferenceRunner's .input_images (then run() writes the network's
    input in place), otherwise a fresh tensor is allocated.  max_src = (rows, cols) capacity of a source, at most 1024 x 1024."""

    def __init__(self, batch, size, mode="train", amount=0.1, out=None, max_src=None, device="cuda"):
        if mode not in MODES:
            raise ValueError("ImageBuilder: mode must be 'train' or 'test', got %r" % (mode,))
        if not torch.cuda.is_available():
            raise L.AbcNetHipError("ImageBuilder needs an MI355X; abcnet_amd has no CPU fallback")
        S = int(size)
        if S < 8 or S % 8 or S > 8192:
            raise ValueError("ImageBuilder: size must be a multiple of 8 (8 .. 8192), got %d" % S)
        max_h, max_w = (S, S) if max_src is None else (int(max_src[0]), int(max_src[1]))
        if not (1 <= max_h <= 1024 and 1 <= max_w <= 1024):
            raise ValueError("ImageBuilder: sources are at most 1024 x 1024, got max_src %s" % ((max_h, max_w),))
        if mode == "test" and (max_h < S or max_w < S):
            raise ValueError("ImageBuilder(mode='test'): the sources are %d x %d, max_src must hold that" % (S, S))
        shape = (batch, 1, S, S)
        if out is None:
            out = torch.zeros(shape, dtype=torch.float32, device=device)
        if tuple(out.shape) != shape:
            raise L.AbcNetHipError("ImageBuilder: out %s does not match the contract %s (a %d-channel input is not an image of this "
                                   "loader)" % (tuple(out.shape), shape, out.shape[1] if out.dim() == 4 else -1))
        require_device_tensor(out, torch.float32, "ImageBuilder: out")
        self.lib = L.load()
        self.out, self.B, self.S, self.mode, self.amount = out, batch, S, mode, float(amount)
        self.max_h, self.max_w = max_h, max_w
        self.pitch = -(-max_w // 16) * 16
        dev = out.device
        self.staging = PinnedStaging(dev, {"src": ((batch, max_h, self.pitch), torch.uint8, 255), "par": ((batch, L.IMG_NPARAM), torch.int32)})
        self.h_src, self.h_par = self.staging.host.values()
        self.d_src, self.d_par = self.staging.dev.values()
        self._np_src, self._np_par = self.h_src.numpy(), self.h_par.numpy()
        d = L.ImageDesc()
        d.out, d.src, d.params = out.data_ptr(), self.d_src.data_ptr(), self.d_par.data_ptr()
        d.params_host = self.h_par.data_ptr()      # (what the last load staged: checked by every eager call)
        d.src_stride, d.src_pitch, d.src_max_h = max_h * self.pitch, self.pitch, max_h
        d.B, d.S, d.mode = batch, S, MODES[mode]
        d.test_max_ink = test_ink_max() if mode == "test" else 0
        self.d = d

    def draw(self, rng, src_shapes):
        """draw_augment for every image of a batch, in order"""
        return [draw_augment(rng, self.amount, s, self.S) for s in src_shapes]

    def load(self, images_u8, params=None):
        """images_u8: B 2-d uint8 arrays (decoded grey renders); params: B AugmentDraw (mode "train"), None in mode "test".
        Host work: the checks and one memcpy per image into pinned staging, then an asynchronous H2D copy."""
        if len(images_u8) != self.B:
            raise ValueError("expected %d images" % self.B)
        if self.mode == "train" and (params is None or len(params) != self.B):
            raise ValueError("mode 'train' needs one AugmentDraw per image")
        rows = []
        for b, img in enumerate(images_u8):
            img = np.asarray(img)
            if img.dtype != np.uint8 or img.ndim != 2:
                raise ValueError("image %d: a 2-d uint8 array, got %s %s" % (b, img.dtype, img.shape))
            h, w = img.shape
            if h > self.max_h or w > self.max_w:
                raise ValueError("image %d: %d x %d exceeds the staging capacity %d x %d" % (b, h, w, self.max_h, self.max_w))
            if self.mode == "test":
                if (h, w) != (self.S, self.S):
                    raise ValueError("image %d: test mode takes %d x %d sources, got %d x %d" % (b, self.S, self.S, h, w))
                rows.append(param_row((h, w), None, self.S))
            else:
                p = params[b]
                if not (1 <= p.rows <= self.S and 1 <= p.cols <= self.S and 0 <= p.ddx <= self.S - p.rows and 0 <= p.ddy <= self.S - p.cols):
                    raise ValueError("image %d: %d x %d at (%d, %d) leaves the %d x %d canvas" % (b, p.rows, p.cols, p.ddx, p.ddy, self.S, self.S))
                rows.append(param_row((h, w), p, self.S))
        self.staging.wait()
        for b, img in enumerate(images_u8):
            img = np.asarray(img)
            self._np_src[b, :img.shape[0], :img.shape[1]] = img
            self._np_par[b] = rows[b]
        self.staging.commit()

    def run(self, stream=None):
        """one launch (graph-capturable): the f32 batch into self.out"""
        L.check(self.lib.abc_build_images(C.byref(self.d), stream_or_current(stream, self.out.device)), "build_images")
        return self.out


# ------------------------------------------------------------------------------------------------------------------ scans
POLARITIES = {"dark": L.SCAN_DARK, "light": L.SCAN_LIGHT, "auto": L.SCAN_AUTO}
# the coverage a destination pixel needs (in 1/256 of its source box) when none is given: the one with the best mean environment
# similarity on the frozen trained fixture, the smaller one on a tie (profiles/r13_scan.md, profiles/tools/scan_step.py)
DEFAULT_COVER_Q8 = 128


def otsu_threshold(hist):
    """the threshold rule of abc_build_scan_images on a 256-bin histogram (any integer counts, total <= 2^24): the smallest
    admissible t (both sides non-empty) with maximal sigma(t) = (d * d) / (w0 * w1) in float64, d = S w0 - N s0 exact in int64;
    None when the image holds a single value.  Pure host arithmetic, bit for bit what the device computes."""
    h = np.asarray(hist).astype(np.int64).reshape(256)
    w0 = np.cumsum(h)
    s0 = np.cumsum(h * np.arange(256, dtype=np.int64))
    N, S = int(w0[-1]), int(s0[-1])
    w1 = N - w0
    ok = (w0 > 0) & (w1 > 0)
    if not ok.any():
        return None
    d = (S * w0 - N * s0).astype(np.float64)
    num = d * d
    den = w0.astype(np.float64) * w1.astype(np.float64)
    sigma = np.full(256, -1.0)
    sigma[ok] = num[ok] / den[ok]
    return int(np.argmax(sigma))      # (the first index of the maximum)


def fit_scan(bh, bw, size, margin):
    """the fit rule of abc_build_scan_images: (rows, cols, ddx, ddy) of a bh x bw bounding box on a size x size canvas; never
    upscales, floor division"""
    bh, bw, S, margin = int(bh), int(bw), int(size), int(margin)
    if bh < 1 or bw < 1 or not 0 <= 2 * margin < S:
        raise ValueError("fit_scan: a box of at least 1 x 1 and 0 <= 2 * margin < size, got %s" % ((bh, bw, S, margin),))
    lim, m = S - 2 * margin, max(bh, bw)
    rows, cols = (bh, bw) if m <= lim else (max(1, bh * lim // m), max(1, bw * lim // m))
    return rows, cols, (S - rows) // 2, (S - cols) // 2


def scan_record_offsets(y0, x0, bh, bw, rows, cols, ddx, ddy):
    """(scale_x, scale_y, ddx', ddy'): the affine map of SOURCE coordinates onto the canvas, what raster.parse_record and
    parse_graph take -- x * scale_x + ddx' with scale_x = rows / bh and ddx' = ddx - y0 * scale_x (x indexes rows)"""
    scale_x, scale_y = rows / bh, cols / bw
    return scale_x, scale_y, ddx - y0 * scale_x, ddy - x0 * scale_y


class ScanBuilder:
    """raw grey scans into f32 [batch, 1, size, size] on the device (csrc/scan.hip; the contract: include/abcnet_hip.h,
    abc_scan_desc): per image a histogram, an Otsu threshold, the polarity, the ink's bounding box, an aspect-preserving fit
    with `margin` that never upscales, and a downscale by coverage -- a destination pixel is ink when its source box holds
    at least one ink pixel and at least cover / 256 of its area.  `out` may be an InferenceRunner's or a Trainer's
    .input_images, as with ImageBuilder.  max_src = (rows, cols) capacity of a source, at most 4096 x 4096.

    margin defaults to the margin=20 of synthetic.drawn_molecules at 512, scaled: size * 20 // 512.  cover (0 .. 256, in
    1 / 256) defaults to DEFAULT_COVER_Q8, the value with the best mean environment similarity of the frozen trained fixture
    in profiles/r13_scan.md -- measured on SYNTHETIC drawings made into scans on the host, because no real scan was
    available.  No CPU fallback.

    thin, stroke_radius, drop_isolated: the stroke normalisation of ops.StrokeNormalizer (csrc/stroke.hip), off by default.  With
    any of them set, run() appends it as a sixth launch on the same stream, over `out` in place, skipping the images whose
    geometry status is non-zero (a CONSTANT image stays blank, a BAD_PARAMS one keeps its NaN); stroke_stats() returns its rows.
    The geometry rows do not change: `ink` stays the source's count.  size is then at most L.STROKE_MAX_SIZE.  Recommended where it
    is used: thin=1, stroke_radius=1, the one setting of twelve that beat the unnormalised scans under both candidate rules in
    profiles/r14_stroke.md (synthetic scans again, and by little); thinning to the skeleton turns a solid wedge into a line.

    clean_cell, clean_min_ink, clean_keep: the cell component filter (the contract: include/abcnet_hip.h, abc_scan_clean_desc), off
    by default (clean_cell=None is the object above, calling abc_build_scan_images).  With clean_cell in 8 / 16 / 32 / 64, run()
    calls abc_build_scan_images_clean instead: ink closer than about one cell belongs together, each group of cells is weighed
    by its ink, and only the groups with at least clean_min_ink ink pixels and at least clean_keep / 256 of the heaviest group's
    weight are kept; the box and the resample read ink from kept cells only, so a speck of dirt or a caption far from the
    drawing no longer sets the crop.  An image with nothing kept is blank with status L.SCAN_NO_COMPONENT.  clean_stats() returns
    the rows of L.SCAN_CLEAN_COLUMNS; debug_cells=True also keeps every cell's label and keep bit for clean_cells().  The stroke
    launch, when asked for, still follows and still skips rows with non-zero status.  Recommended where scans carry specks of
    dirt: clean_cell=16, clean_min_ink=64, clean_keep=0, the setting of profiles/r16_scan_clean.md (synthetic scans made dirty
    on the host; no real scan was available) that dropped every added speck, took ink from no drawing and had the best mean
    similarity under the `peaks` rule; it keeps a caption of letter-sized blobs.  clean_keep=256 (the heaviest group alone) is
    NOT recommended: those drawings are several groups at every cell size tried (a label, a second fragment), and it took ink
    from all of them."""

    def __init__(self, batch, size, out=None, max_src=(1024, 1024), margin=None, cover=None, polarity="dark", device="cuda",
                 thin=None, stroke_radius=None, drop_isolated=False, clean_cell=None, clean_min_ink=0, clean_keep=0,
                 debug_cells=False):
        if polarity not in POLARITIES:
            raise ValueError("ScanBuilder: polarity must be 'dark', 'light' or 'auto', got %r" % (polarity,))
        if clean_cell is None:
            if clean_min_ink or clean_keep or debug_cells:
                raise ValueError("ScanBuilder: clean_min_ink, clean_keep and debug_cells need clean_cell (one of %s)" % (L.SCAN_CLEAN_CELLS,))
        else:
            if isinstance(clean_cell, bool) or clean_cell not in L.SCAN_CLEAN_CELLS:
                raise ValueError("ScanBuilder: clean_cell must be one of %s or None, got %r" % (L.SCAN_CLEAN_CELLS, clean_cell))
            if int(clean_min_ink) != clean_min_ink or clean_min_ink < 0 or clean_min_ink >= 2 ** 31:
                raise ValueError("ScanBuilder: clean_min_ink is a count of ink pixels, an integer >= 0, got %r" % (clean_min_ink,))
            if int(clean_keep) != clean_keep or not 0 <= clean_keep <= 256:
                raise ValueError("ScanBuilder: clean_keep is in 1 / 256 of the heaviest component, 0 .. 256, got %r" % (clean_keep,))
        normalise = stroke_max_iter(thin, "ScanBuilder") != 0 or stroke_radius is not None or bool(drop_isolated)
        if normalise and int(size) > L.STROKE_MAX_SIZE:
            raise ValueError("ScanBuilder: thin / stroke_radius / drop_isolated need size <= %d (the normaliser holds an image in "
                             "LDS), got %d" % (L.STROKE_MAX_SIZE, int(size)))
        if not torch.cuda.is_available():
            raise L.AbcNetHipError("ScanBuilder needs an MI355X; abcnet_amd has no CPU fallback")
        S = int(size)
        if S < 8 or S % 8 or S > 8192:
            raise ValueError("ScanBuilder: size must be a multiple of 8 (8 .. 8192), got %d" % S)
        max_h, max_w = int(max_src[0]), int(max_src[1])
        if not (1 <= max_h <= 4096 and 1 <= max_w <= 4096):
            raise ValueError("ScanBuilder: sources are at most 4096 x 4096, got max_src %s" % ((max_h, max_w),))
        if not 1 <= batch <= 65535:
            raise ValueError("ScanBuilder: batch must be 1 .. 65535, got %d" % batch)
        margin = S * 20 // 512 if margin is None else int(margin)
        cover = DEFAULT_COVER_Q8 if cover is None else int(cover)
        if not 0 <= 2 * margin < S:
            raise ValueError("ScanBuilder: 0 <= 2 * margin < size, got margin %d at size %d" % (margin, S))
        if not 0 <= cover <= 256:
            raise ValueError("ScanBuilder: cover is in 1 / 256, 0 .. 256, got %d" % cover)
        shape = (batch, 1, S, S)
        if out is None:
            out = torch.zeros(shape, dtype=torch.float32, device=device)
        if tuple(out.shape) != shape:
            raise L.AbcNetHipError("ScanBuilder: out %s does not match the contract %s (a %d-channel input is not an image of this "
                                   "loader)" % (tuple(out.shape), shape, out.shape[1] if out.dim() == 4 else -1))
        require_device_tensor(out, torch.float32, "ScanBuilder: out")
        self.lib = L.load()
        self.out, self.B, self.S, self.margin, self.cover, self.polarity = out, batch, S, margin, cover, polarity
        self.max_h, self.max_w = max_h, max_w
        self.pitch = -(-max_w // 16) * 16
        dev = out.device
        self.staging = PinnedStaging(dev, {"src": ((batch, max_h, self.pitch), torch.uint8, 255), "par": ((batch, L.SCAN_NPARAM), torch.int32)})
        self.h_src, self.h_par = self.staging.host.values()
        self.d_src, self.d_par = self.staging.dev.values()
        self._np_src, self._np_par = self.h_src.numpy(), self.h_par.numpy()
        self.hist = torch.zeros((batch, 256), dtype=torch.int32, device=dev)             # (uint32 bit patterns)
        self.box = torch.zeros((batch, L.SCAN_NBOX), dtype=torch.int32, device=dev)
        self.geom = torch.zeros((batch, len(L.SCAN_GEOM_COLUMNS)), dtype=torch.int32, device=dev)
        d = L.ScanDesc()
        d.out, d.src, d.params = out.data_ptr(), self.d_src.data_ptr(), self.d_par.data_ptr()
        d.params_host = self.h_par.data_ptr()      # (what the last load staged: checked by every eager call)
        d.src_stride, d.src_pitch, d.src_max_h = max_h * self.pitch, self.pitch, max_h
        d.B, d.S, d.margin, d.cover_q8, d.polarity = batch, S, margin, cover, POLARITIES[polarity]
        d.hist, d.box, d.geom = self.hist.data_ptr(), self.box.data_ptr(), self.geom.data_ptr()
        self.d = d
        # the cell component filter, when asked for: its descriptor, its scratch and its outputs
        self.clean = None
        if clean_cell is not None:
            cell = int(clean_cell)
            self.cap_cells = (-(-max_h // cell), -(-self.pitch // cell))
            nbytes = self.lib.abc_scan_clean_scratch_bytes(batch, max_h, self.pitch, cell)
            if nbytes < 0:
                raise L.AbcNetHipError("scan_clean_scratch_bytes: %s" % self.lib.abc_last_error().decode())
            self.clean_scratch = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
            self.clean_rows = torch.zeros((batch, len(L.SCAN_CLEAN_COLUMNS)), dtype=torch.int32, device=dev)
            q = L.ScanCleanDesc()
            q.scratch, q.stats = self.clean_scratch.data_ptr(), self.clean_rows.data_ptr()
            q.cell, q.min_ink, q.keep_q8 = cell, int(clean_min_ink), int(clean_keep)
            self.cell_labels = self.cell_keep = None
            if debug_cells:
                self.cell_labels = torch.zeros((batch,) + self.cap_cells, dtype=torch.int32, device=dev)
                self.cell_keep = torch.zeros((batch,) + self.cap_cells, dtype=torch.uint8, device=dev)
                q.labels_out, q.keep_out = self.cell_labels.data_ptr(), self.cell_keep.data_ptr()
            self.clean = q
        # the last launch, when asked for: in place over out, the geometry status column as its skip words
        self.strokes = None
        if normalise:
            self.strokes = StrokeNormalizer(out, thin=thin, radius=0 if stroke_radius is None else stroke_radius,
                                            drop_isolated=drop_isolated, skip=self.geom[:, L.SCAN_GEOM_COLUMNS.index("status")])

    def load(self, images_u8):
        """images_u8: B 2-d uint8 arrays (decoded grey scans), each within max_src.  Host work: the checks and one memcpy per
        image into pinned staging, then an asynchronous H2D copy."""
        if len(images_u8) != self.B:
            raise ValueError("expected %d images" % self.B)
        imgs = []
        for b, img in enumerate(images_u8):
            img = np.asarray(img)
            if img.dtype != np.uint8 or img.ndim != 2:
                raise ValueError("image %d: a 2-d uint8 array, got %s %s" % (b, img.dtype, img.shape))
            h, w = img.shape
            if h < 1 or w < 1:
                raise ValueError("image %d: an empty array (%d x %d)" % (b, h, w))
            if h > self.max_h or w > self.max_w:
                raise ValueError("image %d: %d x %d exceeds the staging capacity %d x %d" % (b, h, w, self.max_h, self.max_w))
            imgs.append(img)
        self.staging.wait()
        for b, img in enumerate(imgs):
            self._np_src[b, :img.shape[0], :img.shape[1]] = img
            self._np_par[b] = img.shape
        self.staging.commit()

    def run(self, stream=None):
        """five launches in order on one stream (graph-capturable): the f32 batch into self.out, the geometry rows beside it; a
        sixth, the stroke normaliser, when thin / stroke_radius / drop_isolated ask for it.  With clean_cell set the five are the
        nine of abc_build_scan_images_clean, the same number whatever the images hold"""
        stream = stream_or_current(stream, self.out.device)
        if self.clean is None:
            L.check(self.lib.abc_build_scan_images(C.byref(self.d), stream), "build_scan_images")
        else:
            L.check(self.lib.abc_build_scan_images_clean(C.byref(self.d), C.byref(self.clean), stream), "build_scan_images_clean")
        if self.strokes is not None:
            self.strokes.run(stream)
        return self.out

    def clean_stats(self):
        """the cleaning rows of the last run() as a structured numpy array [B] with the int32 fields L.SCAN_CLEAN_COLUMNS
        (components, kept, ink_kept, ink_dropped, heaviest, occupied_cells); all zeros for a CONSTANT or BAD_PARAMS image
        (synchronises)"""
        if self.clean is None:
            raise ValueError("ScanBuilder: no cleaning was asked for (clean_cell)")
        rows = np.ascontiguousarray(self.clean_rows.cpu().numpy())
        return rows.view(np.dtype([(c, np.int32) for c in L.SCAN_CLEAN_COLUMNS])).reshape(self.B)

    def clean_cells(self):
        """(labels int32, keep uint8), each [B, cap_ch, cap_cw] over the capacity grid of cells, of the last run(): an occupied
        cell's label is the smallest cy * cap_cw + cx of its component, every other cell holds -1; keep is 1 for a kept occupied
        cell (synchronises).  Needs debug_cells=True"""
        if self.clean is None or self.cell_labels is None:
            raise ValueError("ScanBuilder: clean_cells() needs clean_cell and debug_cells=True")
        return self.cell_labels.cpu().numpy(), self.cell_keep.cpu().numpy()

    def stroke_stats(self):
        """the normaliser's rows of the last run(): ops.StrokeNormalizer.stats() (synchronises)"""
        if self.strokes is None:
            raise ValueError("ScanBuilder: no stroke normalisation was asked for (thin, stroke_radius, drop_isolated)")
        return self.strokes.stats()

    def geometry(self):
        """the geometry rows of the last run() as a structured numpy array [B] with the int32 fields L.SCAN_GEOM_COLUMNS (thr,
        inverted, status, y0, x0, bh, bw, rows, cols, ddx, ddy, ink).  The only call here that synchronises."""
        rows = np.ascontiguousarray(self.geom.cpu().numpy())
        return rows.view(np.dtype([(c, np.int32) for c in L.SCAN_GEOM_COLUMNS])).reshape(self.B)

    def record_offsets(self, b):
        """(scale_x, scale_y, ddx', ddy') of image b after run(): what raster.parse_record / parse_graph take, so that
        annotations in the scan's own coordinates can be graded with the evaluators that exist (synchronises: geometry())"""
        g = self.geometry()[b]
        if g["status"]:
            raise ValueError("image %d has no drawing (status %d)" % (b, int(g["status"])))
        return scan_record_offsets(*(int(g[c]) for c in ("y0", "x0", "bh", "bw", "rows", "cols", "ddx", "ddy")))


def scan_page_positions(offsets, xy):
    """the inverse of scan_record_offsets: canvas positions xy [..., 2] (x indexes rows, y columns, as everywhere here) back
    into SOURCE coordinates, float64 -- x_src = (x - ddx') / scale_x, y_src = (y - ddy') / scale_y"""
    scale_x, scale_y, ddx, ddy = offsets
    xy = np.asarray(xy, dtype=np.float64)
    if xy.shape[-1:] != (2,):
        raise ValueError("scan_page_positions: positions are [..., 2] (x, y), got shape %s" % (xy.shape,))
    return (xy - np.array([ddx, ddy], dtype=np.float64)) / np.array([scale_x, scale_y], dtype=np.float64)


# the cell and the reach PageSplitter uses when none is given: the pair that merged no drawing with its caption and, among those,
# left the most drawings whole on the composed pages of profiles/r27_page_split.md (profiles/tools/page_split_step.py)
DEFAULT_SPLIT_CELL, DEFAULT_SPLIT_REACH = 32, 3


class PageSplitter:
    """page scans into their drawings, one f32 canvas [1, size, size] each, on the device (csrc/scan.hip; the contract:
    include/abcnet_hip.h, abc_scan_split_desc, and DESIGN.md section 7).  `pages` grey pages per load, `canvases` canvases per
    run: `out` is [canvases, 1, size, size] and may be an InferenceRunner.input_images of batch `canvases`.  Per page the
    threshold, the polarity and the cells are ScanBuilder's; occupied cells within `reach` cells of each other (Chebyshev
    distance) are one group, a group is kept when it has at least min_ink ink pixels and keep / 256 of the page's heaviest, a
    page's kept groups are its drawings in the reading order of their first cells, at most max_per_page of them, and the
    drawings of all pages fill the canvases in order without holes; each is cropped by its own box and fitted as ScanBuilder
    fits.  Unused canvases are blank with status L.SCAN_NO_COMPONENT.  `total` is a device int32 [2] (canvases written, kept
    groups of all pages); `n_canvases` is its first word as a [1] view, the format of InferenceRunner.n_valid:
    runner.n_valid.copy_(splitter.n_canvases) needs no sync.  A page that held more than max_per_page groups carries
    L.SCAN_SPLIT_PAGE_FULL in its status, a page that lost a drawing to `canvases` L.SCAN_SPLIT_BATCH_FULL.  No CPU fallback.

    cell and reach default to DEFAULT_SPLIT_CELL and DEFAULT_SPLIT_REACH (32 and 3; a first guess was 32 and 2), the measured
    choice of profiles/r27_page_split.md: pages composed on the host from synthetic drawings with white gutters and a caption
    under each, because no real page was available.  Those drawings are sparse, and no pair tried kept all of them whole: a
    page of known layout deserves a cell and reach of its own (reach * cell is about the gap, in pixels, that still joins).  Not covered: drawings that touch (one group), a caption within reach of its drawing (joins it), deskewing, and
    pages whose Otsu threshold takes a ground or a frame for ink."""

    def __init__(self, pages, canvases, size, out=None, max_src=(2048, 2048), max_per_page=16, cell=None, reach=None, min_ink=0,
                 keep=0, margin=None, cover=None, polarity="dark", device="cuda", debug_cells=False):
        if polarity not in POLARITIES:
            raise ValueError("PageSplitter: polarity must be 'dark', 'light' or 'auto', got %r" % (polarity,))
        cell = DEFAULT_SPLIT_CELL if cell is None else cell
        reach = DEFAULT_SPLIT_REACH if reach is None else reach
        if isinstance(cell, bool) or cell not in L.SCAN_CLEAN_CELLS:
            raise ValueError("PageSplitter: cell must be one of %s, got %r" % (L.SCAN_CLEAN_CELLS, cell))
        if isinstance(reach, bool) or int(reach) != reach or not 1 <= reach <= L.SCAN_SPLIT_MAX_REACH:
            raise ValueError("PageSplitter: reach is a distance in cells, 1 .. %d, got %r" % (L.SCAN_SPLIT_MAX_REACH, reach))
        if isinstance(max_per_page, bool) or int(max_per_page) != max_per_page or not 1 <= max_per_page <= L.SCAN_SPLIT_MAX_PER_PAGE:
            raise ValueError("PageSplitter: max_per_page must be 1 .. %d, got %r" % (L.SCAN_SPLIT_MAX_PER_PAGE, max_per_page))
        if int(min_ink) != min_ink or min_ink < 0 or min_ink >= 2 ** 31:
            raise ValueError("PageSplitter: min_ink is a count of ink pixels, an integer >= 0, got %r" % (min_ink,))
        if int(keep) != keep or not 0 <= keep <= 256:
            raise ValueError("PageSplitter: keep is in 1 / 256 of the heaviest group, 0 .. 256, got %r" % (keep,))
        S = int(size)
        if S < 8 or S % 8 or S > 8192:
            raise ValueError("PageSplitter: size must be a multiple of 8 (8 .. 8192), got %d" % S)
        max_h, max_w = int(max_src[0]), int(max_src[1])
        if not (1 <= max_h <= 4096 and 1 <= max_w <= 4096):
            raise ValueError("PageSplitter: sources are at most 4096 x 4096, got max_src %s" % ((max_h, max_w),))
        if not 1 <= pages <= 65535:
            raise ValueError("PageSplitter: pages must be 1 .. 65535, got %d" % pages)
        if not 1 <= canvases <= 65535:
            raise ValueError("PageSplitter: canvases must be 1 .. 65535, got %d" % canvases)
        margin = S * 20 // 512 if margin is None else int(margin)
        cover = DEFAULT_COVER_Q8 if cover is None else int(cover)
        if not 0 <= 2 * margin < S:
            raise ValueError("PageSplitter: 0 <= 2 * margin < size, got margin %d at size %d" % (margin, S))
        if not 0 <= cover <= 256:
            raise ValueError("PageSplitter: cover is in 1 / 256, 0 .. 256, got %d" % cover)
        if not torch.cuda.is_available():
            raise L.AbcNetHipError("PageSplitter needs an MI355X; abcnet_amd has no CPU fallback")
        P, D, cell = int(pages), int(canvases), int(cell)
        shape = (D, 1, S, S)
        if out is None:
            out = torch.zeros(shape, dtype=torch.float32, device=device)
        if tuple(out.shape) != shape:
            raise L.AbcNetHipError("PageSplitter: out %s does not match the contract %s (a %d-channel input is not an image of this "
                                   "loader)" % (tuple(out.shape), shape, out.shape[1] if out.dim() == 4 else -1))
        require_device_tensor(out, torch.float32, "PageSplitter: out")
        self.lib = L.load()
        self.out, self.P, self.D, self.S, self.margin, self.cover, self.polarity = out, P, D, S, margin, cover, polarity
        self.max_h, self.max_w = max_h, max_w
        self.pitch = -(-max_w // 16) * 16
        self.cap_cells = (-(-max_h // cell), -(-self.pitch // cell))
        dev = out.device
        self.staging = PinnedStaging(dev, {"src": ((P, max_h, self.pitch), torch.uint8, 255), "par": ((P, L.SCAN_NPARAM), torch.int32)})
        self.h_src, self.h_par = self.staging.host.values()
        self.d_src, self.d_par = self.staging.dev.values()
        self._np_src, self._np_par = self.h_src.numpy(), self.h_par.numpy()
        self.hist = torch.zeros((P, 256), dtype=torch.int32, device=dev)                 # (uint32 bit patterns)
        self.box = torch.zeros((D, L.SCAN_NBOX), dtype=torch.int32, device=dev)
        self.geom = torch.zeros((D, len(L.SCAN_GEOM_COLUMNS)), dtype=torch.int32, device=dev)
        self.page_rows = torch.zeros((P, len(L.SCAN_PAGE_COLUMNS)), dtype=torch.int32, device=dev)
        self.drawing_rows = torch.zeros((D, len(L.SCAN_DRAWING_COLUMNS)), dtype=torch.int32, device=dev)
        self.total = torch.zeros(2, dtype=torch.int32, device=dev)
        self.n_canvases = self.total[:1]
        nbytes = self.lib.abc_scan_split_scratch_bytes(P, max_h, self.pitch, cell, D)
        if nbytes < 0:
            raise L.AbcNetHipError("scan_split_scratch_bytes: %s" % self.lib.abc_last_error().decode())
        self.scratch = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        d = L.ScanDesc()
        d.out, d.src, d.params = out.data_ptr(), self.d_src.data_ptr(), self.d_par.data_ptr()
        d.params_host = self.h_par.data_ptr()      # (what the last load staged: checked by every eager call)
        d.src_stride, d.src_pitch, d.src_max_h = max_h * self.pitch, self.pitch, max_h
        d.B, d.S, d.margin, d.cover_q8, d.polarity = P, S, margin, cover, POLARITIES[polarity]
        d.hist, d.box, d.geom = self.hist.data_ptr(), self.box.data_ptr(), self.geom.data_ptr()
        q = L.ScanSplitDesc()
        q.scratch, q.pages, q.drawings, q.total = (self.scratch.data_ptr(), self.page_rows.data_ptr(), self.drawing_rows.data_ptr(),
                                                   self.total.data_ptr())
        q.canvases, q.max_per_page, q.cell, q.reach, q.min_ink, q.keep_q8 = D, int(max_per_page), cell, int(reach), int(min_ink), int(keep)
        self.cell_labels = self.cell_canvas = None
        if debug_cells:
            self.cell_labels = torch.zeros((P,) + self.cap_cells, dtype=torch.int32, device=dev)
            self.cell_canvas = torch.zeros((P,) + self.cap_cells, dtype=torch.int32, device=dev)
            q.labels_out, q.canvas_out = self.cell_labels.data_ptr(), self.cell_canvas.data_ptr()
        self.d, self.q = d, q

    def load(self, images_u8):
        """images_u8: `pages` 2-d uint8 arrays (decoded grey pages), each within max_src.  Host work: the checks and one memcpy
        per page into pinned staging, then an asynchronous H2D copy."""
        if len(images_u8) != self.P:
            raise ValueError("expected %d images" % self.P)
        imgs = []
        for b, img in enumerate(images_u8):
            img = np.asarray(img)
            if img.dtype != np.uint8 or img.ndim != 2:
                raise ValueError("image %d: a 2-d uint8 array, got %s %s" % (b, img.dtype, img.shape))
            h, w = img.shape
            if h < 1 or w < 1:
                raise ValueError("image %d: an empty array (%d x %d)" % (b, h, w))
            if h > self.max_h or w > self.max_w:
                raise ValueError("image %d: %d x %d exceeds the staging capacity %d x %d" % (b, h, w, self.max_h, self.max_w))
            imgs.append(img)
        self.staging.wait()
        for b, img in enumerate(imgs):
            self._np_src[b, :img.shape[0], :img.shape[1]] = img
            self._np_par[b] = img.shape
        self.staging.commit()

    def run(self, stream=None):
        """ten launches in order on one stream (graph-capturable), the same number whatever the pages hold: the canvases into
        self.out, their geometry rows, the page and drawing tables and `total` beside them"""
        L.check(self.lib.abc_split_scan_pages(C.byref(self.d), C.byref(self.q), stream_or_current(stream, self.out.device)),
                "split_scan_pages")
        return self.out

    @staticmethod
    def _structured(t, columns):
        rows = np.ascontiguousarray(t.cpu().numpy())
        return rows.view(np.dtype([(c, np.int32) for c in columns])).reshape(rows.shape[0])

    def geometry(self):
        """the canvases' geometry rows of the last run() as a structured numpy array [canvases] with the int32 fields
        L.SCAN_GEOM_COLUMNS; thr and inverted are the page's, ink the drawing's weight (synchronises)"""
        return self._structured(self.geom, L.SCAN_GEOM_COLUMNS)

    def pages(self):
        """the page rows of the last run() as a structured numpy array [pages] with the int32 fields L.SCAN_PAGE_COLUMNS (status,
        groups, kept, first, taken, ink_kept, ink_dropped, occupied_cells) (synchronises)"""
        return self._structured(self.page_rows, L.SCAN_PAGE_COLUMNS)

    def drawings(self):
        """the drawing rows of the last run() as a structured numpy array [canvases] with the int32 fields L.SCAN_DRAWING_COLUMNS
        (page, label, weight, rank_in_page); -1, -1, 0, -1 for an unused canvas (synchronises)"""
        return self._structured(self.drawing_rows, L.SCAN_DRAWING_COLUMNS)

    def cells(self):
        """(labels int32, canvas int32), each [pages, cap_ch, cap_cw] over the capacity grid of cells, of the last run(): an
        occupied cell's label is the smallest cy * cap_cw + cx of its group, the canvas the one its ink went to; -1 elsewhere
        (synchronises).  Needs debug_cells=True"""
        if self.cell_labels is None:
            raise ValueError("PageSplitter: cells() needs debug_cells=True")
        return self.cell_labels.cpu().numpy(), self.cell_canvas.cpu().numpy()

    def record_offsets(self, j):
        """(scale_x, scale_y, ddx', ddy') of canvas j after run(), by scan_record_offsets: the map of its PAGE's coordinates onto
        the canvas, what raster.parse_record / parse_graph take (synchronises: geometry())"""
        g = self.geometry()[j]
        if g["status"]:
            raise ValueError("canvas %d has no drawing (status %d)" % (j, int(g["status"])))
        return scan_record_offsets(*(int(g[c]) for c in ("y0", "x0", "bh", "bw", "rows", "cols", "ddx", "ddy")))

    def page_positions(self, j, xy):
        """positions xy [..., 2] on canvas j (decoded atom positions: x indexes rows, y columns) back into the coordinates of its
        page, drawings()[j]["page"]: the inverse of record_offsets(j) (synchronises)"""
        return scan_page_positions(self.record_offsets(j), xy)


class SampleBuilder:
    """a whole batch on the device: an ImageBuilder over owner.input_images and a TargetRasterizer over owner.targets, fed with
    the SAME draws (utils.py:42-228 for every image).  `owner` is a Trainer, or an InferenceRunner(evaluate=True) -- the loop of
    test_accuracy.py:94-269 reads the same MolecularImageDataset.  sparse=True: the rasteriser's sparse form, registered with
    owner.use_sparse_targets.  Over a runner load() takes n <= B samples (a short last batch): the rows past n get an empty
    record and a blank image, and owner.n_valid becomes n."""

    def __init__(self, trainer, amount=0.1, max_src=None, sparse=True, max_atoms=256, max_bonds=256):
        from .raster import TargetRasterizer
        img = trainer.input_images
        B, S = img.shape[0], img.shape[2]
        if img.shape[3] != S:
            raise ValueError("SampleBuilder: the augmentation builds square S x S inputs, the %s takes %s" % (type(trainer).__name__, tuple(img.shape[2:]),))
        self.trainer = trainer
        self.short_batches = hasattr(trainer, "n_valid")      # (an evaluating InferenceRunner counts its first n_valid images)
        self.images = ImageBuilder(B, S, "train", amount, out=img, max_src=max_src)
        self.raster = TargetRasterizer(B, trainer.eng.h, trainer.eng.w, max_atoms=max_atoms, max_bonds=max_bonds, targets=trainer.targets,
                                       sparse=sparse)
        if sparse:
            trainer.use_sparse_targets(self.raster)
        self.B, self.S, self.h = B, S, trainer.eng.h

    def load(self, images_u8, atoms_strings, bonds_strings, rng):
        """one draw per image (draw_augment), its offsets to both halves; returns the draws"""
        from .raster import parse_graph, parse_record
        n = len(images_u8)
        if not (n == len(atoms_strings) == len(bonds_strings)) or not (n == self.B or (self.short_batches and 0 <= n < self.B)):
            raise ValueError("expected %s%d images and annotation pairs" % ("up to " if self.short_batches else "", self.B))
        # (an InferenceRunner(score_graphs=True) or (score_similarity=True): both read graph records)
        scored = getattr(self.trainer, "wants_graph_records", False)
        draws, records, graphs = [], [], []
        for img, a, q in zip(images_u8, atoms_strings, bonds_strings):
            dr, offs = draw_augment(rng, self.images.amount, np.shape(img), self.S)
            draws.append(dr)
            records.append(parse_record(a, q, *offs, h=self.h))
            if scored:
                graphs.append(parse_graph(a, q, *offs, h=self.h))
        if n < self.B:      # a white 1 x 1 source, copied without noise, and nothing to draw
            images_u8 = list(images_u8) + [np.full((1, 1), 255, dtype=np.uint8)] * (self.B - n)
            blank = AugmentDraw(1, 1, 0, 0, 1, 1, 0.0, 0.0, 0)
            empty = (np.zeros((0, 5), dtype=np.int32), np.zeros((0, 5), dtype=np.int32), np.zeros(0, dtype=np.float64))
            self.images.load(images_u8, draws + [blank] * (self.B - n))
            self.raster.load(records + [empty] * (self.B - n))
        else:
            self.images.load(images_u8, draws)
            self.raster.load(records)
        if scored:
            self.trainer.load_graphs(graphs)
        if self.short_batches:
            self.trainer.n_valid.fill_(n)
        return draws

    def run(self, stream=None):
        self.images.run(stream)
        self.raster.run(stream)
        return self.images.out
