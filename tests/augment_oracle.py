"""numpy restatement of the input-image half of utils.py:42-81 and utils_for_test.py:21-27 -- what csrc/augment.hip computes --
with the noise fields taken as arguments (the reference's np.random fields, or the device hash's through abcnet_amd.augment.noise_hash).

    resize_linear   cv2.resize(img_f32, (cols, rows), INTER_LINEAR): horizontal pass, then vertical, float32, every multiply and add
                    rounded on its own, edge taps clamped with weight (1, 0)
    ink_train       the resize (only when the shape changes), the white S x S canvas, (canvas / 255) < 0.6 in float32
    compose         (ink | salt) & ~pepper as f32 -- utils.py:73-81's logical_or / 1 - logical_or(1 - img, pepper)
"""
import numpy as np


def _taps(n_dst, n_src):
    scale = n_src / float(n_dst)
    fx = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    lo = sx < 0
    sx[lo], fx[lo] = 0, np.float32(0)
    hi = sx >= n_src - 1
    sx[hi], fx[hi] = n_src - 1, np.float32(0)
    return sx, np.minimum(sx + 1, n_src - 1), fx


def resize_linear(img, rows, cols):
    """OpenCV INTER_LINEAR of a float32 image to rows x cols (cv2.resize(img, (cols, rows)))"""
    img = np.asarray(img, dtype=np.float32)
    H, W = img.shape
    s0, s1, fx = _taps(cols, W)
    one = np.float32(1)
    r = img[:, s0] * (one - fx) + img[:, s1] * fx               # float32 ops: each rounded on its own
    t0, t1, fy = _taps(rows, H)
    fy = fy[:, None]
    return (r[t0] * (one - fy) + r[t1] * fy).astype(np.float32)


def ink_train(src_u8, S, rows, cols, ddx, ddy):
    """bool [S, S]: resize (when the shape changes), pad onto the white canvas, threshold"""
    img = np.asarray(src_u8).astype(np.float32)
    if img.shape != (rows, cols):
        img = resize_linear(img, rows, cols)
    canvas = np.full((S, S), 255, dtype=np.float32)
    canvas[ddx:ddx + rows, ddy:ddy + cols] = img
    return threshold(canvas)


def threshold(v):
    """utils.py:63: (img / 255) < 0.6 on float32 -- numpy's float32 division and compare"""
    return (np.asarray(v, dtype=np.float32) / np.float32(255)) < np.float32(0.6)


def compose(ink, salt, pepper):
    return ((ink | salt) & ~pepper).astype(np.float32)


def hash_fields(key, S, salt_thr, pepper_thr):
    """the device's salt / pepper fields: h(key, 2p) < salt_thr, h(key, 2p + 1) < pepper_thr over the pixels p of an S x S image"""
    from abcnet_amd.augment import noise_hash
    p = np.arange(S * S, dtype=np.uint64)
    salt = noise_hash(2 * p, key) < np.uint32(salt_thr) if salt_thr else np.zeros(S * S, bool)
    pepper = noise_hash(2 * p + 1, key) < np.uint32(pepper_thr) if pepper_thr else np.zeros(S * S, bool)
    return salt.reshape(S, S), pepper.reshape(S, S)


def build_train(src_u8, S, draw):
    """the device kernel's output for one image and its AugmentDraw (noise from the hash mirror)"""
    from abcnet_amd.augment import noise_threshold
    ink = ink_train(src_u8, S, draw.rows, draw.cols, draw.ddx, draw.ddy)
    salt, pepper = hash_fields(draw.key, S, noise_threshold(draw.salt), noise_threshold(draw.pepper))
    return compose(ink, salt, pepper)


def build_test(src_u8):
    """utils_for_test.py:21-27: 1 - ((u8 / 255).astype(f32) > 0.2)"""
    return (1 - ((np.asarray(src_u8) / 255).astype("float32") > 0.2)).astype(np.float32)


def fixture_render(seed, h, w):
    """a seeded grey-level 'render': white paper, dark antialiased strokes and discs, grey levels around every threshold"""
    rs = np.random.RandomState(seed)
    img = np.full((h, w), 255.0)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(12):
        y0, x0, y1, x1 = rs.uniform(0, h), rs.uniform(0, w), rs.uniform(0, h), rs.uniform(0, w)
        dy, dx = y1 - y0, x1 - x0
        L2 = dy * dy + dx * dx + 1e-9
        t = np.clip(((yy - y0) * dy + (xx - x0) * dx) / L2, 0, 1)
        d = np.hypot(yy - (y0 + t * dy), xx - (x0 + t * dx))
        img = np.minimum(img, np.clip((d - rs.uniform(0.5, 2.5)) * 128, 0, 255) + rs.uniform(0, 40))
    for _ in range(6):
        cy, cx, r = rs.uniform(0, h), rs.uniform(0, w), rs.uniform(2, 9)
        img = np.minimum(img, np.clip((np.hypot(yy - cy, xx - cx) - r) * 90, 0, 255))
    img[rs.uniform(size=(h, w)) < 0.002] = 153        # exactly the train threshold's neighbourhood
    img[rs.uniform(size=(h, w)) < 0.002] = 152
    img[rs.uniform(size=(h, w)) < 0.002] = 51         # and the test one's
    img[rs.uniform(size=(h, w)) < 0.002] = 52
    return np.round(img).astype(np.uint8)
