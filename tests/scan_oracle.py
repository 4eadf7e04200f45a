"""numpy transcription of the scan contract (include/abcnet_hip.h, abc_scan_desc): histogram, Otsu
threshold, polarity, bounding box, fit, coverage resample, geometry row.  Written from the rules, not from the kernels: plain
loops over destination pixels, Python integers for everything that must be exact."""
import numpy as np

DARK, LIGHT, AUTO = 0, 1, 2
CONSTANT, BAD_PARAMS = 1, 2
GEOM = ("thr", "inverted", "status", "y0", "x0", "bh", "bw", "rows", "cols", "ddx", "ddy", "ink")


def histogram(img):
    return np.bincount(np.asarray(img, dtype=np.uint8).ravel(), minlength=256).astype(np.int64)


def sigmas(hist):
    """(sigma[256] float64 with -1 where t is not admissible, w0[256] as Python ints)"""
    h = [int(v) for v in hist]
    N = sum(h)
    S = sum(v * c for v, c in enumerate(h))
    out = np.full(256, -1.0, dtype=np.float64)
    w0s, w0, s0 = [], 0, 0
    for t in range(256):
        w0 += h[t]
        s0 += t * h[t]
        w0s.append(w0)
        w1 = N - w0
        if w0 > 0 and w1 > 0:
            d = S * w0 - N * s0
            assert abs(d) < 2 ** 56
            x = np.float64(d)                      # (one rounding of the exact integer, as a C cast)
            out[t] = (x * x) / (np.float64(w0) * np.float64(w1))
    return out, w0s


def threshold(hist):
    """the smallest admissible t with maximal sigma, None for a single-valued image"""
    s, _ = sigmas(hist)
    if s.max() < 0:
        return None
    best = s.max()
    return min(t for t in range(256) if s[t] == best)


def fit(bh, bw, S, margin):
    lim = S - 2 * margin
    m = max(bh, bw)
    if m <= lim:
        rows, cols = bh, bw
    else:
        rows, cols = max(1, (bh * lim) // m), max(1, (bw * lim) // m)
    return rows, cols, (S - rows) // 2, (S - cols) // 2


def build(img, S, margin, cover_q8, polarity):
    """(out f32 [S, S], geometry row as a dict of ints) of one source"""
    img = np.asarray(img, dtype=np.uint8)
    out = np.zeros((S, S), dtype=np.float32)
    g = dict.fromkeys(GEOM, 0)
    h = histogram(img)
    thr = threshold(h)
    if thr is None:
        g["thr"], g["status"] = -1, CONSTANT
        return out, g
    N = int(h.sum())
    w0 = int(h[:thr + 1].sum())
    inv = polarity == LIGHT or (polarity == AUTO and 2 * w0 > N)
    ink = (img > thr) if inv else (img <= thr)
    ys, xs = np.nonzero(ink)
    y0, y1, x0, x1 = int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())
    bh, bw = y1 - y0 + 1, x1 - x0 + 1
    rows, cols, ddx, ddy = fit(bh, bw, S, margin)
    # ink counts of boxes through a summed-area table (exact integers)
    sat = np.zeros((bh + 1, bw + 1), dtype=np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(ink[y0:y1 + 1, x0:x1 + 1].astype(np.int64), 0), 1)
    for r in range(rows):
        ra, rb = (r * bh) // rows, -((-(r + 1) * bh) // rows)          # [ra, rb): floor and ceil
        for c in range(cols):
            ca, cb = (c * bw) // cols, -((-(c + 1) * bw) // cols)
            assert 0 <= ra < rb <= bh and 0 <= ca < cb <= bw
            n = int(sat[rb, cb] - sat[ra, cb] - sat[rb, ca] + sat[ra, ca])
            a = (rb - ra) * (cb - ca)
            if n >= 1 and n * 256 >= cover_q8 * a:
                out[ddx + r, ddy + c] = 1.0
    g.update(thr=thr, inverted=int(inv), status=0, y0=y0, x0=x0, bh=bh, bw=bw, rows=rows, cols=cols, ddx=ddx, ddy=ddy,
             ink=int(ink.sum()))
    return out, g


def geom_row(g):
    return [g[k] for k in GEOM]
