"""numpy / Python transcription of the cell component filter's contract (include/abcnet_hip.h, abc_scan_clean_desc; DESIGN.md
section 7): cells, their 8-connected components by a flood fill, weights, the keep rule, the masked box and resample, the
geometry row, the stats row and the two debug slices.  Written from the rules, not from the kernels (no union-find here); the
threshold and the fit are scan_oracle's."""
import numpy as np

import scan_oracle as so

NO_COMPONENT, CLEAN_FAILED = 4, 8
STATS = ("components", "kept", "ink_kept", "ink_dropped", "heaviest", "occupied_cells")
CELLS = (8, 16, 32, 64)


def cdiv(a, b):
    return -(-a // b)


def cell_ink(ink, cell):
    """ink pixels per cell of the image's own grid, int64 [ceil(h / cell), ceil(w / cell)]"""
    h, w = ink.shape
    ch, cw = cdiv(h, cell), cdiv(w, cell)
    pad = np.zeros((ch * cell, cw * cell), dtype=np.int64)
    pad[:h, :w] = ink
    return pad.reshape(ch, cell, cw, cell).sum(axis=(1, 3))


def partition(occupied):
    """8-connected components of a boolean grid by a flood fill: int array of the same shape, -1 where unoccupied, else the
    smallest row-major index (y * width + x) of the cell's component"""
    occupied = np.asarray(occupied, dtype=bool)
    h, w = occupied.shape
    lab = np.full((h, w), -1, dtype=np.int64)
    for y in range(h):
        for x in range(w):
            if not occupied[y, x] or lab[y, x] >= 0:
                continue
            first = y * w + x                                  # row-major order: the first cell met is the smallest
            lab[y, x] = first
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for ny in range(max(cy - 1, 0), min(cy + 2, h)):
                    for nx in range(max(cx - 1, 0), min(cx + 2, w)):
                        if occupied[ny, nx] and lab[ny, nx] < 0:
                            lab[ny, nx] = first
                            stack.append((ny, nx))
    return lab


def build(img, S, margin, cover_q8, polarity, cell, min_ink, keep_q8, cap):
    """one source -> (out f32 [S, S], geometry dict, stats dict, labels int32 [cap_ch, cap_cw], keep uint8 [cap_ch, cap_cw]);
    cap = (src_max_h, src_pitch), the capacities that fix cap_ch, cap_cw and the labels"""
    assert cell in CELLS and min_ink >= 0 and 0 <= keep_q8 <= 256
    img = np.asarray(img, dtype=np.uint8)
    cap_ch, cap_cw = cdiv(cap[0], cell), cdiv(cap[1], cell)
    out = np.zeros((S, S), dtype=np.float32)
    g = dict.fromkeys(so.GEOM, 0)
    st = dict.fromkeys(STATS, 0)
    labels = np.full((cap_ch, cap_cw), -1, dtype=np.int32)
    keep = np.zeros((cap_ch, cap_cw), dtype=np.uint8)
    h = so.histogram(img)
    thr = so.threshold(h)
    if thr is None:
        g["thr"], g["status"] = -1, so.CONSTANT
        return out, g, st, labels, keep
    N = int(h.sum())
    w0 = int(h[:thr + 1].sum())
    inv = polarity == so.LIGHT or (polarity == so.AUTO and 2 * w0 > N)
    ink = (img > thr) if inv else (img <= thr)
    total = int(ink.sum())
    # cells on the capacity grid (cells outside the image's own grid hold no ink), components, weights
    cells = np.zeros((cap_ch, cap_cw), dtype=np.int64)
    own = cell_ink(ink, cell)
    cells[:own.shape[0], :own.shape[1]] = own
    lab = partition(cells > 0)
    weight = {}
    for cy, cx in zip(*np.nonzero(cells)):
        weight[int(lab[cy, cx])] = weight.get(int(lab[cy, cx]), 0) + int(cells[cy, cx])
    H = max(weight.values())
    kept = {k for k, w in weight.items() if w >= min_ink and 256 * w >= keep_q8 * H}
    labels[:] = lab
    for cy, cx in zip(*np.nonzero(cells)):
        keep[cy, cx] = int(lab[cy, cx]) in kept
    ink_kept = sum(weight[k] for k in kept)
    st.update(components=len(weight), kept=len(kept), ink_kept=ink_kept, ink_dropped=total - ink_kept, heaviest=H,
              occupied_cells=int((cells > 0).sum()))
    g.update(thr=thr, inverted=int(inv), ink=total)
    if not kept:
        assert min_ink > H
        g["status"] = NO_COMPONENT
        return out, g, st, labels, keep
    # the ink of kept cells, pixel by pixel
    ih, iw = ink.shape
    pix_keep = np.kron(keep, np.ones((cell, cell), dtype=np.uint8))[:ih, :iw].astype(bool)
    kink = ink & pix_keep
    assert int(kink.sum()) == ink_kept
    ys, xs = np.nonzero(kink)
    y0, y1, x0, x1 = int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())
    bh, bw = y1 - y0 + 1, x1 - x0 + 1
    rows, cols, ddx, ddy = so.fit(bh, bw, S, margin)
    sat = np.zeros((bh + 1, bw + 1), dtype=np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(kink[y0:y1 + 1, x0:x1 + 1].astype(np.int64), 0), 1)
    for r in range(rows):
        ra, rb = (r * bh) // rows, -((-(r + 1) * bh) // rows)
        for c in range(cols):
            ca, cb = (c * bw) // cols, -((-(c + 1) * bw) // cols)
            n = int(sat[rb, cb] - sat[ra, cb] - sat[rb, ca] + sat[ra, ca])
            a = (rb - ra) * (cb - ca)
            if n >= 1 and n * 256 >= cover_q8 * a:
                out[ddx + r, ddy + c] = 1.0
    g.update(status=0, y0=y0, x0=x0, bh=bh, bw=bw, rows=rows, cols=cols, ddx=ddx, ddy=ddy)
    return out, g, st, labels, keep


def stats_row(st):
    return [st[k] for k in STATS]
