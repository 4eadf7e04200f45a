"""numpy / Python transcription of the page splitter's contract (include/abcnet_hip.h, abc_scan_split_desc):
cells, their groups by a flood fill under the reach rule, weights, the keep rule per page, the order by label, the packing into
canvases, and per canvas the masked box, fit and resample, the geometry row and the tables.  Written from the rules, not from
the kernels (no union-find, no scan, no atomics here); the histogram, the threshold and the fit are scan_oracle's, the cells
scan_clean_oracle's."""
import numpy as np

import scan_clean_oracle as co
import scan_oracle as so

PAGE_FULL, BATCH_FULL = 16, 32
PAGE = ("status", "groups", "kept", "first", "taken", "ink_kept", "ink_dropped", "occupied_cells")
DRAWING = ("page", "label", "weight", "rank_in_page")
BAD = None                    # a page given as None stands for one whose src_h / src_w leaves its slot (BAD_PARAMS)


def partition(occupied, reach):
    """groups of a boolean grid by a flood fill: two occupied cells within Chebyshev distance `reach` belong together.  int array
    of the same shape, -1 where unoccupied, else the smallest row-major index (y * width + x) of the cell's group"""
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
                ya, yb, xa, xb = max(cy - reach, 0), min(cy + reach + 1, h), max(cx - reach, 0), min(cx + reach + 1, w)
                ny, nx = np.nonzero(occupied[ya:yb, xa:xb] & (lab[ya:yb, xa:xb] < 0))
                for j, i in zip(ny + ya, nx + xa):
                    lab[j, i] = first
                    stack.append((int(j), int(i)))
    return lab


def brute_partition(occupied, reach):
    """the same partition as the transitive closure of the relation itself: a boolean matrix over the occupied cells, squared
    until it stops growing (for the host test of partition on small grids)"""
    occupied = np.asarray(occupied, dtype=bool)
    h, w = occupied.shape
    ys, xs = np.nonzero(occupied)
    lab = np.full((h, w), -1, dtype=np.int64)
    if not len(ys):
        return lab
    rel = np.maximum(np.abs(ys[:, None] - ys[None, :]), np.abs(xs[:, None] - xs[None, :])) <= reach
    while True:
        nxt = (rel.astype(np.int64) @ rel.astype(np.int64)) > 0
        if np.array_equal(nxt, rel):
            break
        rel = nxt
    idx = ys * w + xs
    for k in range(len(ys)):
        lab[ys[k], xs[k]] = idx[rel[k]].min()
    return lab


def _canvas(ink, mine, S, margin, cover_q8):
    """(out [S, S], y0, x0, bh, bw, rows, cols, ddx, ddy) of the ink pixels `mine` (a subset of `ink`): box over mine, n over mine"""
    out = np.zeros((S, S), dtype=np.float32)
    ys, xs = np.nonzero(mine)
    y0, y1, x0, x1 = int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())
    bh, bw = y1 - y0 + 1, x1 - x0 + 1
    rows, cols, ddx, ddy = so.fit(bh, bw, S, margin)
    sat = np.zeros((bh + 1, bw + 1), dtype=np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(mine[y0:y1 + 1, x0:x1 + 1].astype(np.int64), 0), 1)
    for r in range(rows):
        ra, rb = (r * bh) // rows, -((-(r + 1) * bh) // rows)
        for c in range(cols):
            ca, cb = (c * bw) // cols, -((-(c + 1) * bw) // cols)
            n = int(sat[rb, cb] - sat[ra, cb] - sat[rb, ca] + sat[ra, ca])
            a = (rb - ra) * (cb - ca)
            if n >= 1 and n * 256 >= cover_q8 * a:
                out[ddx + r, ddy + c] = 1.0
    return out, (y0, x0, bh, bw, rows, cols, ddx, ddy)


def analyse(img, polarity, cell, reach, cap):
    """one page -> None for a CONSTANT page, else (thr, inv, ink bool [h, w], cells int64 [cap_ch, cap_cw], lab, weight dict)"""
    img = np.asarray(img, dtype=np.uint8)
    cap_ch, cap_cw = co.cdiv(cap[0], cell), co.cdiv(cap[1], cell)
    h = so.histogram(img)
    thr = so.threshold(h)
    if thr is None:
        return None
    N = int(h.sum())
    w0 = int(h[:thr + 1].sum())
    inv = polarity == so.LIGHT or (polarity == so.AUTO and 2 * w0 > N)
    ink = (img > thr) if inv else (img <= thr)
    cells = np.zeros((cap_ch, cap_cw), dtype=np.int64)
    own = co.cell_ink(ink, cell)
    cells[:own.shape[0], :own.shape[1]] = own
    lab = partition(cells > 0, reach)
    weight = {}
    for cy, cx in zip(*np.nonzero(cells)):
        weight[int(lab[cy, cx])] = weight.get(int(lab[cy, cx]), 0) + int(cells[cy, cx])
    return thr, int(inv), ink, cells, lab, weight


def split(pages, D, K, S, margin, cover_q8, polarity, cell, reach, min_ink, keep_q8, cap):
    """a batch of pages (2-d uint8 arrays, BAD for a page with bad params) -> dict of out f32 [D, S, S], geom int [D, 12], pages
    int [P, 8], drawings int [D, 4], total [2], labels and canvas int [P, cap_ch, cap_cw]; cap = (src_max_h, src_pitch)"""
    assert cell in co.CELLS and 1 <= reach <= 4 and 1 <= K <= 64 and D >= 1 and min_ink >= 0 and 0 <= keep_q8 <= 256
    P = len(pages)
    cap_ch, cap_cw = co.cdiv(cap[0], cell), co.cdiv(cap[1], cell)
    out = np.zeros((D, S, S), dtype=np.float32)
    geom = np.zeros((D, len(so.GEOM)), dtype=np.int64)
    geom[:, so.GEOM.index("thr")] = -1
    geom[:, so.GEOM.index("status")] = co.NO_COMPONENT
    rows = np.zeros((P, len(PAGE)), dtype=np.int64)
    drawings = np.tile(np.array([-1, -1, 0, -1], dtype=np.int64), (D, 1))
    labels = np.full((P, cap_ch, cap_cw), -1, dtype=np.int64)
    canvas = np.full((P, cap_ch, cap_cw), -1, dtype=np.int64)
    nxt, true_count = 0, 0
    for p, img in enumerate(pages):
        r = dict.fromkeys(PAGE, 0)
        r["first"] = nxt
        if img is BAD:
            r["status"] = so.BAD_PARAMS
        else:
            a = analyse(img, polarity, cell, reach, cap)
            if a is None:
                r["status"] = so.CONSTANT
            else:
                thr, inv, ink, cells, lab, weight = a
                labels[p] = lab
                H = max(weight.values())
                kept = sorted(k for k, w in weight.items() if w >= min_ink and 256 * w >= keep_q8 * H)
                ink_kept = sum(weight[k] for k in kept)
                r.update(groups=len(weight), kept=len(kept), ink_kept=ink_kept, ink_dropped=int(ink.sum()) - ink_kept,
                         occupied_cells=int((cells > 0).sum()))
                true_count += len(kept)
                if not kept:
                    assert min_ink > H
                    r["status"] |= co.NO_COMPONENT
                if len(kept) > K:
                    r["status"] |= PAGE_FULL
                    kept = kept[:K]
                if nxt + len(kept) > D:
                    r["status"] |= BATCH_FULL
                    kept = kept[:D - nxt]
                r["taken"] = len(kept)
                ih, iw = ink.shape
                for rank, k in enumerate(kept):
                    j = nxt + rank
                    member = lab == k
                    canvas[p][member] = j
                    mine = ink & np.kron(member, np.ones((cell, cell), dtype=bool))[:ih, :iw]
                    assert int(mine.sum()) == weight[k]
                    out[j], box = _canvas(ink, mine, S, margin, cover_q8)
                    geom[j] = [thr, inv, 0] + list(box) + [weight[k]]
                    drawings[j] = [p, k, weight[k], rank]
                nxt += len(kept)
        rows[p] = [r[c] for c in PAGE]
    return dict(out=out, geom=geom, pages=rows, drawings=drawings, total=np.array([nxt, true_count], dtype=np.int64),
                labels=labels, canvas=canvas)


def erase_outside(img, member, cell, paper):
    """the page with every cell outside the boolean cell grid `member` painted as paper (for the comparison with the plain builder)"""
    img = np.asarray(img, dtype=np.uint8).copy()
    h, w = img.shape
    inside = np.kron(np.asarray(member, dtype=bool), np.ones((cell, cell), dtype=bool))[:h, :w]
    img[~inside] = paper
    return img
