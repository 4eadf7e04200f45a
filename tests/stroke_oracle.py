"""numpy transcription of the stroke contract (include/abcnet_hip.h, abc_stroke_desc): despeckle, Guo-Hall
thinning in two subiterations, dilation by a disk, the stats row.  Written from the rules, per pixel: every neighbour is an
integer 0 / 1 array the size of the image, C, N1 and N2 are integer sums and N their minimum -- nothing is packed into words and
no count is turned into Boolean algebra, which is what the kernel does."""
import numpy as np

UNTIL_STABLE = -1
STATS = ("iterations", "converged", "ink_in", "ink_out", "skipped")


def _neighbours(a):
    """(p2 .. p9) of every pixel, clockwise from north, paper outside the canvas; int64 arrays of 0 / 1"""
    h, w = a.shape
    p = np.zeros((h + 2, w + 2), dtype=np.int64)
    p[1:-1, 1:-1] = a

    def at(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1)


def despeckle(a):
    """every ink pixel without ink among its eight neighbours deleted, all at once"""
    a = np.asarray(a).astype(bool)
    return a & (sum(_neighbours(a)) > 0)


def _subiteration(a, second):
    p2, p3, p4, p5, p6, p7, p8, p9 = _neighbours(a)
    n = 1 - np.stack([p2, p3, p4, p5, p6, p7, p8, p9])          # the negations, as integers
    n2, n4, n5, n6, n8, n9 = n[0], n[2], n[3], n[4], n[6], n[7]
    C = n2 * np.maximum(p3, p4) + n4 * np.maximum(p5, p6) + n6 * np.maximum(p7, p8) + n8 * np.maximum(p9, p2)
    N1 = np.maximum(p9, p2) + np.maximum(p3, p4) + np.maximum(p5, p6) + np.maximum(p7, p8)
    N2 = np.maximum(p2, p3) + np.maximum(p4, p5) + np.maximum(p6, p7) + np.maximum(p8, p9)
    N = np.minimum(N1, N2)
    if second:
        m = np.maximum(np.maximum(p2, p3), n5) * p4
    else:
        m = np.maximum(np.maximum(p6, p7), n9) * p8
    delete = a & (C == 1) & (N >= 2) & (N <= 3) & (m == 0)
    return a & ~delete, bool(delete.any())


def thin(a, max_iter):
    """(image, iterations, converged); max_iter 0: none, k >= 1: at most k iterations, UNTIL_STABLE: until an iteration deletes
    nothing (that iteration is counted)"""
    a = np.asarray(a).astype(bool)
    iterations, converged = 0, 0
    while max_iter != 0:
        a, d1 = _subiteration(a, False)
        a, d2 = _subiteration(a, True)
        iterations += 1
        if not (d1 or d2):
            converged = 1
            break
        if max_iter > 0 and iterations >= max_iter:
            break
    return a, iterations, converged


def disk(r):
    """the offsets (dy, dx) with dy^2 + dx^2 <= r^2"""
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r]


def dilate(a, r):
    a = np.asarray(a).astype(bool)
    h, w = a.shape
    out = np.zeros_like(a)
    ys, xs = np.nonzero(a)
    for dy, dx in disk(r):
        y, x = ys + dy, xs + dx
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        out[y[ok], x[ok]] = True
    return out


def max_iter_of(thin_arg):
    """the `thin` argument of the Python surface as a max_iter"""
    if thin_arg is None:
        return 0
    return UNTIL_STABLE if thin_arg == "stable" else int(thin_arg)


def normalize(a, thin_arg=None, radius=0, drop_isolated=False):
    """(f32 image of 0 / 1, stats row as a dict) of one f32 image: ink iff > 0.5"""
    with np.errstate(invalid="ignore"):
        ink = np.asarray(a) > 0.5
    cur = despeckle(ink) if drop_isolated else ink
    cur, iterations, converged = thin(cur, max_iter_of(thin_arg))
    cur = dilate(cur, radius)
    stats = dict(iterations=iterations, converged=converged, ink_in=int(ink.sum()), ink_out=int(cur.sum()), skipped=0)
    return cur.astype(np.float32), stats


def stats_row(s):
    return [s[k] for k in STATS]


# ---------------------------------------------------------------------------------------------------- drawings for the tests
def stroke(a, y0, x0, y1, x1, width):
    """a straight stroke `width` pixels wide (a width x width square stamped along the line), clipped at the canvas"""
    h, w = a.shape
    n = max(abs(y1 - y0), abs(x1 - x0), 1)
    lo = (width - 1) // 2
    for k in range(n + 1):
        y = y0 + (y1 - y0) * k // n - lo
        x = x0 + (x1 - x0) * k // n - lo
        a[max(y, 0):max(y + width, 0), max(x, 0):max(x + width, 0)] = True
    return a


def drawing(seed, S, strokes=5, forced=True, widest=7):
    """a seeded bool [S, S] drawing of straight strokes 1 .. widest pixels wide.  forced: strokes across the word seams that exist
    (columns 31 / 32 and 63 / 64), and along the first and the last row and column"""
    rs = np.random.RandomState(seed)
    a = np.zeros((S, S), dtype=bool)
    for _ in range(strokes):
        y0, x0, y1, x1 = (int(v) for v in rs.randint(0, S, size=4))
        stroke(a, y0, x0, y1, x1, int(rs.randint(1, widest + 1)))
    if forced:
        for seam in (32, 64):
            if seam < S:      # a slanted stroke over the seam, and a vertical one that straddles it
                y = int(rs.randint(0, S))
                stroke(a, y, max(seam - 9, 0), min(y + 5, S - 1), min(seam + 9, S - 1), int(rs.randint(1, 8)))
                stroke(a, int(rs.randint(0, S // 2)), seam, int(rs.randint(S // 2, S)), seam, int(rs.randint(2, 6)))
        k = int(rs.randint(1, 4))
        stroke(a, 0, int(rs.randint(0, S // 2)), 0, S - 1, k)                    # the first row
        stroke(a, S - 1, 0, S - 1, int(rs.randint(S // 2, S)), k)                # the last row
        stroke(a, int(rs.randint(0, S // 2)), 0, S - 1, 0, int(rs.randint(1, 4)))        # the first column
        stroke(a, 0, S - 1, int(rs.randint(S // 2, S)), S - 1, int(rs.randint(1, 4)))    # the last column
    return a
