"""Goldens of the input-image half of the reference's loaders (needs the reference checkout: it reads the reference's
text; what it writes travels, the reference does not).

  augment_512.npz       utils.py:42-81 (MolecularImageDataset.__getitem__ from the imread to img[0] = ...) executed from the
                        reference text on seeded fixture renders: `cv2.imread` returns the fixture, `resize` is the oracle's
                        INTER_LINEAR restatement (OpenCV is not a dependency), `np.random` a seeded RandomState whose draws are
                        recorded.  Cases: row resize, column resize, no resize, a source smaller than 512 with and without a
                        resize, each with amount 0 and 0.2.  Stored per case: seed, amount, source, scalar draws, the resized shape
                        and offsets, the salt / pepper masks the fields gave and the output, bit-packed.
  augment_test_512.npz  utils_for_test.py:21-27 on seeded 512 x 512 fixtures: source and bit-packed output.

    python tests/golden/make_golden_augment.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import augment_oracle as ao  # noqa: E402
from make_golden import REF, slice_text  # noqa: E402

S = 512
# (tag, source shape, branch): branch = which way the first two rand() calls go
BRANCHES = [("row", (512, 512), "row"), ("col", (512, 512), "col"), ("none", (512, 512), "none"),
            ("small", (400, 460), "none"), ("small_row", (300, 450), "row")]
AMOUNTS = [0.0, 0.2]


class RecordingRandom:
    """np.random for the slice: a seeded RandomState whose scalar draws and fields are recorded"""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.scalars, self.fields = [], []

    def rand(self):
        v = self.rs.rand()
        self.scalars.append(v)
        return v

    def uniform(self, low=0.0, high=1.0, size=None):
        v = self.rs.uniform(low, high, size)
        (self.scalars if size is None else self.fields).append(v)
        return v


def branch_of(seed):
    rs = np.random.RandomState(seed)
    r1, r2 = rs.rand(), rs.rand()
    return "none" if r1 >= 0.2 else ("row" if r2 < 0.5 else "col")


def run_train_slice(src, seed, amount):
    rec = RecordingRandom(seed)
    npx = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    npx.random = rec
    sizes = []

    def resize(img, dsize):                     # cv2.resize(img, (width, height))
        sizes.append((dsize[1], dsize[0]))
        return ao.resize_linear(img, dsize[1], dsize[0])

    this = types.SimpleNamespace(amount=amount)
    ns = {"np": npx, "cv2": types.SimpleNamespace(imread=lambda path, flags=0: src.copy()), "resize": resize, "path": "fixture",
          "self": this}
    exec(slice_text(os.path.join(REF, "utils.py"), 42, 81), ns)
    rows, cols = sizes[0] if sizes else src.shape
    salt = rec.fields[0] < rec.scalars[-2]
    pepper = rec.fields[1] < rec.scalars[-1]
    return ns, rec, (rows, cols), salt, pepper


def train_goldens():
    res = {}
    ci = 0
    for tag, shape, branch in BRANCHES:
        for amount in AMOUNTS:
            seed = 1000 + 97 * ci
            while branch_of(seed) != branch:
                seed += 1
            src = ao.fixture_render(50 + ci, *shape)
            ns, rec, (rows, cols), salt, pepper = run_train_slice(src, seed, amount)
            out = ns["img"]
            assert out.shape == (1, S, S) and out.dtype == np.float32 and set(np.unique(out)) <= {0.0, 1.0}
            p = "c%d_" % ci
            res[p + "tag"] = np.array(tag)
            res[p + "seed"] = np.array(seed)
            res[p + "amount"] = np.array(amount)
            res[p + "src"] = src
            res[p + "scalars"] = np.array(rec.scalars, dtype=np.float64)
            res[p + "geom"] = np.array([rows, cols, ns["ddx"], ns["ddy"]], dtype=np.int64)
            res[p + "scale"] = np.array([ns["scale_x"], ns["scale_y"]], dtype=np.float64)
            res[p + "salt"] = np.packbits(salt)
            res[p + "pepper"] = np.packbits(pepper)
            res[p + "out"] = np.packbits(out[0].astype(np.uint8))
            print("train case", ci, tag, amount, "seed", seed, "rows x cols", rows, cols, "ink", int(out.sum()))
            ci += 1
    res["n"] = np.array(ci)
    np.savez_compressed(os.path.join(HERE, "augment_512.npz"), **res)


def test_goldens():
    res = {}
    for ci in range(3):
        src = ao.fixture_render(300 + ci, S, S)
        ns = {"np": np, "cv2": types.SimpleNamespace(imread=lambda path, flags=0, _s=src: _s.copy()), "path": "fixture"}
        exec(slice_text(os.path.join(REF, "utils_for_test.py"), 21, 27), ns)
        out = ns["img"]
        assert out.shape == (1, S, S) and out.dtype == np.float32
        res["c%d_src" % ci] = src
        res["c%d_out" % ci] = np.packbits(out[0].astype(np.uint8))
    res["n"] = np.array(3)
    np.savez_compressed(os.path.join(HERE, "augment_test_512.npz"), **res)
    print("test cases", 3)


if __name__ == "__main__":
    train_goldens()
    test_goldens()
