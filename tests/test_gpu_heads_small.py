"""The fused heads pass (abc_heads_fused_fwd_bwd) held to byte equality with tests/golden/heads_small.npz: everything it wrote for
the same seeded inputs BEFORE the five one-tile heads left the seven-way kernel for a kernel of their own (heads_small_kernel,
profiles/r25_heads_small.md).  The new path reorders loads and runs the data gradient in channel halves, but keeps the K order of
every MFMA chain, the wave -> pixel mapping and the order of every sum across waves, so the logits, the loss sums, the BatchNorm
sums, g, d(logits), the in-pass weight-gradient partials, the tile mask and the keep bits may not change by a bit.

Cases, inputs and the runner live in profiles/tools/heads_small_golden.py (which also wrote the fixture): one chunk, chunks across
an image boundary, many chunks; dropout off / on; dense targets, none (every wave skips), one pixel (one wave of one chunk fires);
logits stored / NULL; no_zero_skip 0 / 1.  An array above 2 KiB is compared by its SHA-256.  What the values themselves should be
is held by test_gpu_heads_fused.py and test_gpu_heads_zero_skip.py against torch and the oracle.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("heads_small_golden", os.path.join(ROOT, "profiles", "tools", "heads_small_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

CASES = G.cases()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return L.load()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "heads_small.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_case_and_nothing_else(golden):
    want = set()
    for c in CASES:
        names = ["dl", "g", "bnpart", "losspart", "work", "keep", "dl_tiles"] + (["logits%d" % i for i in range(8)] if c["logits"] else [])
        want |= {"%s.%s" % (c["name"], n) for n in names}
    assert len(CASES) == 72 and set(golden) == want


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_heads_pass_bytes(lib, golden, c):
    got = G.run(lib, c)
    bad = []
    for k, t in got.items():
        key = "%s.%s" % (c["name"], k)
        a, b = G.as_bytes(t), golden[key]
        if a.shape != b.shape or not np.array_equal(a, b):
            nbytes = t.numel() * t.element_size()
            bad.append("%s (%d bytes%s)" % (k, nbytes, ", compared by SHA-256" if nbytes > G.DIGEST_ABOVE else ""))
    assert not bad, "%s differs from the fixture in: %s" % (c["name"], ", ".join(bad))


def test_the_cases_reach_the_skip_and_the_full_path(lib):
    """the target sets do what their names say, read back from what the pass wrote: with no target every loss sum and every small
    head's g is zero; with one pixel exactly one chunk has loss terms and only wave 1's 32 pixels of it have a non-zero g"""
    pick = lambda t: next(c for c in CASES if c["B"] == 2 and c["drop_p"] == 0.2 and c["targets"] == t and c["logits"] and not c["noskip"])
    z = G.run(lib, pick("zero"))
    # (bond types, rho and the softmax heads are exactly zero; the two centre heads and omega still have their background terms)
    assert not z["losspart"][:, [1, 2, 3, 5, 6]].any() and not z["g"][:, 128:512].any()
    o = G.run(lib, pick("one_wave"))
    g = o["g"][:, 128:512].float().view(-1, 32, 384)         # [32-pixel wave][pixel][channels of heads 1-3]
    fired = g.abs().sum((1, 2)) != 0
    assert fired.nonzero().flatten().tolist() == [1]
    assert (o["losspart"][:, [1, 2, 3]] != 0).any(1).nonzero().flatten().tolist() == [0]
