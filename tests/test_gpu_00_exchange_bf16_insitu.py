"""The bf16 gradient exchange in situ (Trainer(exchange="direct", exchange_dtype="bf16")): ONE fresh child
process (tests/exchange_bf16_worker.py: RCCL, world 1, the exchange forced on, hipGraph replays included) whose results this
process only reads -- it starts nothing else on the GPU, and nothing at all when the child ended with a fault, an abort or at its
time limit.  Sorts right after test_gpu_00_dataparallel.py: like that file it never touches the GPU itself."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import distributed as D  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def insitu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("exchange_bf16") / "res.json")
    codes = D.launch_ranks([os.path.join(HERE, "exchange_bf16_worker.py"), out], 1, timeout=600, env=dict(os.environ), rank0_stdout=sys.stderr)
    assert codes == [0], "exchange_bf16_worker.py: exit codes %s" % codes
    with open(out) as f:
        return json.load(f)


def test_bf16_exchange_leaves_the_rounded_gradients_of_the_plain_step(insitu):
    r = insitu
    print("bf16 exchange in situ:", r, file=sys.stderr)
    assert r["backend"] == "nccl" and r["plain"]["segments"] == 1
    b = r["direct_bf16"]
    # it really ran: several buckets between graph segments, nothing fell back
    assert (b["mode"], b["wire_dtype"], b["fallback"]) == ("direct", "bf16", None), b
    assert b["buckets"] >= 3 and b["segments"] >= 3 and b["graphs"], b
    assert b["segments"] == r["direct_f32"]["segments"] and b["buckets"] == r["direct_f32"]["buckets"]
    # the whole padded store == bf16_rne(plain), bit for bit; the gradients are there and the rounding did change them
    assert r["nonzero"] > r["store_elems"] // 2 and b["nan"] == 0
    assert b["changed_by_rounding"] > r["store_elems"] // 4
    assert b["equals_rounded_plain"] and b["differing"] == 0, b
    # one rank sends nothing; two would send half of every bucket on each leg at 2 bytes per element
    assert b["wire_bytes_per_step"] == 0 and b["wire_bytes_w2"] == 2 * r["store_elems"]
    assert r["direct_f32"]["wire_bytes_w2"] == 4 * r["store_elems"]


def test_f32_direct_exchange_still_equals_plain(insitu):
    f = insitu["direct_f32"]
    assert (f["mode"], f["wire_dtype"], f["fallback"]) == ("direct", "f32", None), f
    assert f["equals_plain"] and f["graphs"] and f["segments"] >= 3
