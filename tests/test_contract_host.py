"""CPU tier of abcnet_amd.contract and of the formatting helpers of abcnet_amd.ops: the 8-target contract (written out here a
second time, on purpose, in the collate order of the reference's utils.py), its one checker under every caller's exception class
and prefix, the head-map check, the meter and loss-term dictionaries, and the aliases other modules keep."""
import math

import pytest
import torch

import abcnet_amd  # noqa: F401
from abcnet_amd import _lib as L
from abcnet_amd import contract as K
from abcnet_amd import loss, ops

# (exc, what) as FusedLoss, loss._check, FusedMetrics, EvalTables and TargetRasterizer call check_targets
CALLERS = [(ValueError, "fused loss"), (ValueError, "abc_loss"), (L.AbcNetHipError, "metrics"), (L.AbcNetHipError, "EvalTables"),
           (L.AbcNetHipError, "raster")]
B, H, W = 2, 8, 12
SHAPES = [(2, 1, 8, 12), (2, 14, 8, 12), (2, 3, 8, 12), (2, 2, 8, 12), (2, 1, 8, 12), (2, 6, 60, 8, 12), (2, 60, 8, 12), (2, 60, 8, 12)]
DTYPES = [torch.float32] * 6 + [torch.float64] * 2


def _good():
    return [torch.zeros(s, dtype=dt) for s, dt in zip(SHAPES, DTYPES)]


def test_target_shapes_and_alloc():
    assert K.target_shapes(B, H, W) == SHAPES
    tg = K.alloc_targets(B, H, W, "cpu")
    assert [tuple(t.shape) for t in tg] == SHAPES and [t.dtype for t in tg] == DTYPES
    assert all(t.is_contiguous() and not t.any() for t in tg)


def _bad_inputs(i):
    """three wrong tensors for position i: one dimension off, the other float dtype, a non-contiguous view of the right shape"""
    s, dt = SHAPES[i], DTYPES[i]
    wrong_dim = torch.zeros(s[:-1] + (s[-1] + 1,), dtype=dt)
    other_dtype = torch.zeros(s, dtype=torch.float64 if dt == torch.float32 else torch.float32)
    view = torch.zeros(s[:-2] + (s[-1], s[-2]), dtype=dt).transpose(-1, -2)
    assert tuple(view.shape) == s and not view.is_contiguous()
    return {"wrong_dim": wrong_dim, "other_dtype": other_dtype, "non_contiguous": view}


@pytest.mark.parametrize("i", range(8))
def test_check_targets_refuses_every_position_under_every_callers_exception(i):
    for kind, bad in _bad_inputs(i).items():
        tg = _good()
        tg[i] = bad
        for exc, what in CALLERS:
            with pytest.raises(exc, match=r"%s: target %d " % (what, i)) as e:
                K.check_targets(tg, B, H, W, what, exc, require_cuda=False)
            assert type(e.value) is exc, kind
        # (abc_loss makes its targets contiguous itself: its call does not ask for that, and asks for everything else)
        if kind == "non_contiguous":
            K.check_targets(tg, B, H, W, "abc_loss", ValueError, require_cuda=False, require_contiguous=False)
        else:
            with pytest.raises(ValueError, match="target %d " % i):
                K.check_targets(tg, B, H, W, "abc_loss", ValueError, require_cuda=False, require_contiguous=False)


def test_check_targets_accepts_the_contract_and_wants_a_device_by_default():
    for exc, what in CALLERS:
        K.check_targets(_good(), B, H, W, what, exc, require_cuda=False)
        with pytest.raises(exc, match="%s: target 0 .*device" % what):
            K.check_targets(_good(), B, H, W, what, exc)
        with pytest.raises(exc):
            K.check_targets(_good(), B, H, W, what, exc, require_cuda=True)


def test_check_head_maps():
    heads = [1, 14, 3, 2, 1, 360, 60, 60]
    good = [torch.zeros(B, c, H, W) for c in heads]
    K.check_head_maps(good, B, H, W, set(), "x")
    for optional in (set(), {6}, {5, 6}, {5}):
        for i in range(8):
            maps = list(good)
            maps[i] = None
            if i in optional:
                K.check_head_maps(maps, B, H, W, optional, "x")
            else:
                with pytest.raises(ValueError, match=r"x: head %d must be \[2, %d, 8, 12\].*got None" % (i, heads[i])):
                    K.check_head_maps(maps, B, H, W, optional, "x")
    for i in range(8):
        maps = list(good)
        maps[i] = torch.zeros(B, heads[i] + 1, H, W)
        with pytest.raises(ValueError, match=r"x: head %d must be \[2, %d, 8, 12\].*got \(2, %d, 8, 12\)" % (i, heads[i], heads[i] + 1)):
            K.check_head_maps(maps, B, H, W, {5, 6}, "x")


def test_require_device_tensor_refuses_cpu_tensors_and_non_tensors():
    for t in (torch.zeros(4), None, [1.0]):
        with pytest.raises(L.AbcNetHipError, match="x must be a contiguous float32 device tensor"):
            K.require_device_tensor(t, torch.float32, "x")
    with pytest.raises(ValueError, match="int32 / uint32"):
        K.require_device_tensor(torch.zeros(4), (torch.int32, torch.uint32), "x", exc=ValueError)


def test_meters_dict():
    table = torch.arange(34, dtype=torch.float64).reshape(17, 2) + 1.0      # row i = (2 i + 1, 2 i + 2)
    table[3, 1] = 0.0
    last = table.flip(1).clone()                                           # row i = (2 i + 2, 2 i + 1); row 3 = (0, 7)
    last[5, 1] = 0.0
    out = ops.meters_dict(table)
    assert list(out) == ops.METER_NAMES and len(out) == 17
    for i, n in enumerate(ops.METER_NAMES):
        assert list(out[n]) == ["sum", "count", "avg"]
        assert out[n]["sum"] == 2 * i + 1 and out[n]["count"] == (0.0 if i == 3 else 2 * i + 2)
        if i == 3:
            assert math.isnan(out[n]["avg"])
        else:
            assert out[n]["avg"] == (2 * i + 1) / (2 * i + 2)
    out = ops.meters_dict(table, last)
    for i, n in enumerate(ops.METER_NAMES):
        assert list(out[n]) == ["sum", "count", "avg", "val"]
        if i == 5:
            assert math.isnan(out[n]["val"])
        else:
            assert out[n]["val"] == (0.0 if i == 3 else (2 * i + 2) / (2 * i + 1))
    out = ops.meters_dict(table, extra={"rank_mean": torch.arange(17, dtype=torch.float64) / 4})
    for i, n in enumerate(ops.METER_NAMES):
        assert list(out[n]) == ["sum", "count", "avg", "rank_mean"] and out[n]["rank_mean"] == i / 4


def test_terms_dict():
    r = ops.terms_dict(torch.arange(17, dtype=torch.float64))
    assert r["total"] == 0 and len(r) == 17
    for i, n in enumerate(K.HEAD_NAMES):
        assert r[n] == 1 + i and r["raw_" + n] == 9 + i
    assert loss.terms_dict is ops.terms_dict


def test_aliases_and_the_one_head_list():
    from abcnet_amd import arch
    assert K.HEADS == (1, 14, 3, 2, 1, 360, 60, 60) == tuple(arch.TRAIN_HEADS)
    assert ops.EXTRACT_HEADS == K.HEADS and loss.HEADS == K.HEADS
    assert ops.HEAD_NAMES == K.HEAD_NAMES and len(K.HEAD_NAMES) == 8
    assert loss.TARGET_CHANNELS == K.TARGET_CHANNELS and loss.TARGET_DTYPES == K.TARGET_DTYPES == tuple(DTYPES)
    assert [c[-1] if len(c) == 1 else c[0] * c[1] for c in K.TARGET_CHANNELS] == list(K.HEADS)
