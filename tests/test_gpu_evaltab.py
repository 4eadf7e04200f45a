"""GPU parity: the device-side evaluation tables (abc_eval_tables_update through ops.EvalTables and InferenceRunner(evaluate=True))
against the golden generated from the reference text (test_accuracy.py:105-269) and the torch oracle (tests/evaltab_oracle.py).
Integer tables compare exactly; the rho MAE numerator, a float sum, at 1e-6 relative."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.ops import METER_NAMES, EvalTables, nms_peaks  # noqa: E402
from abcnet_amd.synthetic import synthetic_images, synthetic_targets  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402

import evaltab_oracle as eo  # noqa: E402

DEV = "cuda"


def _device_eval(lg, tg, use_idx=False, n_valid=None):
    """EvalTables on the masks of the device NMS (img2smiles2.py:61-79, bit-identical to the oracle's: test_gpu_kernels)"""
    d = [t.to(DEV).contiguous() for t in lg]
    am, bm, rho, om = nms_peaks(d[0], d[4], d[6], d[7])
    idx = None
    if use_idx:
        B, _, h, w = d[5].shape
        idx = d[5].view(B, 6, 60, h, w).argmax(1).to(torch.uint8).contiguous()
        d[5] = None
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=DEV)
    return EvalTables(am, bm, om, rho, d, [t.to(DEV) for t in tg], btype_idx=idx, n_valid=nv)


def _check(res, want):
    for k in eo.TABLES:
        assert np.array_equal(res[k], want[k]), (k, res[k], want[k])
    for k, m in want["confusion"].items():
        assert np.array_equal(res["confusion"][k], m), k
    for n in METER_NAMES:
        num, den = want["meters"][n]
        tol = 1e-6 * max(1.0, abs(num)) if n == "bond_rhos_mae" else 0.0
        assert abs(res["meters"][n]["sum"] - num) <= tol + 1e-9, (n, res["meters"][n]["sum"], num)
        assert abs(res["meters"][n]["count"] - den) <= 1e-9, (n, res["meters"][n]["count"], den)
    prec, rec = eo.derived(want)
    for k in eo.TABLES:
        assert np.array_equal(res["precision"][k], prec[k]) and np.array_equal(res["recall"][k], rec[k]), k


@pytest.fixture(scope="module")
def case128():
    tg = synthetic_targets(2, 128, seed=3)
    lg = eo.confusable_logits(tg, seed=19)
    return lg, tg, eo.evaluate(lg, tg)


def test_tables_match_golden_and_oracle(case128, golden_dir):
    lg, tg, want = case128
    gold = np.load(os.path.join(golden_dir, "evaltab_128.npz"))
    ev = _device_eval(lg, tg)
    ev.run()
    res = ev.result()
    for k in eo.TABLES:
        assert np.array_equal(res[k], gold[k]), (k, res[k], gold[k])
        assert np.array_equal(res["last"][k], gold[k]), k
    for n, s, c in zip(METER_NAMES, gold["sum"], gold["count"]):
        assert abs(res["meters"][n]["sum"] - s) <= 1e-5 * max(1.0, abs(s)), (n, res["meters"][n]["sum"], s)
        assert abs(res["meters"][n]["count"] - c) <= 1e-5 * max(1.0, abs(c)), (n, res["meters"][n]["count"], c)
    _check(res, want)


@pytest.mark.parametrize("B,h", [(1, 32), (3, 40)])
def test_other_shapes_match_oracle(B, h):
    """a pixel count that is no multiple of the workgroup (3 * 40 * 40), borders, an image without any target: every denominator
    that can be zero stays a clean zero in the table"""
    tg = synthetic_targets(B, h, seed=5)
    for t in tg:
        t[0].zero_()
    lg = eo.confusable_logits(tg, seed=23)
    ev = _device_eval(lg, tg)
    ev.run()
    res = ev.result()
    _check(res, eo.evaluate(lg, tg))
    if B == 1:
        for n in ("atom_targets_recall", "atom_types_acc", "bond_types_acc", "bond_rhos_mae", "bond_omega_recall", "bond_omega_precision"):
            assert res["meters"][n]["sum"] == 0.0 and res["meters"][n]["count"] == 0.0, n
        assert res["atom_detection"][0, 2] > 0 and not res["atom_type"].any()
    assert all(np.isfinite(res[k]).all() for k in eo.TABLES)


def test_ties_and_class_zero():
    """type, charge, bond-type and omega logits on a coarse grid, so that the arg max is decided by the first-index rule at many
    weighted pixels; a peak on a pixel without any target is a false positive of class 0"""
    tg = synthetic_targets(2, 32, seed=9)
    lg = eo.confusable_logits(tg, seed=41)
    for i in (1, 2, 5):
        lg[i] = torch.round(lg[i] / 4) * 4
    lg[7] = torch.round(lg[7])
    free = (torch.nn.functional.max_pool2d(tg[0], 5, 1, 2) == 0) & (tg[1].sum(1, keepdim=True) == 0)
    y, x = [int(v) for v in free[0, 0].nonzero()[0]]
    lg[0][0, 0, y, x] = 50.0
    top2 = lg[1].topk(2, dim=1).values
    assert int(((top2[:, 0] == top2[:, 1]) & ((tg[1] == 1).sum(1) > 0)).sum()) > 0          # ties where they carry weight
    t6 = lg[5].view(2, 6, 60, 32, 32).topk(2, dim=1).values
    assert int(((t6[:, 0] == t6[:, 1]) & ((tg[5] == 1).sum(1) > 0)).sum()) > 0
    want = eo.evaluate(lg, tg)
    assert want["atom_detection"][0, 2] >= 1
    ev = _device_eval(lg, tg)
    ev.run()
    _check(ev.result(), want)


def test_argmax_map_equals_logit_planes(case128):
    lg, tg, want = case128
    a, b = _device_eval(lg, tg), _device_eval(lg, tg, use_idx=True)
    a.run()
    b.run()
    torch.cuda.synchronize()
    assert torch.equal(a.counts_last, b.counts_last) and torch.equal(a.meters_last, b.meters_last)
    assert torch.equal(a.counts_totals, b.counts_totals) and torch.equal(a.meters_totals, b.meters_totals)
    _check(b.result(), want)


def test_accumulation_reset_and_reproducibility(case128):
    lg, tg, _ = case128
    ev = _device_eval(lg, tg)
    ev.run()
    torch.cuda.synchronize()
    c1, m1 = ev.counts_totals.clone(), ev.meters_totals.clone()
    assert torch.equal(c1, ev.counts_last) and torch.equal(m1, ev.meters_last) and int(c1.sum()) > 0
    ev.run()
    torch.cuda.synchronize()
    assert torch.equal(ev.counts_totals, 2 * c1) and torch.equal(ev.meters_totals, 2 * m1)       # x2 is exact in both types
    assert torch.equal(ev.counts_last, c1) and torch.equal(ev.meters_last, m1)
    ev.reset()
    ev.run()
    torch.cuda.synchronize()
    assert torch.equal(ev.counts_totals, c1) and torch.equal(ev.meters_totals, m1)
    fresh = _device_eval(lg, tg)
    fresh.run()
    torch.cuda.synchronize()
    assert torch.equal(fresh.counts_totals, c1) and torch.equal(fresh.meters_totals, m1)          # bit for bit


def test_n_valid_counts_the_leading_images_only():
    tg = synthetic_targets(3, 40, seed=5)
    lg = eo.confusable_logits(tg, seed=23)
    ev = _device_eval(lg, tg, n_valid=1)
    ev.run()
    _check(ev.result(), eo.evaluate([t[:1] for t in lg], [t[:1] for t in tg]))
    ev.keep[-1].fill_(7)          # past B: clamped to all three
    ev.reset()
    ev.run()
    _check(ev.result(), eo.evaluate(lg, tg))


def _model(variant, dtype):
    from abcnet_amd.unet import UNet
    from abcnet_amd.unet2 import UNet as UNet2
    m = (UNet if variant == "unet" else UNet2)(1, uo.HEADS, dtype=dtype, dropout_p=0.0)
    m.load_state_dict(uo.filled_state(variant, 1, uo.HEADS, seed=0))
    return m.to(DEV)


def _drive(run, B, S, n_valids, tg, full=None):
    """steps (eager, capture, replay ...) with another batch and another n_valid each; the oracle on the logits of `full` (a runner
    that stores all eight maps; default: `run` itself), accumulated like the meters"""
    acc = None
    for step, nv in enumerate(n_valids):
        x = synthetic_images(B, S, seed=7 + step).to(DEV)
        run.load_batch(x, [t.to(DEV) for t in tg], n_valid=nv)
        run.step()
        if full is not None:
            full.load_batch(x)
            full.step()
        torch.cuda.synchronize()
        lg = [t.cpu() for t in (full or run).logits]
        acc = eo.accumulate(acc, eo.evaluate([t[:nv] for t in lg], [t[:nv] for t in tg]))
        _check(run.evaluation(), acc)
    return acc


@pytest.mark.parametrize("variant", ["unet", "unet2"])
def test_inference_runner_evaluates_inside_the_graph(variant):
    """InferenceRunner(evaluate=True), fp32, B = 2 at 64 x 64: the tables ride inside the captured step and see the logits and the
    n_valid of THAT step"""
    from abcnet_amd.infer import InferenceRunner
    B, S = 2, 64
    tg = synthetic_targets(B, S // 4, seed=1)
    run = InferenceRunner(_model(variant, "fp32"), B, S, S, use_graph=True, evaluate=True)
    acc = _drive(run, B, S, [2, 1, 2], tg)
    assert sum(acc[k].sum() for k in eo.TABLES) > 0
    run.reset_evaluation()
    res = run.evaluation()
    assert not any(res[k].any() for k in eo.TABLES) and all(v["count"] == 0 for v in res["meters"].values())


@pytest.mark.parametrize("form", ["decode", "nms_kernel", "fp8", "fp8_decode"])
def test_inference_runner_forms(form):
    """the other forms of the inference graph, bf16 folded, B = 2 at 128 x 128: decode mode (bond types from the uint8 arg-max map,
    |rho| only), the NMS kernel writing |rho| and the omega mask, the e4m3 graph"""
    from abcnet_amd.infer import InferenceRunner
    B, S = 2, 128
    fp8, decode = form.startswith("fp8"), form.endswith("decode")
    tg = synthetic_targets(B, S // 4, seed=1)
    m = _model("unet", "bf16")
    run = InferenceRunner(m, B, S, S, use_graph=True, fold_bn=True, fp8=fp8, decode=decode, nms_in_heads=form != "nms_kernel", evaluate=True)
    assert run.decode == decode and run.nms_in_heads == (form != "nms_kernel")
    full = InferenceRunner(m, B, S, S, use_graph=True, fold_bn=True, fp8=fp8) if decode else None
    _drive(run, B, S, [2, 2, 1], tg, full=full)


def test_runner_without_evaluate_is_unchanged_and_refuses():
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd._lib import AbcNetHipError
    run = InferenceRunner(_model("unet", "fp32"), 2, 64, 64, use_graph=False)
    assert run.evaluator is None and not hasattr(run, "eval_targets") and not hasattr(run, "n_valid")
    with pytest.raises(AbcNetHipError):
        run.evaluation()
    with pytest.raises(AbcNetHipError):
        run.load_batch(synthetic_images(2, 64, seed=7).to(DEV), n_valid=1)


def test_eval_tables_fail_loudly_on_cpu_tensors_and_wrong_heads():
    tg = synthetic_targets(1, 32, seed=5)
    lg = eo.confusable_logits(tg, seed=23)
    with pytest.raises(Exception):
        EvalTables(lg[0], lg[4], lg[7], lg[6], lg, tg)
    d = [t.to(DEV) for t in lg]
    dt = [t.to(DEV) for t in tg]
    with pytest.raises(ValueError):
        EvalTables(d[0], d[4], d[7], d[6], d[:1] + [d[1][:, :13].contiguous()] + d[2:], dt)
    with pytest.raises(ValueError):
        EvalTables(d[0], d[4], d[7][:, :30].contiguous(), d[6], d, dt)
