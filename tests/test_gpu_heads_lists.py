"""GPU tests of UNet(in_channels, heads) with the OTHER head lists the reference uses (tests/golden/heads_*.npz, make_golden.py heads):
unet.py:78's default [1,21,5,1,4,2] (with unet.py:122-134's own 480 x 480 three-channel self-check), multi_gpu_train.py:47's
[1,20,5,1,90,90,30,30], one head, three odd widths on a size that is no multiple of 32, unet2.py's default.  The merged heads' conv1,
the batched 1x1 launches, the batched finalisers and the per-head dropout salts all run with other head counts and widths here than
the train.py:47 list every other GPU test uses."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.unet import UNet  # noqa: E402
from abcnet_amd.unet2 import UNet as UNet2  # noqa: E402
from oracle import nms_oracle  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402

from test_gpu_model import PRE_BN_BIAS, _check_grads  # noqa: E402
from test_oracle_golden import HEADS_CASES, heads_case, heads_case_shapes  # noqa: E402

DEV = "cuda"
CASES = dict(HEADS_CASES)


def _model(variant, cin, heads, dtype="fp32", dropout_p=0.0):
    m = (UNet if variant == "unet" else UNet2)(cin, heads, dtype=dtype, dropout_p=dropout_p)
    m.load_state_dict(uo.filled_state(variant, cin, heads, seed=0))
    return m.to(DEV)


def _surrogate(ys):
    return sum((y ** 2).mean() for y in ys)


@pytest.mark.parametrize("tag,variant", HEADS_CASES)
def test_other_head_lists_fp32_forward_match_golden_and_oracle(tag, variant, golden_dir):
    """fp32 logits, eval and train: as many maps as heads, each of its head's width, within the 1e-3 gate of the reference's
    golden (samples, full maps where stored) and of the oracle"""
    gold, heads, cin, x = heads_case(golden_dir, tag, variant)
    sd0 = uo.filled_state(variant, cin, heads, seed=0)
    m = _model(variant, cin, heads)
    for mode in ("eval", "train"):
        m.load_state_dict(sd0)
        m.train(mode == "train")
        with torch.no_grad():
            ys = m(x.to(DEV))
            ref = uo.forward(variant, uo.clone_state(sd0), x, train=(mode == "train"))
        assert isinstance(ys, list) and len(ys) == len(ref) == len(heads) == int(gold["%s_%s_nmaps" % (tag, mode)])
        for i, (y, r) in enumerate(zip(ys, ref)):
            k = "%s_%s_head%d" % (tag, mode, i)
            assert tuple(y.shape) == tuple(r.shape) == tuple(gold[k + "_shape"]) and y.shape[1] == heads[i] and y.dtype == torch.float32
            y = y.cpu()
            assert (y - r).abs().max().item() < 1e-3, (tag, mode, i)
            f = y.reshape(-1)
            step = max(f.numel() // 257, 1)
            np.testing.assert_allclose(f[::step][:257].double().numpy(), gold[k + "_sample"], atol=1e-3, err_msg=k)
            if k in gold.files:
                np.testing.assert_allclose(y.numpy(), gold[k], rtol=0, atol=1e-3, err_msg=k)


@pytest.mark.parametrize("tag,variant", [c for c in HEADS_CASES if c[0] != "selfcheck"])
def test_other_head_lists_fp32_gradients_through_module_autograd(tag, variant, golden_dir):
    """loss.backward() through the module (_UNetFn) under the golden's surrogate loss sum_i mean(head_i ** 2): every parameter against
    the oracle's f32 / f64 autograd with _check_grads' bar, every gradient norm within 2e-2 of the reference's.  (selfcheck: its
    480 x 480 backward is too slow for the CPU oracle; its forward is above)"""
    gold, heads, cin, x = heads_case(golden_dir, tag, variant)
    sd0 = uo.filled_state(variant, cin, heads, seed=0)
    m = _model(variant, cin, heads)
    m.train()
    loss = _surrogate(m(x.to(DEV)))
    loss.backward()
    assert abs(loss.item() - gold["%s_loss" % tag].item()) <= 1e-4 * abs(gold["%s_loss" % tag].item())
    sds = []
    for dt in (torch.float32, torch.float64):
        sd = uo.clone_state({k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd0.items()}, requires_grad=True)
        _surrogate(uo.forward(variant, sd, x.to(dt), train=True)).backward()
        sds.append(sd)
    named = dict(m.named_parameters())
    assert list(named) == [k for k, v in sds[0].items() if v.requires_grad]
    # one-element gradients (unet2.py's 7x7 spatial-attention biases: a near-cancelling sum over every pixel) have no norm to average
    # the f32 summation noise over: the CPU's own f32 run is 0.4-0.7 % off its f64 run there, the device's (another order) 2.3-2.6 %
    _check_grads(lambda name: named[name].grad, sds[0], {k: v for k, v in sds[1].items() if v.numel() > 1})
    for k, v in sds[1].items():
        if v.numel() == 1 and v.grad is not None and not k.endswith(PRE_BN_BIAS):
            ref = v.grad.double().item()
            assert abs(named[k].grad.double().item() - ref) <= 1e-1 * abs(ref) + 1e-9, (k, named[k].grad.item(), ref)
    for name, p in named.items():
        key = "%s_gnorm/%s" % (tag, name)
        if name == "s" or name.endswith(PRE_BN_BIAS):
            continue
        gn = gold[key].item()
        bar = 1e-1 if p.numel() == 1 else 2e-2       # (one-element gradients: see above)
        assert abs(p.grad.double().norm().item() - gn) <= bar * gn + 1e-12, (name, p.grad.double().norm().item(), gn)


@pytest.mark.parametrize("tag,variant", HEADS_CASES)
def test_other_head_lists_bf16_forward_bound(tag, variant, golden_dir):
    """bf16 throughput mode (merged conv1 over 128 x nh channels, batched 1x1 heads): the bounds of test_forward_bf16_bound"""
    _gold, heads, cin, x = heads_case(golden_dir, tag, variant)
    sd0 = uo.filled_state(variant, cin, heads, seed=0)
    m = _model(variant, cin, heads, dtype="bf16")
    for mode, bound in (("eval", 0.08), ("train", 0.6)):
        m.load_state_dict(sd0)
        m.train(mode == "train")
        with torch.no_grad():
            ys = m(x.to(DEV))
            ref = uo.forward(variant, uo.clone_state(sd0), x, train=(mode == "train"))
        assert [tuple(y.shape) for y in ys] == [tuple(r.shape) for r in ref]
        worst = max((y.cpu() - r).abs().max().item() for y, r in zip(ys, ref))
        assert worst < bound, (tag, mode, worst)


@pytest.mark.parametrize("tag", ["default", "mgpu", "one", "default2"])
def test_other_head_lists_batched_heads_equal_one_by_one_launches(tag, golden_dir):
    """bf16 train mode, dropout 0.2: the plan with the heads batched / merged and the plan with one launch per head, driven as the
    module's autograd drives them (forward, d(surrogate)/d(logits), backward): logits bit for bit, the heads' 1x1 and BatchNorm
    gradients within 1e-5, the rest within the bars of test_batched_heads_equal_one_by_one_launches.  Bit equality of the logits
    needs the heads' BatchNorm batch statistics summed over the same partition of the pixels: the merged conv1 and the per-head
    conv1 write the same number of partial-sum rows at these sizes (asserted; at 2 x 256 x 256 they do not -- 64 rows against 128 --,
    so the multi-GPU list runs at 2 x 64 x 64 here)"""
    from abcnet_amd.synthetic import synthetic_images
    variant = CASES[tag]
    _gold, heads, cin, x = heads_case(golden_dir, tag, variant)
    if tag == "mgpu":
        x = synthetic_images(2, 64, seed=7)
    xd = x.to(DEV)

    def run(batched):
        m = _model(variant, cin, heads, dtype="bf16", dropout_p=0.2)
        m.train()
        eng = m._engine_for(xd, True, batched_heads=batched)
        st = torch.cuda.current_stream().cuda_stream
        m._load_image(eng, xd)
        eng.run_pack(st)
        eng.run_forward(st)
        lg = [t.clone() for t in eng.logits]
        for t, d in zip(eng.logits, eng.dlogits):
            d.copy_(2.0 * t / t.numel())
        eng.chan_scale.fill_(1.0)
        eng.run_backward(st)
        torch.cuda.synchronize()
        kinds = set(op[4]["kernel"] for op in eng.fwd_ops + eng.bwd_ops)
        return lg, m._flat_grad.clone(), kinds, dict(m._lay_p), eng.head_recs[0].stats.shape[0]

    lg_b, g_b, kinds_b, lay, rows_b = run(True)
    lg_s, g_s, kinds_s, _, rows_s = run(False)
    assert rows_b == rows_s
    assert "heads_fwd_batch" in kinds_b and "heads_fwd_batch" not in kinds_s
    # (the heads' weight-gradient kernel takes whole 128-pixel chunks: unet2's 24 x 24 maps go to the general one)
    assert ("heads_wgrad_batch" in kinds_b) == (lg_b[0].shape[2] * lg_b[0].shape[3] % 128 == 0)
    assert len(lg_b) == len(heads)
    for a, b in zip(lg_b, lg_s):
        assert torch.equal(a, b)
    for name, (off, n) in lay.items():
        if name == "s":
            continue
        a, b = g_b[off:off + n].double(), g_s[off:off + n].double()
        rel = (a - b).norm().item() / (b.norm().item() + 1e-30)
        if name.startswith("out_modules.") and "conv1" not in name:
            assert rel <= 1e-5, (name, rel)
        elif n == 1:
            assert rel <= 1.0, (name, rel)
        else:
            assert rel <= 1e-1, (name, rel)


@pytest.mark.parametrize("dtype,bound", [("bf16", 0.6), ("fp32", 1e-3)])
def test_dropout_masks_with_six_heads_mirror_the_device_hash(dtype, bound, golden_dir):
    """unet.py:69 with unet.py:78's six heads, p = 0.2, train mode: the module's logits are the oracle's forward under the masks
    abcnet_amd.dropout mirrors for a 6 x 128-channel feature row (the per-head salts and strides assume no 8 heads): within the
    bf16 train bound, and within the 1e-3 gate in fp32"""
    from abcnet_amd.dropout import head_keep_masks
    _gold, heads, cin, x = heads_case(golden_dir, "default", "unet")
    m = _model("unet", cin, heads, dtype=dtype, dropout_p=0.2)
    m.train()
    with torch.no_grad():
        ys = m(x.to(DEV))
    eng = m._engine_for(x.to(DEV), True)
    B, _, h, w = ys[0].shape
    masks = head_keep_masks(B, h, w, len(heads), eng.dropout_seed(1), 0.2)
    sd0 = uo.filled_state("unet", cin, heads, seed=0)
    with torch.no_grad():
        ref = uo.forward("unet", uo.clone_state(sd0), x, train=True, dropout_masks=masks)
        plain = uo.forward("unet", uo.clone_state(sd0), x, train=True)
    worst = max((y.cpu() - r).abs().max().item() for y, r in zip(ys, ref))
    assert worst < bound, worst
    # (the masks matter: without them the oracle is further away than the bar)
    assert max((y.cpu() - r).abs().max().item() for y, r in zip(ys, plain)) > bound


def test_multi_gpu_list_folded_inference_fp8_and_generic_nms(golden_dir):
    """multi_gpu_train.py:47's [1,20,5,1,90,90,30,30] at 2 x 1 x 256 x 256 in the BatchNorm-folded eval graph: bf16 within the bound of
    test_folded_inference_graph_matches_oracle, the e4m3 form (calibrated from the bf16 graph as InferenceRunner does) within the bound
    of test_fp8_inference_graph_against_oracle_and_bf16_graph; the NMS of img2smiles2.py:61-79 on the graph's own logits with 30 omega
    bins (abc_nms_peaks' general n_omega path; the bond-centre map of this list is head 3, multi_proc_img2smiles.py:275) bit-equal to
    the oracle's.  InferenceRunner itself refuses this list (its bond-centre map is not head 4)."""
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.ops import nms_peaks
    _gold, heads, cin, x = heads_case(golden_dir, "mgpu", "unet")
    m = _model("unet", cin, heads, dtype="bf16")
    m.eval()
    with pytest.raises(ValueError, match="heads"):
        InferenceRunner(m, x.shape[0], x.shape[2], x.shape[3], fold_bn=True)
    xd = x.to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    e16 = m._engine_for(xd, False, fold_bn=True)
    e16.img.copy_(xd)
    e16.run_pack(st)
    e16.run_forward(st)
    lg16 = [t.clone() for t in e16.logits]
    e8 = m._engine_for(xd, False, fold_bn=True, fp8=True)
    e8.img.copy_(xd)
    e8.calibrate_fp8(e16, st, 1.0)
    e8.run_pack(st)
    e8.run_forward(st)
    torch.cuda.synchronize()
    assert e8.fp8_calibrated and e8.hfeat_q is not None
    lg8 = [t.clone() for t in e8.logits]
    with torch.no_grad():
        ref = uo.forward("unet", uo.filled_state("unet", cin, heads, seed=0), x, train=False)
    assert [tuple(t.shape) for t in lg8] == [tuple(t.shape) for t in lg16] == [tuple(r.shape) for r in ref]
    d16 = max((a.cpu() - r).abs().max().item() for a, r in zip(lg16, ref))
    d8 = max((a.cpu() - r).abs().max().item() for a, r in zip(lg8, ref))
    assert d16 < 0.08 and d8 < 0.5, (d16, d8)
    for lg in (lg16, lg8):
        am, bm, r, om = nms_peaks(lg[0], lg[3], lg[6], lg[7])
        torch.cuda.synchronize()
        got = [t.cpu() for t in lg]
        da, db, dr, do = nms_oracle.nms(got[0], got[3], got[6], got[7])
        assert tuple(om.shape) == tuple(r.shape) == (x.shape[0], 30, x.shape[2] // 4, x.shape[3] // 4)
        assert torch.equal(am.cpu(), da) and torch.equal(bm.cpu(), db) and torch.equal(om.cpu(), do) and torch.equal(r.cpu(), dr)
        assert do.sum() > 0


@pytest.mark.parametrize("tag", ["default", "one"])
def test_inference_runner_and_nms_refuse_lists_without_the_nms_maps(tag, golden_dir):
    """lists without img2smiles2.py's eight maps: a clear ValueError from InferenceRunner and model.nms (no IndexError, no launch)"""
    from abcnet_amd.infer import InferenceRunner
    _gold, heads, cin, x = heads_case(golden_dir, tag, "unet")
    m = _model("unet", cin, heads, dtype="bf16")
    with pytest.raises(ValueError, match=r"heads \[%s\]" % ", ".join(map(str, heads))):
        InferenceRunner(m, x.shape[0], x.shape[2], x.shape[3])
    with pytest.raises(ValueError, match=r"heads \[%s\]" % ", ".join(map(str, heads))):
        m.nms(x.to(DEV))
    m2 = _model("unet", 1, [1, 20, 5, 1, 90, 90, 30, 30], dtype="bf16")
    with pytest.raises(ValueError, match="heads"):
        InferenceRunner(m2, 2, 64, 64, extract=True)


@pytest.mark.parametrize("tag,variant", HEADS_CASES)
def test_trainer_refuses_other_head_lists(tag, variant, golden_dir):
    """the fused training step (loss of train.py:95-137, meters, fused heads pass) is defined for train.py:47's list only"""
    from abcnet_amd.train import Trainer
    _gold, heads, cin, _x = heads_case(golden_dir, tag, variant)
    for fused in (True, False):
        m = _model(variant, cin, heads, dtype="bf16")
        with pytest.raises(ValueError, match=r"heads \[%s\]" % ", ".join(map(str, heads))):
            Trainer(m, 2, 64, 64, use_graph=False, fused_heads=fused)


@pytest.mark.parametrize("tag,variant", HEADS_CASES)
def test_other_head_lists_state_dict_interchange(tag, variant, golden_dir):
    """a state_dict keyed as the reference's (the golden's keys and shapes) loads into the module on the device and comes back bit
    for bit, also with the 'module.' prefix of nn.DataParallel checkpoints (train.py:435, img2smiles2.py:43-44)"""
    from collections import OrderedDict
    gold, heads, cin, _x = heads_case(golden_dir, tag, variant)
    keys, shapes = heads_case_shapes(gold, tag)
    g = torch.Generator().manual_seed(41)
    sd = OrderedDict()
    for k, s in zip(keys, shapes):
        sd[k] = torch.tensor(7, dtype=torch.int64) if k.endswith("num_batches_tracked") else torch.randn(s, generator=g)
    for prefix in ("", "module."):
        m = _model(variant, cin, heads)
        m.load_state_dict(OrderedDict((prefix + k, v) for k, v in sd.items()))
        back = m.state_dict()
        assert list(back.keys()) == keys
        for k, v in sd.items():
            assert back[k].device.type == "cuda" and back[k].dtype == v.dtype and torch.equal(back[k].cpu(), v), k
