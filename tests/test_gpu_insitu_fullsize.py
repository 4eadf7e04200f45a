"""Flip-free backward parity AT THE BENCHMARKED SIZE AND DTYPE (BASELINE.json configs 1-3; train.py:94-141).

tests/test_gpu_fullsize.py holds one bf16 step at batch 16, 384x384 to the fp32 oracle end to end -- but at fresh weights
thousands of ReLU decisions flip under bf16, the measured per-tensor gradient deviation is O(1) for the reference arithmetic
too, and an end-to-end bound that loose cannot see a broken weight gradient.  The launch shapes that exist ONLY at full size
(the 6144-tile merged heads convolution, persistent tiles with a balanced last round, XCD remaps, the 1024-row merged weight
gradient with 16 K-splits, the fused heads pass at 2 M threads) are therefore held here link by link:

  * test_backward_links_in_situ_bf16_b16_384 (unet.py, bf16, fused heads, no graph): every sampled data gradient, weight
    gradient, bias gradient, BatchNorm backward (dgamma, dbeta, dY) and the fused heads pass (logits, g, conv2 gradients)
    against torch ops / autograd applied ON THE GPU to the engine's OWN bf16 tensors, with every decision (ReLU sign,
    dropout keep) taken from the engine's tensors -- no flip can enter, so the bounds are those of one bf16 rounding:
    relative L2 4e-3 ... 1e-2 and 3e-2 of the largest element (what tests/test_gpu_kernels.py uses per kernel).
    CAN detect: a wrong tile / split / remap / tap / channel offset in any sampled launch (a missing tile of 768 moves the
    relative L2 by 3.6e-2), a wrong normaliser, a dropped K-split.  CANNOT detect: an error in an UNSAMPLED layer at THIS size
    (tests/test_gpu_insitu_all_layers.py walks every layer with the same links, tests/insitu_links.py, at small and ragged sizes;
    the end-to-end test bounds the rest here), nor a deviation below bf16 rounding.
  * test_fp32_train_step_at_config1_workload: the fp32 (exact-f32 MFMA) step at 4 x 1 x 384 x 384 -- config 1's workload on
    the HIP path -- against the oracle: loss 2e-4, every gradient under tests/test_gpu_model.py::_check_grads.
  * test_unet2_links_in_situ_bf16_b16_384: the same link-by-link statement for unet2.py's CBAM blocks and convolutions.
    (Its first run FOUND a bf16-only defect the end-to-end bound had absorbed: the conv epilogue took CBAM's global max before the
    rounding to bf16, the backward looked for a pixel of the stored tensor equal to it, found none, and dropped the max-pool
    branch's gradient -- d(y2) off by 6-10 %, dgamma2 by 9-21 %.  Now: max / min of the values as stored, and the gradient goes
    to the FIRST maximal pixel, torch's rule, found by an integer atomic min in the forward's per-pixel pass.)
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.dropout import head_keep_masks  # noqa: E402
from abcnet_amd.synthetic import synthetic_images, synthetic_targets  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
# the link checks themselves: tests/insitu_links.py (shared with tests/test_gpu_insitu_all_layers.py, which walks every layer)
from insitu_links import Report, _cbam_links, _conv2_links, _conv_links, _convT_links, _heads_links  # noqa: E402

HEADS = uo.HEADS
DEV = "cuda"
# the torch references run on the GPU through the native im2col + GEMM convolutions (no MIOpen kernel search / JIT on a fresh box)
torch.backends.cudnn.enabled = False


def _model(variant, dtype, dropout_p):
    if variant == "unet2":
        from abcnet_amd.unet2 import UNet
    else:
        from abcnet_amd.unet import UNet
    m = UNet(1, HEADS, dtype=dtype, dropout_p=dropout_p)
    m.load_state_dict(uo.filled_state(variant, 1, HEADS, seed=0))
    return m.to(DEV)


UNET_SAMPLE = ("dconv2.double_conv.3", "dconv2.double_conv.0", "up3.conv.double_conv.0", "inc3.double_conv.3",
               "down2.maxpool_conv.1.double_conv.0", "down1.maxpool_conv.1.double_conv.3", "inc2.double_conv.3", "inc1.double_conv.3",
               "down4.maxpool_conv.1.double_conv.0", "down5.maxpool_conv.1.double_conv.3", "up1.conv.double_conv.0")


def test_backward_links_in_situ_bf16_b16_384():
    from abcnet_amd.train import Trainer
    B, S = 16, 384
    x = synthetic_images(B, S, seed=7)
    tg = synthetic_targets(B, S // 4, seed=1)
    m = _model("unet", "bf16", 0.2)
    tr = Trainer(m, B, S, S, lr=0.0, use_graph=False)
    eng = tr.eng
    assert eng.hf is not None, "the benchmark's step runs the fused heads pass"
    tr.load_batch(x.to(DEV), [t.to(DEV) for t in tg])
    tr.step()
    torch.cuda.synchronize()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rep = Report()
    with torch.enable_grad():
        _heads_links(eng, m, rep, sd, tg, B, S // 4, S // 4)
        recs = {r.cname: r for r in eng.recs if r.kind == "conv"}
        for cn in UNET_SAMPLE:
            _conv_links(recs[cn], m, rep, sd)
            torch.cuda.empty_cache()
        for r in eng.recs:
            if r.kind == "convT" and r.cname in ("up1.up", "up3.up"):
                _convT_links(r, m, rep, sd)
    rep.finish()


def test_fp32_train_step_at_config1_workload():
    """BASELINE.json config 1's workload (unet.py forward + backward on 4 x 1 x 384 x 384, fp32) on the HIP path"""
    from test_gpu_model import _check_grads, _oracle_grads
    from abcnet_amd.train import Trainer
    B, S = 4, 384
    x = synthetic_images(B, S, seed=7)
    tg = synthetic_targets(B, S // 4, seed=1)
    m = _model("unet", "fp32", 0.2)
    tr = Trainer(m, B, S, S, lr=0.0, use_graph=False)
    masks = head_keep_masks(B, S // 4, S // 4, 8, tr.eng.dropout_seed(1), 0.2)
    sd, total, weighted, _ = _oracle_grads(x, tg, dropout_masks=masks)
    sd64 = _oracle_grads(x, tg, dropout_masks=masks, dtype=torch.float64)[0]
    tr.load_batch(x.to(DEV), [t.to(DEV) for t in tg])
    tr.step()
    torch.cuda.synchronize()
    res = tr.loss_value()
    assert abs(res["total"] - total.item()) < 2e-4 * abs(total.item()), (res["total"], total.item())
    for k in ("atom_t", "bond_t", "atom_types", "atom_charges", "bond_types", "bond_rhos", "bond_omega", "atom_hs"):
        assert abs(res[k] - weighted[k].item()) < 5e-4 * abs(weighted[k].item()) + 1e-6, k
    _check_grads(lambda n: m.grad_of(n), sd, sd64)


UNET2_CONVS = ("dconv2.double_conv.3", "dconv2.double_conv.0", "inc2.double_conv.3", "inc2.double_conv.0", "down1.maxpool_conv.1.double_conv.0",
               "down5.maxpool_conv.1.double_conv.3", "up3.conv.double_conv.0")
UNET2_BLOCKS = ("dconv2", "inc2", "down2.maxpool_conv.1", "up1.conv")


def test_unet2_links_in_situ_bf16_b16_384():
    from abcnet_amd.train import Trainer
    B, S = 16, 384
    x = synthetic_images(B, S, seed=7)
    tg = synthetic_targets(B, S // 4, seed=1)
    m = _model("unet2", "bf16", 0.0)
    tr = Trainer(m, B, S, S, lr=0.0, use_graph=False)
    eng = tr.eng
    tr.load_batch(x.to(DEV), [t.to(DEV) for t in tg])
    tr.step()
    torch.cuda.synchronize()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rep = Report()
    with torch.enable_grad():
        if eng.hf is not None:
            _heads_links(eng, m, rep, sd, tg, B, S // 4, S // 4)
        recs = {r.cname: r for r in eng.recs if r.kind == "conv"}
        for cn in UNET2_CONVS:
            _conv2_links(eng, recs[cn], m, rep, sd)
            torch.cuda.empty_cache()
        blks = {u.prefix: u for k, u in eng.units2 if k == "blk"}
        for pf in UNET2_BLOCKS:
            _cbam_links(eng, blks[pf], m, rep, sd)
            torch.cuda.empty_cache()
        for k, u in eng.units2:
            if k == "convT" and u.cname == "up3.up":
                _convT_links(u, m, rep, sd)
    rep.finish()
