"""CPU tier of the drop-in loss and optimiser (abcnet_amd.loss, abcnet_amd.optim): the new C-ABI descriptors match the
library, the launchers refuse bad descriptors on the host, and the torch-facing objects refuse what they do not support
before anything touches a device."""
import ctypes as C

import pytest
import torch

import abcnet_amd  # noqa: F401
from abcnet_amd import _lib as L

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]


def test_new_structs_match_abc_sizeof():
    lib = L.load()
    for st in (L.LossScaleDesc, L.AdamSeg, L.AdamClass, L.AdamMultiDesc):
        i = L._STRUCTS.index(st)
        assert lib.abc_sizeof(i) == C.sizeof(st), st.__name__
    assert lib.abc_sizeof(len(L._STRUCTS)) == -1
    assert lib.abc_adam_multi_chunk() > 0 and lib.abc_adam_multi_chunk() % 4 == 0


def test_launchers_refuse_bad_descriptors_on_the_host():
    lib = L.load()
    d = L.LossScaleDesc()
    d.head_scale, d.ds, d.grad_out = 16, 16, 16    # never dereferenced: the refusal comes first
    d.dlogits[0], d.n[0] = 4, 8                    # not 16-byte aligned
    assert lib.abc_loss_scale_grads(C.byref(d), None) == -1
    assert b"aligned" in lib.abc_last_error()
    d.head_scale = None
    assert lib.abc_loss_scale_grads(C.byref(d), None) == -1
    m = L.AdamMultiDesc()
    m.segs, m.nseg, m.nclass, m.chunk_total = None, 0, 1, 1
    assert lib.abc_adam_multi(C.byref(m), None) == -1
    m.segs, m.nseg, m.nclass = 16, 1, L.ADAM_MAX_CLASSES + 1
    assert lib.abc_adam_multi(C.byref(m), None) == -1
    m.nclass, m.chunk_total = 1, 0
    assert lib.abc_adam_multi(C.byref(m), None) == -1


@pytest.mark.parametrize("flag", [{"amsgrad": True}, {"fused": True}, {"maximize": True}, {"capturable": True},
                                  {"differentiable": True}])
def test_adam_refuses_unsupported_options(flag):
    from abcnet_amd.optim import Adam
    with pytest.raises(ValueError, match=list(flag)[0]):
        Adam([torch.zeros(4)], **flag)


def test_adam_refuses_cpu_and_non_f32_params():
    from abcnet_amd.optim import Adam
    with pytest.raises(L.AbcNetHipError, match="GPU"):
        Adam([torch.zeros(4)])
    with pytest.raises(L.AbcNetHipError):
        Adam([{"params": [torch.zeros(4, dtype=torch.float64)], "lr": 1e-3}])


def _inputs(B=1, h=4, w=4, heads=HEADS):
    preds = [torch.zeros((B, c, h, w)) for c in heads]
    tg = [torch.zeros((B, 1, h, w)), torch.zeros((B, 14, h, w)), torch.zeros((B, 3, h, w)), torch.zeros((B, 2, h, w)),
          torch.zeros((B, 1, h, w)), torch.zeros((B, 6, 60, h, w)), torch.zeros((B, 60, h, w), dtype=torch.float64),
          torch.zeros((B, 60, h, w), dtype=torch.float64)]
    return preds, tg, torch.zeros(10)


def test_abc_loss_refuses_wrong_layouts_before_touching_a_device():
    from abcnet_amd.loss import ABCLoss, abc_loss
    preds, tg, s = _inputs(heads=[1, 14, 3, 2, 1, 360, 60, 30])
    with pytest.raises(ValueError, match="heads"):
        abc_loss(preds, tg, s)
    preds, tg, s = _inputs()
    with pytest.raises(ValueError, match="8 head maps"):
        abc_loss(preds[:7], tg, s)
    tg[6] = tg[6].float()                       # rho target must be f64 (utils.py:91)
    with pytest.raises(ValueError, match="target 6"):
        abc_loss(preds, tg, s)
    preds, tg, s = _inputs()
    preds[3] = preds[3].double()
    with pytest.raises(ValueError, match="float32"):
        ABCLoss()(preds, tg, s)
    preds, tg, s = _inputs()
    tg[5] = torch.zeros((1, 360, 4, 4))         # bond types are [B, 6, 60, h, w]
    with pytest.raises(ValueError, match="target 5"):
        abc_loss(preds, tg, s)
    preds, tg, s = _inputs()
    with pytest.raises(ValueError, match="s must"):
        abc_loss(preds, tg, torch.zeros(9))
    # a valid layout on the CPU: refused, there is no CPU fallback
    with pytest.raises(L.AbcNetHipError, match="GPU"):
        abc_loss(preds, tg, s)
