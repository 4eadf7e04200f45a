"""Oracle (test infrastructure, not product): the evaluation of the reference's src/test_accuracy.py:105-298 restated in
torch as a function of the RAW head maps and the targets, with the hard-coded 128 x 128 replaced by the size of the tensors.

The structure follows the text: the inference NMS of lines 105-124, the five (tp, tn, fp, fn) tables of lines 128-186 filled by
the same per-class loops, the 17 meters of lines 188-269 (every one an AverageMeter.update(num / den, den), i.e. sum += num,
count += den: the (num, den) pair of one batch is returned, in float64), and the derived precision / recall of lines 285-298.
Pinned by tests/golden/evaltab_128.npz (the reference text itself, executed by tests/golden/make_golden_evaltab.py).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from abcnet_amd.ops import METER_NAMES
from abcnet_amd.synthetic import correlated_logits

TABLES = ["atom_detection", "atom_type", "atom_charge", "bond_detection", "bond_type"]


def confusable_logits(targets, seed, class_noise=2.0, centre_noise=1.5, blackout=0.25, cell=8):
    """synthetic.correlated_logits made confusable: plain correlated logits give nearly diagonal tables (0-2 fp / fn per class, no
    missed centre at all), so Gaussian class noise is added to the type, charge and bond-type heads, and the two centre heads get
    stronger pixel noise plus a coarse one -- whole cell x cell blocks pushed down by 6 with probability `blackout` -- so that
    some target centres have no peak anywhere in their 3 x 3 neighbourhood"""
    lg = correlated_logits(targets, seed=seed, centre_noise=centre_noise)
    g = torch.Generator().manual_seed(seed + 1000)
    B, _, h, w = lg[0].shape
    for i in (1, 2, 5):
        lg[i] = lg[i] + class_noise * torch.randn(lg[i].shape, generator=g)
    for i in (0, 4):
        coarse = (torch.rand((B, 1, -(-h // cell), -(-w // cell)), generator=g) < blackout).float()
        coarse = coarse.repeat_interleave(cell, dim=2).repeat_interleave(cell, dim=3)[:, :, :h, :w]
        lg[i] = lg[i] - 6.0 * coarse
    return lg


def _circ3(t):
    """lines 117-122 / 241-243 / 251-254 / 264-267: circular 3-tap max over the omega bins through the padded permute / reshape"""
    n, c, h, w = t.shape
    ring = torch.cat([t[:, c - 1:], t, t[:, :1]], dim=1).permute(0, 2, 3, 1).reshape(-1, h * w, c + 2)
    return F.max_pool1d(ring.float(), stride=1, kernel_size=3, padding=0).reshape(-1, h, w, c).permute(0, 3, 1, 2)


def _pool3(t):
    return F.max_pool2d(t, kernel_size=3, stride=1, padding=1)


def evaluate(preds, targets, confusion=True):
    """one batch.  preds: the 8 raw head maps [B, {1,14,3,2,1,360,60,60}, h, w] f32; targets: the 8 target maps of the loss.
    Returns {table name: float64 [n, 4]} for the five tables, "meters": {name: (num, den)} floats, "confusion": {atom_type,
    atom_charge, bond_type: float64 C[target][predicted]} (confusion=False: left out -- the reference does not compute them)"""
    (atom_targets_pred, atom_types_pred, atom_charges_pred, atom_hs_pred, bond_targets_pred, bond_types_pred, bond_rhos_pred,
     bond_omega_types_pred) = preds
    atom_targets, atom_types, atom_charges, atom_hs, bond_targets, bond_types, bond_rhos, bond_omega_types = targets
    B, _, h, w = atom_targets.shape
    # ---- lines 105-126
    atom_targets_pred = (_pool3(atom_targets_pred) == atom_targets_pred) * (atom_targets_pred > -1).float()
    bond_targets_pred = (_pool3(bond_targets_pred) == bond_targets_pred) * (bond_targets_pred > -1).float()
    bond_rhos_pred = torch.abs(bond_rhos_pred)
    bond_types_pred = bond_types_pred.view(-1, 6, 60, h, w)
    bond_omega_types_pred = ((_circ3(bond_omega_types_pred) == bond_omega_types_pred) * (bond_omega_types_pred > -1)).float()
    atom_targets = (atom_targets == 1).float()
    bond_targets = (bond_targets == 1).float()
    tab = {"atom_detection": np.zeros((14, 4)), "atom_type": np.zeros((14, 4)), "atom_charge": np.zeros((3, 4)),
           "bond_detection": np.zeros((6, 4)), "bond_type": np.zeros((6, 4))}
    num = lambda t: float(t.sum().double().item())

    def detection(name, n, cls, pred, tgt):
        # lines 128-136 / 165-173
        for i in range(n):
            tab[name][i, 0] += num((cls == i) * (pred * _pool3(tgt)))
            tab[name][i, 2] += num((cls == i) * (pred * (_pool3(tgt) == 0)))
            tab[name][i, 3] += num((cls == i) * ((_pool3(pred) == 0) * tgt))

    def typing(name, n, tgt, pred):
        # lines 138-162 / 175-186
        wgt = torch.sum(tgt == 1, dim=1)
        t, p = tgt.argmax(1), pred.argmax(1)
        for i in range(n):
            tab[name][i, 0] += num(wgt * ((t == i) * (p == i)))
            tab[name][i, 1] += num(wgt * ((t != i) * (p != i)))
            tab[name][i, 2] += num(wgt * ((t != i) * (p == i)))
            tab[name][i, 3] += num(wgt * ((t == i) * (p != i)))
        conf = np.zeros((n, n))
        for i in range(n if confusion else 0):
            for j in range(n):
                conf[i, j] = num(wgt * ((t == i) * (p == j)))
        return conf

    conf = {}
    detection("atom_detection", 14, atom_types.argmax(1, keepdims=True), atom_targets_pred, atom_targets)
    conf["atom_type"] = typing("atom_type", 14, atom_types, atom_types_pred)
    conf["atom_charge"] = typing("atom_charge", 3, atom_charges, atom_charges_pred)
    detection("bond_detection", 6, bond_types.sum(2).argmax(1, keepdims=True), bond_targets_pred, bond_targets)
    conf["bond_type"] = typing("bond_type", 6, bond_types, bond_types_pred)
    # ---- lines 188-269
    m = {}

    def centre(prefix, pred, tgt):
        m[prefix + "_precision"] = (num(pred * tgt), num(pred))
        m[prefix + "_precision3"] = (num(pred * _pool3(tgt)), num(pred))
        m[prefix + "_recall"] = (num(tgt * pred), num(tgt))
        m[prefix + "_recall3"] = (num(tgt * _pool3(pred)), num(tgt))

    def acc(tgt, pred, eps=0.0):
        return (num(torch.sum(tgt, dim=1) * (tgt.argmax(1) == pred.argmax(1)).float()), eps + num(tgt))

    centre("atom_targets", atom_targets_pred, atom_targets)
    m["atom_types_acc"] = acc(atom_types, atom_types_pred)
    m["atom_charges_acc"] = acc(atom_charges, atom_charges_pred)
    m["atom_hs_acc"] = acc(atom_hs, atom_hs_pred, eps=0.01)
    centre("bond_targets", bond_targets_pred, bond_targets)
    m["bond_types_acc"] = acc(bond_types, bond_types_pred)
    m["bond_rhos_mae"] = (num(torch.abs(bond_rhos_pred - bond_rhos) * torch.sum(bond_types, dim=1)), num(bond_types))
    temp = ((_circ3(bond_omega_types_pred) == bond_omega_types_pred) * (bond_omega_types_pred > 0.25)).float() * bond_targets
    bond_omega_types = (bond_omega_types == 1)
    m["bond_omega_precision"] = (num(bond_omega_types * temp), num(temp))
    temp2 = _circ3(temp)
    m["bond_omega_recall3"] = (num(bond_omega_types * temp2), num(bond_omega_types))
    m["bond_omega_recall"] = (num(bond_omega_types * temp), num(bond_omega_types))
    temp3 = _circ3(bond_omega_types)
    m["bond_omega_precision3"] = (num(temp3 * temp), num(temp))
    assert list(m) == METER_NAMES
    out = dict(tab)
    out["meters"] = m
    out["confusion"] = conf
    return out


def accumulate(acc, one):
    """AverageMeter / += semantics over batches"""
    if acc is None:
        return one
    out = {k: acc[k] + one[k] for k in TABLES}
    out["meters"] = {k: (acc["meters"][k][0] + one["meters"][k][0], acc["meters"][k][1] + one["meters"][k][1]) for k in METER_NAMES}
    out["confusion"] = {k: acc["confusion"][k] + one["confusion"][k] for k in one["confusion"]}
    return out


def derived(tab):
    """lines 285-298"""
    return ({k: tab[k][:, 0] / (tab[k][:, 0] + tab[k][:, 2] + 1e-4) for k in TABLES},
            {k: tab[k][:, 0] / (tab[k][:, 0] + tab[k][:, 3] + 1e-4) for k in TABLES})


def non_degenerate(tab):
    """the condition the golden has to meet for the tables to test anything: None, or a text saying what is missing"""
    for k in ("atom_type", "atom_charge", "bond_type"):
        n = tab[k].shape[0]
        if 2 * (tab[k][:, 2] > 0).sum() < n or 2 * (tab[k][:, 3] > 0).sum() < n:
            return "%s: fewer than half the classes have fp > 0 and fn > 0" % k
    for k in ("atom_detection", "bond_detection"):
        n = tab[k].shape[0]
        if (tab[k][:, 3] > 0).sum() < 3 or 2 * (tab[k][:, 0] > 0).sum() < n:
            return "%s: fewer than three classes with fn > 0 or fewer than half with tp > 0" % k
    return None
