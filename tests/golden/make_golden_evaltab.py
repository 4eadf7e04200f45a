"""Golden of the evaluation tables (needs the reference checkout: it reads the reference's text; what it writes travels, the
reference does not).

  evaltab_128.npz   test_accuracy.py:33-38 (the five zeroed tables) and the text of :105-269 (inference NMS, the per-class loops,
                    the 17 meters) executed with the reference's meter.AverageMeter on synthetic_targets(2, 128, seed=3) and
                    evaltab_oracle.confusable_logits(..., seed=19).  Stored: the five tables and sum / count of every meter after
                    ONE batch.  The inputs are regenerated from the seeds, not stored.

The generator refuses to write a degenerate golden (evaltab_oracle.non_degenerate: tables with empty fp / fn columns test nothing).

    python tests/golden/make_golden_evaltab.py
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import PRED_NAMES, REF, TGT_NAMES, slice_text  # noqa: E402

import evaltab_oracle as eo  # noqa: E402
from abcnet_amd.synthetic import synthetic_targets  # noqa: E402

SCRIPT = os.path.join(REF, "test_accuracy.py")
TABLE_VARS = {"atom_detection": "atom_detection_metrics", "atom_type": "atom_type_metrics", "atom_charge": "atom_charge_metrics",
              "bond_detection": "bond_detection_metrics", "bond_type": "bond_type_metrics"}


def main():
    from meter import AverageMeter
    tg = synthetic_targets(2, 128, seed=3)
    preds = eo.confusable_logits(tg, seed=19)
    ns = {"torch": torch, "np": np}
    for n, v in zip(PRED_NAMES, preds):
        ns[n] = v
    for n, v in zip(TGT_NAMES, tg):
        ns[n] = v
    text = slice_text(SCRIPT, 105, 269)
    names = []
    for m in re.finditer(r"(train_\w+)\.update", text):
        if m.group(1) not in names:
            names.append(m.group(1))
    for n in names:
        ns[n] = AverageMeter()
    exec(slice_text(SCRIPT, 33, 38), ns)
    exec(text, ns)
    tab = {k: np.asarray(ns[v], dtype=np.float64) for k, v in TABLE_VARS.items()}
    for k in eo.TABLES:
        print(k)
        print(tab[k].astype(np.int64))
    why = eo.non_degenerate(tab)
    assert why is None, "degenerate golden, tune confusable_logits: " + why
    res = dict(tab)
    res["names"] = np.array(names)
    res["sum"] = np.array([float(ns[n].sum) for n in names])
    res["count"] = np.array([float(ns[n].count) for n in names])
    np.savez(os.path.join(HERE, "evaltab_128.npz"), **res)
    for n in names:
        print("  %-36s sum %14.6f count %12.4f" % (n, ns[n].sum, ns[n].count))
    print("wrote evaltab_128.npz")


if __name__ == "__main__":
    main()
