"""Test infrastructure, not product: what the tests of the decoder's stages (assemble, molblock, graphscore, graphsim) share --
hand-made molecule rows on the device, graph records as arrays, the molecule a score oracle reads, the trained fixture."""
import os
import sys

import numpy as np

EMPTY, TRUNCATED = 1, 2          # L.MOL_EMPTY, L.MOL_TRUNCATED


class Heads:
    """the least of a model the InferenceRunner constructor reads before its refusals"""
    heads = [1, 14, 3, 2, 1, 360, 60, 60]


def upload_molecules(mols, cap_atoms, cap_mol_bonds, junk_bond, device="cuda"):
    """mols: dict(atoms [(x, y, vocabulary index, charge)], bonds [(end 1, end 2 (1-based), order)], truncated) or None per image ->
    (mol_counts, mol_atoms, mol_bonds) device tensors of the assembler's layout.  The rows past the counts hold junk that must
    not be read: 7 in every atom word, `junk_bond` in every bond row."""
    import torch
    B = len(mols)
    cnt = np.zeros((B, 4), dtype=np.int32)
    atoms = np.full((B, cap_atoms, 5), 7, dtype=np.int32)
    bonds = np.zeros((B, cap_mol_bonds, 4), dtype=np.int32)
    bonds[:] = junk_bond
    for b, m in enumerate(mols):
        if m is None:
            cnt[b] = (3, 2, 0, EMPTY | TRUNCATED)                   # (an empty image counts nothing but `none`, whatever else it says)
            continue
        cnt[b] = (len(m["atoms"]), len(m["bonds"]), 0, TRUNCATED if m["truncated"] else 0)
        for i, a in enumerate(m["atoms"]):
            atoms[b, i] = (a[0], a[1], a[2], a[3], -1)
        for i, q in enumerate(m["bonds"]):
            bonds[b, i] = (q[0], q[1], q[2], i)
    return tuple(torch.from_numpy(t).to(device) for t in (cnt, atoms, bonds))


def records_to_numpy(recs):
    """[(atoms, bonds)] as lists of tuples -> the int32 [n, 4] / [m, 3] arrays GraphRecords.load takes"""
    return [(np.array(a, dtype=np.int32).reshape(-1, 4), np.array(q, dtype=np.int32).reshape(-1, 3)) for a, q in recs]


def for_score_oracle(m, symbols):
    """a molecule as upload_molecules takes it -> the dict graphscore_oracle.score reads (symbols: its ATOM_SYMBOLS)"""
    if m is None:
        return None
    return dict(symbols=[symbols[a[2]] for a in m["atoms"]], charges=[a[3] for a in m["atoms"]],
                positions=[[a[0], a[1]] for a in m["atoms"]], bonds=[[q[0], q[1]] for q in m["bonds"]],
                orders=[q[2] for q in m["bonds"]], truncated=m["truncated"])


def trained_unet(golden_dir, device="cuda"):
    """the frozen trained fixture (tests/golden/trained_unet_state.npz): the network is fully convolutional, so the weights
    trained at 384 x 384 load at any input size"""
    sys.path.insert(0, golden_dir)
    from make_trained_fixture import unpack_state
    from abcnet_amd.unet import UNet
    m = UNet(1, Heads.heads, dtype="bf16", dropout_p=0.2)
    m.load_state_dict(unpack_state(os.path.join(golden_dir, "trained_unet_state.npz")))
    return m.to(device).eval()


def fake_desc(struct, pointers, defaults, **fields):
    """a descriptor for the launchers' refusals: `pointers` hold an address that is never dereferenced (the refusals come first),
    the other fields `defaults`, then `fields`"""
    d = struct()
    for f in pointers:
        setattr(d, f, 256)
    for k, v in dict(defaults, **fields).items():
        setattr(d, k, v)
    return d


MOL_POINTERS = ("mol_counts", "mol_atoms", "mol_bonds")
SCORE_POINTERS = MOL_POINTERS + ("rec_atoms", "rec_bonds", "rec_counts", "rows", "totals")
SCORE_DEFAULTS = dict(B=2, cap_atoms=512, cap_mol_bonds=2048, max_atoms=256, max_bonds=256)
ASSEMBLE_POINTERS = MOL_POINTERS + ("counts", "atoms", "bonds", "bond_rho", "trig", "mol_implh", "work")
ASSEMBLE_DEFAULTS = dict(B=2, cap_atoms=512, cap_bonds=16384, cap_mol_bonds=2048)


def filled_unet(dtype="fp32", device="cuda", **kw):
    """unet.py with the oracle's seeded state (oracle.unet_oracle.filled_state)"""
    from abcnet_amd.unet import UNet
    from oracle import unet_oracle as uo
    m = UNet(1, uo.HEADS, dtype=dtype, **kw)
    m.load_state_dict(uo.filled_state("unet", 1, uo.HEADS, seed=0))
    return m.to(device)


def assemble_golden(golden_dir):
    """[(name, arrays)] of tests/golden/assemble_128.npz, the reference's own assembly and mol block of every rule's case"""
    g = np.load(os.path.join(golden_dir, "assemble_128.npz"))
    out = []
    for ci in range(int(g["n"])):
        p = "c%d_" % ci
        out.append((str(g[p + "name"]), {k[len(p):]: g[k] for k in g.files if k.startswith(p)}))
    return out
