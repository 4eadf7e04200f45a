"""Oracle (test infrastructure, not product): the candidate extraction of the reference's inference drivers under either omega
rule, one image at a time.

  "raw"    img2smiles2.py:113-191 -- exactly oracle.decode_oracle.extract (the call is handed on): every bin whose RAW omega logit
           is non-zero is tried (img2smiles2.py:139).
  "peaks"  img2smiles3.py:75-81,135-172 (img2smiles.py:139 walks the same mask): every bin of the circular 3-tap omega peak mask

               mask[k] = v[k] == max(v[(k+59)%60], v[k], v[(k+1)%60]) and v[k] > -1

           is tried (`bond_omega_img2[:, x, y].nonzero()`, img2smiles3.py:140); there is no v != 0 test, so a peak whose logit is
           exactly 0 is a candidate.

Under both rules a tried bin survives unless the opposite direction wins (oracle.decode_oracle._keep_bin: `<` for bins 0..29,
`<=` for bins 30..59), and the atom list is the same.  Pinned by tests/golden/decode3_128.npz (exec of the reference text by
tests/golden/make_golden_decode3.py).
"""
import torch

from oracle import decode_oracle

RULES = ("raw", "peaks")


def omega_peak_bins(v):
    """v: the 60 raw omega logits of one pixel (Python floats) -> the bins of the mask of img2smiles3.py:75-81, ascending"""
    n = len(v)
    return [k for k in range(n) if v[k] == max(v[(k + n - 1) % n], v[k], v[(k + 1) % n]) and v[k] > -1]


def tried_bins(v, omega_rule):
    if omega_rule == "raw":
        return [k for k in range(len(v)) if v[k] != 0.0]
    if omega_rule == "peaks":
        return omega_peak_bins(v)
    raise ValueError("omega_rule must be one of %s, got %r" % (RULES, omega_rule))


def kept_bins(v, omega_rule):
    """the bins of one bond peak that become candidates, ascending"""
    return [k for k in tried_bins(v, omega_rule) if decode_oracle._keep_bin(v, k)]


def extract(atom_mask, bond_mask, types, charges, hs, btypes, rho_abs, omega, omega_rule="raw", max_bond_peaks=None):
    """the arguments and the result of oracle.decode_oracle.extract; max_bond_peaks: expand only the first so many bond peaks in
    raster order (the extractor's 4096-peak limit)"""
    if omega_rule not in RULES:
        raise ValueError("omega_rule must be one of %s, got %r" % (RULES, omega_rule))
    if omega_rule == "raw" and max_bond_peaks is None:
        return decode_oracle.extract(atom_mask, bond_mask, types, charges, hs, btypes, rho_abs, omega)
    atoms, _, _ = decode_oracle.extract(atom_mask, torch.zeros_like(bond_mask), types, charges, hs, btypes, rho_abs, omega)
    h, w = bond_mask.shape
    bt = btypes.reshape(6, 60, h, w)
    bonds, rhos = [], []
    peaks = bond_mask.nonzero(as_tuple=False).tolist()
    for x, y in peaks if max_bond_peaks is None else peaks[:max_bond_peaks]:
        v = omega[:, x, y].tolist()
        for k in kept_bins(v, omega_rule):
            bonds.append([x, y, k, int(bt[:, k, x, y].argmax().item())])
            rhos.append(rho_abs[k, x, y].item())
    return atoms, torch.tensor(bonds, dtype=torch.int64).reshape(-1, 4), torch.tensor(rhos, dtype=torch.float32)


def hand_made_maps(gold, size):
    """the 8 head maps [B, c, size, size] (f32, heads [1, 14, 3, 2, 1, 360, 60, 60]) of the hand-made cases of decode3_128.npz:
    centre logits -5 except 3 at the stored atom / bond peaks, every other map 0 except the stored rows at those peaks.  The
    positions all lie inside 32 x 32, so any size >= 32 gives the same lists."""
    bpos, apos = gold["hand_bond_pos"], gold["hand_atom_pos"]
    B = int(max(bpos[:, 0].max(), apos[:, 0].max())) + 1
    lg = [torch.zeros((B, c, size, size), dtype=torch.float32) for c in (1, 14, 3, 2, 1, 360, 60, 60)]
    lg[0].fill_(-5.0)
    lg[4].fill_(-5.0)
    for i, (b, x, y) in enumerate(apos.tolist()):
        lg[0][b, 0, x, y] = 3.0
        lg[1][b, :, x, y] = torch.from_numpy(gold["hand_atom_types"][i])
        lg[2][b, :, x, y] = torch.from_numpy(gold["hand_atom_charges"][i])
        lg[3][b, :, x, y] = torch.from_numpy(gold["hand_atom_hs"][i])
    for i, (b, x, y) in enumerate(bpos.tolist()):
        lg[4][b, 0, x, y] = 3.0
        lg[5][b, :, x, y] = torch.from_numpy(gold["hand_btypes"][i])
        lg[6][b, :, x, y] = torch.from_numpy(gold["hand_rho"][i])
        lg[7][b, :, x, y] = torch.from_numpy(gold["hand_omega"][i])
    return lg
