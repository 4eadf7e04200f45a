"""The device graph assembly (csrc/assemble.hip, ops.GraphAssembler) measured on config 5, one process: b64 @ 512 x 512, the
frozen trained fixture (tests/golden/trained_unet_state.npz) on drawn_molecules(seed 777).

  step     InferenceRunner.step() with extract=True against assemble=True (graph replay, alternating blocks, median device time)
  launch   abc_assemble_graphs alone on the lists of that batch (device events around back-to-back launches, so launch gaps
           count; the kernel's own time: run --parts launch under `rocprofv3 --kernel-trace --stats --`)
  host     candidates() against molecules(): wall time of the D2H copies plus the host work, and the bytes each copies
  graphs   the share of images whose assembled graph equals the drawn annotation: the same bonded atoms (head-map cell, element,
           charge) and the same bonds (unordered pair of cells, order; a wedge counts as order 5 / 6).  Reported, not a test.
           Beside it the device's own count: InferenceRunner(score_graphs=True) at radius 0 (csrc/graph_score.hip), one sync.
  score    abc_graph_score_update alone (as `launch`), and InferenceRunner.step() with assemble=True, evaluate=True against the
           same with score_graphs=True (as `step`); the targets of both come from the annotation records (sparse rasteriser)
  similarity  abc_graph_similarity_update alone beside abc_graph_score_update (as `launch`), the fixture's mean environment similarity,
           refine_equal and exact (InferenceRunner(score_graphs=True, score_similarity=True), one step, csrc/graph_sim.hip), and
           step() with score_graphs=True against the same with score_similarity=True as well (as `step`)

  identity abc_graph_identity_update alone beside abc_graph_similarity_update (as `launch`; with --parent-lib also the parent commit's
           build of the launch on the same descriptor); the fixture's verified `same` between
           `exact` and `refine_equal` with `undecided` and the largest levels / tries / rounds of an image
           (InferenceRunner(score_graphs=True, score_similarity=True, score_identity=True), one step, csrc/graph_ident.hip); and
           step() with score_graphs=True, score_similarity=True against the same with score_identity=True as well (as `text`'s
           step: eight alternated blocks, the spread of the block medians)

  text     the mol block text written on the device (csrc/molblock.hip, InferenceRunner(molblocks=True)): molecules() plus
           Molecule.molblock() of every image on the host against molblocks() (wall time per batch, alternated, median of the
           repetitions), abc_write_molblocks alone (its two launches, as `launch`), the bytes molblocks() copies, and step() with
           assemble=True against the same with molblocks=True (as `step`, with the spread of the block medians)

  smiles   a SMILES string written on the device (csrc/smiles.hip, InferenceRunner(smiles=True)): molecules() plus
           Molecule.smiles() of every image on the host against smiles() (as `text`), abc_write_smiles alone beside
           abc_write_molblocks (two launches each, as `launch`), the bytes smiles() copies, and step() with assemble=True against the
           same with molblocks=True and with smiles=True (as `text`'s step)
           --stereo: a fourth runner with smiles_stereo=True beside the plain one -- abc_write_smiles_stereo alone beside
           abc_write_smiles, its step against the plain stage's in the same alternated blocks, smiles() against
           Molecule.smiles(stereo=True), and what became of the fixture's wedge rows (stereo_stats: wedge rows, marked, flat,
           unqualified)
           --double-bonds: the double-bond marks (abc_write_smiles_ez, InferenceRunner(smiles=True, smiles_double_bonds=True)) under
           BOTH omega rules in this one process -- the two launches of the four instantiations (plain, tetrahedral, double bonds,
           both) alone and alternated, the step of the four forms in the same alternated blocks, smiles() against
           Molecule.smiles(double_bonds=True, ...), and what became of the fixture's class-2 rows (double_bond_stats: marked, flat,
           ring, twin, and the rows that are no candidate).  profiles/r23_smiles_double_bonds.md is one run
           --canonical: the canonical atom order (csrc/graph_canon.hip, InferenceRunner(smiles=True, smiles_canonical=True)) under
           BOTH omega rules in this one process -- abc_canonical_order alone beside abc_write_smiles, the step with the stage
           against the same step without it (alternated blocks), the images left UNDECIDED, the largest work of an image, smiles()
           against Molecule.smiles(canonical=True), and how many of the 64 strings equal the canonical string of their annotation
           (the identity's `same` of profiles/r15_identity.md, position-free: 0 under raw, 7 under peaks).  Writes what it measured
           to profiles/r21_canonical.md
           --isomeric: the canonical ISOMERIC form (csrc/stereo.hip and the stereo instantiation of csrc/graph_canon.hip,
           InferenceRunner(smiles=True, smiles_isomeric=True)) under BOTH omega rules in this one process -- abc_perceive_stereo
           alone, abc_canonical_order_stereo beside abc_canonical_order, the writer with both marks and with the double-bond marks
           alone (with --parent-lib also the parent commit's build of the plain and the stereo search, the perception and both
           writers, each on the same descriptor), the step with and without, the fixture's stereo elements and third-key counters, smiles() against
           Molecule.smiles(isomeric=True).  Writes what it measured to profiles/r24_isomeric.md

  aromatize (or --aromatize beside other parts): the aromaticity perception (csrc/aromatic.hip, InferenceRunner(aromatize=True)) under
           BOTH omega rules in this one process -- abc_perceive_aromatic alone, on the molecule rows and on the graph records, beside
           abc_canonical_order; the evaluating step with every graph stage with and without it (alternated blocks); the pass's stats;
           the identity's exact / same / refine_equal and the count of canonical strings equal to their annotation's, with and
           without it.  Writes what it measured to profiles/r22_aromatic.md

  --records-from-smiles (beside any parts, or with --parts none): the SMILES reader (csrc/smiles_read.hip, InferenceRunner.load_smiles) --
           every annotation record of the fixture written as a string by the host writer and loaded as a string: abc_read_smiles
           alone, decode.parse_smiles + GraphRecords.load on the host for the same strings, load + step with load_smiles against the
           same with load_graphs, the identity and similarity totals both ways (they must be equal).  profiles/r26_smiles_reader.md

  --omega-rule {raw,peaks}: the extractor's candidate rule of every runner built here (InferenceRunner(omega_rule=...): "raw" is
           img2smiles2.py:139, "peaks" img2smiles.py:139 / img2smiles3.py:140); `graphs` and `score` then also report the candidates
           per image and abc_extract_peaks alone (as `launch`).  profiles/r09_omega_rule.md is one run per rule.

One JSON line per measurement, each naming the rule.

    python profiles/tools/assemble_step.py [--steps 40] [--warmup 5] [--parts step,launch,host,graphs,score,similarity,identity,text,smiles] [--omega-rule raw] [--stereo] [--double-bonds] [--canonical] [--aromatize] [--isomeric] [--parent-lib PATH] [--records-from-smiles]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import torch  # noqa: E402

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.infer import InferenceRunner  # noqa: E402
from abcnet_amd.synthetic import drawn_molecules  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402

HEADS = [1, 14, 3, 2, 1, 360, 60, 60]
B, S = 64, 512
RULE = "raw"      # --omega-rule


def emit(d):
    print(json.dumps(dict(d, omega_rule=RULE)), flush=True)


def model():
    from make_trained_fixture import unpack_state
    m = UNet(1, HEADS, dtype="bf16", dropout_p=0.2)
    m.load_state_dict(unpack_state(os.path.join(ROOT, "tests", "golden", "trained_unet_state.npz")))
    return m.to("cuda").eval()


def runners(m, x):
    out = {}
    for name, kw in (("extract=True", dict(extract=True)), ("assemble=True", dict(assemble=True))):
        r = InferenceRunner(m, B, S, S, use_graph=True, omega_rule=RULE, **kw)
        r.load_batch(x.to("cuda"))
        out[name] = r
    return out


def scoring_runners(m, x, notes, similarity=False, identity=False):
    """the evaluating step without and with the score after assembly (similarity: and with the environment similarity on top;
    identity: and with the verified isomorphism test on top of that); targets drawn once from the annotation records"""
    from abcnet_amd.raster import TargetRasterizer, parse_graph, parse_record
    recs = [parse_record(a, b, h=S // 4) for a, b in notes]
    graphs = [parse_graph(a, b, h=S // 4) for a, b in notes]
    out = {}
    forms = [("assemble+evaluate", {}), ("assemble+evaluate+score", dict(score_graphs=True, score_radius=0))]
    if similarity:
        forms.append(("assemble+evaluate+score+similarity", dict(score_graphs=True, score_radius=0, score_similarity=True)))
    if identity:
        forms.append(("assemble+evaluate+score+similarity+identity",
                      dict(score_graphs=True, score_radius=0, score_similarity=True, score_identity=True)))
    for name, kw in forms:
        r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, evaluate=True, omega_rule=RULE, **kw)
        rz = TargetRasterizer(B, S // 4, targets=r.targets, sparse=True)
        r.use_sparse_targets(rz)
        rz.load(recs)
        rz.run()
        r.load_batch(x.to("cuda"))
        if r.records is not None:
            r.load_graphs(graphs)
        out[name] = r
    return out


def part_step(rs, steps, warmup, part="step", diff=("assemble=True", "extract=True"), diff_name="assemble_minus_extract_ms"):
    for r in rs.values():
        for _ in range(warmup):
            r.step()
    torch.cuda.synchronize()
    times = {k: [] for k in rs}
    for blk in range(4):
        for name, r in (rs.items() if blk % 2 == 0 else reversed(list(rs.items()))):
            ev = []
            for _ in range(steps // 4):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r.step()
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            times[name] += [a.elapsed_time(b) for a, b in ev]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        emit({"part": part, "form": k, "batch": B, "size": S, "steps": len(v), "ms_per_step_median": round(med[k], 4),
              "ms_min": round(min(v), 4), "img_per_s": round(B * 1000.0 / med[k], 1)})
    emit({"part": part, diff_name: round(med[diff[0]] - med[diff[1]], 4)})


def launch_us(run, iters=200):
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / iters


def part_launch(r, iters=200):
    us = launch_us(r.assembler.run, iters)
    cnt = r.extractor.counts.cpu()
    emit({"part": "launch", "batch": B, "us_per_launch": round(us, 2),
          "atoms_per_image_mean": round(float(cnt[:, 1].float().mean()), 1), "candidates_per_image_mean": round(float(cnt[:, 3].float().mean()), 1),
          "candidates_per_image_max": int(cnt[:, 3].max()),
          "method": "device events around %d back-to-back launches (launch gaps included)" % iters})


def part_host(r, reps=20):
    def timed(f):
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = f()
        return (time.perf_counter() - t0) * 1000 / reps, out
    t_c, lists = timed(r.candidates)
    t_m, mols = timed(r.molecules)
    cnt, mc = r.extractor.counts.cpu(), r.assembler.mol_counts.cpu()
    na, nb = int(cnt[:, 1].max()), int(cnt[:, 3].max())
    bytes_c = B * (16 + na * 20 + nb * 16 + nb * 4)
    bytes_m = B * (16 + int(mc[:, 0].max()) * 20 + int(mc[:, 1].max()) * 16 + int(mc[:, 2].max()) * 4)
    t0 = time.perf_counter()
    blocks = [m.molblock() for m in mols if m is not None]
    t_b = (time.perf_counter() - t0) * 1000
    emit({"part": "host", "candidates_ms": round(t_c, 3), "molecules_ms": round(t_m, 3), "candidates_d2h_bytes": bytes_c,
          "molecules_d2h_bytes": bytes_m, "molblock_ms_per_batch": round(t_b, 3), "molecules": len(blocks),
          "note": "wall time of one call per batch of %d: D2H copies + host list building, one host thread" % B})


def step_blocks(rs, steps, warmup, part):
    """the step of every runner of rs in eight alternated blocks: one line per form with the median of its block medians and their
    spread; returns {form: that median}"""
    for q in rs.values():
        for _ in range(warmup):
            q.step()
    torch.cuda.synchronize()
    blocks = {k: [] for k in rs}
    for blk in range(8):
        for name, q in (rs.items() if blk % 2 == 0 else reversed(list(rs.items()))):
            ev = []
            for _ in range(max(steps // 8, 1)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                q.step()
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            blocks[name].append(statistics.median(a.elapsed_time(b) for a, b in ev))
    med = {k: statistics.median(v) for k, v in blocks.items()}
    for k, v in blocks.items():
        emit({"part": part, "what": "step", "form": k, "batch": B, "size": S, "blocks": len(v), "ms_per_step_median": round(med[k], 4),
              "block_medians_min_max": [round(min(v), 4), round(max(v), 4)],
              "block_spread_percent": round(100 * (max(v) - min(v)) / med[k], 3)})
    return med


def part_text(m, x, steps, warmup, reps=30, iters=200):
    rs = {}
    for name, kw in (("assemble=True", dict(assemble=True)), ("assemble+molblocks", dict(assemble=True, molblocks=True))):
        r = InferenceRunner(m, B, S, S, use_graph=True, omega_rule=RULE, **kw)
        r.load_batch(x.to("cuda"))
        for _ in range(2):
            r.step()
        rs[name] = r
    torch.cuda.synchronize()
    r = rs["assemble+molblocks"]

    def host():
        return [mol.molblock() if mol is not None else None for mol in r.molecules()]
    want, got = host(), r.molblocks()
    wall = {"host": [], "device": []}
    for _ in range(reps):
        for name, f in (("host", host), ("device", r.molblocks)):
            t0 = time.perf_counter()
            f()
            wall[name].append((time.perf_counter() - t0) * 1000)
    off = r.texter.index.cpu().tolist()[:B + 1]
    med = {k: statistics.median(v) for k, v in wall.items()}
    emit({"part": "text", "what": "host", "batch": B, "molecules_plus_molblock_ms": round(med["host"], 4),
          "molecules_plus_molblock_ms_min": round(min(wall["host"]), 4), "molblocks_ms": round(med["device"], 4),
          "molblocks_ms_min": round(min(wall["device"]), 4), "ratio": round(med["host"] / med["device"], 2), "equal": got == want,
          "molecules": sum(t is not None for t in got), "text_bytes": off[B], "index_bytes": 4 * (2 * B + 1),
          "cap_text": r.texter.cap_text, "note": "wall time of one call per batch of %d, %d alternated repetitions, one host thread" % (B, reps)})
    us = [launch_us(r.texter.run, iters) for _ in range(3)]
    emit({"part": "text", "what": "launch", "batch": B, "us_per_call": [round(v, 2) for v in us],
          "assemble_us_per_launch": round(launch_us(r.assembler.run, iters), 2),
          "method": "device events around %d back-to-back calls of two launches each (launch gaps included)" % iters})
    # the step: block medians of each form as well, for the block-to-block spread
    med = step_blocks(rs, steps, warmup, "text")
    emit({"part": "text", "molblocks_minus_assemble_ms": round(med["assemble+molblocks"] - med["assemble=True"], 4)})


def part_smiles(m, x, steps, warmup, reps=30, iters=200, stereo=False):
    rs = {}
    forms = [("assemble=True", dict(assemble=True)), ("assemble+molblocks", dict(assemble=True, molblocks=True)),
             ("assemble+smiles", dict(assemble=True, smiles=True))]
    if stereo:
        forms.append(("assemble+smiles+stereo", dict(assemble=True, smiles=True, smiles_stereo=True)))
    for name, kw in forms:
        r = InferenceRunner(m, B, S, S, use_graph=True, omega_rule=RULE, **kw)
        r.load_batch(x.to("cuda"))
        for _ in range(2):
            r.step()
        rs[name] = r
    torch.cuda.synchronize()
    r = rs["assemble+smiles"]

    def host():
        return [mol.smiles() if mol is not None else None for mol in r.molecules()]
    status = r.smiler.status()
    refused = sum(bool(s & ~3) for s in status)      # (BAD_ROW, OVERFLOW, RING_LIMIT: smiles() would raise)
    wall = {"host": [], "device": []}
    if not refused:
        want, got = host(), r.smiles()
        for _ in range(reps):
            for name, f in (("host", host), ("device", r.smiles)):
                t0 = time.perf_counter()
                f()
                wall[name].append((time.perf_counter() - t0) * 1000)
        off = r.smiler.index.cpu().tolist()[:B + 1]
        mc = r.assembler.mol_counts.cpu()
        med = {k: statistics.median(v) for k, v in wall.items()}
        emit({"part": "smiles", "what": "host", "batch": B, "molecules_plus_smiles_ms": round(med["host"], 4),
              "molecules_plus_smiles_ms_min": round(min(wall["host"]), 4), "smiles_ms": round(med["device"], 4),
              "smiles_ms_min": round(min(wall["device"]), 4), "ratio": round(med["host"] / med["device"], 2), "equal": got == want,
              "molecules": sum(t is not None for t in got), "text_bytes": off[B], "index_bytes": 4 * (2 * B + 1),
              "longest_text": max(len(t) for t in got if t is not None), "cap_text": r.smiler.cap_text,
              "molecule_atoms_mean_max": [round(float(mc[:, 0].float().mean()), 1), int(mc[:, 0].max())],
              "molecule_bonds_mean_max": [round(float(mc[:, 1].float().mean()), 1), int(mc[:, 1].max())],
              "note": "wall time of one call per batch of %d, %d alternated repetitions, one host thread" % (B, reps)})
    else:
        emit({"part": "smiles", "what": "host", "refused_images": refused, "status": status})
    us = [(launch_us(r.smiler.run, iters), launch_us(rs["assemble+molblocks"].texter.run, iters)) for _ in range(3)]
    emit({"part": "smiles", "what": "launch", "batch": B, "us_per_call": [round(a, 2) for a, _ in us],
          "molblocks_us_per_call": [round(b, 2) for _, b in us], "assemble_us_per_launch": round(launch_us(r.assembler.run, iters), 2),
          "method": "device events around %d back-to-back calls of two launches each (launch gaps included)" % iters})
    if stereo:
        part_smiles_stereo(rs["assemble+smiles+stereo"], r, reps, iters)
    med = step_blocks(rs, steps, warmup, "smiles")
    out = {"part": "smiles", "smiles_minus_assemble_ms": round(med["assemble+smiles"] - med["assemble=True"], 4),
           "molblocks_minus_assemble_ms": round(med["assemble+molblocks"] - med["assemble=True"], 4)}
    if stereo:
        out["stereo_minus_smiles_ms"] = round(med["assemble+smiles+stereo"] - med["assemble+smiles"], 4)
    emit(out)


def part_smiles_stereo(r, plain, reps, iters):
    """the stereo form beside the plain one: the fixture's wedge rows and what became of them, smiles() against the host form,
    the two launches of each alternated"""
    status = r.smiler.status()
    refused = sum(bool(s & ~3) for s in status)
    st = r.stereo_stats()
    mols = r.molecules()
    out = {"part": "smiles", "what": "stereo fixture", "batch": B, "refused_images": refused,
           "images_with_a_wedge_row": sum(row[3] > 0 for row in st["rows"]), "images_with_a_mark": sum(row[0] > 0 for row in st["rows"]),
           "wedge_rows_per_image_max": max(row[3] for row in st["rows"])}
    out.update({k: st[k] for k in ("wedge_rows", "marked", "flat", "unqualified")})
    if not refused:
        def host():
            return [mol.smiles(stereo=True) if mol is not None else None for mol in mols]
        want, got = host(), r.smiles()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r.smiles()
            wall.append((time.perf_counter() - t0) * 1000)
        out.update({"equal": got == want, "texts_that_differ_from_plain": sum(a != b for a, b in zip(got, plain.smiles())),
                    "smiles_ms": round(statistics.median(wall), 4), "text_bytes": r.smiler.index.cpu().tolist()[B]})
    emit(out)
    us = [(launch_us(r.smiler.run, iters), launch_us(plain.smiler.run, iters)) for _ in range(3)]
    emit({"part": "smiles", "what": "stereo launch", "batch": B, "stereo_us_per_call": [round(a, 2) for a, _ in us],
          "plain_us_per_call": [round(b, 2) for _, b in us],
          "method": "device events around %d back-to-back calls of two launches each (launch gaps included), alternated" % iters})


def part_smiles_double_bonds(m, x, steps, warmup, iters=200):
    """--double-bonds: both omega rules in this process; the four instantiations of the writer side by side"""
    global RULE
    kept = RULE
    forms = [("plain", {}), ("tetrahedral", dict(smiles_stereo=True)), ("double_bonds", dict(smiles_double_bonds=True)),
             ("both", dict(smiles_stereo=True, smiles_double_bonds=True))]
    for RULE in ("raw", "peaks"):
        rs = {}
        for name, kw in forms:
            r = InferenceRunner(m, B, S, S, use_graph=True, omega_rule=RULE, assemble=True, smiles=True, **kw)
            r.load_batch(x.to("cuda"))
            for _ in range(2):
                r.step()
            rs[name] = r
        torch.cuda.synchronize()
        mols = rs["plain"].molecules()
        refused = sum(bool(s & ~3) for s in rs["both"].smiler.status())
        st = rs["double_bonds"].double_bond_stats()
        out = {"part": "smiles", "what": "double-bond fixture", "batch": B, "refused_images": refused,
               "class_2_rows": sum(sum(o == 2 for o in mol.orders) for mol in mols if mol is not None),
               "images_with_a_class_2_row": sum(any(o == 2 for o in mol.orders) for mol in mols if mol is not None),
               "images_with_a_mark": sum(row[0] > 0 for row in st["rows"]), "stats_of_both": {k: rs["both"].double_bond_stats()[k] for k in st if k != "rows"}}
        out.update({k: st[k] for k in ("marked", "flat", "ring", "twin")})
        out["not_a_candidate"] = out["class_2_rows"] - sum(st[k] for k in ("marked", "flat", "ring", "twin"))
        if not refused:
            got = {k: r.smiles() for k, r in rs.items()}
            want = {k: [None if mol is None else mol.smiles(stereo="smiles_stereo" in kw, double_bonds="smiles_double_bonds" in kw) for mol in mols]
                    for k, kw in forms}
            out.update({"equal": got == want, "texts_that_differ_from_plain": sum(a != b for a, b in zip(got["double_bonds"], got["plain"])),
                        "symbols": sum(t.count("/") + t.count("\\") for t in got["double_bonds"] if t is not None),
                        "text_bytes": {k: r.smiler.index.cpu().tolist()[B] for k, r in rs.items()}})
        emit(out)
        us = [{k: round(launch_us(r.smiler.run, iters), 2) for k, r in rs.items()} for _ in range(3)]
        emit({"part": "smiles", "what": "double-bond launch", "batch": B, "us_per_call": {k: [u[k] for u in us] for k in rs},
              "method": "device events around %d back-to-back calls of two launches each (launch gaps included), the four alternated" % iters})
        med = step_blocks({"assemble+smiles " + k: r for k, r in rs.items()}, steps, warmup, "smiles")
        emit({"part": "smiles", "what": "double-bond step",
              "double_bonds_minus_plain_ms": round(med["assemble+smiles double_bonds"] - med["assemble+smiles plain"], 4),
              "both_minus_tetrahedral_ms": round(med["assemble+smiles both"] - med["assemble+smiles tetrahedral"], 4)})
        del rs
    RULE = kept


def part_smiles_canonical(m, x, notes, steps, warmup, reps=30, iters=200):
    """--canonical: both omega rules in this process; the lines are printed and written to profiles/r21_canonical.md"""
    import numpy as np
    from abcnet_amd import _lib as L
    from abcnet_amd.decode import ATOM_SYMBOLS, Molecule
    from abcnet_amd.raster import parse_graph
    global RULE
    lines, keep = [], RULE

    def note(d):
        lines.append(dict(d, omega_rule=RULE))
        emit(d)
    # the canonical string of every annotation: its graph record as a molecule (only bonded atoms, no listed atom)
    want = []
    for atoms_s, bonds_s in notes:
        a, q = parse_graph(atoms_s, bonds_s, h=S // 4)
        T = sorted({int(e) for row in q for e in row[:2]})
        num = {t: k + 1 for k, t in enumerate(T)}
        mol = Molecule([ATOM_SYMBOLS[int(a[t][2])] if 0 <= int(a[t][2]) < 14 else "?" for t in T], [int(a[t][3]) for t in T], [0] * len(T),
                       [[int(a[t][0]), int(a[t][1])] for t in T], [[num[int(i)], num[int(j)]] for i, j, _ in q], [int(o) for _, _, o in q], [])
        try:
            want.append(mol.smiles(canonical=True))
        except ValueError:
            want.append(None)
    for RULE in ("raw", "peaks"):
        rs = {}
        for name, kw in (("assemble+smiles", dict(smiles=True)), ("assemble+smiles+canonical", dict(smiles=True, smiles_canonical=True))):
            r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, omega_rule=RULE, **kw)
            r.load_batch(x.to("cuda"))
            for _ in range(2):
                r.step()
            rs[name] = r
        torch.cuda.synchronize()
        r, plain = rs["assemble+smiles+canonical"], rs["assemble+smiles"]
        st = r.canonical_stats()
        refused = sum(bool(s & ~3) for s in r.smiler.status())
        mols = r.molecules()
        out = {"part": "smiles", "what": "canonical fixture", "batch": B, "refused_images": refused,
               "undecided_images": int(((st["status"] & L.CANON_UNDECIDED) != 0).sum()), "collision_images": int(((st["status"] & L.CANON_COLLISION) != 0).sum()),
               "molecules": sum(mol is not None for mol in mols), "molecules_with_a_listed_atom": sum(mol is not None and bool(mol.implicit_hs) for mol in mols)}
        out.update({c + "_max": int(st[c].max()) for c in ("leaves", "tries", "rounds", "levels_max", "automorphisms")})
        if not refused:
            got = r.smiles()
            host = [mol.smiles(canonical=True) if mol is not None else None for mol in mols]
            wall = []
            for _ in range(reps):
                t0 = time.perf_counter()
                r.smiles()
                wall.append((time.perf_counter() - t0) * 1000)
            out.update({"equal_to_host_form": got == host, "texts_that_differ_from_plain": sum(a != b for a, b in zip(got, plain.smiles())),
                        "distinct_strings": len({t for t in got if t is not None}),
                        "strings_equal_to_their_annotation": sum(t is not None and t == w for t, w in zip(got, want)),
                        # (the identity does not read the implicit-H list; the canonical order does: the same count without it)
                        "equal_to_their_annotation_without_listed_atoms": sum(
                            mol is not None and Molecule(mol.symbols, mol.charges, mol.hs, mol.positions, mol.bonds, mol.orders, []).smiles(canonical=True) == w
                            for mol, w in zip(mols, want)),
                        "smiles_ms": round(statistics.median(wall), 4)})
        note(out)
        us = [(launch_us(r.canonicalizer.run, iters), launch_us(r.smiler.run, iters), launch_us(plain.smiler.run, iters)) for _ in range(3)]
        note({"part": "smiles", "what": "canonical launch", "batch": B, "canonical_order_us_per_launch": [round(a, 2) for a, _, _ in us],
              "smiles_on_canonical_rows_us_per_call": [round(b, 2) for _, b, _ in us], "plain_smiles_us_per_call": [round(c, 2) for _, _, c in us],
              "method": "device events around %d back-to-back calls (launch gaps included), alternated" % iters})
        med = step_blocks(rs, steps, warmup, "smiles")
        note({"part": "smiles", "what": "canonical step", "ms_per_step": {k: round(v, 4) for k, v in med.items()},
              "canonical_minus_smiles_ms": round(med["assemble+smiles+canonical"] - med["assemble+smiles"], 4)})
        del rs, r, plain
    RULE = keep
    path = os.path.join(ROOT, "profiles", "r21_canonical.md")
    with open(path, "w") as f:
        f.write("# The canonical atom order on the trained fixture (b%d @ %d x %d, drawn_molecules(seed 777))\n\n" % (B, S, S))
        f.write("`python profiles/tools/assemble_step.py --parts smiles --canonical`, one process, both omega rules; the step with the stage "
                "against the same commit's step without it, the launch beside the plain SMILES stage's two launches.  "
                "`strings_equal_to_their_annotation` is position-free; a listed implicit hydrogen is part of this graph and not of the identity's, "
                "so it is `equal_to_their_annotation_without_listed_atoms` that is the identity's `same` of r15_identity.md (0 under raw, 7 under "
                "peaks).\n\n```\n")
        for d in lines:
            f.write(json.dumps(d) + "\n")
        f.write("```\n")
    print("wrote", path, flush=True)


def part_smiles_isomeric(m, x, steps, warmup, parent_lib=None, iters=200):
    """--isomeric: the canonical ISOMERIC form (InferenceRunner(smiles=True, smiles_isomeric=True)) under both omega rules in this one
    process -- the perception launch alone, the stereo search launch beside the plain one, the writer with both marks and with the
    double-bond marks alone (with --parent-lib each also of the parent commit's library on the same descriptor, alternated), the step with the form against the plain canonical step and
    the step without either; the stereo elements of the fixture, the third key's counters and how many strings equal their host
    form.  The lines are printed and written to profiles/r24_isomeric.md (whose section on instruction counts is kept)."""
    import ctypes as C
    from abcnet_amd import _lib as L
    from abcnet_amd.contract import current_stream
    from abcnet_amd.ops import SmilesWriter
    global RULE
    lines, keep = [], RULE
    parent = None
    if parent_lib:
        parent = C.CDLL(parent_lib)
        parent.abc_canonical_order.restype, parent.abc_canonical_order.argtypes = C.c_int, [C.POINTER(L.CanonDesc), C.c_void_p]
        parent.abc_canonical_order_stereo.restype, parent.abc_canonical_order_stereo.argtypes = C.c_int, [C.POINTER(L.CanonStereoDesc), C.c_void_p]
        parent.abc_perceive_stereo.restype, parent.abc_perceive_stereo.argtypes = C.c_int, [C.POINTER(L.StereoDesc), C.c_void_p]
        parent.abc_write_smiles_ez.restype, parent.abc_write_smiles_ez.argtypes = C.c_int, [C.POINTER(L.SmilesEzDesc), C.c_void_p]

    def note(d):
        lines.append(dict(d, omega_rule=RULE))
        emit(d)
    for RULE in ("raw", "peaks"):
        rs = {}
        for name, kw in (("assemble+smiles", dict(smiles=True)), ("assemble+smiles+canonical", dict(smiles=True, smiles_canonical=True)),
                         ("assemble+smiles+isomeric", dict(smiles=True, smiles_isomeric=True))):
            r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, omega_rule=RULE, **kw)
            r.load_batch(x.to("cuda"))
            for _ in range(2):
                r.step()
            rs[name] = r
        torch.cuda.synchronize()
        r, plain = rs["assemble+smiles+isomeric"], rs["assemble+smiles+canonical"]
        st, search, el = r.canonical_stats(), r.stereo_search(), r.canonicalizer.perceiver.stats()
        refused = sum(bool(s & ~3) for s in r.smiler.status())
        mols = r.molecules()
        out = {"part": "smiles", "what": "isomeric fixture", "batch": B, "refused_images": refused, "molecules": sum(mol is not None for mol in mols),
               "marked_centres": int(el["centres"].sum()), "marked_double_bonds": int(el["double_bonds"].sum()), "flat": int(el["flat"].sum()),
               "images_with_a_marked_element": int(((el["centres"] + el["double_bonds"]) > 0).sum()),
               "images_with_unequal_words": int((search["unequal"] > 0).sum()), "stereo_improvements": int(search["improved"].sum()),
               "stereo_automorphisms": int(search["automorphisms"].sum()),
               "undecided_images": int(((st["status"] & L.CANON_UNDECIDED) != 0).sum()), "collision_images": int(((st["status"] & L.CANON_COLLISION) != 0).sum()),
               "keys_equal_the_plain_search": bool((r.canonical_keys() == plain.canonical_keys()).all())}
        out.update({c + "_max": int(st[c].max()) for c in ("leaves", "tries", "rounds")})
        if not refused:
            got = r.smiles()
            host = [mol.smiles(isomeric=True) if mol is not None else None for mol in mols]
            out.update({"strings_equal_to_host_form": sum(a == b for a, b in zip(got, host)), "strings": len(got),
                        "texts_that_differ_from_plain_canonical": sum(a != b for a, b in zip(got, plain.smiles()))})
        note(out)
        cz = r.canonicalizer

        def order_only():
            L.check(cz.lib.abc_canonical_order_stereo(C.byref(cz.d), current_stream()), "canonical_order_stereo")

        def parent_order():
            L.check(parent.abc_canonical_order(C.byref(plain.canonicalizer.d), current_stream()), "parent canonical_order")
        # the writer with the double-bond marks alone, on the same canonical rows (the runner's own writes both marks); of the parent
        # commit's build the perception and both of these writers, each on this build's descriptor
        ez = SmilesWriter(cz.rows(), double_bonds=True)

        def of_parent(entry, d):
            return (lambda: L.check(getattr(parent, entry)(C.byref(d), current_stream()), "parent " + entry)) if parent else None
        beside = {"canonical_order_stereo": of_parent("abc_canonical_order_stereo", cz.d),
                  "perceive_stereo": of_parent("abc_perceive_stereo", cz.perceiver.d), "smiles_both_marks": of_parent("abc_write_smiles_ez", r.smiler.d),
                  "smiles_double_bonds": of_parent("abc_write_smiles_ez", ez.d)}
        us = [(launch_us(cz.perceiver.run, iters), launch_us(order_only, iters), launch_us(plain.canonicalizer.run, iters),
               launch_us(parent_order, iters) if parent else None, launch_us(r.smiler.run, iters), launch_us(plain.smiler.run, iters),
               launch_us(ez.run, iters), {k: launch_us(f, iters) for k, f in beside.items() if f}) for _ in range(3)]
        note({"part": "smiles", "what": "isomeric launch", "batch": B, "perceive_stereo_us_per_launch": [round(u[0], 2) for u in us],
              "canonical_order_stereo_us_per_launch": [round(u[1], 2) for u in us], "canonical_order_us_per_launch": [round(u[2], 2) for u in us],
              "parent_build_canonical_order_us_per_launch": [round(u[3], 2) for u in us] if parent else None,
              "smiles_both_marks_us_per_call": [round(u[4], 2) for u in us], "plain_smiles_on_canonical_rows_us_per_call": [round(u[5], 2) for u in us],
              "smiles_double_bonds_us_per_call": [round(u[6], 2) for u in us],
              "parent_build_us": {k: [round(u[7][k], 2) for u in us] for k in us[0][7]} if parent else None,
              "method": "device events around %d back-to-back calls (launch gaps included), alternated" % iters})
        med = step_blocks(rs, steps, warmup, "smiles")
        note({"part": "smiles", "what": "isomeric step", "ms_per_step": {k: round(v, 4) for k, v in med.items()},
              "isomeric_minus_canonical_ms": round(med["assemble+smiles+isomeric"] - med["assemble+smiles+canonical"], 4),
              "isomeric_minus_smiles_ms": round(med["assemble+smiles+isomeric"] - med["assemble+smiles"], 4)})
        del rs, r, plain, cz, ez
    RULE = keep
    path = os.path.join(ROOT, "profiles", "r24_isomeric.md")
    marker, tail = "## Instruction counts", ""
    if os.path.exists(path):
        old = open(path).read()
        tail = old[old.index(marker):] if marker in old else ""
    with open(path, "w") as f:
        f.write("# The canonical isomeric form on the trained fixture (b%d @ %d x %d, drawn_molecules(seed 777))\n\n" % (B, S, S))
        f.write("`python profiles/tools/assemble_step.py --parts smiles --isomeric [--parent-lib <the parent commit's library>]`, one process, both "
                "omega rules.  The perception launch alone; the stereo search launch beside the plain one of this build and of the parent "
                "commit's build on the same descriptor (56 / 62 us in r21_canonical.md); the step with the form against the plain canonical "
                "step and the step without either, in alternated blocks.\n\n```\n")
        for d in lines:
            f.write(json.dumps(d) + "\n")
        f.write("```\n\n" + tail)
    print("wrote", path, flush=True)


def part_aromatize(m, x, notes, steps, warmup, iters=200):
    """--aromatize: both omega rules in this process -- abc_perceive_aromatic alone (molecule rows, then graph records) beside
    abc_canonical_order, the evaluating step with every graph stage without and with aromatize=True (alternated blocks), the stats
    of the pass, GraphIdentity's exact / same / refine_equal without and with it, and how many canonical strings equal their
    annotation's.  The lines are printed and written to profiles/r22_aromatic.md"""
    from abcnet_amd import _lib as L
    from abcnet_amd.decode import ATOM_SYMBOLS, Molecule
    from abcnet_amd.raster import TargetRasterizer, parse_graph, parse_record
    global RULE
    lines, keep = [], RULE

    def note(d):
        lines.append(dict(d, omega_rule=RULE))
        emit(d)
    recs = [parse_record(a, b, h=S // 4) for a, b in notes]
    graphs = [parse_graph(a, b, h=S // 4) for a, b in notes]
    # the annotation of every image as a molecule (only bonded atoms, no listed atom), as --canonical builds it
    annotated = []
    for a, q in graphs:
        T = sorted({int(e) for row in q for e in row[:2]})
        num = {t: k + 1 for k, t in enumerate(T)}
        annotated.append(Molecule([ATOM_SYMBOLS[int(a[t][2])] if 0 <= int(a[t][2]) < 14 else "?" for t in T], [int(a[t][3]) for t in T], [0] * len(T),
                                  [[int(a[t][0]), int(a[t][1])] for t in T], [[num[int(i)], num[int(j)]] for i, j, _ in q], [int(o) for _, _, o in q], []))

    def text(mol, aromatize):
        try:
            return None if mol is None else mol.smiles(canonical=True, aromatize=aromatize)
        except ValueError:
            return None
    for RULE in ("raw", "peaks"):
        rs = {}
        for name, kw in (("graph stages", {}), ("graph stages+aromatize", dict(aromatize=True))):
            r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, evaluate=True, smiles=True, smiles_canonical=True, score_graphs=True,
                                score_radius=0, score_similarity=True, score_identity=True, omega_rule=RULE, **kw)
            rz = TargetRasterizer(B, S // 4, targets=r.targets, sparse=True)
            r.use_sparse_targets(rz)
            rz.load(recs)
            rz.run()
            r.load_batch(x.to("cuda"))
            r.load_graphs(graphs)
            for _ in range(2):
                r.step()
            rs[name] = r
        torch.cuda.synchronize()
        r, plain = rs["graph stages+aromatize"], rs["graph stages"]
        st_mol, st_rec = r.aromatic_stats()
        out = {"part": "aromatize", "what": "fixture", "batch": B}
        for side, st in (("molecules", st_mol), ("records", st_rec)):
            out[side] = {c: int(st[c].sum()) for c in L.AROMATIC_COLUMNS[1:]}
            out[side]["images_with_an_aromatic_cycle"] = int((st["aromatic"] > 0).sum())
            out[side]["cycles_max"] = int(st["cycles"].max())
        for name, q in (("without", plain), ("with", r)):
            q.reset_evaluation()
            q.step()
            ev = q.evaluation()
            mols = q.molecules()
            got = q.smiles()
            out[name] = {"exact": ev["molecules"]["exact"], "same": ev["identity"]["same"], "undecided": ev["identity"]["undecided"],
                         "refine_equal": ev["similarity"]["refine_equal"], "similarity": round(ev["similarity"]["similarity"], 4),
                         "equal_to_host_form": got == [text(mol, name == "with") for mol in mols],
                         "strings_equal_to_their_annotation": sum(t is not None and t == text(w, name == "with") for t, w in zip(got, annotated))}
            q.reset_evaluation()
        note(out)
        us = [(launch_us(r.aromatizer.run, iters), launch_us(r.record_aromatizer.run, iters), launch_us(r.canonicalizer.run, iters),
               launch_us(plain.canonicalizer.run, iters)) for _ in range(3)]
        note({"part": "aromatize", "what": "launch", "batch": B, "perceive_molecules_us_per_launch": [round(u[0], 2) for u in us],
              "perceive_records_us_per_launch": [round(u[1], 2) for u in us], "canonical_order_on_perceived_rows_us_per_launch": [round(u[2], 2) for u in us],
              "canonical_order_us_per_launch": [round(u[3], 2) for u in us],
              "method": "device events around %d back-to-back calls (launch gaps included), alternated" % iters})
        for q in rs.values():
            q.reset_evaluation()
        med = step_blocks(rs, steps, warmup, "aromatize")
        note({"part": "aromatize", "what": "step", "ms_per_step": {k: round(v, 4) for k, v in med.items()},
              "aromatize_minus_plain_ms": round(med["graph stages+aromatize"] - med["graph stages"], 4)})
        del rs, r, plain
    RULE = keep
    path = os.path.join(ROOT, "profiles", "r22_aromatic.md")
    with open(path, "w") as f:
        f.write("# Aromaticity perception on the trained fixture (b%d @ %d x %d, drawn_molecules(seed 777))\n\n" % (B, S, S))
        f.write("`python profiles/tools/assemble_step.py --parts aromatize --aromatize`, one process, both omega rules.  The step is the "
                "evaluating step with every graph stage (canonical SMILES, score, similarity, identity), with the two perception launches "
                "against the same commit's step without them in alternated blocks; the launches stand beside abc_canonical_order's "
                "(56 / 62 us in r21_canonical.md).  `without` / `with` are the scores and the canonical strings of the same batch "
                "without and with `aromatize`; the stats are sums over the batch.\n\n```\n")
        for d in lines:
            f.write(json.dumps(d) + "\n")
        f.write("```\n\n")
        fixtures = [d for d in lines if d["what"] == "fixture"]
        f.write("Images with an aromatic cycle (%s): molecules %s, records %s of %d.  The scores and strings %s.\n"
                % (" / ".join(d["omega_rule"] for d in fixtures), " / ".join(str(d["molecules"]["images_with_an_aromatic_cycle"]) for d in fixtures),
                   " / ".join(str(d["records"]["images_with_an_aromatic_cycle"]) for d in fixtures), B,
                   "are the same with and without the stage: this fixture has no molecule the perception decides"
                   if all(d["with"] == d["without"] for d in fixtures) else "differ with the stage"))
    print("wrote", path, flush=True)


def annotated_graph(atoms_s, bonds_s):
    atoms = {}
    for a in atoms_s.strip(";").split(";"):
        el, rest = a.split(":")
        f = [int(v) for v in rest.split(",")]
        atoms[(f[0] // 4, f[1] // 4)] = (el, f[2])
    pts = list(atoms)

    def nearest(x, y):
        return min(pts, key=lambda p: (p[0] - x / 4) ** 2 + (p[1] - y / 4) ** 2)
    bonds = set()
    for b in bonds_s.strip(";").split(";") if bonds_s else []:
        order, rest = b.split(":")
        x, y, dx, dy, stereo, _direction = (int(v) for v in rest.split(","))
        code = {1: 5, 6: 6}.get(stereo, int(order))
        bonds.add((frozenset((nearest(x - dx, y - dy), nearest(x + dx, y + dy))), code))
    shown = set().union(*[set(p) for p, _ in bonds]) if bonds else set()
    return {(p,) + atoms[p] for p in shown}, bonds


def part_score(rs, steps, warmup, iters=200):
    r = rs["assemble+evaluate+score"]
    sc = r.scorer
    keep = sc.totals.clone()
    us = launch_us(sc.run, iters)
    us_asm, us_eval = launch_us(r.assembler.run, iters), launch_us(r.evaluator.run, iters)
    us_ext = launch_us(r.extractor.run, iters)
    sc.totals.copy_(keep)
    r.reset_evaluation()
    mc, rc = r.assembler.mol_counts.cpu(), r.records.staging.dev["cnt"].cpu()
    emit({"part": "score", "what": "launch", "batch": B, "us_per_launch": round(us, 2), "assemble_us_per_launch": round(us_asm, 2),
          "extract_us_per_launch": round(us_ext, 2),
          "evaluation_us_per_call": round(us_eval, 2), "molecule_atoms_mean": round(float(mc[:, 0].float().mean()), 1),
          "molecule_bonds_mean": round(float(mc[:, 1].float().mean()), 1), "record_atoms_mean": round(float(rc[0].float().mean()), 1),
          "record_bonds_mean": round(float(rc[1].float().mean()), 1),
          "method": "device events around %d back-to-back launches (launch gaps included)" % iters})
    part_step(rs, steps, warmup, part="score", diff=("assemble+evaluate+score", "assemble+evaluate"), diff_name="score_minus_plain_ms")


def part_similarity(rs, steps, warmup, iters=200):
    from abcnet_amd._lib import GRAPH_SIM_COLUMNS
    r = rs["assemble+evaluate+score+similarity"]
    sim, sc = r.similarity, r.scorer
    keep = sim.totals.clone(), sc.totals.clone()
    us = [(launch_us(sim.run, iters), launch_us(sc.run, iters)) for _ in range(3)]      # the two launches alternated, three figures each
    sim.totals.copy_(keep[0])
    sc.totals.copy_(keep[1])
    emit({"part": "similarity", "what": "launch", "batch": B, "us_per_launch": [round(a, 2) for a, _ in us],
          "graph_score_us_per_launch": [round(b, 2) for _, b in us],
          "method": "device events around %d back-to-back launches (launch gaps included)" % iters})
    r.reset_evaluation()
    r.step()
    ev = r.evaluation()
    res = ev["similarity"]
    out = {"part": "similarity", "what": "fixture", "images": res["counted"], "similarity": round(res["similarity"], 4),
           "exact": ev["molecules"]["exact"]}
    out.update({k: res[k] for k in GRAPH_SIM_COLUMNS[1:]})
    rows = res["rows"]
    q = sorted(rows[:, GRAPH_SIM_COLUMNS.index("dice_q20")].tolist())
    out["dice_min_median_max"] = [round(v / float(1 << 20), 4) for v in (q[0], q[len(q) // 2], q[-1])]
    emit(out)
    r.reset_evaluation()
    pair = {k: rs[k] for k in ("assemble+evaluate+score", "assemble+evaluate+score+similarity")}
    part_step(pair, steps, warmup, part="similarity", diff=("assemble+evaluate+score+similarity", "assemble+evaluate+score"),
              diff_name="similarity_minus_score_ms")


def part_identity(rs, steps, warmup, parent_lib=None, iters=200):
    import ctypes as C
    from abcnet_amd import _lib as L
    from abcnet_amd._lib import GRAPH_IDENT_COLUMNS
    from abcnet_amd.contract import current_stream
    with_id, without = "assemble+evaluate+score+similarity+identity", "assemble+evaluate+score+similarity"
    r = rs[with_id]
    ident, sim = r.identity, r.similarity
    keep = ident.totals.clone(), sim.totals.clone()
    parent_run = None
    if parent_lib:      # the parent commit's build of the launch on this build's descriptor, alternated with this build's
        parent = C.CDLL(parent_lib)
        parent.abc_graph_identity_update.restype, parent.abc_graph_identity_update.argtypes = C.c_int, [C.POINTER(type(ident.d)), C.c_void_p]

        def parent_run():
            L.check(parent.abc_graph_identity_update(C.byref(ident.d), current_stream()), "parent graph_identity_update")
    us = [(launch_us(ident.run, iters), launch_us(sim.run, iters), launch_us(parent_run, iters) if parent_run else None)
          for _ in range(3)]      # the launches alternated, three figures each
    ident.totals.copy_(keep[0])
    sim.totals.copy_(keep[1])
    emit({"part": "identity", "what": "launch", "batch": B, "us_per_launch": [round(a, 2) for a, _, _ in us],
          "graph_similarity_us_per_launch": [round(b, 2) for _, b, _ in us],
          "parent_build_us_per_launch": [round(c, 2) for _, _, c in us] if parent_run else None,
          "method": "device events around %d back-to-back launches (launch gaps included)" % iters})
    r.reset_evaluation()
    r.step()
    ev = r.evaluation()
    res = ev["identity"]
    out = {"part": "identity", "what": "fixture", "images": res["counted"], "exact": ev["molecules"]["exact"],
           "refine_equal": ev["similarity"]["refine_equal"], "dice_one": ev["similarity"]["dice_one"]}
    out.update({k: res[k] for k in GRAPH_IDENT_COLUMNS[1:]})
    rows = res["rows"]
    out.update({"max_" + k: int(rows[:, GRAPH_IDENT_COLUMNS.index(k)].max()) for k in ("levels", "tries", "backtracks", "rounds")})
    out["ordered"] = bool(out["exact"] <= res["same"] <= out["refine_equal"])
    emit(out)
    r.reset_evaluation()
    pair = {k: rs[k] for k in (without, with_id)}
    med = step_blocks(pair, steps, warmup, "identity")
    emit({"part": "identity", "identity_minus_similarity_ms": round(med[with_id] - med[without], 4)})


def part_graphs_device(r):
    """the device's count of the same thing: the scorer's rows of the last step (radius 0)"""
    from abcnet_amd._lib import GRAPH_SCORE_COLUMNS
    r.reset_evaluation()
    r.step()
    res = r.evaluation()["molecules"]
    cnt = r.extractor.counts.cpu()
    out = {"part": "graphs", "where": "device", "images": res["counted"], "candidates_per_image_mean": round(float(cnt[:, 3].float().mean()), 1),
           "candidates_per_image_max": int(cnt[:, 3].max()), "bond_peaks_per_image_mean": round(float(cnt[:, 2].float().mean()), 1)}
    out.update({k: res[k] for k in GRAPH_SCORE_COLUMNS[1:]})
    out["share"] = round(res["share_exact"], 4)
    emit(out)


def part_graphs(r, notes):
    mols = r.molecules()
    same = atoms_same = bonds_same = 0
    for m, (a, b) in zip(mols, notes):
        want_a, want_b = annotated_graph(a, b)
        if m is None:
            continue
        got_a = {(tuple(p), s, c) for p, s, c in zip(m.positions, m.symbols, m.charges)}
        got_b = {(frozenset((tuple(m.positions[i - 1]), tuple(m.positions[j - 1]))), o) for (i, j), o in zip(m.bonds, m.orders)}
        atoms_same += got_a == want_a
        bonds_same += got_b == want_b
        same += got_a == want_a and got_b == want_b
    emit({"part": "graphs", "where": "host", "images": len(mols), "none": sum(m is None for m in mols), "truncated": sum(bool(m and m.truncated) for m in mols),
          "graph_equals_annotation": same, "atoms_equal": atoms_same, "bonds_equal": bonds_same,
          "share": round(same / len(mols), 4)})


def part_records_from_smiles(m, x, notes, steps, warmup, iters=200, reps=20):
    """--records-from-smiles: every annotation record of the fixture written as a string (the host writer on the record's graph) and
    loaded as a string -- abc_read_smiles alone, decode.parse_smiles + GraphRecords.load for the same strings, the evaluating step
    fed by load_smiles against the same step fed by load_graphs, and the identity and similarity totals both ways (equal, or it raises)"""
    import ctypes as C
    from abcnet_amd.decode import ATOM_SYMBOLS, Molecule, parse_smiles
    from abcnet_amd.raster import parse_graph
    strings = []
    for a, q in (parse_graph(a, b, h=S // 4) for a, b in notes):
        mol = Molecule([ATOM_SYMBOLS[max(int(t), 0)] for t in a[:, 2]], a[:, 3].tolist(), [0] * len(a), a[:, :2].tolist(),
                       [[int(i) + 1, int(j) + 1] for i, j, _ in q], q[:, 2].tolist(), [])
        strings.append(mol.smiles())
    rs = {}
    for name in ("load_graphs", "load_smiles"):
        r = InferenceRunner(m, B, S, S, use_graph=True, assemble=True, evaluate=True, score_similarity=True, score_identity=True, omega_rule=RULE)
        r.load_batch(x.to("cuda"))
        rs[name] = r
    parsed = lambda: [parse_smiles(t, 256, 256)[1:] for t in strings]
    loads = {"load_graphs": lambda: rs["load_graphs"].load_graphs(parsed()), "load_smiles": lambda: rs["load_smiles"].load_smiles(strings)}
    totals = {}
    for name, r in rs.items():
        loads[name]()
        for _ in range(2):
            r.step()
        r.reset_evaluation()
        r.step()
        ev = r.evaluation()
        totals[name] = {key: {k: (v.tolist() if k == "rows" else v) for k, v in ev[key].items() if k == "rows" or v == v} for key in ("identity", "similarity")}
    if totals["load_graphs"] != totals["load_smiles"]:
        raise SystemExit("the scores differ between load_graphs and load_smiles")
    reader = rs["load_smiles"].smiles_reader
    status = reader.status()
    emit({"part": "records_from_smiles", "what": "fixture", "strings": len(strings), "bytes": sum(len(t) for t in strings),
          "bytes_max": max(len(t) for t in strings), "read": status.count(0), "stats": {k: v for k, v in reader.stats().items() if k != "rows"},
          "identity": {k: v for k, v in totals["load_smiles"]["identity"].items() if k != "rows"},
          "similarity": {k: v for k, v in totals["load_smiles"]["similarity"].items() if k != "rows"}, "equal_both_ways": True})
    lib, st = reader.lib, torch.cuda.current_stream().cuda_stream
    us = [launch_us(lambda: lib.abc_read_smiles(C.byref(reader.d), st), iters) for _ in range(3)]

    def wall(f):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(out), 4)

    emit({"part": "records_from_smiles", "what": "load", "batch": B, "read_smiles_us_per_launch": [round(u, 2) for u in us],
          "host_parse_smiles_ms": wall(parsed), "host_parse_smiles_plus_records_load_ms": wall(loads["load_graphs"]),
          "load_smiles_ms": wall(loads["load_smiles"]),
          "method": "device events around %d back-to-back launches; wall clock between device syncs, median of %d" % (iters, reps)})
    for r in rs.values():
        for _ in range(warmup):
            r.step()
    times = {k: [] for k in rs}
    for blk in range(4):
        for name in (list(rs) if blk % 2 == 0 else list(rs)[::-1]):
            for _ in range(steps // 4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loads[name]()
                rs[name].step()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        emit({"part": "records_from_smiles", "what": "load + step", "form": k, "batch": B, "size": S, "steps": len(v),
              "ms_median": round(med[k], 4), "ms_min": round(min(v), 4)})
    emit({"part": "records_from_smiles", "load_smiles_minus_load_graphs_ms": round(med["load_smiles"] - med["load_graphs"], 4)})
    # the launch at the limit: 64 copies of one 4096-byte string, four shapes (the bracket walk and the ring lanes are the one-lane phases)
    from abcnet_amd.contract import GraphRecords
    from abcnet_amd.ops import SmilesReader
    long_reader = SmilesReader(GraphRecords(B, 4096, 4096, "cuda"))
    shapes = {"chain": "C" * 4096, "nested 1365 deep": "C(" * 1365 + "C" + ")" * 1365, "1023 branches": "C(C)" * 1023 + "CCCC",
              "819 rings": "C1CC1" * 819 + "C", "longest fixture string": max(strings, key=len)}
    for name, text in shapes.items():
        long_reader.load([text] * B)
        us = [launch_us(lambda: lib.abc_read_smiles(C.byref(long_reader.d), st), iters) for _ in range(3)]
        emit({"part": "records_from_smiles", "what": "launch at the limit", "shape": name, "bytes": len(text), "batch": B,
              "read": long_reader.status().count(0), "read_smiles_us_per_launch": [round(u, 2) for u in us]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parts", default="step,launch,host,graphs")
    ap.add_argument("--omega-rule", choices=("raw", "peaks"), default="raw")
    ap.add_argument("--stereo", action="store_true", help="the smiles part: the stereo form beside the plain one")
    ap.add_argument("--double-bonds", action="store_true", help="the smiles part: the double-bond marks, the four instantiations under both omega rules")
    ap.add_argument("--canonical", action="store_true", help="the smiles part: the canonical atom order, under both omega rules")
    ap.add_argument("--aromatize", action="store_true", help="the aromatize part: the aromaticity perception, under both omega rules")
    ap.add_argument("--isomeric", action="store_true", help="the smiles part: the canonical isomeric form, under both omega rules")
    ap.add_argument("--parent-lib", default=None, help="--isomeric, --parts identity: a libabcnet_hip.so of the parent commit, whose launches are timed beside this build's")
    ap.add_argument("--records-from-smiles", action="store_true",
                    help="the annotation records as SMILES strings: abc_read_smiles and load_smiles against parse_smiles + load_graphs")
    a = ap.parse_args()
    global RULE
    RULE = a.omega_rule
    parts = a.parts.split(",")
    m = model()
    x, notes = drawn_molecules(B, S, seed=777)
    rs = runners(m, x) if set(parts) & {"step", "launch", "host"} else {}
    ss = {}
    if set(parts) & {"graphs", "score", "similarity", "identity"}:
        ss = scoring_runners(m, x, notes, similarity=bool(set(parts) & {"similarity", "identity"}), identity="identity" in parts)
    for r in list(rs.values()) + list(ss.values()):
        for _ in range(2):
            r.step()
    torch.cuda.synchronize()
    if "step" in parts:
        part_step(rs, a.steps, a.warmup)
    if "launch" in parts:
        part_launch(rs["assemble=True"])
    if "host" in parts:
        part_host(rs["assemble=True"])
    if "graphs" in parts:
        part_graphs(ss["assemble+evaluate+score"], notes)
        part_graphs_device(ss["assemble+evaluate+score"])
    if "score" in parts:
        part_score({k: ss[k] for k in ("assemble+evaluate", "assemble+evaluate+score")}, a.steps, a.warmup)
    if "similarity" in parts:
        part_similarity(ss, a.steps, a.warmup)
    if "identity" in parts:
        part_identity(ss, a.steps, a.warmup, parent_lib=a.parent_lib)
    if "text" in parts:
        part_text(m, x, a.steps, a.warmup)
    if "smiles" in parts:
        part_smiles(m, x, a.steps, a.warmup, stereo=a.stereo)
        if a.double_bonds:
            part_smiles_double_bonds(m, x, a.steps, a.warmup)
        if a.canonical:
            part_smiles_canonical(m, x, notes, a.steps, a.warmup)
        if a.isomeric:
            part_smiles_isomeric(m, x, a.steps, a.warmup, parent_lib=a.parent_lib)
    if a.aromatize or "aromatize" in parts:
        part_aromatize(m, x, notes, a.steps, a.warmup)
    if a.records_from_smiles:
        part_records_from_smiles(m, x, notes, a.steps, a.warmup)


if __name__ == "__main__":
    main()
