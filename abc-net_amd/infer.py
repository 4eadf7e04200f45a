"""Inference harness: the heat-map half of /root/reference/src/img2smiles2.py:42-79 on the HIP kernels.

    model.eval(); preds = model(imgs)                       (img2smiles2.py:56-59)
    3x3 / circular 3-tap local-max masks, |rho|             (img2smiles2.py:61-79)

One step = eval-mode forward (running-statistics BatchNorm folded into the convolution weights / biases at refresh()
time, activations in the convolutions' epilogues, no dropout) + the peak-NMS kernel, on a batch already resident in HBM, replayed from one hipGraph.  The weights do not change between
steps, so re-packing them and deriving the eval-mode BatchNorm coefficients happens in `refresh()`, not in the step;
call it again after `load_state_dict`.  The step ends with the four mask / |rho| maps the decoder reads; opt-in, the candidate
lists (extract=True, img2smiles2.py:113-191), the assembled molecules (assemble=True, :193-311) and their mol block text
(molblocks=True, generate_smiles.py:18-105) in the same graph, and a SMILES string of each by this project's own text rule
(smiles=True).  RDKit (generate_smiles.py:115-119) and its canonical SMILES are out of scope.

evaluate=True makes the step the loop body of the reference's src/test_accuracy.py:94-269 as well: the targets of the batch sit in
static device buffers and one more launch sequence after the NMS (ops.EvalTables) adds the batch to the per-class tables and the 17
inference-flavour meters; evaluation() reads them.  score_graphs=True adds the score after assembly to that step: the assembled
molecules against the annotated graphs (ops.GraphScore), accumulated like the tables; score_similarity=True the graded,
position-free score of the same molecules (ops.GraphSimilarity); score_identity=True the certain, position-free answer whether they ARE
the annotated molecules (ops.GraphIdentity).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .contract import HEADS, GraphRecords, alloc_targets, check_sparse_rasterizer, current_stream, refuse_dense_targets, resolve_device


# the optional stages behind the NMS in launch order, each under the constructor flag that builds it
STAGES = {"extractor": "extract", "assembler": "assemble", "canonicalizer": "smiles_canonical", "texter": "molblocks", "smiler": "smiles", "scorer": "score_graphs",
          "similarity": "score_similarity", "identity": "score_identity", "evaluator": "evaluate",
          "aromatizer": "aromatize", "record_aromatizer": "aromatize"}
# ... but for the aromaticity perception, which is launched right behind the assembler (the molecule rows, then the staged graph
# records): every stage after it but the mol block text reads what it wrote
LAUNCH_AFTER = {"aromatizer": "assembler", "record_aromatizer": "aromatizer"}


def launch_order():
    """the attributes of STAGES in the order their stages are launched"""
    order = [attr for attr in STAGES if attr not in LAUNCH_AFTER]
    for attr, before in LAUNCH_AFTER.items():
        order.insert(order.index(before) + 1, attr)
    return order


# flags, the flags each of them needs, what the refusal says the flag does -- checked in this order, then FLAG_REFUSED in its order
FLAG_NEEDS = ((("score_graphs", "score_similarity", "score_identity"), ("assemble", "evaluate"), "scores the assembled molecules of an evaluating step"),
              (("molblocks", "smiles"), ("assemble",), "writes the text of the assembled molecules of the step"),
              (("aromatize",), ("assemble",), "perceives the aromatic rings of the assembled molecules of the step"),
              (("smiles_stereo", "smiles_double_bonds", "smiles_canonical"), ("smiles",), "is a form of the SMILES stage"))
# a flag, the flag it is refused with, why
FLAG_REFUSED = (("smiles_canonical", "smiles_double_bonds", "a text with double-bond marks on the canonical order would not be canonical "
                 "(the drawn geometry is not in the invariant)"),
                ("smiles_canonical", "smiles_stereo", "a stereo text on the canonical order would not be canonical (wedge ownership and the "
                 "drawn geometry are not in the invariant)"))


def check_flags(flags):
    """ValueError for the first rule of FLAG_NEEDS, then of FLAG_REFUSED, that the constructor flags {name: value} break"""
    for group, needs, does in FLAG_NEEDS:
        for flag in group:
            if flags[flag] and not all(flags[n] for n in needs):
                raise ValueError("InferenceRunner(%s=True) %s: it needs %s" % (flag, does, " and ".join(n + "=True" for n in needs)))
    for flag, other, why in FLAG_REFUSED:
        if flags[flag] and flags[other]:
            raise ValueError("InferenceRunner(%s=True, %s=True): %s" % (flag, other, why))


def check_isomeric(smiles_isomeric, flags):
    """the rule of smiles_isomeric, a flag of its own beside FLAG_NEEDS / FLAG_REFUSED (checked after check_flags): ValueError unless
    smiles=True, and with each of the three forms it already is"""
    if not smiles_isomeric:
        return
    if not flags["smiles"]:
        raise ValueError("InferenceRunner(smiles_isomeric=True) is a form of the SMILES stage: it needs smiles=True")
    for other in ("smiles_canonical", "smiles_stereo", "smiles_double_bonds"):
        if flags[other]:
            raise ValueError("InferenceRunner(smiles_isomeric=True, %s=True): smiles_isomeric already is smiles_canonical, smiles_stereo "
                             "and smiles_double_bonds in one -- the canonical order that reads the stereo elements; give it alone" % other)


class InferenceRunner:
    def __init__(self, model, batch, height, width, use_graph=True, device=None, extract=False, cap_atoms=512, cap_bonds=16384,
                 fold_bn=None, fp8=False, fp8_margin=1.0, guards=False, heads_epilogue=False, nms_in_heads=True, decode=False,
                 assemble=False, cap_mol_bonds=None, evaluate=False, score_graphs=False, score_radius=0, omega_rule="raw",
                 score_similarity=False, molblocks=False, score_identity=False, smiles=False, smiles_stereo=False,
                 smiles_canonical=False, aromatize=False, smiles_double_bonds=False, smiles_isomeric=False):
        """fp8: the e4m3 form of the BatchNorm-folded graph (unet.py, bf16 model): the 128-channel 3x3 convolutions at the output
        resolution on the block-scaled MFMA over e4m3 activations and weights (Engine(fp8=True)); the per-tensor activation scales
        are calibrated on the FIRST batch loaded (calibrate(); again on demand) by running the bf16 folded graph on it.
        fold_bn: run the eval graph with every BatchNorm folded into the convolution in front of it and the activation in
        that convolution's epilogue (weights re-packed times gamma / sqrt(running_var + eps) by refresh()); default: on for
        unet.py, off for unet2.py (whose CBAM reads the un-activated BatchNorm output)
        nms_in_heads (default): |rho| and the omega-bin mask of img2smiles2.py:73-79 are second outputs of the heads' 1x1 kernel
        (computed from the very f32 values it stores: bit-identical to the NMS kernel reading the maps back), and the NMS kernel
        does the two 3x3 centre masks only -- 0.5 GB less read per batch of 64; False: the round-3 plan
        decode (with nms_in_heads): store only what the decoder of img2smiles2.py:104-191 reads -- |rho| instead of the raw rho map
        (:73) and, for the 360 bond-type planes, their six-way arg max per omega bin as a uint8 map (:71,112; .btype_idx);
        .logits[5] and .logits[6] are then None, the candidate lists (extract=True) are unchanged bit for bit.  1.7 GB less written
        per batch of 64 at 512 x 512
        assemble (implies extract): the graph assembly of img2smiles2.py:193-311 (ops.GraphAssembler) on the candidate lists, in the same
        captured graph after the extractor; molecules() returns the result.  It reads the lists, not the maps: the same with
        decode=True and fp8=True
        evaluate: the evaluation tables of test_accuracy.py:105-298 (ops.EvalTables) in the same captured graph after the NMS, from the
        masks, |rho|, the atom heads and the bond-type maps (decode: their arg-max map) against .eval_targets, the static target
        buffers load_batch(imgs, targets, n_valid) fills; only the first .n_valid images count (a device int32, so a replayed graph
        evaluates a short last batch); evaluation() / reset_evaluation().  The targets may instead be drawn on the device from
        annotation records: .targets names the same buffers for raster.TargetRasterizer / augment.SampleBuilder(self), and
        use_sparse_targets(rasterizer) lets the evaluation launches read them only where something was drawn
        score_graphs (needs assemble=True and evaluate=True): the score after assembly (ops.GraphScore) in the same captured graph
        after the assembler -- the molecules of the step against the graph records load_graphs(records) staged
        (raster.parse_graph; augment.SampleBuilder(self).load stages them itself), located within score_radius cells, on the
        first .n_valid images; evaluation()["molecules"] holds the running result
        score_similarity (needs assemble=True and evaluate=True): the environment similarity of the assembled molecules to the same
        graph records (ops.GraphSimilarity: the graded, position-free stand-in for cal_acc.py's fingerprint similarity), in the same
        captured graph after the assembler; both scores read the runner's one contract.GraphRecords (.records), which load_graphs
        fills; evaluation()["similarity"] holds the running result
        score_identity (needs assemble=True and evaluate=True): the verified isomorphism test of the assembled molecules against the
        same graph records (ops.GraphIdentity: `same` is certain and free of positions, between score_graphs' `exact` and
        score_similarity's `refine_equal`), in the same captured graph after the similarity; it reads the runner's one
        contract.GraphRecords too; evaluation()["identity"] holds the running result, `undecided` beside `same`
        molblocks (needs assemble=True): the mol block text of the assembled molecules (ops.MolBlockWriter), written in the same
        captured graph right after the assembler; molblocks() returns the strings that go into Chem.MolFromMolBlock -- two small
        copies per batch instead of molecules() and Molecule.molblock() per image on the host
        smiles (needs assemble=True): a SMILES string of every assembled molecule (ops.SmilesWriter), written in the same captured
        graph after the assembler (and after the mol block text, if both are on); smiles() returns the strings.  The text rule is
        this project's: deterministic, its graph is the assembled graph, NOT RDKit's canonical SMILES
        smiles_stereo (needs smiles=True): the same stage writes the tetrahedral centres that the predicted wedge bonds and the atom
        positions decide as `@` / `@@` (SmilesWriter(stereo=True)): smiles() is then `m.smiles(stereo=True)`, stereo_stats() says
        how many wedge rows there were and how many centres were marked, flat or unqualified.  The same two launches in the same place
        smiles_double_bonds (needs smiles=True, refused with smiles_canonical=True; smiles_stereo is allowed): the same stage writes
        the single bonds at every double bond whose geometry the atom positions decide as `/` or `\\`
        (SmilesWriter(double_bonds=True)): smiles() is then `m.smiles(double_bonds=True, ...)`, double_bond_stats() says how many
        double bonds were marked, flat, on a cycle or had twin leaves, double_bond_codes() gives the code of every bond row.  The
        same two launches in the same place; off (the default): no launch and no byte changes
        smiles_canonical (needs smiles=True, refused with smiles_stereo=True): the canonical atom order of every assembled molecule
        (ops.GraphCanonicalizer) in the same captured chain right after the assembler; the SMILES stage then reads the CANONICAL rows, so
        smiles() is `m.smiles(canonical=True)`: equal strings if and only if equal graphs (this project's rule on a canonical order, not
        RDKit's canonical SMILES).  molblocks=True keeps reading the assembler's rows: the mol block stays the reference's bytes.
        canonical_stats() returns the search's rows (an UNDECIDED image is reported there), canonical_keys() the hash keys.  Stereo is
        refused: wedge ownership and the drawn geometry are not in the invariant
        smiles_isomeric (needs smiles=True; refused with each of smiles_canonical, smiles_stereo and smiles_double_bonds, because it
        already is all three): the canonical ISOMERIC form.  .canonicalizer is GraphCanonicalizer(rows, stereo=True) -- the stereo
        elements are perceived (ops.StereoPerceiver, a launch inside the canonicaliser op) and the search reads them as a third key
        -- and the SMILES stage writes both marks on its canonical rows: smiles() is `m.smiles(isomeric=True)`, equal strings if and
        only if equal STEREO graphs (unless canonical_stats() says UNDECIDED or COLLISION).  canonical_stats(), canonical_keys(),
        stereo_stats(), double_bond_stats() work; stereo_search() is the read-back of the third key.  The old combination
        smiles_canonical + smiles_stereo stays refused: the plain canonical order does not see the stereo, this one does
        aromatize (needs assemble=True): the aromatic rings of every assembled molecule are perceived (ops.AromaticityPerceiver, one
        launch right after the assembler in the same captured chain) and, when graph records are staged, those of every record (a
        second launch); the canonical order, the SMILES text and the three scores then read the PERCEIVED rows and records, so a ring
        drawn with alternating orders 1 / 2 and the same ring drawn with order 4 are one molecule.  smiles() is then
        `m.aromatized().smiles(...)` (smiles_stereo is allowed); molblocks=True keeps reading the assembler's rows: the mol block
        stays the reference's bytes.  aromatic_stats() returns the pass's rows.  The rule is this project's,
        not RDKit's.  Off (the default): no launch is added and no byte changes
        omega_rule: the extractor's candidate rule (ops.PeakExtractor): "raw" (img2smiles2.py:139, the default) or "peaks"
        (img2smiles.py:139 / img2smiles3.py:140).  Everything after the extractor reads lists, not rules, so assemble, score_graphs,
        decode and fp8 work with either; .omega_rule names the one chosen"""
        flags = dict(assemble=assemble, evaluate=evaluate, score_graphs=score_graphs, score_similarity=score_similarity,
                     score_identity=score_identity, molblocks=molblocks, smiles=smiles, aromatize=aromatize, smiles_stereo=smiles_stereo,
                     smiles_double_bonds=smiles_double_bonds, smiles_canonical=smiles_canonical)
        from .ops import OMEGA_RULES, AromaticityPerceiver, GraphAssembler, GraphCanonicalizer, GraphIdentity, GraphScore, GraphSimilarity, MolBlockWriter, PeakExtractor, SmilesWriter, check_nms_heads
        if omega_rule not in OMEGA_RULES:
            raise ValueError("InferenceRunner: omega_rule must be one of %s, got %r" % (sorted(OMEGA_RULES), omega_rule))
        self.omega_rule = omega_rule
        check_flags(flags)
        check_isomeric(smiles_isomeric, flags)
        extract = bool(extract) or bool(assemble)
        check_nms_heads(model.heads, "InferenceRunner")
        if extract and tuple(model.heads) != HEADS:
            raise ValueError("InferenceRunner(extract=True): the peak extractor reads heads %s, got heads %s" % (list(HEADS), list(model.heads)))
        self.dev = dev = resolve_device(model, device, "InferenceRunner")
        self.model = model
        model.eval()
        with torch.cuda.device(dev):
            x0 = torch.zeros((batch, model.n_channels, height, width), device=dev)
            if fold_bn is None:
                fold_bn = model.VARIANT == "unet"
            self.fold_bn = bool(fold_bn)
            self.fp8 = bool(fp8)
            self.fp8_margin = float(fp8_margin)
            if self.fp8 and not (self.fold_bn and model.VARIANT == "unet" and model.compute_dtype == "bf16"):
                raise L.AbcNetHipError("fp8 inference is a form of the BatchNorm-folded bf16 graph of unet.py")
            # heads_epilogue (folded graph, opt-in: exact but slower than the default plan): the heads' 1x1
            # convolutions in the epilogue of the convolution that makes their features
            self.eng = eng = model._engine_for(x0, False, fold_bn=self.fold_bn, fp8=self.fp8, guards=guards, heads_epilogue=heads_epilogue,
                                               nms_heads=bool(nms_in_heads) and not heads_epilogue,
                                               decode=bool(decode) and bool(nms_in_heads) and not heads_epilogue)
            # (bf16 graph with its feature tensor materialised: calibration only)
            self._ref = model._engine_for(x0, False, fold_bn=True, heads_epilogue=False) if self.fp8 else None
        lg = eng.logits
        self.atom_mask, self.bond_mask = torch.empty_like(lg[0]), torch.empty_like(lg[4])
        self.nms_in_heads = eng.nms_rho is not None
        self.decode = eng.decode and eng.btype_idx is not None
        self.btype_idx = eng.btype_idx
        if self.nms_in_heads:
            self.rho_abs, self.omega_mask = eng.nms_rho, eng.nms_omega      # (written by the forward plan itself)
        else:
            self.rho_abs, self.omega_mask = torch.empty_like(lg[6]), torch.empty_like(lg[7])
        d = L.NmsDesc()
        d.atom, d.bond, d.omega = lg[0].data_ptr(), lg[4].data_ptr(), lg[7].data_ptr()
        d.rho = None if lg[6] is None else lg[6].data_ptr()      # (decode: not stored, and not read -- n_omega = 0)
        d.B, d.h, d.w, d.n_omega = eng.B, eng.h, eng.w, (0 if self.nms_in_heads else lg[7].shape[1])
        d.atom_mask, d.bond_mask = self.atom_mask.data_ptr(), self.bond_mask.data_ptr()
        d.rho_abs, d.omega_mask = self.rho_abs.data_ptr(), self.omega_mask.data_ptr()
        self._nms = d
        # img2smiles2.py:113-191: compact candidate lists for the CPU graph-assembly stage, inside the same graph
        self.extractor = self.assembler = self.canonicalizer = self.texter = self.smiler = self.evaluator = self._rasterizer = None
        self.aromatizer = self.record_aromatizer = None
        rows = None                      # what the stages behind the assembler read: its rows, or the perceived ones
        with torch.cuda.device(dev):
            if extract:
                self.extractor = PeakExtractor(lg, self.atom_mask, self.bond_mask, cap_atoms=cap_atoms, cap_bonds=cap_bonds,
                                               btype_idx=self.btype_idx if self.decode else None, rho_abs=self.rho_abs if self.decode else None,
                                               omega_rule=omega_rule)
            if assemble:
                self.assembler = GraphAssembler.from_extractor(self.extractor, cap_mol_bonds=cap_mol_bonds)
                rows = self.assembler.rows
            if aromatize:
                self.aromatizer = AromaticityPerceiver.from_assembler(self.assembler)
                rows = self.aromatizer.rows()
            if molblocks:
                self.texter = MolBlockWriter.from_assembler(self.assembler)
            if smiles_isomeric:
                self.canonicalizer = GraphCanonicalizer(rows, stereo=True)
                self.smiler = SmilesWriter(self.canonicalizer.rows(), stereo=True, double_bonds=True)
            elif smiles_canonical:
                self.canonicalizer = GraphCanonicalizer(rows)
                self.smiler = SmilesWriter(self.canonicalizer.rows())
            elif smiles:
                self.smiler = SmilesWriter(rows, stereo=bool(smiles_stereo), double_bonds=bool(smiles_double_bonds))
        if evaluate:
            if tuple(model.heads) != HEADS:
                raise ValueError("InferenceRunner(evaluate=True): the evaluation tables read heads %s, got heads %s" % (list(HEADS), list(model.heads)))
            with torch.cuda.device(dev):
                self.eval_targets = alloc_targets(eng.B, eng.h, eng.w, dev)
                self.n_valid = torch.full((1,), eng.B, dtype=torch.int32, device=dev)
            self._build_evaluator(None)
        self.records = self.scorer = self.similarity = self.identity = None
        self.smiles_reader = None      # (load_smiles builds it on first use)
        # (one set, staged once per batch, whichever score reads it)
        self.wants_graph_records = bool(score_graphs or score_similarity or score_identity)
        if self.wants_graph_records:
            with torch.cuda.device(dev):
                self.records = records = GraphRecords(eng.B, 256, 256, dev)      # (.records: the STAGED ones, what load_graphs fills)
                if aromatize:
                    self.record_aromatizer = AromaticityPerceiver.from_records(self.records)
                    records = self.record_aromatizer.records()
                if score_graphs:
                    self.scorer = GraphScore(rows, radius=score_radius, n_valid=self.n_valid, records=records)
                if score_similarity:
                    self.similarity = GraphSimilarity(rows, n_valid=self.n_valid, records=records)
                if score_identity:
                    self.identity = GraphIdentity(rows, n_valid=self.n_valid, records=records)
        self._stages = [attr for attr in launch_order() if getattr(self, attr) is not None]
        self.use_graph = use_graph
        self._graph = None
        self.steps = 0
        self.refresh()

    def refresh(self):
        """re-pack the (changed) weights and re-derive the eval-mode BatchNorm coefficients (both functions of the
        parameters alone; call again after load_state_dict)"""
        with torch.cuda.device(self.dev):
            self.eng.run_pack(current_stream())

    def _need(self, attr):
        op = getattr(self, attr)
        if op is None:
            raise L.AbcNetHipError("InferenceRunner was built without %s=True" % STAGES[attr])
        return op

    def _read(self, attr, method):
        """a host read-back of the stage `attr` (built, or AbcNetHipError) with the runner's device current"""
        op = self._need(attr)
        with torch.cuda.device(self.dev):
            return getattr(op, method)()

    def _build_evaluator(self, target_flags):
        from .ops import EvalTables
        old = self.evaluator
        with torch.cuda.device(self.dev):
            self.evaluator = EvalTables(self.atom_mask, self.bond_mask, self.omega_mask, self.rho_abs, list(self.eng.logits), self.eval_targets,
                                        btype_idx=self.btype_idx if self.decode else None, n_valid=self.n_valid, target_flags=target_flags)
            if old is not None:      # (what was accumulated so far stays)
                self.evaluator.counts_totals.copy_(old.counts_totals)
                self.evaluator.meters_totals.copy_(old.meters_totals)
                self.evaluator.counts_last.copy_(old.counts_last)
                self.evaluator.meters_last.copy_(old.meters_last)

    @property
    def targets(self):
        """evaluate=True: .eval_targets under the name augment.SampleBuilder and raster.TargetRasterizer(targets=...) callers use"""
        self._need("evaluator")
        return self.eval_targets

    def use_sparse_targets(self, rasterizer):
        """rasterizer: a TargetRasterizer(sparse=True, targets=self.targets) -- the evaluation launches then read only the target planes
        of the 32-pixel groups the rasteriser drew into (abc_eval_tables_update_sparse), and the batch's targets come from
        `rasterizer.load(records); rasterizer.run()` in front of step() instead of a dense copy; None: back to reading every plane.
        The tables and meters are unchanged bit for bit."""
        self._need("evaluator")
        if rasterizer is None:
            self._build_evaluator(None)
            self._rasterizer = None
        else:
            check_sparse_rasterizer(rasterizer, self.eval_targets, "InferenceRunner")
            rasterizer.invalidate()      # (an earlier dense load may have left maps the records know nothing about)
            self._build_evaluator(rasterizer.group_flags)
            self._rasterizer = rasterizer
        self._graph = None

    def load_batch(self, imgs, targets=None, n_valid=None):
        """targets (evaluate=True): the 8 target maps of the batch, copied into .eval_targets; n_valid: how many of its images count
        (default: all; rows past it may hold anything).  Under use_sparse_targets() the targets come from the rasteriser: images and
        n_valid only."""
        self.eng.img.copy_(imgs.reshape(self.eng.img.shape), non_blocking=True)
        if targets is not None or n_valid is not None:
            self._need("evaluator")
            if targets is not None:
                refuse_dense_targets(self._rasterizer)
                for dst, t in zip(self.eval_targets, targets):
                    dst.copy_(t.reshape(dst.shape), non_blocking=True)
            self.n_valid.fill_(self.eng.B if n_valid is None else int(n_valid))
        if self.fp8 and not self.eng.fp8_calibrated:
            self.calibrate()

    @property
    def input_images(self):
        """the static f32 input buffer [B, C, H, W] the step reads (augment.ImageBuilder(out=...) writes it in place)"""
        return self.eng.img

    def calibrate(self):
        """fp8: set the per-tensor e4m3 scales from the batch in the image buffer (the bf16 folded graph runs once on it), then
        re-pack the weights (their scales fold the input scale in).  No host sync; call again when the data distribution moves."""
        if not self.fp8:
            return
        with torch.cuda.device(self.dev):
            st = current_stream()
            ref = self._ref
            ref.img.copy_(self.eng.img)
            ref.run_pack(st)
            ref.run_forward(st)
            self.eng.calibrate_fp8(ref, st, self.fp8_margin)
            self.eng.run_pack(st)
            self._graph = None

    def _run(self, st):
        self.eng.run_forward(st)
        L.check(self.eng.lib.abc_nms_peaks(C.byref(self._nms), st), "nms_peaks")
        for attr in self._stages:
            getattr(self, attr).run(st)

    def evaluation(self):
        """the tables and meters accumulated since the last reset_evaluation() (ops.EvalTables.result(); host sync; needs evaluate=True)"""
        out = self._need("evaluator").result()
        for attr, key in (("scorer", "molecules"), ("similarity", "similarity"), ("identity", "identity")):
            if attr in self._stages:
                out[key] = getattr(self, attr).result()
        return out

    def reset_evaluation(self):
        self._need("evaluator")
        for attr in ("evaluator", "scorer", "similarity", "identity"):
            if attr in self._stages:
                getattr(self, attr).reset()

    def load_graphs(self, records):
        """score_graphs=True, score_similarity=True or score_identity=True: the graph records (raster.parse_graph) of the batch, n <= batch of them (the
        rows past n get an empty record; n_valid says how many images count); staged once, whichever of them read them"""
        if self.records is None:
            self._need("scorer")
        with torch.cuda.device(self.dev):
            self.records.load(records)

    def load_smiles(self, strings):
        """score_similarity=True or score_identity=True: the batch's truth as SMILES strings, n <= batch of them -- a dataset's
        SMILES column in place of annotation records (cal_acc.py's `df['Smiles']`).  An ops.SmilesReader, built on first use, reads
        them on the device into the same .records load_graphs fills, on the same stream; a string the reading rule (DESIGN.md
        section 7) refuses leaves an empty record, a miss for the scores (record_status() says which).  Refused with
        score_graphs=True: that score reads positions and a SMILES has none."""
        if self.records is None:
            self._need("similarity")
        if self.scorer is not None:
            raise ValueError("InferenceRunner.load_smiles: score_graphs=True compares positions, and a SMILES string has none; "
                             "load annotation records (load_graphs), or build the runner without score_graphs")
        with torch.cuda.device(self.dev):
            if self.smiles_reader is None:
                from .ops import SmilesReader
                self.smiles_reader = SmilesReader(self.records)
            self.smiles_reader.load(strings)

    def record_status(self):
        """one L.READ_* value per string of the last load_smiles (host sync)"""
        if self.smiles_reader is None:
            raise L.AbcNetHipError("InferenceRunner.record_status: load_smiles was never called")
        with torch.cuda.device(self.dev):
            return self.smiles_reader.status()

    def candidates(self):
        """the per-image atom / bond candidate lists of the last step (host sync; needs extract=True)"""
        return self._need("extractor").lists()

    def molecules(self):
        """the assembled molecule (decode.Molecule) of every image of the last step, None where the reference finds no key point
        (host sync; needs assemble=True); `Chem.MolFromMolBlock(m.molblock())` is the reference's next call"""
        return self._need("assembler").molecules()

    def molblocks(self):
        """the mol block (str) of every image of the last step, written on the device: what `m.molblock()` gives for the m of
        molecules(), None where that is None (host sync; needs molblocks=True)"""
        return self._read("texter", "molblocks")

    def smiles(self):
        """a SMILES string of every image of the last step, written on the device: what `m.smiles()` gives for the m of
        molecules(), None where that is None (host sync; needs smiles=True); with smiles_stereo=True it is `m.smiles(stereo=True)`,
        with smiles_canonical=True `m.smiles(canonical=True)`, with smiles_double_bonds=True `m.smiles(double_bonds=True, ...)`, with
        smiles_isomeric=True `m.smiles(isomeric=True)` (aromatize=True beside it where that flag is on)"""
        return self._read("smiler", "smiles")

    def canonical_stats(self):
        """the canonical search of every image of the last step (GraphCanonicalizer.stats: the L.CANON_COLUMNS, `status` with the
        L.CANON_UNDECIDED / L.CANON_COLLISION bits; host sync; needs smiles_canonical=True)"""
        return self._read("canonicalizer", "stats")

    def canonical_keys(self):
        """the two hash words of every image's canonical graph (GraphCanonicalizer.keys; host sync; needs smiles_canonical=True)"""
        return self._read("canonicalizer", "keys")

    def stereo_search(self):
        """the third key of the canonical search of every image of the last step (GraphCanonicalizer.stereo_search: the
        L.STEREO_SEARCH_COLUMNS; host sync; needs smiles_isomeric=True)"""
        if self.canonicalizer is None or not self.canonicalizer.stereo:
            raise L.AbcNetHipError("InferenceRunner was built without smiles_isomeric=True")
        return self._read("canonicalizer", "stereo_search")

    def aromatic_stats(self):
        """the aromaticity perception of every image of the last step (AromaticityPerceiver.stats: the L.AROMATIC_COLUMNS -- status,
        candidates, cycles, aromatic, rows_changed, listed; host sync; needs aromatize=True); with staged graph records a pair:
        the molecules' rows, then the records'"""
        stats = self._read("aromatizer", "stats")
        return stats if self.record_aromatizer is None else (stats, self._read("record_aromatizer", "stats"))

    def stereo_stats(self):
        """what became of the wedge rows of the last step (SmilesWriter.stereo_stats: marked, flat, unqualified, wedge_rows and the
        per-image rows; host sync; needs smiles=True and smiles_stereo=True)"""
        return self._read("smiler", "stereo_stats")

    def double_bond_stats(self):
        """what became of the candidate double bonds of the last step (SmilesWriter.double_bond_stats: marked, flat, ring, twin and
        the per-image rows; host sync; needs smiles=True and smiles_double_bonds=True)"""
        return self._read("smiler", "double_bond_stats")

    def double_bond_codes(self):
        """the code of every bond row of the last step (SmilesWriter.double_bond_codes: int32 [B, cap_mol_bonds] on the host; host
        sync; needs smiles=True and smiles_double_bonds=True)"""
        return self._read("smiler", "double_bond_codes")

    def step(self):
        """forward + NMS on the batch in the static image buffer; results in .logits / .atom_mask / ..."""
        if self.records is not None and not self.records.loaded:
            raise L.AbcNetHipError("InferenceRunner(score_graphs=True): no graph records were loaded (load_graphs, or SampleBuilder.load)")
        with torch.cuda.device(self.dev):
            self._step()

    def _step(self):
        if self.use_graph and self._graph is None and self.steps >= 1:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._run(current_stream())
            self._graph = g
        if self._graph is not None:
            self._graph.replay()
        else:
            self._run(current_stream())
        self.steps += 1

    @property
    def logits(self):
        return self.eng.logits

    def profile(self, iters=3):
        """eager steps with a HIP event pair around every launch on the launch stream (as Trainer.profile)"""
        from .ops import fold_marks, per_iteration, timed
        eng = self.eng
        torch.cuda.set_device(self.dev)
        stream = torch.cuda.current_stream(self.dev)
        st = stream.cuda_stream
        acc = {}
        for _ in range(iters):
            marks = []
            for fn, args, what, _w, meta in eng.fwd_ops:
                L.check(timed(stream, marks, meta["kernel"], meta["flops"], meta["bytes"], lambda: fn(*args, st)), what)
            L.check(timed(stream, marks, "nms", 0.0, float(eng.B * eng.h * eng.w * (2 if self.nms_in_heads else 122) * 4 * 2),
                          lambda: eng.lib.abc_nms_peaks(C.byref(self._nms), st)), "nms_peaks")
            torch.cuda.synchronize()
            fold_marks(acc, marks, ("flops", "bytes"))
        per_iteration(acc, iters)
        return acc
