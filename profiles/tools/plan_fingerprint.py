"""Fingerprint of the launch plans the engine builds, without a GPU.

    python profiles/tools/plan_fingerprint.py [--repo TREE] [--only SUBSTRING] [--dump DIR] [--routes FILE] [--conv-routes FILE]

Builds every plan of configs(), then of more_configs(), with Engine(..., device="cpu") and replays pack_ops, fwd_ops and bwd_ops against a proxy of the library that
forwards the plan-time queries and, for a launch (any call whose last argument is the replay's stream), records the function name and
every argument instead of launching: scalars as they are, ctypes structures and arrays (through byref()._obj too) field by field.  Every
pointer -- argument or field -- becomes (owner ordinal, byte offset): the owner is the tensor storage that holds the address, numbered in
order of first appearance, so that a change of allocation order does not show; at its first appearance the owner's shape, dtype and a
hash of its contents are recorded as well.  Each op's label, `writes` and `meta` go in beside its call.  One SHA-256 per plan; --dump
keeps the full text per plan for diffing.  Two trees build the same plans exactly when their columns of hashes agree: run this same file
on both (--repo names the tree whose package is imported; it needs its libabcnet_hip.so).

--routes FILE collects every distinct abc_wgrad_desc the plans hand to the library, query or launch, and writes them as JSON with the
answers of that tree's library to abc_wgrad_rowsum_ok / _fuses_apply / _pads / _tile / _blocks: the fixture tests/golden/wgrad_routes.json
(tests/test_cabi_and_host.py rebuilds the descriptors from it), a table of numbers with one row per descriptor.  Pointers are kept as
null / non-null only; the distinct abc_wgrad_reduce_desc are counted (no query takes one).

--conv-routes FILE does the same for abc_conv_desc: every distinct one handed to a query or a launch, the arrays given to
abc_conv_batch_ok, abc_conv_fwd_batch and abc_heads_batch included, with that library's answers to abc_conv_variant / _weight_layout /
_stat_blocks / _tile / _actbwd_ok, and a second table of the distinct arrays as row indices with abc_conv_batch_ok's answer: the fixture
tests/golden/conv_routes.json.  A descriptor is recorded as it is when it is handed over, so one that the engine asks about before and
after it sets `stats` is two rows.  The tool checks that the rebuilt descriptor gets the answers the engine's own one got."""
import json
import argparse
import ctypes as C
import gc
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--only", default="")
ap.add_argument("--dump", default=None)
ap.add_argument("--routes", default=None)
ap.add_argument("--conv-routes", default=None)
args = ap.parse_args()
sys.path.insert(0, args.repo)
sys.path.insert(0, os.path.join(args.repo, "tests"))

import torch  # noqa: E402
import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.engine import Engine  # noqa: E402
from abcnet_amd.unet import UNet  # noqa: E402
from abcnet_amd.unet2 import UNet as UNet2  # noqa: E402
from test_cabi_and_host import HEADS, OTHER_HEADS  # noqa: E402

STREAM = 0x5EED0000


class Proxy:
    """stands in for the loaded library: queries go through, launches on STREAM are recorded"""

    def __init__(self, real):
        self.real, self.rec = real, None
        self.collect = True                        # (--routes / --conv-routes) False while the plans of more_configs() are built
        self.wgrads, self.reduces = {}, set()      # (--routes) distinct descriptors seen, in order of first appearance
        self.convs, self.batches = {}, {}          # (--conv-routes) the same, and the distinct arrays as tuples of descriptor keys

    def note(self, v):
        v = getattr(v, "_obj", v)      # byref(x)
        if isinstance(v, C.Array):
            for x in v:
                self.note(x)
        elif isinstance(v, L.WgradDesc):
            f = desc_fields(v)
            self.wgrads.setdefault(json.dumps(f, sort_keys=True), f)
        elif isinstance(v, L.WgradReduceDesc):
            self.reduces.add(json.dumps(desc_fields(v), sort_keys=True))
        elif isinstance(v, L.ConvDesc) and args.conv_routes:
            f = desc_fields(v)
            key, ans = json.dumps(f, sort_keys=True), conv_answers(self.real, v)
            if self.convs.setdefault(key, (f, ans))[1] != ans:
                raise RuntimeError("a query reads more of a descriptor than null / non-null pointers: %s" % key)
            return key

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        types = L.SYMBOLS[name][1] if name in L.SYMBOLS else None

        def call(*a):
            if self.collect and (args.routes or args.conv_routes):
                for v in a:
                    self.note(v)
            if self.collect and args.conv_routes and name in ("abc_conv_batch_ok", "abc_conv_fwd_batch", "abc_heads_batch"):
                self.batches.setdefault(tuple(self.note(a[0][i]) for i in range(a[1])), self.real.abc_conv_batch_ok(a[0], a[1]))
            if self.rec is not None and a and a[-1] == STREAM and isinstance(a[-1], int):
                self.rec.call(name, a[:-1], types)
                return 0
            return fn(*a)
        return call


def desc_fields(v, prefix=""):
    """a descriptor as plain data, nested fields as "p.Hx": pointers as null / non-null, tap arrays up to ntaps.  What the engine fills in
    only after it has asked (nsplit, the slab pointers) is left out: no query can depend on it"""
    out = {}
    for n, ft in v._fields_:
        x = getattr(v, n)
        if isinstance(v, L.WgradDesc) and n in ("nsplit", "partial", "rowsum_partial"):
            continue
        if isinstance(x, C.Structure):
            out.update(desc_fields(x, n + "."))
        elif isinstance(x, C.Array):
            out[n] = list(x)[:max(0, v.ntaps)]
        else:
            out[prefix + n] = int(bool(x)) if ft is C.c_void_p else x
    return out


def desc_build(f, cls=L.WgradDesc):
    """the inverse: a non-null pointer is a dummy address (the queries read through none of them)"""
    v = cls()
    for name, x in f.items():
        o, n = v, name
        if "." in name:
            o, n = getattr(v, name.split(".")[0]), name.split(".")[1]
        if isinstance(x, list):
            for i, t in enumerate(x):
                getattr(o, n)[i] = t
        elif dict(o._fields_)[n] is C.c_void_p:
            setattr(o, n, 0x1000 if x else None)
        else:
            setattr(o, n, x)
    return v


ANSWERS = ("rowsum_ok", "fuses_apply", "pads_rc", "ca_pad", "cb_pad", "tile_rc", "at", "bt", "blocks")


def answers(lib, d):
    ca, cb, at, bt = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    rp, rt = lib.abc_wgrad_pads(C.byref(d), C.byref(ca), C.byref(cb)), lib.abc_wgrad_tile(C.byref(d), C.byref(at), C.byref(bt))
    return [lib.abc_wgrad_rowsum_ok(C.byref(d)), lib.abc_wgrad_fuses_apply(C.byref(d)), rp, ca.value, cb.value, rt, at.value, bt.value,
            lib.abc_wgrad_blocks(C.byref(d))]


CONV_ANSWERS = ("variant", "layout", "stat_blocks", "tile_rc", "bn", "mt", "ck", "actbwd_ok")


def conv_answers(lib, d):
    bn, mt, ck = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    rt = lib.abc_conv_tile(C.byref(d), C.byref(bn), C.byref(mt), C.byref(ck))
    return [lib.abc_conv_variant(C.byref(d)), lib.abc_conv_weight_layout(C.byref(d)), lib.abc_conv_stat_blocks(C.byref(d)), rt, bn.value,
            mt.value, ck.value, lib.abc_conv_actbwd_ok(C.byref(d))]


def routes_table(lib, descs, cls=L.WgradDesc, operands="pq", answers=answers, names_of_answers=ANSWERS):
    """the fixture: one row of numbers per descriptor -- its own fields in `columns` order, where the operands ("p", "q"; "src") and
    "taps" are indices into the tables of distinct operands (fields in `operand` order) and tap lists -- then the answers"""
    names = [n for n in descs[0] if n not in ("tap_dy", "tap_dx") and any(f[n] for f in descs)]      # (zero everywhere: left out)
    opnd = sorted({n.split(".")[1] for n in names if "." in n}, key=[n for n, _t in L.ActSrc._fields_].index)
    cols = [n for n in names if "." not in n]
    tabs, rows = dict({o: [] for o in operands}, taps=[]), []

    def index(tab, x):
        if x not in tab:
            tab.append(x)
        return tab.index(x)
    for f in descs:
        rows.append([index(tabs[o], [f[o + "." + n] for n in opnd]) for o in operands] + [f[n] for n in cols] +
                    [index(tabs["taps"], [f["tap_dy"], f["tap_dx"]])] + answers(lib, desc_build(f, cls)))
    return dict(tabs, columns=list(operands) + cols + ["taps"] + list(names_of_answers), operand=opnd, rows=rows)


def write_table(path, tab, keys):
    """`keys` one per line, then the rows, eight to a line"""
    rows = tab.pop("rows")
    enc = lambda x: json.dumps(x, separators=(",", ":"))      # noqa: E731
    with open(path, "w") as f:
        f.write("{" + "".join('"%s":%s,\n' % (k, enc(tab[k])) for k in keys) + '"rows":[\n')
        f.write(",\n".join(",".join(enc(r) for r in rows[i:i + 8]) for i in range(0, len(rows), 8)) + "\n]}\n")
    return len(rows)


def tensors_of(x, depth=0):
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, (list, tuple)) and depth < 4:
        for y in x:
            yield from tensors_of(y, depth + 1)
    elif isinstance(x, dict) and depth < 4:
        for y in x.values():
            yield from tensors_of(y, depth + 1)


class Recorder:
    def __init__(self, eng):
        self.lines, self.ordinal = [], {}
        # owners: every tensor storage the plan can point into -- the four arenas, the plan's buffers, what the engine holds by attribute
        cands = [eng.params, eng.grads, eng.buffers, eng.counters]
        cands += [raw for raw, _n, _s, _d in eng._guarded]
        cands += list(tensors_of(eng.keep))
        for v in vars(eng).values():
            cands += list(tensors_of(v))
        for op in eng.pack_ops + eng.fwd_ops + eng.bwd_ops:      # (tensors an op keeps alive itself)
            cands += list(tensors_of(list(op[1]) if isinstance(op[1], (list, tuple)) else []))
        own = {}
        for t in cands:
            st = t.untyped_storage()
            key = st.data_ptr()
            size = t.numel() * t.element_size()
            if key not in own or size > own[key][2]:
                own[key] = (key, st.nbytes(), size, t)
        self.owners = sorted(own.values(), key=lambda o: o[0])
        # the two device tables that hold addresses are recorded through what they were written from, not as bytes: the weight-packing
        # table (abc_pack_item_fill's items: the engine's PackDesc list, in order) and the heads-epilogue table (HeadsEpi structures)
        self.tables, self.pack_descs = {}, eng._pack_descs
        hepi = getattr(eng, "hepi", None)
        if hepi is not None:
            self.tables[hepi.untyped_storage().data_ptr()] = \
                lambda: "heads_epi " + self.value((L.HeadsEpi * (hepi.numel() // C.sizeof(L.HeadsEpi))).from_buffer_copy(hepi.numpy().tobytes()))

    def pointer(self, p):
        if not p:
            return "null"
        if p == STREAM:
            return "stream"
        lo, hi = 0, len(self.owners)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if self.owners[mid][0] <= p:
                lo = mid
            else:
                hi = mid
        base, nbytes, _size, t = self.owners[lo]
        if not (base <= p < base + max(nbytes, 1)):
            raise RuntimeError("pointer %#x lies in no tensor the plan owns" % p)
        if base not in self.ordinal:
            self.ordinal[base] = len(self.ordinal)
            whole = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())
            esz = t.element_size()
            rows = whole[:whole.numel() // esz * esz].view(-1, esz)
            if base in self.tables:
                content = self.tables[base]()
            elif rows.numel() and bool((rows == rows[0]).all()):
                content = "const " + bytes(rows[0].tolist()).hex()
            else:
                content = hashlib.sha256(whole.numpy().tobytes()).hexdigest()
            self.lines.append("  owner %d: shape %s %s, %d bytes, %s" % (self.ordinal[base], tuple(t.shape), t.dtype, nbytes, content))
        return "(%d+%d)" % (self.ordinal[base], p - base)

    def value(self, v, ctype=None):
        if type(v).__name__ == "CArgObject":      # byref(x)
            return self.value(v._obj)
        if isinstance(v, C.Structure):
            return "{" + ", ".join("%s=%s" % (n, self.value(getattr(v, n), ft)) for n, ft in v._fields_) + "}"
        if isinstance(v, C.Array):
            return "[" + ", ".join(self.value(x, v._type_) for x in v) + "]"
        if isinstance(v, C.c_void_p):
            return self.pointer(v.value)
        if isinstance(v, C._SimpleCData):
            return repr(v.value)
        if ctype is not None and (ctype is C.c_void_p or hasattr(ctype, "contents")):
            return self.pointer(v)
        return repr(v)

    def call(self, name, a, types):
        if types is None or len(types) != len(a) + 1:
            raise RuntimeError("%s: %d arguments for %s" % (name, len(a) + 1, types))
        if name == "abc_pack_batch":
            self.tables[a[0]] = lambda: "pack items " + " ".join(self.value(pd) for pd in self.pack_descs)
        self.lines.append("  call %s(%s)" % (name, ", ".join(self.value(v, t) for v, t in zip(a, types))))


def fingerprint(eng, proxy):
    rec = Recorder(eng)
    proxy.rec = rec
    try:
        for title, ops in (("pack", eng.pack_ops), ("forward", eng.fwd_ops), ("backward", eng.bwd_ops)):
            rec.lines.append("%s: %d ops" % (title, len(ops)))
            for op in ops:
                rec.lines.append(" op %r writes=%r meta=%r" % (op[2], tuple(op[3]), sorted(op[4].items())))
                n = len(rec.lines)
                eng._run([op], STREAM)
                if sum(ln.startswith("  call") for ln in rec.lines[n:]) != 1:
                    raise RuntimeError("op %r made no single launch" % (op[2],))
    finally:
        proxy.rec = None
    text = "\n".join(rec.lines) + "\n"
    return hashlib.sha256(text.encode()).hexdigest(), text


def configs():
    big = (16, 384, 384)
    out = [("unet bf16 train 16x384x384 fused_heads", "unet", 1, HEADS, big, "bf16", True, dict(fused_heads=True))]
    for k in ("actbwd_epilogue", "merge_reduce", "dual_wgrad", "fused_convt"):
        out.append(("unet bf16 train 16x384x384 fused_heads %s=False" % k, "unet", 1, HEADS, big, "bf16", True, {"fused_heads": True, k: False}))
    out.append(("unet bf16 train 16x384x384 fused_heads=False", "unet", 1, HEADS, big, "bf16", True, dict(fused_heads=False)))
    out.append(("unet bf16 train 16x384x384 fused_heads=False batched_heads=False", "unet", 1, HEADS, big, "bf16", True,
                dict(fused_heads=False, batched_heads=False)))
    out.append(("unet fp32 train 2x64x64", "unet", 1, HEADS, (2, 64, 64), "fp32", True, {}))
    out.append(("unet fp32 train 1x72x88", "unet", 1, HEADS, (1, 72, 88), "fp32", True, {}))
    out.append(("unet2 bf16 train 16x384x384", "unet2", 1, HEADS, big, "bf16", True, {}))
    out.append(("unet2 fp32 train 1x72x88", "unet2", 1, HEADS, (1, 72, 88), "fp32", True, {}))
    for variant, cin, heads, B, H, W in OTHER_HEADS:
        for dtype in ("bf16", "fp32"):
            for train in (True, False):
                out.append(("%s in%d heads %s %s %s %dx%dx%d fused_heads" % (variant, cin, heads, dtype, "train" if train else "eval", B, H, W),
                            variant, cin, heads, (B, H, W), dtype, train, dict(fused_heads=True)))
    small = (2, 64, 64)
    for label, kw in (("", {}), (" fold_bn", dict(fold_bn=True)), (" fold_bn nms_heads", dict(fold_bn=True, nms_heads=True)),
                      (" fold_bn nms_heads decode", dict(fold_bn=True, nms_heads=True, decode=True)),
                      (" fold_bn heads_epilogue", dict(fold_bn=True, heads_epilogue=True)), (" fold_bn fp8", dict(fold_bn=True, fp8=True))):
        out.append(("unet bf16 eval 2x64x64" + label, "unet", 1, HEADS, small, "bf16", False, kw))
    out.append(("unet2 bf16 eval 2x64x64", "unet2", 1, HEADS, small, "bf16", False, {}))
    out.append(("unet bf16 train 2x64x64 fused_heads guards", "unet", 1, HEADS, small, "bf16", True, dict(fused_heads=True, guards=True)))
    out.append(("unet2 fp32 train 2x64x64 guards", "unet2", 1, HEADS, small, "fp32", True, dict(guards=True)))
    return out


def more_configs():
    """the heads' forms the 44 plans of configs() leave out (profiles/r28_heads_plan.md).  Hashed and dumped after them, so the dump
    indices of the 44 stay; kept out of --routes / --conv-routes, so the two fixtures stay the 44 plans' tables"""
    small = (2, 64, 64)
    six = OTHER_HEADS[0][2]
    out = []
    for label, kw in ((" fold_bn fp8 nms_heads", dict(fold_bn=True, fp8=True, nms_heads=True)),      # (InferenceRunner(fp8=True)'s default)
                      (" fold_bn fp8 nms_heads decode", dict(fold_bn=True, fp8=True, nms_heads=True, decode=True)),
                      (" fold_bn fp8 heads_epilogue", dict(fold_bn=True, fp8=True, heads_epilogue=True)),
                      (" fold_bn batched_heads=False", dict(fold_bn=True, batched_heads=False))):
        out.append(("unet bf16 eval 2x64x64" + label, "unet", 1, HEADS, small, "bf16", False, kw))
    # (six heads: the NMS second outputs must not be granted)
    out.append(("unet heads %s bf16 eval 2x64x64 fold_bn nms_heads" % six, "unet", 1, six, small, "bf16", False, dict(fold_bn=True, nms_heads=True)))
    # (an image of 2x40x24 does not build -- five poolings need 32 x 32; ragged head maps instead: 160 x 96 gives the 40 x 24 map of
    #  tests/test_gpu_fp8.py, ragged tiles; 72 x 88 gives 18 x 22, (h * w) % 64 != 0: the e4m3 features fall away)
    for shape in ((2, 160, 96), (1, 72, 88)):
        for label, kw in ((" fold_bn heads_epilogue", dict(fold_bn=True, heads_epilogue=True)), (" fold_bn fp8", dict(fold_bn=True, fp8=True)),
                          (" fold_bn fp8 heads_epilogue", dict(fold_bn=True, fp8=True, heads_epilogue=True))):
            out.append(("unet bf16 eval %dx%dx%d" % shape + label, "unet", 1, HEADS, shape, "bf16", False, kw))
    # (72 x 88: (h * w) % 128 != 0 too, the fused heads pass is asked for and falls back)
    out.append(("unet bf16 train 1x72x88 fused_heads", "unet", 1, HEADS, (1, 72, 88), "bf16", True, dict(fused_heads=True)))
    out.append(("unet bf16 train 2x64x64 fused_heads=False", "unet", 1, HEADS, small, "bf16", True, dict(fused_heads=False)))
    out.append(("unet bf16 train 2x64x64 fused_heads zero_skip=False", "unet", 1, HEADS, small, "bf16", True, dict(fused_heads=True, zero_skip=False)))
    return out


def main():
    proxy = Proxy(L.load())
    L._lib = proxy
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    first = configs()
    for i, (name, variant, cin, heads, (B, H, W), dtype, train, kw) in enumerate(first + more_configs()):
        if args.only not in name:
            continue
        proxy.collect = i < len(first)
        torch.manual_seed(1234)
        m = (UNet if variant == "unet" else UNet2)(cin, heads, dtype=dtype)
        m._flat_grad = torch.zeros_like(m._flat.data)
        try:
            eng = Engine(variant, cin, heads, m._flat.data, m._flat_grad, m._flat_buf, m._counters, (m._lay_p, m._lay_b, m._lay_c), B, H, W,
                         dtype, train, device="cpu", **kw)
        except Exception as e:      # noqa: BLE001  (a plan that does not build without a GPU is reported, not hidden)
            print("%-100s DOES NOT BUILD: %s: %s" % (name, type(e).__name__, str(e)[:120]), flush=True)
            continue
        digest, text = fingerprint(eng, proxy)
        print("%-100s %s" % (name, digest), flush=True)
        if args.dump:
            with open(os.path.join(args.dump, "%02d.txt" % i), "w") as f:
                f.write(name + "\n" + text)
        del eng, m
        gc.collect()
    if args.routes:
        n = write_table(args.routes, routes_table(proxy.real, list(proxy.wgrads.values())), ("columns", "operand", "p", "q", "taps"))
        print("%d distinct abc_wgrad_desc, %d distinct abc_wgrad_reduce_desc" % (n, len(proxy.reduces)), file=sys.stderr)
    if args.conv_routes:
        keys = list(proxy.convs)
        tab = routes_table(proxy.real, [f for f, _a in proxy.convs.values()], L.ConvDesc, ("src",), conv_answers, CONV_ANSWERS)
        if [r[-len(CONV_ANSWERS):] for r in tab["rows"]] != [a for _f, a in proxy.convs.values()]:
            raise RuntimeError("a rebuilt abc_conv_desc is answered differently from the engine's own")
        tab["batches"] = []
        for batch, ok in proxy.batches.items():
            idx = [keys.index(k) for k in batch]
            arr = (L.ConvDesc * len(idx))(*[desc_build(proxy.convs[k][0], L.ConvDesc) for k in batch])
            if proxy.real.abc_conv_batch_ok(arr, len(idx)) != ok:
                raise RuntimeError("a rebuilt batch is answered differently from the engine's own")
            tab["batches"].append([idx, ok])
        n = write_table(args.conv_routes, tab, ("columns", "operand", "src", "taps", "batches"))
        print("%d distinct abc_conv_desc, %d distinct batches" % (n, len(tab["batches"])), file=sys.stderr)

main()
