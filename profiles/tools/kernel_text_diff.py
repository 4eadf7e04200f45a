"""Do two builds of the library hold the same device code?

    python profiles/tools/kernel_text_diff.py A/libabcnet_hip.so B/libabcnet_hip.so

Extracts the gfx950 code objects of both libraries the way build_hip.sh does (llvm-objdump --offloading, then -d), splits the disassembly
per symbol, drops the address / encoding comments and hashes the instruction text of every kernel (a symbol with a .kd descriptor) and of
every device function kernels call.  Two things that move with the layout of a code object and not with a kernel are taken out: the
padding behind a code object's last symbol, and the distance in a pc-relative address, which is replaced by its target's name.
Prints the names that are in one library only or whose text differs, one per line, and nothing else on stdout; the counts go to stderr.
Exit status 1 when anything differs."""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile


def objdump():
    cands = []
    try:
        cands.append(os.path.join(subprocess.check_output(["hipconfig", "--rocmpath"], text=True).strip(), "lib/llvm/bin/llvm-objdump"))
    except (OSError, subprocess.CalledProcessError):
        pass
    cands.append("/opt/rocm/lib/llvm/bin/llvm-objdump")
    for c in cands:
        if os.access(c, os.X_OK):
            return c
    sys.exit("llvm-objdump not found")


def kernels(lib, tool):
    """symbol -> (is a kernel, sha256 of its instruction text), over every code symbol of the gfx950 code objects"""
    out = {}
    tmp = tempfile.mkdtemp()
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.check_call([tool, "--offloading", so], stdout=subprocess.DEVNULL)
        for co in sorted(glob.glob(so + ".*gfx950*")):
            syms = subprocess.check_output([tool, "-t", co], text=True)
            kd = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.endswith(".kd")}
            lines = subprocess.check_output([tool, "-d", co], text=True).splitlines()
            at = {int(m.group(1), 16): m.group(2) for m in (re.match(r"^([0-9a-f]+) <(.*)>:$", ln) for ln in lines) if m}
            name, text, pc = None, [], None
            for ln in lines + ["0 <end>:"]:
                m = re.match(r"^[0-9a-f]+ <(.*)>:$", ln)
                if m:
                    # (the padding behind the last symbol of a code object is not the kernel's)
                    while text and text[-1] in ("s_nop 0", "..."):
                        text.pop()
                    if name is not None:
                        h = hashlib.sha256("\n".join(text).encode()).hexdigest()
                        if name in out and (name in kd or out[name][1] != h):
                            sys.exit("%s is defined twice in %s" % (name, lib))
                        out[name] = (name in kd, h)
                    name, text, pc = m.group(1), [], None
                elif ln.strip():
                    ins, _, rest = ln.partition("//")
                    ins = " ".join(ins.split())
                    # a pc-relative address (s_getpc_b64, then s_add_u32 with the distance to the target): name the target, the distance moves
                    # with the layout of the code object
                    m = re.match(r"^s_add_u32 (s\d+), \1, (0x[0-9a-f]+)$", ins)
                    if pc is not None and m:
                        d = int(m.group(2), 16)
                        target = pc + (d - (1 << 32) if d >> 31 else d)
                        if target in at:
                            ins = "s_add_u32 %s, %s, <%s>" % (m.group(1), m.group(1), at[target])
                    pc = int(rest.split(":")[0], 16) + 4 if ins.startswith("s_getpc_b64") else None
                    text.append(ins)
    finally:
        shutil.rmtree(tmp)
    return out


def main():
    tool = objdump()
    a, b = kernels(sys.argv[1], tool), kernels(sys.argv[2], tool)
    diff = sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))
    for n in diff:
        print(n)
    nk = [sum(k for k, _h in x.values()) for x in (a, b)]
    print("%d kernels and %d device functions in %s, %d and %d in %s, %d differ" %
          (nk[0], len(a) - nk[0], sys.argv[1], nk[1], len(b) - nk[1], sys.argv[2], len(diff)), file=sys.stderr)
    return 1 if diff else 0


sys.exit(main())
