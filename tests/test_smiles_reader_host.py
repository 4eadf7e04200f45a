"""The SMILES reader's rule on the host (decode.parse_smiles, the reference of csrc/smiles_read.hip): the hand-derived table, a second
implementation (tests/smiles_reader_oracle.py), the round trip through every form of the writer, and the kernel's own steps run on the
CPU over the shared token functions (tests/smiles_tokens_main.cpp, under a host sanitizer where the compiler has one)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd import decode as D  # noqa: E402
from abcnet_amd.decode import Molecule, parse_smiles  # noqa: E402
import smiles_reader_cases as K  # noqa: E402
import smiles_reader_oracle as RO  # noqa: E402
from smiles_cases import EXAMPLES, random_rows  # noqa: E402

FORMS = (dict(), dict(canonical=True), dict(stereo=True), dict(double_bonds=True), dict(isomeric=True))


def test_the_status_names_are_stated_once():
    assert (D.READ_OK, D.READ_EMPTY, D.READ_TOO_LONG, D.READ_SYNTAX, D.READ_TRUNCATED, D.READ_DUPLICATE) == (K.OK, K.EMPTY, K.TOO_LONG, K.SYNTAX, K.TRUNCATED, K.DUPLICATE)
    assert (L.READ_EMPTY, L.READ_TOO_LONG, L.READ_SYNTAX, L.READ_TRUNCATED, L.READ_DUPLICATE) == (1, 2, 3, 4, 5)
    assert L.MAX_SMILES_READ_BYTES == D.MAX_SMILES_READ_BYTES == K.MAX_BYTES == RO.MAX_BYTES
    header = open(os.path.join(ROOT, "include", "abcnet_hip.h")).read()
    assert "#define ABC_MAX_SMILES_READ_BYTES %d " % L.MAX_SMILES_READ_BYTES in header
    for value, name in enumerate(D.READ_STATUS_NAMES):
        assert "ABC_READ_%s = %d" % (name, value) in header
    assert (L.SmilesReadDesc, "abc_smiles_read_desc_size") in L.SELF_SIZED_SINCE and L.SmilesReadDesc not in L._STRUCTS
    assert "smiles_read" in open(os.path.join(ROOT, "build_hip.sh")).read()


def test_the_hand_table_exactly():
    for text, n, m, classes, orders, charges in K.TABLE:
        status, atoms, bonds = parse_smiles(text)
        assert status == K.OK, text
        assert atoms.dtype == np.int32 and bonds.dtype == np.int32 and atoms.shape == (n, 4) and bonds.shape == (m, 3), text
        assert atoms[:, 2].tolist() == classes and atoms[:, 3].tolist() == charges and not atoms[:, :2].any(), text
        assert sorted(bonds[:, 2].tolist()) == orders, text
        assert ((0 <= bonds[:, 0]) & (bonds[:, 0] < bonds[:, 1]) & (bonds[:, 1] < n)).all(), text
    for text, (atoms, bonds) in K.FULL_ROWS.items():
        assert K.as_rows(*parse_smiles(text)) == (K.OK, list(atoms), list(bonds)), text
    assert K.as_rows(*parse_smiles("[Fe+2]")) == K.as_rows(*parse_smiles("[Fe++]"))
    # every example of the writer's rule is in the table
    assert {t for _, _, t in EXAMPLES} <= {row[0] for row in K.TABLE}


def test_the_refusals():
    for text, want in K.REFUSED:
        status, atoms, bonds = parse_smiles(text)
        assert status == want and atoms.shape == (0, 4) and bonds.shape == (0, 3), (text[:40], D.READ_STATUS_NAMES[status])
    for cap in (1, 7, 64):
        assert parse_smiles(K.truncated(cap), max_atoms=cap)[0] == K.TRUNCATED
        assert parse_smiles(K.truncated(cap), max_atoms=cap + 1, max_bonds=cap - 1)[0] == K.TRUNCATED
        assert parse_smiles(K.truncated(cap), max_atoms=cap + 1, max_bonds=cap)[0] == K.OK
    # the priority: a syntax error wins over the capacities, the capacities over the pair bonded twice
    assert parse_smiles("C12CCC12(", max_atoms=1)[0] == K.SYNTAX and parse_smiles("C12CCC12", max_atoms=1)[0] == K.TRUNCATED
    assert parse_smiles("C" * K.MAX_BYTES)[0] == K.OK and parse_smiles(b"C\xc3\xa9")[0] == K.SYNTAX
    with pytest.raises(ValueError):
        parse_smiles(12)


def test_the_implicit_bond_is_aromatic_only_between_two_aromatic_atoms():
    """what a rule "no symbol is always 1" would get wrong"""
    orders = lambda t: parse_smiles(t)[2][:, 2].tolist()
    assert orders("cc") == [4] and orders("c-c") == [1] and orders("cC") == [1] and orders("Cc") == [1] and orders("C:C") == [4]
    assert orders("c1ccccc1") == [4] * 6 and orders("c1ccccc1c1ccccc1").count(4) == 13 and orders("c1ccccc1-c1ccccc1").count(4) == 12
    assert orders("c1cc[nH]c1") == [4] * 5 and orders("c1ccccc1C") == [4] * 6 + [1]


def test_host_form_equals_the_second_implementation():
    strings = [row[0] for row in K.TABLE] + [s for s, _ in K.REFUSED] + K.mutated(2000)
    refused = 0
    for text in strings:
        for caps in ((None, None), (6, 5)):
            got, want = K.as_rows(*parse_smiles(text, *caps)), K.as_rows(*RO.parse(text, *caps))
            assert got == want, (text, caps, got, want)
        refused += got[0] != K.OK
    print("%d strings, %d refused at capacities (6, 5)" % (len(strings), refused))
    assert len(strings) // 2 < refused < len(strings)


def _graph_of_record(atoms, bonds):
    g = nx.Graph()
    for i, (_, _, cls, charge) in enumerate(np.asarray(atoms).reshape(-1, 4).tolist()):
        g.add_node(i, cls=cls, charge=charge)
    for i, j, order in np.asarray(bonds).reshape(-1, 3).tolist():
        g.add_edge(i, j, order=order)
    return g


def _graph_of_rows(rows):
    atoms, bonds, _ = rows
    g = nx.Graph()
    for i, (_, _, t, charge, _) in enumerate(atoms):
        g.add_node(i, cls=1 if t == 0 else t, charge=charge)
    for e1, e2, order, _ in bonds:
        g.add_edge(e1 - 1, e2 - 1, order=1 if order in (5, 6) else order)
    return g


def test_round_trip_through_every_form_of_the_writer():
    rng = np.random.default_rng(26)
    cases = [rows for _, rows, _ in EXAMPLES] + [random_rows(rng) for _ in range(500)]
    written = 0
    for k, rows in enumerate(cases):
        atoms, bonds, implh = rows
        mol = Molecule.from_device_rows(np.asarray(atoms).reshape(-1, 5), np.asarray(bonds).reshape(-1, 4), implh)
        want = _graph_of_rows(rows)
        for form in FORMS:
            text = mol.smiles(**form)        # (valid rows, at most 80 bonds: the writer gives a string for every one)
            status, a, q = parse_smiles(text)
            assert status == K.OK and len(a) == len(atoms) and len(q) == len(bonds), (k, form, text)
            assert nx.is_isomorphic(_graph_of_record(a, q), want, node_match=lambda x, y: x == y, edge_match=lambda x, y: x == y), (k, form, text)
            assert K.as_rows(status, a, q) == K.as_rows(*RO.parse(text)), (k, form, text)
            written += 1
    assert written == len(cases) * len(FORMS)


def test_the_launcher_refuses_before_it_touches_a_device():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libabcnet_hip.so is not built")
    lib = L.load()
    assert lib.abc_smiles_read_desc_size() == C.sizeof(L.SmilesReadDesc)

    def refused(**fields):
        d = L.SmilesReadDesc()
        base = dict(text=1 << 20, offsets=2 << 20, rec_atoms=3 << 20, rec_bonds=4 << 20, rec_counts=5 << 20, B=2, max_atoms=64, max_bonds=64,
                    cap_text=8192, status=6 << 20)      # (addresses that are never dereferenced: the refusals come first)
        for k, v in dict(base, **fields).items():
            setattr(d, k, v)
        return lib.abc_read_smiles(C.byref(d), None), lib.abc_last_error().decode()

    assert lib.abc_read_smiles(None, None) == -1
    for field in ("text", "offsets", "rec_atoms", "rec_bonds", "rec_counts", "status"):
        rc, msg = refused(**{field: None})
        assert rc == -1 and "read_smiles" in msg and "null" in msg, field
    for fields in (dict(B=0), dict(B=-3), dict(max_atoms=0), dict(max_bonds=0), dict(cap_text=0)):
        assert refused(**fields)[0] == -1, fields


# ------------------------------------------------------------------------------------- the kernel's steps on the CPU, same header
def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_the_token_functions_on_the_cpu(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe, src = str(tmp_path / "smiles_tokens_main"), os.path.join(ROOT, "tests", "smiles_tokens_main.cpp")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "abc-net_amd", "csrc"), src, "-o", exe]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode == 0
    if not sanitized:
        subprocess.run(base, check=True)
    deep = "C(" * 300 + "C" + ")" * 300
    rings = "".join("C%s" % (k if k < 10 else "%%%02d" % k) for k in range(100)) + "".join("C%s" % (k if k < 10 else "%%%02d" % k) for k in range(100))
    strings = ([row[0] for row in K.TABLE] + [s for s, _ in K.REFUSED] + K.mutated(2000) + [deep, rings, "C" * K.MAX_BYTES, "[" * K.MAX_BYTES,
               "[" + "1" * (K.MAX_BYTES - 3) + "C]", "C%", "C%1", "[C@", "[C+", "[C:", "[", "C("])
    cases = [(s, caps) for s in strings for caps in ((4096, 4096), (6, 5))]
    path = tmp_path / "cases.txt"
    path.write_text("".join("%s %d %d\n" % (D.smiles_bytes(s).hex() or "-", a, b) for s, (a, b) in cases))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    for (s, caps), line in zip(cases, lines):
        v = [int(x) for x in line.split()]
        status, n, m = v[:3]
        got = (status, [(0, 0) + tuple(v[3 + 2 * i:5 + 2 * i]) for i in range(n)], [tuple(v[3 + 2 * n + 3 * j:6 + 2 * n + 3 * j]) for j in range(m)])
        assert got == K.as_rows(*parse_smiles(s, *caps)), (s[:60], caps)
    print("sanitized build: %s" % sanitized)
