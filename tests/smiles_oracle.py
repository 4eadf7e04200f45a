"""Test infrastructure, not product: the SMILES text rule of DESIGN.md section 7 written a second time, recursively and straight from
the rule's text (`write`; it shares no code with abcnet_amd.decode), and a reader for the subset of SMILES the writer emits
(`parse`), so that a test can ask whether the text's graph IS the rows' graph."""
import sys

SYMBOLS = ["C", "C", "N", "O", "P", "F", "Cl", "S", "Br", "B", "Se", "I", "H", "Si"]      # the vocabulary, index 0 read as carbon
MAY_BE_AROMATIC = {"B", "C", "N", "O", "P", "S", "Se"}
NO_BRACKETS = {"B", "C", "N", "O", "P", "S", "F", "Cl", "Br", "I"}
# charge -> the valences tried, in order
VALENCES = {
    "B": {-1: [4], 0: [3], 1: [2]}, "C": {-1: [3], 0: [4], 1: [3]}, "N": {-1: [2], 0: [3], 1: [4]}, "O": {-1: [1], 0: [2], 1: [3]},
    "F": {-1: [], 0: [1], 1: [2]}, "Si": {-1: [3, 5], 0: [4], 1: [3]}, "P": {-1: [2, 4, 6], 0: [3, 5], 1: [4]},
    "S": {-1: [1], 0: [2, 4, 6], 1: [3, 5]}, "Cl": {-1: [], 0: [1], 1: [2, 4, 6]}, "Se": {-1: [1], 0: [2, 4, 6], 1: [3, 5]},
    "Br": {-1: [], 0: [1], 1: [2, 4, 6]}, "I": {-1: [], 0: [1], 1: [2, 4, 6]},
}


class Refused(Exception):
    """the rule gives no text: .cause is "bad_row" or "ring_limit" """

    def __init__(self, cause, why):
        Exception.__init__(self, "%s: %s" % (cause, why))
        self.cause = cause


def order_class(order):
    return 1 if order in (5, 6) else order


def classes(atoms, bonds, implh):
    """(symbols, charges, aromatic flags, listed flags, {frozenset(u, v): class}) of valid rows, 0-based"""
    n = len(atoms)
    for row in atoms:
        if not 0 <= int(row[2]) <= 13:
            raise Refused("bad_row", "vocabulary index %d" % row[2])
        if not -15 <= int(row[3]) <= 15:
            raise Refused("bad_row", "charge %d" % row[3])
    edge = {}
    for row in bonds:
        e1, e2, order = int(row[0]), int(row[1]), int(row[2])
        if order < 1 or order > 6:
            raise Refused("bad_row", "order %d" % order)
        if e1 < 1 or e1 > n or e2 < 1 or e2 > n:
            raise Refused("bad_row", "end outside 1..n")
        if e1 == e2:
            raise Refused("bad_row", "both ends on one atom")
        if frozenset((e1 - 1, e2 - 1)) in edge:
            raise Refused("bad_row", "a pair listed twice")
        edge[frozenset((e1 - 1, e2 - 1))] = order_class(order)
    symbols = [SYMBOLS[int(row[2])] for row in atoms]
    charges = [int(row[3]) for row in atoms]
    aromatic = [symbols[a] in MAY_BE_AROMATIC and any(c == 4 for pair, c in edge.items() if a in pair) for a in range(n)]
    listed = [any(int(k) == a + 1 for k in implh) for a in range(n)]
    return symbols, charges, aromatic, listed, edge


def write(atoms, bonds, implh):
    """atoms [n][5] (x, y, vocabulary index, charge, hs), bonds [m][4] (end 1, end 2 (1-based), order, source), implh [k] 1-based:
    the text of the rule, or Refused"""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    n = len(atoms)
    symbols, charges, aromatic, listed, edge = classes(atoms, bonds, implh)
    neighbours = [[] for _ in range(n)]
    for pair in edge:
        u, v = tuple(pair)
        neighbours[u].append(v)
        neighbours[v].append(u)
    neighbours = [sorted(x) for x in neighbours]

    def symbol_between(u, v):
        c = edge[frozenset((u, v))]
        if c == 1:
            return "-" if aromatic[u] and aromatic[v] else ""
        if c == 2:
            return "="
        if c == 3:
            return "#"
        return "" if aromatic[u] and aromatic[v] else ":"

    def atom_token(a):
        sym, q = symbols[a], charges[a]
        shown = sym.lower() if aromatic[a] else sym
        if q == 0 and not listed[a] and sym in NO_BRACKETS:
            return shown
        if listed[a]:
            h = 1
        elif sym == "H" or abs(q) > 1:
            h = 0
        else:
            s2 = 0
            for v in neighbours[a]:
                c = edge[frozenset((a, v))]
                s2 += 3 if c == 4 else 2 * c
            v = s2 // 2
            h = 0
            for t in VALENCES[sym][q]:
                if t >= v:
                    h = t - v
                    break
        text = "[" + shown
        if h == 1:
            text += "H"
        elif h >= 2:
            text += "H%d" % h
        if q == 1:
            text += "+"
        elif q == -1:
            text += "-"
        elif q > 0:
            text += "+%d" % q
        elif q < 0:
            text += "-%d" % -q
        return text + "]"

    # ---- the walk
    preorder, rank_of, children, roots = [], {}, {}, []
    ring_bonds, ring_edges = [], set()      # (opener, closer) in the order found; the same bonds as unordered pairs

    def walk(a, tree_parent):
        rank_of[a] = len(preorder)
        preorder.append(a)
        children[a] = []
        for x in neighbours[a]:      # (one scan, never restarted: it goes on after every child's walk)
            if x == tree_parent or frozenset((a, x)) in ring_edges:
                continue
            if x in rank_of:
                ring_bonds.append((x, a))
                ring_edges.add(frozenset((a, x)))
            else:
                children[a].append(x)
                walk(x, a)

    for a in range(n):
        if a not in rank_of:
            roots.append(a)
            walk(a, None)

    # ---- digits at every atom, in preorder
    in_use, number, digits = set(), {}, {}
    for a in preorder:
        closing = sorted((b for b in ring_bonds if b[1] == a), key=lambda b: rank_of[b[0]])
        opening = sorted((b for b in ring_bonds if b[0] == a), key=lambda b: rank_of[b[1]])
        text = ""
        for b in closing:
            text += symbol_between(b[0], b[1]) + _digits(number[b])
        for b in opening:
            k = next((i for i in range(1, 100) if i not in in_use), None)
            if k is None:
                raise Refused("ring_limit", "more than 99 ring bonds open")
            in_use.add(k)
            number[b] = k
            text += _digits(k)
        for b in closing:
            in_use.discard(number[b])
        digits[a] = text

    def text_of(a):
        out = atom_token(a) + digits[a]
        kids = children[a]
        for child in kids[:-1]:
            out += "(" + symbol_between(a, child) + text_of(child) + ")"
        if kids:
            out += symbol_between(a, kids[-1]) + text_of(kids[-1])
        return out

    return ".".join(text_of(r) for r in roots)


def _digits(k):
    return "%d" % k if k <= 9 else "%%%02d" % k


# ----------------------------------------------------------------------------------------------------------------- the reader
ELEMENTS = ("Cl", "Br", "Se", "Si", "se", "B", "C", "N", "O", "P", "S", "F", "I", "H", "b", "c", "n", "o", "p", "s")
BOND_CLASS = {"-": 1, "=": 2, "#": 3, ":": 4}


def parse(text):
    """-> (atoms [(symbol, aromatic, charge, h or None)], bonds [(i, j, class)]) of a string of the writer's subset; an unmarked
    bond between two aromatic atoms is class 4, any other unmarked bond class 1.  Asserts on anything malformed."""
    atoms, bonds, pairs = [], [], set()
    open_rings = {}          # number -> atom
    stack, prev, pending, i = [], None, None, 0

    def bond(u, v, mark):
        assert u != v, "a bond from an atom to itself"
        assert frozenset((u, v)) not in pairs, "atoms %d and %d are bonded twice" % (u, v)
        pairs.add(frozenset((u, v)))
        bonds.append((u, v, BOND_CLASS[mark] if mark else (4 if atoms[u][1] and atoms[v][1] else 1)))

    def element(at):
        for e in ELEMENTS:
            if text.startswith(e, at):
                return e
        raise AssertionError("no element at %d in %r" % (at, text))

    def new_atom(symbol, charge, h):
        nonlocal prev, pending
        aromatic = symbol[0].islower()
        atoms.append((symbol.capitalize() if aromatic else symbol, aromatic, charge, h))
        a = len(atoms) - 1
        if prev is not None:
            bond(prev, a, pending)
        else:
            assert pending is None, "a bond symbol in front of a component's first atom"
        prev, pending = a, None

    while i < len(text):
        ch = text[i]
        if ch == "[":
            j = text.index("]", i)
            body = text[i + 1:j]
            sym = element(i + 1)
            assert body.startswith(sym)
            rest, h, charge = body[len(sym):], 0, 0
            if rest.startswith("H"):
                k = 1
                while k < len(rest) and rest[k].isdigit():
                    k += 1
                h = int(rest[1:k]) if k > 1 else 1
                assert h >= 1 and (k == 1 or h >= 2), "H0 or H1 written with a digit"
                rest = rest[k:]
            if rest:
                assert rest[0] in "+-" and (rest[1:] == "" or (rest[1:].isdigit() and int(rest[1:]) >= 2)), "charge %r" % rest
                charge = (1 if rest[0] == "+" else -1) * (int(rest[1:]) if rest[1:] else 1)
            new_atom(sym, charge, h)
            i = j + 1
        elif ch in BOND_CLASS:
            assert pending is None and prev is not None, "a stray bond symbol"
            pending = ch
            i += 1
        elif ch.isdigit() or ch == "%":
            if ch == "%":
                assert text[i + 1:i + 3].isdigit() and int(text[i + 1:i + 3]) >= 10, "%%nn"
                k, i = int(text[i + 1:i + 3]), i + 3
            else:
                k, i = int(ch), i + 1
                assert k >= 1
            assert prev is not None, "a ring digit without an atom"
            if k in open_rings:
                assert open_rings[k] != prev, "ring %d opened and closed on one atom" % k
                bond(open_rings.pop(k), prev, pending)
            else:
                assert pending is None, "a bond symbol at a ring opening"
                open_rings[k] = prev
            pending = None
        elif ch == "(":
            assert prev is not None and pending is None
            stack.append(prev)
            i += 1
        elif ch == ")":
            assert stack and pending is None
            prev = stack.pop()
            i += 1
        elif ch == ".":
            assert not stack and pending is None and prev is not None, "a dot inside a branch"
            prev = None
            i += 1
        else:
            new_atom(element(i), 0, None)
            i += len(element(i))
    assert not open_rings, "unclosed rings %s" % sorted(open_rings)
    assert not stack and pending is None, "an unclosed branch or a trailing bond symbol"
    return atoms, bonds
