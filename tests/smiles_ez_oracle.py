"""Test infrastructure, not product: the double-bond rule of DESIGN.md section 7 a second and a third time.

`write` starts from the PLAIN text of smiles_oracle.write (or from smiles_stereo_oracle.write's, with the tetrahedral marks) and never
looks at a walk: which bond stands where is read OFF THAT TEXT (`bonds_in_text`: the atom in front and the atom behind, or the atom
that bears a closing digit and the atom that opened the number, and the offset at which that bond's symbol stands or would stand).
A bridge is a bond without which its ends fall apart (a search with the bond taken out), a side is the turn a -> b -> s, and the
symbols are not derived from an orientation per double bond: around one marked double bond two substituent bonds, each read OUTWARD
from its end, bear the same symbol iff their substituents lie on the same side of the line through the double bond; the first
unset symbol in the text becomes "/", and what follows from it is filled in until nothing changes.  It shares no code and no
formulation with abcnet_amd.decode.

`read` is the check of the checker: it takes a text with marks and says, per "=" bond and pair of marked neighbours (one at each
end), together or opposite, from what "/" and "\\" MEAN: in `x/y` the atom y is above x, in `x\\y` below, a symbol at a closing digit
is read from the atom that bears it."""
import re

import smiles_oracle as O
import smiles_stereo_oracle as S

NONE, FLAT, RING, TWIN = 0, 2, 3, 4
LIMIT = 199999
FLIP = {"/": "\\", "\\": "/"}


# ------------------------------------------------------------------------------------------------------------------ the text
def bonds_in_text(text):
    """-> (number of atoms, bonds [(first, second, symbol, offset)] in text order): atoms by text position; symbol "" or one of
    "-=#:/\\"; offset: where the symbol stands, or where one would be inserted"""
    bonds, open_rings, stack = [], {}, []
    count, prev, pending, i = 0, None, None, 0
    while i < len(text):
        ch = text[i]
        m = S.ATOM.match(text, i)
        if m:
            if prev is not None:
                bonds.append((prev, count, pending[0] if pending else "", pending[1] if pending else i))
            else:
                assert pending is None
            prev, count, pending, i = count, count + 1, None, m.end()
        elif ch.isdigit() or ch == "%":
            k, end = (int(text[i + 1:i + 3]), i + 3) if ch == "%" else (int(ch), i + 1)
            if k in open_rings:
                bonds.append((prev, open_rings.pop(k), pending[0] if pending else "", pending[1] if pending else i))
            else:
                assert pending is None, "a symbol at an opening digit in %r" % text
                open_rings[k] = prev
            pending, i = None, end
        elif ch == "(":
            stack.append(prev)
            i += 1
        elif ch == ")":
            prev = stack.pop()
            i += 1
        elif ch == ".":
            prev = None
            i += 1
        else:
            assert ch in "-=#:/\\" and pending is None, "unexpected %r in %r" % (ch, text)
            pending = (ch, i)
            i += 1
    assert not open_rings and not stack and pending is None
    return count, bonds


def turn(p, q, r):
    """+1 if p -> q -> r turns one way, -1 the other, 0 on a line"""
    t = (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])
    return (t > 0) - (t < 0)


def apart(n, edge, a, b):
    """does atom b fall off atom a when the bond between them is taken out"""
    seen, todo = {a}, [a]
    while todo:
        x = todo.pop()
        for pair in edge:
            if x in pair and pair != frozenset((a, b)):
                (y,) = pair - {x}
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
    return b not in seen


def double_bonds(atoms, bonds, implh):
    """-> (codes per bond row, marked {(a, b): {(end, substituent): turn a -> b -> substituent}}), 0-based, a < b"""
    n = len(atoms)
    symbols, charges, _, listed, edge = O.classes(atoms, bonds, implh)
    around = [sorted(x for pair in edge if a in pair for x in pair if x != a) for a in range(n)]
    where = [(int(r[0]), int(r[1])) for r in atoms]
    codes, marked = [NONE] * len(bonds), {}
    for k, row in enumerate(bonds):
        if int(row[2]) != 2:
            continue
        a, b = sorted((int(row[0]) - 1, int(row[1]) - 1))
        subs = {a: [x for x in around[a] if x != b], b: [x for x in around[b] if x != a]}
        if not all(symbols[e] in ("C", "N") and 1 <= len(subs[e]) <= 2 and all(edge[frozenset((e, x))] == 1 for x in subs[e]) for e in (a, b)):
            continue
        if not apart(n, edge, a, b):
            codes[k] = RING
            continue
        if any(len(subs[e]) == 2 and all(len(around[x]) == 1 for x in subs[e])
               and len({(symbols[x], charges[x], listed[x]) for x in subs[e]}) == 1 for e in (a, b)):
            codes[k] = TWIN
            continue
        six = [a, b] + subs[a] + subs[b]
        turns = {(e, x): turn(where[a], where[b], where[x]) for e in (a, b) for x in subs[e]}
        if (any(not 0 <= v <= LIMIT for x in six for v in where[x]) or 0 in turns.values()
                or any(len(subs[e]) == 2 and len({turns[(e, x)] for x in subs[e]}) == 1 for e in (a, b))):
            codes[k] = FLAT
            continue
        codes[k] = 1 if turns[(a, subs[a][0])] == turns[(b, subs[b][0])] else -1
        marked[(a, b)] = turns
    return codes, marked


def write(atoms, bonds, implh, tetrahedral=False):
    """rows as smiles_oracle.write takes them -> (text with "/" and "\\", codes per bond row, stats (marked, flat, ring, twin),
    marked: as double_bonds gives it); smiles_oracle.Refused as there"""
    base = S.write(atoms, bonds, implh)[0] if tetrahedral else O.write(atoms, bonds, implh)
    codes, marked = double_bonds(atoms, bonds, implh)
    n, in_text = bonds_in_text(base)
    preorder = S.preorder_of(len(atoms), bonds)
    assert n == len(atoms)
    written = {}      # frozenset(atom pair) -> (first, second, offset) by atom index
    for first, second, symbol, offset in in_text:
        written[frozenset((preorder[first], preorder[second]))] = (preorder[first], preorder[second], offset, symbol)
    symbol_of = {}    # frozenset(atom pair) -> the symbol as the text reads the bond
    claimed = sorted((written[frozenset(es)][2], frozenset(es)) for turns in marked.values() for es in turns)

    def outward(e, x):
        """the symbol of the bond e - x read from e, None if not set"""
        c = symbol_of.get(frozenset((e, x)))
        return None if c is None else (c if written[frozenset((e, x))][0] == e else FLIP[c])

    for _, pair in claimed:
        if pair in symbol_of:
            continue
        symbol_of[pair] = "/"
        changed = True
        while changed:
            changed = False
            for turns in marked.values():
                known = {turns[es]: outward(*es) for es in turns if outward(*es) is not None}
                if not known:
                    continue
                t0, c0 = next(iter(known.items()))
                for (e, x), t in turns.items():
                    c = c0 if t == t0 else FLIP[c0]
                    if outward(e, x) is None:
                        symbol_of[frozenset((e, x))] = c if written[frozenset((e, x))][0] == e else FLIP[c]
                        changed = True
                    else:
                        assert outward(e, x) == c, "the symbols around a double bond contradict each other"
    text = base
    for pair, c in sorted(symbol_of.items(), key=lambda kv: -written[kv[0]][2]):
        _, _, offset, symbol = written[pair]
        assert symbol == "", "a marked bond with a symbol of its own in %r" % base
        text = text[:offset] + c + text[offset:]
    stats = (sum(c in (1, -1) for c in codes), codes.count(FLAT), codes.count(RING), codes.count(TWIN))
    return text, codes, stats, marked


# ---------------------------------------------------------------------------------------------------------------- the reader
def read(text):
    """a SMILES of the writer's subset with "/" and "\\" -> {(i, j, x, y): "together" | "opposite"} by TEXT position of the atoms,
    for every "=" bond i - j (i < j) and every marked neighbour x of i and y of j"""
    n, bonds = bonds_in_text(text)
    height = {}       # (end, neighbour) -> +1 the neighbour is above the end, -1 below
    for first, second, symbol, _ in bonds:
        if symbol in FLIP:
            up = 1 if symbol == "/" else -1       # the second atom, seen from the first
            height[(first, second)] = up
            height[(second, first)] = -up
    out = {}
    for first, second, symbol, _ in bonds:
        if symbol != "=":
            continue
        i, j = sorted((first, second))
        for (e, x), hx in height.items():
            for (f, y), hy in height.items():
                if e == i and f == j and x != j and y != i:
                    out[(i, j, x, y)] = "together" if hx == hy else "opposite"
    return out


def strip(text):
    return re.sub(r"[/\\]", "", text)
