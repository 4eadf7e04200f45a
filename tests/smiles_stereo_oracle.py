"""Test infrastructure, not product: the tetrahedral rule of DESIGN.md section 7 a second and a third time.

`write` starts from the plain text of smiles_oracle.write and never looks at a walk: the order in which a SMILES names an atom's
neighbours is read OFF THAT TEXT (`structure`: the atom in front, a bracket's hydrogen, the ring numbers on the atom, the atoms behind),
the chirality is the sign of the 4 x 4 determinant of the homogeneous rows (x, y, z, 1) expanded over all 24 permutations, taken once
in text order (the mark) and once in index order (the code).  It shares no code and no formulation with abcnet_amd.decode.

`read` is the check of the checker: it takes a text with marks, the positions and the elevations in the text's own atom order and
recomputes every mark from what "@" MEANS -- look from the first neighbour toward the other three, put them on a screen, and ask which
way round they run (a signed area on that screen) -- with the hydrogen placed opposite the three drawn bonds."""
import itertools
import re

import smiles_oracle as O

NONE, FLAT, UNQUALIFIED = 0, 2, 3
LIMIT = 199999
ATOM = re.compile(r"\[[^\]]*\]|Cl|Br|[BCNOPSFIbcnops]")
HYDROGEN = "H"      # the name of a bracket's hydrogen in a neighbour list


# ------------------------------------------------------------------------------------------------------------------ the text
def structure(text):
    """-> (spans [(start, end)] of the atom tokens in text order, neighbours: per atom the atoms (by text order) and HYDROGEN in the
    order a SMILES names them, marks: per atom "", "@" or "@@", behind: per atom whether it stands behind an atom of its component,
    which is then the first it names).  Reads the writer's subset; a bracket's hydrogen counts once."""
    spans, neighbours, marks, behind = [], [], [], []
    open_rings, stack, prev, i = {}, [], None, 0
    while i < len(text):
        ch = text[i]
        m = ATOM.match(text, i)
        if m:
            a = len(spans)
            spans.append(m.span())
            neighbours.append([] if prev is None else [prev])
            behind.append(prev is not None)
            if prev is not None:
                neighbours[prev].append(a)
            body = m.group()
            marks.append("@@" if "@@" in body else ("@" if "@" in body else ""))
            inner = re.fullmatch(r"\[(Cl|Br|Se|Si|se|[BCNOPSFIHbcnops])(@{0,2})(H\d*)?([+-]\d*)?\]", body) if body[0] == "[" else None
            assert body[0] != "[" or inner, "a bracket token this reader does not know: %r" % body
            if inner and inner.group(3):
                assert inner.group(3) == "H" or not marks[-1], "a marked atom with more than one hydrogen"
                neighbours[a].append(HYDROGEN)
            prev, i = a, m.end()
        elif ch.isdigit() or ch == "%":
            k, i = (int(text[i + 1:i + 3]), i + 3) if ch == "%" else (int(ch), i + 1)
            if k in open_rings:
                x, at = open_rings.pop(k)
                neighbours[x][at] = prev
                neighbours[prev].append(x)
            else:
                open_rings[k] = (prev, len(neighbours[prev]))
                neighbours[prev].append(None)
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
            assert ch in "-=#:", "unexpected %r in %r" % (ch, text)
            i += 1
    assert not open_rings and not stack
    return spans, neighbours, marks, behind


def det4(rows):
    """the determinant of four rows of four integers, by its definition: the sum over all permutations"""
    total = 0
    for perm in itertools.permutations(range(4)):
        inversions = sum(perm[i] > perm[j] for i in range(4) for j in range(i + 1, 4))
        term = -1 if inversions % 2 else 1
        for r, c in enumerate(perm):
            term *= rows[r][c]
        total += term
    return total


def preorder_of(n, bonds):
    """the atoms in the order the rule's walk visits them: roots ascending, neighbours ascending"""
    nb = [[] for _ in range(n)]
    for row in bonds:
        nb[row[0] - 1].append(row[1] - 1)
        nb[row[1] - 1].append(row[0] - 1)
    seen, order = set(), []
    for root in range(n):
        todo = [root]
        while todo:
            a = todo.pop()
            if a in seen:
                continue
            seen.add(a)
            order.append(a)
            todo.extend(sorted((x for x in nb[a] if x not in seen), reverse=True))
    return order


def write(atoms, bonds, implh):
    """rows as smiles_oracle.write takes them -> (text with marks, preorder [atom index by text position], codes [per atom index:
    0, +1, -1, FLAT, UNQUALIFIED], stats (marked, flat, unqualified, wedge rows)); smiles_oracle.Refused as there"""
    plain = O.write(atoms, bonds, implh)
    n = len(atoms)
    symbols, charges, _, listed, edge = O.classes(atoms, bonds, implh)
    preorder = preorder_of(n, bonds)
    spans, named, _, behind = structure(plain)
    assert len(spans) == n and sorted(preorder) == list(range(n))
    place = {a: p for p, a in enumerate(preorder)}
    elevation = {}      # (centre, neighbour) -> +1 / -1, from the centre's OWN wedge rows
    for row in bonds:
        if int(row[2]) in (5, 6):
            elevation[(int(row[0]) - 1, int(row[1]) - 1)] = 1 if int(row[2]) == 5 else -1
    codes, insert = [NONE] * n, {}
    for a in sorted({c for c, _ in elevation}):
        around = sorted(x for pair in edge if a in pair for x in pair if x != a)
        d = len(around)
        if listed[a]:
            h = 1
        elif symbols[a] == "H" or abs(charges[a]) > 1:
            h = 0
        else:
            v = sum(3 if edge[frozenset((a, x))] == 4 else 2 * edge[frozenset((a, x))] for x in around) // 2
            h = next((t - v for t in O.VALENCES[symbols[a]][charges[a]] if t >= v), 0)
        if symbols[a] == "H" or any(edge[frozenset((a, x))] != 1 for x in around) or not ((d == 4 and h == 0) or (d == 3 and h == 1)):
            codes[a] = UNQUALIFIED
            continue
        xa, ya = int(atoms[a][0]), int(atoms[a][1])
        where = {x: (int(atoms[x][0]), int(atoms[x][1])) for x in around}
        if (any(not 0 <= v <= LIMIT for xy in list(where.values()) + [(xa, ya)] for v in xy)
                or any(xy == (xa, ya) for xy in where.values())):
            codes[a] = FLAT
            continue
        row = {x: (where[x][0] - xa, where[x][1] - ya, elevation.get((a, x), 0), 1) for x in around}
        row[HYDROGEN] = (0, 0, 0, 1)
        local = around + ([HYDROGEN] if d == 3 else [])
        t = det4([row[x] for x in local])
        if t == 0:
            codes[a] = FLAT
            continue
        codes[a] = 1 if t > 0 else -1
        in_text = [x if x == HYDROGEN else preorder[x] for x in named[place[a]]]
        if d == 3 and HYDROGEN not in in_text:      # a bare token names no hydrogen: the marked one will, behind the parent
            in_text.insert(1 if behind[place[a]] else 0, HYDROGEN)
        assert sorted(map(str, in_text)) == sorted(map(str, local))
        insert[place[a]] = ("@" if det4([row[x] for x in in_text]) > 0 else "@@", d == 3)
    out, at = [], 0
    for p, (lo, hi) in enumerate(spans):
        out.append(plain[at:lo])
        token = plain[lo:hi]
        if p in insert:
            mark, with_h = insert[p]
            if token[0] != "[":
                token = "[" + token + mark + ("H" if with_h else "") + "]"
            else:
                sym = re.match(r"\[(Cl|Br|Se|Si|[BCNOPSFIH])", token).end()
                token = token[:sym] + mark + token[sym:]
        out.append(token)
        at = hi
    out.append(plain[at:])
    stats = (sum(c in (1, -1) for c in codes), codes.count(FLAT), codes.count(UNQUALIFIED), sum(int(r[2]) in (5, 6) for r in bonds))
    return "".join(out), preorder, codes, stats


# ---------------------------------------------------------------------------------------------------------------- the reader
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def seen_from_first(points):
    """four points in space (integers, relative to the centre), in the order a SMILES names them -> +1 if, looking from the first
    toward the other three, they run counter-clockwise ("@"), -1 if clockwise ("@@"), 0 if they cannot be told (flat).
    The frame is right-handed (row down, column right, z toward the viewer), so the usual cross product holds."""
    eye, rest = points[0], points[1:]
    gaze = tuple(sum(p[k] for p in rest) - 3 * eye[k] for k in range(3))      # toward the middle of the three (times 3)
    if gaze == (0, 0, 0):
        return 0
    axis = min(((1, 0, 0), (0, 1, 0), (0, 0, 1)), key=lambda e: abs(_dot(e, gaze)))
    right = _cross(gaze, axis)          # on the screen, to the right ...
    up = _cross(right, gaze)            # ... and up: right x up points back at the eye, as on any screen one looks at
    assert _dot(_cross(right, up), gaze) < 0
    flat = [(_dot(p, right), _dot(p, up)) for p in rest]
    area2 = sum(flat[i][0] * flat[(i + 1) % 3][1] - flat[(i + 1) % 3][0] * flat[i][1] for i in range(3))
    return (area2 > 0) - (area2 < 0)


def read(text, positions, elevations):
    """text: a SMILES of the writer's subset with marks; positions [(x, y)] and elevations {(centre, neighbour): +1 / -1}, both by
    TEXT order of the atoms -> {text position: (the mark written, the mark the geometry gives or "" for flat)} for every atom that
    carries a mark"""
    _, named, marks, _ = structure(text)
    assert len(named) == len(positions)
    out = {}
    for p, mark in enumerate(marks):
        if not mark:
            continue
        assert len(named[p]) == 4, "a marked atom with %d neighbours in %r" % (len(named[p]), text)
        real = [x for x in named[p] if x != HYDROGEN]
        assert len(real) >= 3 and len(set(real)) == len(real)
        rel = {x: (positions[x][0] - positions[p][0], positions[x][1] - positions[p][1], elevations.get((p, x), 0)) for x in real}
        rel[HYDROGEN] = tuple(-sum(rel[x][k] for x in real) for k in range(3))      # opposite the three drawn bonds
        turn = seen_from_first([rel[x] for x in named[p]])
        out[p] = (mark, {1: "@", -1: "@@", 0: ""}[turn])
    return out


def in_text_order(atoms, bonds, preorder):
    """the reader's two geometric arguments of rows whose text has the given preorder"""
    place = {a: p for p, a in enumerate(preorder)}
    positions = [(int(atoms[a][0]), int(atoms[a][1])) for a in preorder]
    elevations = {(place[int(r[0]) - 1], place[int(r[1]) - 1]): (1 if int(r[2]) == 5 else -1) for r in bonds if int(r[2]) in (5, 6)}
    return positions, elevations
