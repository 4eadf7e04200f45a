"""Test infrastructure, not product: the reading rule of DESIGN.md section 7 ("Reading a SMILES") written a second time -- a regular
expression cuts the tokens, a recursive descent over the OpenSMILES-style productions

    smiles        := chain ('.' chain)*
    chain         := branched_atom (bond? branched_atom)*
    branched_atom := atom ringbond* branch*
    ringbond      := bond? (digit | '%' digit digit)
    branch        := '(' bond? chain ')'

builds the graph.  It shares no code with abcnet_amd.decode.parse_smiles."""
import re
import sys

OK, EMPTY, TOO_LONG, SYNTAX, TRUNCATED, DUPLICATE = range(6)
MAX_BYTES = 4096
VOCAB = {"C": 1, "N": 2, "O": 3, "P": 4, "F": 5, "Cl": 6, "S": 7, "Br": 8, "B": 9, "Se": 10, "I": 11, "H": 12, "Si": 13}
TOKEN = re.compile(r"(?P<bracket>\[[^\[\]]*\])|(?P<atom>Cl|Br|[BCNOPSFI]|[bcnops]|\*)|(?P<bond>[-=#:/\\])|(?P<ring>%[0-9][0-9]|[0-9])"
                   r"|(?P<open>\()|(?P<close>\))|(?P<dot>\.)")
BRACKET = re.compile(r"\[[0-9]*(?P<symbol>\*|[A-Z][a-z]?|se|as|te|[bcnops])(?:@@?(?:[A-Z][A-Z][0-9]+)?)?(?:H[0-9]?)?"
                     r"(?P<charge>\+[0-9][0-9]?|-[0-9][0-9]?|\+{1,3}|-{1,3})?(?::[0-9]+)?\]")
ORDER = {"-": 1, "/": 1, "\\": 1, "=": 2, "#": 3, ":": 4}


class Refused(Exception):
    pass


def tokens(text):
    out, at = [], 0
    while at < len(text):
        m = TOKEN.match(text, at)
        if m is None:
            raise Refused("no token at byte %d" % at)
        out.append((m.lastgroup, m.group()))
        at = m.end()
    return out


def atom_of(kind, word):
    """(class, charge, aromatic)"""
    if kind == "atom":
        return (-1 if word == "*" else VOCAB[word.capitalize()]), 0, word.islower()
    m = BRACKET.fullmatch(word)
    if m is None:
        raise Refused("bracket atom %r" % word)
    symbol, charge = m.group("symbol"), m.group("charge") or ""
    value = 0
    if charge:
        value = int(charge[1:]) if charge[1:].isdigit() else len(charge)
        value = value if charge[0] == "+" else -value
        if not -15 <= value <= 15:
            raise Refused("charge %r" % charge)
    return VOCAB.get(symbol.capitalize(), -1), value, symbol[0].islower()


class Descent:
    def __init__(self, toks):
        self.toks, self.at = toks, 0
        self.atoms, self.aromatic, self.bonds, self.open = [], [], [], {}

    def kind(self, ahead=0):
        return self.toks[self.at + ahead][0] if self.at + ahead < len(self.toks) else "end"

    def take(self, kind):
        if self.kind() != kind:
            raise Refused("expected %s at token %d, found %s" % (kind, self.at, self.kind()))
        self.at += 1
        return self.toks[self.at - 1][1]

    def bond(self, i, j, symbols):
        orders = {ORDER[s] for s in symbols if s}
        if len(orders) > 1:
            raise Refused("two different symbols on one bond")
        self.bonds.append((i, j, orders.pop() if orders else (4 if self.aromatic[i] and self.aromatic[j] else 1)))

    def smiles(self):
        self.chain(None, None)
        while self.kind() == "dot":
            self.take("dot")
            self.chain(None, None)
        if self.kind() != "end":
            raise Refused("a token is left over at %d: %s" % (self.at, self.kind()))
        if self.open:
            raise Refused("rings left open: %s" % sorted(self.open))

    def chain(self, parent, symbol):
        """parent: the atom the chain hangs on (a branch) and the symbol read in front of it"""
        while True:
            kind = self.kind()
            if kind not in ("atom", "bracket"):
                raise Refused("expected an atom at token %d, found %s" % (self.at, kind))
            cls, charge, aromatic = atom_of(kind, self.take(kind))
            a = len(self.atoms)
            self.atoms.append((0, 0, cls, charge))
            self.aromatic.append(aromatic)
            if parent is not None:
                self.bond(parent, a, [symbol])
            while self.kind() == "ring" or (self.kind() == "bond" and self.kind(1) == "ring"):
                mark = self.take("bond") if self.kind() == "bond" else None
                word = self.take("ring")
                number = int(word.lstrip("%"))
                if number in self.open:
                    first, mark0 = self.open.pop(number)
                    if first == a:
                        raise Refused("ring %d opened and closed on one atom" % number)
                    self.bond(first, a, [mark0, mark])
                else:
                    self.open[number] = (a, mark)
            while self.kind() == "open":
                self.take("open")
                inner = self.take("bond") if self.kind() == "bond" else None
                self.chain(a, inner)
                self.take("close")
            parent, symbol = a, None
            if self.kind() == "bond":
                symbol = self.take("bond")
            elif self.kind() not in ("atom", "bracket"):
                return


def parse(text, max_atoms=None, max_bonds=None):
    """-> (status, atoms [(0, 0, class, charge)], bonds [(i, j, order)]): empty lists with every status but OK"""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    if len(text) == 0:
        return EMPTY, [], []
    if len(text) > MAX_BYTES:
        return TOO_LONG, [], []
    try:
        d = Descent(tokens(text))
        d.smiles()
    except Refused:
        return SYNTAX, [], []
    if (max_atoms is not None and len(d.atoms) > max_atoms) or (max_bonds is not None and len(d.bonds) > max_bonds):
        return TRUNCATED, [], []
    if len({(i, j) for i, j, _ in d.bonds}) < len(d.bonds):
        return DUPLICATE, [], []
    return OK, d.atoms, d.bonds
