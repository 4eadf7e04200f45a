// The grammar of the SMILES reader ("Reading a SMILES"; decode.parse_smiles is the host form), one function per
// token class and one per decision, for csrc/smiles_read.hip AND for a plain C++ build: nothing here needs a device.
// A string is n bytes at s; no function reads outside s[0 .. n).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SMILES_HD __host__ __device__ inline
#else
#define SMILES_HD inline
#endif

namespace smiles_read {

// token classes (three bits; NONE is also "before the first token", END "behind the last")
enum { T_NONE = 0, T_ATOM = 1, T_BOND = 2, T_RING = 3, T_OPEN = 4, T_CLOSE = 5, T_DOT = 6, T_BAD = 7, T_END = 8 };
struct Token {
    int cls, len;        // class, bytes
    int val;             // ATOM: the record's atom class (-1 .. 13); BOND: the order 1 .. 4; RING: the number 0 .. 99
    int charge;          // ATOM
    bool aromatic;       // ATOM: written in lower case
};

SMILES_HD int at(const uint8_t* s, int n, int i) { return i >= 0 && i < n ? s[i] : 0; }
SMILES_HD bool is_digit(int c) { return c >= '0' && c <= '9'; }
SMILES_HD bool is_upper(int c) { return c >= 'A' && c <= 'Z'; }
SMILES_HD bool is_lower(int c) { return c >= 'a' && c <= 'z'; }

// the record's atom class of a symbol (first letter in upper case, second letter or 0): the index of raster.ATOM_VOCAB, -1 outside it
SMILES_HD int atom_class(int c0, int c1) {
    if (c1 == 0) {
        switch (c0) {
            case 'C': return 1;
            case 'N': return 2;
            case 'O': return 3;
            case 'P': return 4;
            case 'F': return 5;
            case 'S': return 7;
            case 'B': return 9;
            case 'I': return 11;
            case 'H': return 12;
            default: return -1;
        }
    }
    if (c0 == 'C' && c1 == 'l') return 6;
    if (c0 == 'B' && c1 == 'r') return 8;
    if (c0 == 'S' && c1 == 'e') return 10;
    if (c0 == 'S' && c1 == 'i') return 13;
    return -1;
}

// the order of a bond symbol, 0 for any other byte
SMILES_HD int bond_order(int c) {
    switch (c) {
        case '-': case '/': case '\\': return 1;
        case '=': return 2;
        case '#': return 3;
        case ':': return 4;
        default: return 0;
    }
}
// no symbol: 4 between two atoms written aromatic, else 1 (the OpenSMILES reading)
SMILES_HD int implicit_order(bool aromatic_a, bool aromatic_b) { return aromatic_a && aromatic_b ? 4 : 1; }
// a ring bond: the orders of the symbols at its opening and its closing (0: none); 0 when the two differ
SMILES_HD int ring_order(int at_open, int at_close, bool aromatic_a, bool aromatic_b) {
    if (at_open && at_close && at_open != at_close) return 0;
    return at_open ? at_open : (at_close ? at_close : implicit_order(aromatic_a, aromatic_b));
}

// Byte i OUTSIDE a bracket atom: does a token start here?  Not at the second byte of Cl / Br and not at the digits of %nn (a `C`,
// `B` or `%` outside a bracket always starts a token, so one or two bytes back decide)
SMILES_HD bool is_start(const uint8_t* s, int n, int i) {
    const int c = s[i], p = at(s, n, i - 1);
    if (c == 'l') return p != 'C';
    if (c == 'r') return p != 'B';
    if (is_digit(c)) return !(p == '%' || (is_digit(p) && at(s, n, i - 2) == '%'));
    return true;
}

// an atom outside brackets: B C N O P S F Cl Br I, b c n o p s, *
SMILES_HD bool bare_atom(const uint8_t* s, int n, int i, Token& t) {
    const int c = s[i], c1 = at(s, n, i + 1);
    t.cls = T_ATOM, t.len = 1, t.charge = 0, t.aromatic = false;
    if ((c == 'C' && c1 == 'l') || (c == 'B' && c1 == 'r')) {
        t.len = 2, t.val = atom_class(c, c1);
        return true;
    }
    if (c == 'B' || c == 'C' || c == 'N' || c == 'O' || c == 'P' || c == 'S' || c == 'F' || c == 'I') {
        t.val = atom_class(c, 0);
        return true;
    }
    if (c == 'b' || c == 'c' || c == 'n' || c == 'o' || c == 'p' || c == 's') {
        t.val = atom_class(c - 0x20, 0), t.aromatic = true;
        return true;
    }
    t.val = -1;
    return c == '*';
}

// a bracket atom, s[i] == '[':  isotope? symbol chirality? hcount? charge? class? ']'
SMILES_HD bool bracket_atom(const uint8_t* s, int n, int i, Token& t) {
    int k = i + 1;
    t.cls = T_ATOM, t.charge = 0, t.aromatic = false, t.val = -1, t.len = 0;
    while (is_digit(at(s, n, k))) ++k;                                   // isotope: dropped
    const int c = at(s, n, k), c1 = at(s, n, k + 1);
    if (c == '*') {
        k += 1;
    } else if (is_upper(c)) {                                             // no periodic-table check
        const bool two = is_lower(c1);
        t.val = atom_class(c, two ? c1 : 0), k += two ? 2 : 1;
    } else if ((c == 's' && c1 == 'e') || (c == 'a' && c1 == 's') || (c == 't' && c1 == 'e')) {
        t.val = atom_class(c - 0x20, c1), t.aromatic = true, k += 2;
    } else if (c == 'b' || c == 'c' || c == 'n' || c == 'o' || c == 'p' || c == 's') {
        t.val = atom_class(c - 0x20, 0), t.aromatic = true, k += 1;
    } else {
        return false;
    }
    if (at(s, n, k) == '@') {                                             // chirality: dropped
        k += at(s, n, k + 1) == '@' ? 2 : 1;
        if (is_upper(at(s, n, k)) && is_upper(at(s, n, k + 1)) && is_digit(at(s, n, k + 2))) {
            k += 2;
            while (is_digit(at(s, n, k))) ++k;
        }
    }
    if (at(s, n, k) == 'H') k += is_digit(at(s, n, k + 1)) ? 2 : 1;       // hydrogens: dropped
    const int sign = at(s, n, k);
    if (sign == '+' || sign == '-') {
        int m;
        ++k;
        if (is_digit(at(s, n, k))) {                                      // one or two digits
            m = at(s, n, k++) - '0';
            if (is_digit(at(s, n, k))) m = 10 * m + (at(s, n, k++) - '0');
        } else {                                                          // the sign up to three times
            m = 1;
            while (m < 3 && at(s, n, k) == sign) ++m, ++k;
        }
        if (m > 15) return false;
        t.charge = sign == '+' ? m : -m;
    }
    if (at(s, n, k) == ':') {                                             // atom class: dropped
        if (!is_digit(at(s, n, k + 1))) return false;
        ++k;
        while (is_digit(at(s, n, k))) ++k;
    }
    if (at(s, n, k) != ']') return false;
    t.len = k + 1 - i;
    return true;
}

// a ring number: one digit, or % and two digits
SMILES_HD bool ring_number(const uint8_t* s, int n, int i, Token& t) {
    t.cls = T_RING, t.charge = 0, t.aromatic = false;
    if (s[i] == '%') {
        const int a = at(s, n, i + 1), b = at(s, n, i + 2);
        t.len = 3, t.val = 10 * (a - '0') + (b - '0');
        return is_digit(a) && is_digit(b);
    }
    t.len = 1, t.val = s[i] - '0';
    return is_digit(s[i]);
}

// the token that starts at byte i (is_start, or a '['); T_BAD for anything outside the grammar
SMILES_HD Token classify(const uint8_t* s, int n, int i) {
    Token t;
    const int c = s[i];
    bool ok;
    if (c == '[') ok = bracket_atom(s, n, i, t);
    else if (c == '%' || is_digit(c)) ok = ring_number(s, n, i, t);
    else if (bond_order(c)) t.cls = T_BOND, t.len = 1, t.val = bond_order(c), t.charge = 0, t.aromatic = false, ok = true;
    else if (c == '(' || c == ')' || c == '.') t.cls = c == '(' ? T_OPEN : (c == ')' ? T_CLOSE : T_DOT), t.len = 1, t.val = 0, t.charge = 0, t.aromatic = false, ok = true;
    else ok = bare_atom(s, n, i, t);
    if (!ok) t.cls = T_BAD, t.len = 1;
    return t;
}

// May a token of class c follow one of class p, itself behind one of class p2?  (NONE: the start; c == END: the end of the string.)
// Together with the nesting depth -- never below zero, zero at a dot and at the end -- and the ring pairing this is the whole
// grammar above the tokens: an atom first and behind a dot; a symbol is followed by an atom or by a ring number, the latter only
// where the number could stand without it; `(` is followed by a symbol or an atom; a ring number stands behind its atom, another
// number or their symbol, never behind `)`.
SMILES_HD bool follows(int p2, int p, int c) {
    if (c == T_BAD || c == T_NONE) return false;
    switch (p) {
        case T_NONE: case T_DOT: return c == T_ATOM;
        case T_ATOM: case T_RING: return true;
        case T_BOND: return c == T_ATOM || (c == T_RING && (p2 == T_ATOM || p2 == T_RING));
        case T_OPEN: return c == T_ATOM || c == T_BOND;
        case T_CLOSE: return c != T_RING;
        default: return false;
    }
}

}  // namespace smiles_read
