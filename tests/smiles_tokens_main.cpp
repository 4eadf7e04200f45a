// Test infrastructure, not product: the SMILES reader's steps (abc-net_amd/csrc/smiles_read.hip) run one after the other on the CPU,
// over the same token functions (csrc/smiles_tokens.hpp), so that the grammar can be compared with decode.parse_smiles -- and checked
// under a host sanitizer -- without a device:
//     c++ -std=c++17 -fsanitize=address,undefined -I abc-net_amd/csrc tests/smiles_tokens_main.cpp -o smiles_tokens_main
//     smiles_tokens_main cases.txt        one case per line: the string's bytes in hex ("-" for none), max_atoms, max_bonds
// prints per case one line: status, atoms, bonds, then (class charge) per atom and (i j order) per bond.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "smiles_tokens.hpp"

using namespace smiles_read;

enum { OK = 0, EMPTY = 1, TOO_LONG = 2, SYNTAX = 3, TRUNCATED = 4, DUPLICATE = 5, MAX_BYTES = 4096 };

struct Record {
    std::vector<int> atoms, bonds;      // (class, charge), (i, j, order)
};

static int read_one(const std::vector<uint8_t>& text, int max_atoms, int max_bonds, Record& out) {
    const int n = (int)text.size();
    if (n == 0) return EMPTY;
    if (n > MAX_BYTES) return TOO_LONG;
    const uint8_t* s = text.data();
    // 1: bytes -> tokens
    std::vector<Token> tok;
    int inside = 0;
    for (int i = 0; i < n; ++i) {
        bool start = false;
        if (s[i] == '[') { if (inside != 0) return SYNTAX; ++inside, start = true; }
        else if (s[i] == ']') { if (inside != 1) return SYNTAX; --inside; }
        else if (inside == 0) start = is_start(s, n, i);
        if (!start) continue;
        tok.push_back(classify(s, n, i));
        if (tok.back().cls == T_BAD) return SYNTAX;
    }
    if (inside != 0 || tok.empty()) return SYNTAX;
    // 2: the classes in a row, the depth, the atom in front of every token
    const int nt = (int)tok.size();
    std::vector<int> atom(nt), closing(nt, -1), order(nt, 0);
    std::vector<bool> aromatic;
    int depth = 0;
    for (int q = 0; q < nt; ++q) {
        const int c = tok[q].cls, p = q > 0 ? tok[q - 1].cls : T_NONE, p2 = q > 1 ? tok[q - 2].cls : T_NONE;
        if (!follows(p2, p, c) || (q == nt - 1 && !follows(p, c, T_END))) return SYNTAX;
        if (c == T_ATOM) aromatic.push_back(tok[q].aromatic);
        atom[q] = (int)aromatic.size() - 1;
        if (c == T_OPEN) ++depth;
        if (c == T_CLOSE && --depth < 0) return SYNTAX;
        if (c == T_DOT && depth != 0) return SYNTAX;
    }
    if (depth != 0) return SYNTAX;
    auto symbol_at = [&](int q) { return q > 0 && tok[q - 1].cls == T_BOND ? tok[q - 1].val : 0; };
    // 3: the ring numbers, one at a time; the brackets with a stack
    for (int number = 0; number <= 99; ++number) {
        int open = -1;
        for (int q = 0; q < nt; ++q) {
            if (tok[q].cls != T_RING || tok[q].val != number) continue;
            if (open < 0) { open = q; continue; }
            const int a = atom[open], a2 = atom[q];
            order[q] = ring_order(symbol_at(open), symbol_at(q), aromatic[a], aromatic[a2]);
            if (a == a2 || order[q] == 0) return SYNTAX;
            closing[q] = a, open = -1;
        }
        if (open >= 0) return SYNTAX;
    }
    std::vector<int> stack;
    for (int q = 0; q < nt; ++q) {
        if (tok[q].cls == T_OPEN) atom[q] = atom[q - 1], stack.push_back(atom[q]);
        else if (tok[q].cls == T_CLOSE) atom[q] = stack.back(), stack.pop_back();
    }
    auto predecessor = [&](int q, int& symbol) {
        symbol = symbol_at(q);
        const int f = q - (symbol ? 2 : 1);
        return f < 0 || tok[f].cls == T_DOT ? -1 : atom[f];
    };
    // 4, 5: the rows; a pair bonded twice
    bool twice = false;
    for (int q = 0; q < nt; ++q) {
        int symbol;
        if (tok[q].cls == T_ATOM) {
            out.atoms.push_back(tok[q].val), out.atoms.push_back(tok[q].charge);
            const int i = predecessor(q, symbol);
            if (i >= 0) out.bonds.insert(out.bonds.end(), {i, atom[q], symbol ? symbol : implicit_order(aromatic[i], tok[q].aromatic)});
        } else if (tok[q].cls == T_RING && closing[q] >= 0) {
            out.bonds.insert(out.bonds.end(), {closing[q], atom[q], order[q]});
            for (int f = q - 1; f >= 0; --f) {
                if (tok[f].cls == T_RING) twice |= closing[f] == closing[q];
                else if (tok[f].cls == T_ATOM) { twice |= predecessor(f, symbol) == closing[q]; break; }
                else if (tok[f].cls != T_BOND) break;
            }
        }
    }
    if ((int)out.atoms.size() / 2 > max_atoms || (int)out.bonds.size() / 3 > max_bonds) return TRUNCATED;
    return twice ? DUPLICATE : OK;
}

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s cases.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    std::vector<char> line(3 * MAX_BYTES + 64);
    while (fgets(line.data(), (int)line.size(), f)) {
        char* hex = strtok(line.data(), " \n");
        const char *a = strtok(nullptr, " \n"), *b = strtok(nullptr, " \n");
        if (!hex || !a || !b) continue;
        std::vector<uint8_t> text;
        if (strcmp(hex, "-") != 0)
            for (size_t i = 0; i + 1 < strlen(hex); i += 2) {
                const char byte[3] = {hex[i], hex[i + 1], 0};
                text.push_back((uint8_t)strtol(byte, nullptr, 16));
            }
        Record rec;
        const int status = read_one(text, atoi(a), atoi(b), rec);
        if (status != OK) rec = Record();
        printf("%d %d %d", status, (int)rec.atoms.size() / 2, (int)rec.bonds.size() / 3);
        for (int v : rec.atoms) printf(" %d", v);
        for (int v : rec.bonds) printf(" %d", v);
        printf("\n");
    }
    fclose(f);
    return 0;
}
