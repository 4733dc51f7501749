// d2g_alphabet.h -- the amino-acid alphabets of --protein / --protein14 / --protein8 / --protein6 (spec "D2G-AA", DESIGN section 3
// K1a) on the host alone: the residue groups, their sizes and the largest k whose key fits 64 bits.  The reference keeps these in
// the absent bonsai; ids and names are those of its python/parse.py:8-23.  Header-only, so that the packer (d2g_seqpack.cpp) and the
// plan (d2g_plan.cpp) each build without the other, as the sanitizer programs do.
#pragma once
#include "../../include/d2g.h"
#include <cstdint>

// residue groups of an alphabet, separated by spaces; a residue's code is the position of its group.  nullptr: not a protein alphabet
inline const char *d2g_aa_groups(int alphabet) {
    switch (alphabet) {
    case D2G_ALPHABET_PROTEIN20: return "A C D E F G H I K L M N P Q R S T V W Y";
    case D2G_ALPHABET_PROTEIN_14: return "A C D EQ FY G H IV KR LM N P ST W";          // SE-B(14)
    case D2G_ALPHABET_PROTEIN_3BIT: return "AST C DHN EKQR FWY G ILMV P";               // SE-B(8)
    case D2G_ALPHABET_PROTEIN_6: return "AST CP DEHKNQR FWY G ILMV";                    // SE-B(6)
    default: return nullptr;
    }
}
inline bool d2g_is_protein(int alphabet) { return d2g_aa_groups(alphabet) != nullptr; }
// symbols of the alphabet: 4 for DNA, 0 for an unknown id
inline int d2g_alphabet_size_of(int alphabet) {
    if (alphabet == D2G_ALPHABET_DNA) return 4;
    const char *g = d2g_aa_groups(alphabet);
    if (!g) return 0;
    int n = 1;
    for (; *g; ++g) n += *g == ' ';
    return n;
}
// the largest k with A^k <= 2^64 (DNA: 32); 0 for an unknown id
inline int d2g_alphabet_max_k_of(int alphabet) {
    const unsigned __int128 A = (unsigned)d2g_alphabet_size_of(alphabet), lim = (unsigned __int128)1 << 64;
    if (A == 0) return 0;
    int k = 0;
    for (unsigned __int128 p = A; p <= lim; p *= A) ++k;
    return k;
}
// code of a byte (letters of either case), -1 for anything that ends a run
inline int d2g_alphabet_code_of(int alphabet, unsigned char byte) {
    const unsigned char c = byte >= 'a' && byte <= 'z' ? (unsigned char)(byte - 'a' + 'A') : byte;
    if (alphabet == D2G_ALPHABET_DNA) return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
    const char *g = d2g_aa_groups(alphabet);
    if (!g || c < 'A' || c > 'Z') return -1;
    for (int code = 0; *g; ++g) {
        if (*g == ' ') ++code;
        else if ((unsigned char)*g == c) return code;
    }
    return -1;
}
// bits of the widest key of (k, alphabet): 2k for DNA, the bit length of A^k - 1 for a protein alphabet (0 outside [1, max k])
inline int d2g_key_bits_of(int k, int alphabet) {
    if (k < 1 || k > d2g_alphabet_max_k_of(alphabet)) return 0;
    if (alphabet == D2G_ALPHABET_DNA) return 2 * k;
    unsigned __int128 top = 1;
    for (int j = 0; j < k; ++j) top *= (unsigned)d2g_alphabet_size_of(alphabet);
    top -= 1;
    int bits = 0;
    for (; top; top >>= 1) ++bits;
    return bits;
}
