// frameshift_seq.hpp — what mgta_seqs_frameshift (frameshift.hip) and the `megagta nearest --frameshift` writer share about sequences:
// the nucleotide code, the codon table (the 64 letters main_translate and astar.hip hold, codon = 16 * b0 + 4 * b1 + b2), the residue of
// the codon that ends at a nucleotide row, and, from a state path over 'M' '<' '>' 'I' 'D', the corrected protein, the corrected
// nucleotides and the shift positions.  Plain C++ (no HIP headers): host/frameshift_seq_check.cpp runs it under the sanitizers.
#pragma once
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define MGTA_FS_HD __host__ __device__
#else
#define MGTA_FS_HD
#endif

namespace mgta {

// A, C, G, T of either case are 0 .. 3, every other byte is 4 (unknown)
MGTA_FS_HD inline uint32_t nt_code(uint32_t b) {
    const uint32_t u = b | 32u;
    return b >= 128u ? 4u : u == 'a' ? 0u : u == 'c' ? 1u : u == 'g' ? 2u : u == 't' ? 3u : 4u;
}

// the residue of the codon (b0, b1, b2) by the standard code: 'X' when a letter is unknown, '*' for a stop
MGTA_FS_HD inline char codon_residue(uint32_t b0, uint32_t b1, uint32_t b2) {
    const uint32_t c0 = nt_code(b0), c1 = nt_code(b1), c2 = nt_code(b2);
    if ((c0 | c1 | c2) > 3u) return 'X';
    return "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"[16u * c0 + 4u * c1 + c2];
}

// a(i), i >= 3 (1-based): the residue of (x_{i-2}, x_{i-1}, x_i)
MGTA_FS_HD inline char codon_residue_at(const uint8_t *x, int i) { return codon_residue(x[i - 3], x[i - 2], x[i - 1]); }

// What a path makes of its contig.  prot and nucl: the corrected sequences ('M' the residue and its three letters; '>' the residue of
// the last three of four letters, and those three; '<' X and its two letters and N; 'I' residue and letters in lower case; 'D'
// nothing), nucl three times as long as prot.  shifts: `.` or a comma list of -i (a short codon that ends at nucleotide i, 1-based)
// and +i (the dropped letter of a long codon).  false when the path has another character or does not consume exactly the L letters.
struct Corrected { std::string prot, nucl, shifts; };
inline bool corrected_of(const char *x, size_t L, const char *path, size_t path_len, Corrected *out) {
    out->prot.clear(); out->nucl.clear(); out->shifts.clear();
    const uint8_t *u = reinterpret_cast<const uint8_t *>(x);
    const auto lower = [](char c) { return (c >= 'A' && c <= 'Z') ? (char)(c + 32) : c; };
    size_t pos = 0;                                                       // letters consumed
    for (size_t p = 0; p < path_len; ++p) {
        const char s = path[p];
        const size_t take = (s == 'M' || s == 'I') ? 3 : s == '<' ? 2 : s == '>' ? 4 : s == 'D' ? 0 : 5;
        if (take == 5 || pos + take > L) return false;
        if (s == 'M' || s == '>') {
            if (s == '>') { out->shifts += (out->shifts.empty() ? "+" : ",+") + std::to_string(pos + 1); ++pos; }
            out->prot += codon_residue(u[pos], u[pos + 1], u[pos + 2]);
            out->nucl.append(x + pos, 3);
            pos += 3;
        } else if (s == '<') {
            out->prot += 'X';
            out->nucl.append(x + pos, 2);
            out->nucl += 'N';
            pos += 2;
            out->shifts += (out->shifts.empty() ? "-" : ",-") + std::to_string(pos);
        } else if (s == 'I') {
            out->prot += lower(codon_residue(u[pos], u[pos + 1], u[pos + 2]));
            for (int k = 0; k < 3; ++k) out->nucl += lower(x[pos + k]);
            pos += 3;
        }
    }
    if (out->shifts.empty()) out->shifts = ".";
    return pos == L;
}

}  // namespace mgta
