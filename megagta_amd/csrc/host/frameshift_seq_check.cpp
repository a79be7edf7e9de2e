// frameshift_seq_check.cpp — stand-alone check of frameshift_seq.hpp (no device, no HIP): the nucleotide code, the codon table, the
// residue of the codon that ends at a row, and what a state path makes of its contig (corrected protein, corrected nucleotides, shift
// positions) on designed cases and on random paths, with the refusals.  Build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all host/frameshift_seq_check.cpp -o frameshift_seq_check
// and run it: it prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../frameshift_seq.hpp"

using namespace mgta;

static int fail(const char *what, const std::string &a = "", const std::string &b = "") {
    std::fprintf(stderr, "frameshift_seq_check: %s (%s, %s)\n", what, a.c_str(), b.c_str());
    return 1;
}

static int check_codons() {
    const char *nt = "ACGT";
    const char *table = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";
    for (int b = 0; b < 256; ++b) {
        const uint32_t want = b == 'A' || b == 'a' ? 0 : b == 'C' || b == 'c' ? 1 : b == 'G' || b == 'g' ? 2 : b == 'T' || b == 't' ? 3 : 4;
        if (nt_code((uint32_t)b) != want) return fail("nt_code", std::to_string(b));
    }
    for (int c = 0; c < 64; ++c) {
        const char x[3] = {nt[c >> 4], nt[(c >> 2) & 3], (char)(nt[c & 3] | 32)};
        if (codon_residue((uint8_t)x[0], (uint8_t)x[1], (uint8_t)x[2]) != table[c]) return fail("codon_residue", std::string(x, 3));
        if (codon_residue_at(reinterpret_cast<const uint8_t *>(x), 3) != table[c]) return fail("codon_residue_at", std::string(x, 3));
    }
    if (codon_residue('A', 'N', 'G') != 'X' || codon_residue('-', 'A', 'A') != 'X' || codon_residue('A', 'A', 0xC1) != 'X' || codon_residue('U', 'A', 'A') != 'X')
        return fail("an unknown letter gives X");
    if (codon_residue('T', 'A', 'A') != '*' || codon_residue('t', 'g', 'a') != '*' || codon_residue('A', 'T', 'G') != 'M') return fail("stops and ATG");
    const uint8_t x[] = "GCTATGN";
    if (codon_residue_at(x, 3) != 'A' || codon_residue_at(x, 4) != 'L' || codon_residue_at(x, 6) != 'M' || codon_residue_at(x, 7) != 'X') return fail("rows");
    return 0;
}

static std::string upper(std::string s) {
    for (char &c : s)
        if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    return s;
}

// every corrected pair: three letters per residue, and they translate to it (ignoring case; N gives X)
static int check_pair(const Corrected &c) {
    if (c.nucl.size() != 3 * c.prot.size()) return fail("three letters per residue", c.prot, c.nucl);
    for (size_t r = 0; r < c.prot.size(); ++r) {
        const char a = codon_residue((uint8_t)c.nucl[3 * r], (uint8_t)c.nucl[3 * r + 1], (uint8_t)c.nucl[3 * r + 2]);
        if (a != upper(std::string(1, c.prot[r]))[0]) return fail("the nucleotides translate to the protein", c.prot, c.nucl);
    }
    return 0;
}

static int check_designed() {
    Corrected c;
    //                     M   <  D >    I   M
    const std::string x = "GCTAT" "CGAA" "tgg" "TAA";
    const std::string path = "M<D>IM";
    if (!corrected_of(x.data(), x.size(), path.data(), path.size(), &c)) return fail("a good path is refused");
    if (c.prot != "AXEw*" || c.nucl != "GCTATNGAAtggTAA" || c.shifts != "-5,+6") return fail("designed", c.prot + " " + c.nucl, c.shifts);
    if (check_pair(c)) return 1;
    if (!corrected_of("ACGTTT", 6, "MM", 2, &c) || c.prot != "TF" || c.nucl != "ACGTTT" || c.shifts != ".") return fail("in frame", c.prot, c.shifts);
    if (!corrected_of("acgNNN", 6, "MI", 2, &c) || c.prot != "Tx" || c.nucl != "acgnnn") return fail("case", c.prot, c.nucl);
    if (!corrected_of(nullptr, 0, "", 0, &c) || !c.prot.empty() || !c.nucl.empty() || c.shifts != ".") return fail("empty");
    if (!corrected_of("", 0, "DD", 2, &c) || !c.prot.empty()) return fail("deletes alone");
    // refusals: a path that is too long, too short, or has a foreign character
    if (corrected_of("ACGT", 4, "MM", 2, &c)) return fail("a path beyond the contig is accepted");
    if (corrected_of("ACGTT", 5, "M", 1, &c)) return fail("a path short of the contig is accepted");
    if (corrected_of("ACG", 3, "X", 1, &c)) return fail("a foreign character is accepted");
    if (corrected_of("ACG", 3, ">", 1, &c)) return fail("a long codon over three letters is accepted");
    return 0;
}

static int check_random() {
    uint64_t state = 0x9E3779B97F4A7C15ull;
    const auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
    const char *letters = "ACGTacgtN";
    for (int trial = 0; trial < 2000; ++trial) {
        std::string path, x;
        std::vector<long long> shifts;
        const int n_ops = (int)(next() % 40);
        for (int k = 0; k < n_ops; ++k) {
            const char s = "MMMM<>ID"[next() % 8];
            const size_t take = (s == 'M' || s == 'I') ? 3 : s == '<' ? 2 : s == '>' ? 4 : 0;
            if (s == '<') shifts.push_back(-(long long)(x.size() + 2));
            if (s == '>') shifts.push_back((long long)(x.size() + 1));
            for (size_t t = 0; t < take; ++t) x += letters[next() % 9];
            path += s;
        }
        // exactly sized copies, so that a read past either end is the sanitizer's to see
        std::vector<char> xs(x.begin(), x.end()), ps(path.begin(), path.end());
        Corrected c;
        if (!corrected_of(xs.data(), xs.size(), ps.data(), ps.size(), &c)) return fail("a random path is refused", path, x);
        if (check_pair(c)) return 1;
        std::string want;
        for (long long v : shifts) want += (want.empty() ? "" : ",") + std::string(v > 0 ? "+" : "") + std::to_string(v);
        if (want.empty()) want = ".";
        if (c.shifts != want) return fail("shifts", c.shifts, want);
        size_t residues = 0;
        for (char s : path) residues += s != 'D';
        if (c.prot.size() != residues) return fail("one residue per state but delete", path, c.prot);
        if (!xs.empty() && corrected_of(xs.data(), xs.size() - 1, ps.data(), ps.size(), &c)) return fail("a contig one letter short is accepted", path, x);
    }
    return 0;
}

int main() {
    if (check_codons() || check_designed() || check_random()) return 1;
    std::printf("ok\n");
    return 0;
}
