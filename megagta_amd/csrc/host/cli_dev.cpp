// cli_dev.cpp — the sub-commands that are no step of a run and open no device: `dumpversion`, the host-layer checks of the tests (read
// loaders, graph file reader and writer, HMMER3 parser, the plan of a search batch) and `sdbgmerge` of the multi-GPU driver.
#include "cli.hpp"

namespace mgta_cli {
int main_libdump(int argc, char **argv) {   // libdump <read_lib_prefix> lib|bin <out_prefix> [assist.fa]: writes what buildgraph / findstart would upload
    if (argc < 4) { fprintf(stderr, "Usage %s <read_lib_prefix> lib|bin <out_prefix> [assist.fa]\n", argv[0]); return 1; }
    PackedReads pr;
    if (std::string(argv[2]) == "bin") load_read_bin(std::string(argv[1]) + ".bin", true, pr);
    else load_read_lib(argv[1], true, pr);
    if (argc > 4) {
        if (env_int("MEGAGTA_LIBDUMP_TEXT", 0)) {                       // the in-memory route a worker takes for the contigs its `denovo` has just made
            FILE *tf = fopen(argv[4], "rb");
            if (!tf) die("cannot open %s", argv[4]);
            std::string text;
            char tb[1 << 16];
            for (size_t got; (got = fread(tb, 1, sizeof tb, tf)) > 0;) text.append(tb, got);
            fclose(tf);
            load_fasta_text(text.data(), text.size(), true, pr);
        } else load_assist_fasta(argv[4], true, pr);
    }
    pr.finish();
    FILE *fw = fopen((std::string(argv[3]) + ".words").c_str(), "wb"), *fs = fopen((std::string(argv[3]) + ".start").c_str(), "wb");
    if (!fw || !fs) die("cannot write %s.words / .start", argv[3]);
    fwrite(pr.words.data(), 4, pr.words.size(), fw);
    fwrite(pr.start.data(), 8, pr.start.size(), fs);
    fclose(fw); fclose(fs);
    printf("%zu %zu %d %llu\n", pr.start.size() - 1, pr.words.size(), pr.max_len, (unsigned long long)pr.n_short);
    return 0;
}
int main_sdbgcopy(int argc, char **argv) {   // sdbgcopy <in_prefix> <out_prefix>: the graph files read and written again (one .sdbg.0 file)
    if (argc < 3) { fprintf(stderr, "Usage %s <in_prefix> <out_prefix>\n", argv[0]); return 1; }
    EdgeStream s;
    double t0 = now_s();
    read_sdbg(argv[1], s);
    double t1 = now_s();
    write_sdbg(argv[2], s);
    logf("%zu records: read %.3f s, write %.3f s", s.recs.size(), t1 - t0, now_s() - t1);
    return 0;
}
int main_sdbgmerge(int argc, char **argv) {   // sdbgmerge <sdbg_prefix> <num_parts>: after a build over N GPUs, PREFIX.sdbg_info naming the N files
    if (argc < 3 || atoi(argv[2]) < 1) { fprintf(stderr, "Usage %s <sdbg_prefix> <num_parts>\n", argv[0]); return 1; }
    merge_sdbg_parts(argv[1], atoi(argv[2]));
    return 0;
}
int main_hmmdump(int argc, char **argv) {   // hmmdump <file.hmm>: the tables `search` uploads (the HMMER3 text parser + heuristic), as hex doubles
    if (argc != 2) { fprintf(stderr, "Usage: megagta hmmdump <file.hmm>\n"); return 1; }
    ProfileHmm hm;
    if (!parse_hmm(argv[1], hm)) die("cannot open HMM %s", argv[1]);
    const size_t M1 = (size_t)hm.M + 1;
    printf("M %d\nA %d\nalpha", hm.M, hm.A);
    for (int c = 0; c < 127; ++c) printf(" %d", hm.alpha[c]);
    printf("\ncompo");
    for (int j = 0; j < hm.A; ++j) printf(" %a", hm.compo[j]);
    printf("\n");
    for (int k = 0; k <= hm.M; ++k) {
        printf("msc %d", k);
        for (int j = 0; j < hm.A; ++j) printf(" %a", hm.msc[(size_t)k * hm.A + j]);
        printf("\ntsc %d", k);
        for (int t = 0; t < 7; ++t) printf(" %a", hm.tsc[(size_t)t * M1 + k]);
        printf("\nmaxm %d %a\nh %d %a %a %a\n", k, hm.max_match[k], k, hm.h[k], hm.h[M1 + k], hm.h[2 * M1 + k]);
    }
    return 0;
}
int main_searchplan(int argc, char **argv) {   // searchplan <n_seeds>...: the window and cost term `search` would take for batches of that many seeds
    for (int i = 1; i < argc; ++i) {
        int window = 0, rate = 0, rate2 = 0;
        long long knee = 0;
        search_plan((size_t)atoll(argv[i]), &window, &rate, &knee, &rate2);
        printf("%s %d %d %lld %d\n", argv[i], window, rate, knee, rate2);
    }
    return 0;
}
int main_dumpversion(int, char **) { printf("%s\n", mgta_version()); return 0; }

}  // namespace mgta_cli
