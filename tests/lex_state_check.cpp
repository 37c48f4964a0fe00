// clipcap_amd/csrc/lex_state.h on its own, on the host: includes only that header (no HIP include path), reads a phrase table and the
// expected transition / tokens_met / full values that the Python statement (tests/lexbeam_ref.py) printed, and checks every one.
//   file: "n_phr phr_len V" | n_phr * phr_len table entries | count | count lines "state v next tokens_met_of_state" | "full"
#include "lex_state.h"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: lex_state_check <cases file>\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n_phr = 0, phr_len = 0, V = 0;
    if (std::fscanf(f, "%d %d %d", &n_phr, &phr_len, &V) != 3 || n_phr < 0 || n_phr > LEX_MAX_PHR || phr_len < 1 || phr_len > LEX_MAX_LEN) return 2;
    std::vector<int32_t> table((size_t)n_phr * phr_len + 1, -1);
    for (int i = 0; i < n_phr * phr_len; i++)
        if (std::fscanf(f, "%d", &table[i]) != 1) return 2;
    long count = 0, bad = 0;
    if (std::fscanf(f, "%ld", &count) != 1) return 2;
    for (long i = 0; i < count; i++) {
        int state, v, next, met;
        if (std::fscanf(f, "%d %d %d %d", &state, &v, &next, &met) != 4) return 2;
        const int32_t got = lex_next(state, v, table.data(), n_phr, phr_len);
        const int gmet = lex_tokens_met(state, table.data(), n_phr, phr_len);
        if (got != next || gmet != met || lex_pack(lex_met(state), lex_cur(state), lex_pos(state)) != state) {
            if (bad++ < 10) std::printf("state %#x v %d: next %#x (want %#x), tokens_met %d (want %d)\n", state, v, got, next, gmet, met);
        }
    }
    int full = -1;
    if (std::fscanf(f, "%d", &full) != 1) return 2;
    if (lex_full(table.data(), n_phr, phr_len) != full) { std::printf("full %#x (want %#x)\n", lex_full(table.data(), n_phr, phr_len), full); bad++; }
    std::fclose(f);
    if (bad) { std::printf("FAILED: %ld of %ld\n", bad, count); return 1; }
    std::printf("ok: %ld transitions, V %d\n", count, V);
    return 0;
}
