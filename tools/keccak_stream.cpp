// Feeds kck_words_to_elements (plonky2_demo_amd/csrc/keccak.cuh) -- the one function that turns the Keccak hash onion's words into the
// twelve elements of KeccakPermutation::permute (hash/keccak.rs:84-94), shared by the host Challenger and the proof-of-work kernel -- a
// SYNTHETIC word stream, four words per hash.  Its rejection branch (a word >= p) has probability 2^-32 per word and no real hash reaches
// it; tests/test_keccak.py compiles this file and compares with its own filter.  Host code only.
//   keccak_stream WANT w0 w1 w2 ...   (hex words, a multiple of four)  ->  "hashes_used e0 e1 ..." (hex)
#include <cstdio>
#include <cstdlib>
#include "keccak.cuh"

template <int WANT>
static int run(int nwords, char** words) {
    gl_t out[WANT] = {0};
    uint32_t have = 0;
    int used = 0;
    for (int i = 0; i + 4 <= nwords && have < (uint32_t)WANT; i += 4, used++) {
        uint64_t w[4];
        for (int k = 0; k < 4; k++) w[k] = strtoull(words[i + k], nullptr, 16);
        have = kck_words_to_elements<WANT>(w, have, out);
    }
    if (have < (uint32_t)WANT) { fprintf(stderr, "stream too short: %u of %d elements\n", have, WANT); return 1; }
    printf("%d", used);
    for (int k = 0; k < WANT; k++) printf(" %llx", (unsigned long long)out[k]);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2 || (argc - 2) % 4 != 0) { fprintf(stderr, "usage: keccak_stream WANT(8|12) words...\n"); return 2; }
    const int want = atoi(argv[1]);
    if (want == 12) return run<12>(argc - 2, argv + 2);
    if (want == 8) return run<8>(argc - 2, argv + 2);
    return 2;
}
