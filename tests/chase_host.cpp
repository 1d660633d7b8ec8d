// tests/chase_host.cpp — the threat analysis of the library (cchess_zero_amd/csrc/cz_chase.h, one lane = one position on the
// GPU) compiled for the HOST, so that tests/test_chase_host_cpu.py can hold the very same function to tests/chase_model.py on
// the CPU.  Built twice: as a shared library for ctypes, and (-DCHASE_HOST_MAIN) as a stand-alone program that the test links
// with -fsanitize=address,undefined and runs over a corpus it writes to files.  Test infrastructure: nothing in the product
// path uses it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../cchess_zero_amd/csrc/cz_chase.h"

extern "C" void czc_host_tables(const int16_t *lut, CzmTables *t) { memset(t, 0, sizeof *t); czm_build_tables(lut, t); }
extern "C" int czc_host_sizeof_tables(void) { return (int)sizeof(CzmTables); }
// boards [n][90], side [n] -> chase [n][4]; ok [n]: 0 for a refused board
extern "C" void czc_host_threats(const CzmTables *t, const uint8_t *boards, const uint8_t *side, int n, uint64_t *chase, uint8_t *ok) {
    for (int i = 0; i < n; ++i) {
        uint32_t w[23];
        unsigned char buf[92];
        memcpy(buf, boards + (size_t)i * 90, 90);
        buf[90] = buf[91] = 0;
        memcpy(w, buf, 92);
        uint32_t scratch[CZC_SCRATCH];
        uint64_t out[4];
        ok[i] = czc_position(w, side[i] ? 1 : 0, *t, [&scratch](int k) -> uint32_t & { return scratch[k]; }, out) ? 1 : 0;
        memcpy(chase + (size_t)i * 4, out, sizeof out);
    }
}
// what k_movegen_kingsafe's callers get from czk_attacked, for a test that the fly parameter left it alone:
// attacked [n]: is square k[i] attacked by side as[i]'s pieces (fly != 0: czk_attacked as they call it, else with fly = false)
extern "C" void czc_host_attacked(const CzmTables *t, const uint8_t *boards, const uint8_t *as, const uint8_t *k, int n, int fly, uint8_t *attacked) {
    for (int i = 0; i < n; ++i) {
        uint32_t w[23];
        unsigned char buf[92];
        memcpy(buf, boards + (size_t)i * 90, 90);
        buf[90] = buf[91] = 0;
        memcpy(w, buf, 92);
        const CzmSets S = czm_sets(w, as[i] ? 1 : 0);
        attacked[i] = fly ? czk_attacked(S.occ, czk_pieces(S), as[i] ? 1 : 0, k[i], t->knon[k[i]])
                          : czk_attacked(S.occ, czk_pieces(S), as[i] ? 1 : 0, k[i], t->knon[k[i]], false);
    }
}

#ifdef CHASE_HOST_MAIN
static std::vector<unsigned char> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    std::vector<unsigned char> v;
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
// chase_host LUT BOARDS SIDE OUT: the int16 [90][90] label table, n x 90 board bytes, n side bytes -> n x 4 uint64
int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s lut boards side out\n", argv[0]); return 2; }
    const std::vector<unsigned char> lut = slurp(argv[1]), boards = slurp(argv[2]), side = slurp(argv[3]);
    if (lut.size() != 90 * 90 * 2 || boards.size() != side.size() * 90) { fprintf(stderr, "bad input sizes\n"); return 2; }
    std::vector<int16_t> l(90 * 90);
    memcpy(l.data(), lut.data(), lut.size());
    CzmTables *t = new CzmTables;
    czc_host_tables(l.data(), t);
    const int n = (int)side.size();
    std::vector<uint64_t> chase((size_t)n * 4);
    std::vector<uint8_t> ok(n);
    czc_host_threats(t, boards.data(), side.data(), n, chase.data(), ok.data());
    delete t;
    FILE *f = fopen(argv[4], "wb");
    if (!f || fwrite(chase.data(), 8, chase.size(), f) != chase.size()) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
    fclose(f);
    printf("%d positions\n", n);
    return 0;
}
#endif
