// tests/tablebase_host.cpp — the index mapping and the per-index pass of the tablebase build (cchess_zero_amd/csrc/
// cz_tablebase.h: cztb_parse, cztb_unrank, cztb_rank, cztb_step, one lane = one index on the GPU) compiled for the HOST, so that
// tests/test_tablebase_host_cpu.py can hold the very same text to tests/tablebase_model.py on the CPU.  The loop around the step
// restates k_tb_pass's (cz_tablebase.hip) for one index at a time, IN PLACE like the kernel, and the driver restates
// Tablebase.build's: the closure of sub-signatures first, the stop rule of include/cchess_hip.h.
// Built twice: as a shared library for ctypes, and (-DTABLEBASE_HOST_MAIN) as a stand-alone program that the test builds with
// -fsanitize=address,undefined and runs over whole tables.  Test infrastructure: nothing in the product path uses it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>
#include "../cchess_zero_amd/csrc/cz_tablebase.h"

extern "C" int cztb_host_parse(const char *sig, int32_t *n, uint32_t *entries, uint8_t *code, uint8_t *dom, uint8_t *radix) {
    CztbDesc d;
    const int rc = cztb_parse(sig, &d);
    if (rc) return rc;
    *n = d.n;
    *entries = d.entries;
    memcpy(code, d.code, CZTB_MAX_SLOTS);
    memcpy(dom, d.dom, CZTB_MAX_SLOTS);
    memcpy(radix, d.radix, CZTB_MAX_SLOTS);
    return 0;
}

// the whole descriptor of sig (without < 0) or of cztb_without(sig's, without): fields [5][CZTB_MAX_SLOTS] = code, dom, radix, ord, mult
extern "C" int cztb_host_desc(const char *sig, int without, int32_t *n, uint32_t *entries, uint8_t *fields) {
    CztbDesc d;
    const int rc = cztb_parse(sig, &d);
    if (rc) return rc;
    if (without >= d.n || (without >= 0 && (d.code[without] == 1 || d.code[without] == 8))) return -5;
    if (without >= 0) d = cztb_without(d, without);
    *n = d.n;
    *entries = d.entries;
    memcpy(fields, d.code, CZTB_MAX_SLOTS);
    memcpy(fields + CZTB_MAX_SLOTS, d.dom, CZTB_MAX_SLOTS);
    memcpy(fields + 2 * CZTB_MAX_SLOTS, d.radix, CZTB_MAX_SLOTS);
    memcpy(fields + 3 * CZTB_MAX_SLOTS, d.ord, CZTB_MAX_SLOTS);
    memcpy(fields + 4 * CZTB_MAX_SLOTS, d.mult, CZTB_MAX_SLOTS);
    return 0;
}

// cz_tb_boards for host arrays: boards [G][90], side [G], overlap [G] (an overlapping index gives an empty board)
extern "C" int cztb_host_boards(const char *sig, const uint32_t *index, int G, uint8_t *boards, uint8_t *side, uint8_t *overlap) {
    CztbDesc d;
    if (cztb_parse(sig, &d)) return -1;
    for (int g = 0; g < G; ++g) {
        int sq[CZTB_MAX_SLOTS] = {}, dg[CZTB_MAX_SLOTS] = {};
        bool ov = true;
        int sd = 0;
        if (index[g] < d.entries) sd = cztb_unrank(d, index[g], sq, dg, &ov);
        uint32_t w[23];
        cztb_words(d, sq, !ov, w);
        memcpy(boards + (size_t)g * 90, w, 90);
        side[g] = (uint8_t)sd;
        overlap[g] = ov;
    }
    return 0;
}

// cz_tb_probe's ranking for host arrays: status [G] 0 / CZTB_MISS / CZTB_ILLEGAL, index [G]
extern "C" int cztb_host_rank(const char *sig, const uint8_t *boards, const uint8_t *side, int G, int16_t *status, uint32_t *index) {
    CztbDesc d;
    if (cztb_parse(sig, &d)) return -1;
    for (int g = 0; g < G; ++g) {
        unsigned char buf[92];
        memcpy(buf, boards + (size_t)g * 90, 90);
        buf[90] = buf[91] = 0;
        uint32_t w[23];
        memcpy(w, buf, 92);
        status[g] = (int16_t)cztb_rank(d, w, side[g] ? 1 : 0, index + g);
    }
    return 0;
}

// one pass over a whole table, in place: values [entries], sub[j] the finished table without slot j (NULL for kings) -> the
// number of indices the pass decided
static long long pass_over(const CzmTables &T, const uint16_t *srcdst, const CztbDesc &d, int16_t *values, const int16_t *const *sub, int pass) {
    long long decided = 0;
    uint32_t scratch[CZK_SCRATCH];
    uint16_t list[128];
    auto scr = [&scratch](int k) -> uint32_t & { return scratch[k]; };
    for (uint32_t i = 0; i < d.entries; ++i) {
        const int cur = pass ? values[i] : CZTB_UNKNOWN;
        const bool go = pass == 0 || cur == CZTB_UNKNOWN;
        if (!go) continue;   // the kernel's lane runs along on an empty board: nothing to compute here
        const int v = cztb_step(d, i, cur, pass, go, T, srcdst, scr, [&list](int k, int l) { list[k & 127] = (uint16_t)l; }, []() {}, []() {},
                                [&list](int k) { return list[k & 127]; },
                                [&](int t, uint32_t at) -> int { const int16_t *p = t < 0 ? values : sub[t]; return p ? p[at] : CZTB_UNKNOWN; });
        decided += pass > 0 && v != CZTB_UNKNOWN;
        values[i] = (int16_t)v;
    }
    return decided;
}

struct HostTable { std::vector<int16_t> values; int passes, longest; };   // longest: the largest plies of a decided entry, -1 without one
static std::map<std::string, HostTable> g_done;

static const HostTable *build(const CzmTables &T, const uint16_t *srcdst, const std::string &sig) {
    auto it = g_done.find(sig);
    if (it != g_done.end()) return &it->second;
    CztbDesc d;
    if (cztb_parse(sig.c_str(), &d)) return nullptr;
    const int16_t *sub[CZTB_MAX_SLOTS] = {};
    int S = -1;
    for (int j = 0; j < d.n; ++j) {
        if (d.code[j] == 1 || d.code[j] == 8) continue;
        char name[CZTB_MAX_SLOTS + 2];
        cztb_name(cztb_without(d, j), name);
        const HostTable *s = build(T, srcdst, name);
        if (!s) return nullptr;
        sub[j] = s->values.data();
        S = s->longest > S ? s->longest : S;
    }
    HostTable t;
    t.values.assign(d.entries, (int16_t)CZTB_UNKNOWN);
    pass_over(T, srcdst, d, t.values.data(), sub, 0);
    int pass = 0;
    for (;;) {
        ++pass;
        if (pass_over(T, srcdst, d, t.values.data(), sub, pass) == 0 && pass >= S + 1) break;
    }
    t.passes = pass, t.longest = -1;
    for (auto &v : t.values) {
        if (v == CZTB_UNKNOWN) v = 0;
        if (v != 0 && v != CZTB_ILLEGAL && cztb_plies(v) > t.longest) t.longest = cztb_plies(v);
    }
    return &(g_done[sig] = t);
}

// the table of sig (its closure built on the way) -> values [entries], *passes; returns the number of entries, < 0 for a bad signature
extern "C" long long cztb_host_build(const int16_t *lut, const uint16_t *srcdst, const char *sig, int16_t *values, int32_t *passes) {
    CzmTables *T = new CzmTables;
    memset(T, 0, sizeof *T);
    czm_build_tables(lut, T);
    const HostTable *t = build(*T, srcdst, sig);
    delete T;
    if (!t) return -1;
    if (values) memcpy(values, t->values.data(), t->values.size() * sizeof(int16_t));
    if (passes) *passes = t->passes;
    return (long long)t->values.size();
}

#ifdef TABLEBASE_HOST_MAIN
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
// tablebase_host DIR SIG...: reads DIR/{lut,srcdst}, writes DIR/SIG (the int16 values) for every signature given, and checks the
// rank / unrank round trip of every index on the way
int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s dir signature...\n", argv[0]); return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    const std::vector<unsigned char> lut = slurp((dir + "lut").c_str()), srcdst = slurp((dir + "srcdst").c_str());
    if (lut.size() != 90 * 90 * 2 || srcdst.size() != 2086 * 2) { fprintf(stderr, "bad input sizes\n"); return 2; }
    std::vector<int16_t> lutv(90 * 90);
    std::vector<uint16_t> sdv(2086);
    memcpy(lutv.data(), lut.data(), lut.size());
    memcpy(sdv.data(), srcdst.data(), srcdst.size());
    for (int a = 2; a < argc; ++a) {
        CztbDesc d;
        if (cztb_parse(argv[a], &d)) { fprintf(stderr, "bad signature %s\n", argv[a]); return 2; }
        std::vector<int16_t> values(d.entries);
        int32_t passes = 0;
        if (cztb_host_build(lutv.data(), sdv.data(), argv[a], values.data(), &passes) != (long long)d.entries) return 3;
        long long bad = 0;
        for (uint32_t i = 0; i < d.entries; ++i) {
            uint8_t board[90], side, ov;
            int16_t st;
            uint32_t back;
            cztb_host_boards(argv[a], &i, 1, board, &side, &ov);
            if (ov) continue;
            cztb_host_rank(argv[a], board, &side, 1, &st, &back);
            bad += st != 0 || values[back] != values[i];
        }
        FILE *f = fopen((dir + argv[a]).c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write the output\n"); return 2; }
        fwrite(values.data(), 2, values.size(), f);
        fclose(f);
        printf("%s: %u entries, %d passes, %lld round-trip failures\n", argv[a], d.entries, passes, bad);
        if (bad) return 4;
    }
    return 0;
}
#endif
