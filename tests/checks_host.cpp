// tests/checks_host.cpp — the checking-move generator of the library (czk_position<.., CHECKS = true> of
// cchess_zero_amd/csrc/cz_kingsafe.h, what cz_movegen_checks runs with one lane per position) compiled for the HOST, so that
// tests/test_checks_host_cpu.py can hold the very same function to tests/mate_model.py on the CPU.  Test infrastructure: nothing
// in the product path uses it.
#include <string.h>
#include "../cchess_zero_amd/csrc/cz_kingsafe.h"

extern "C" void czc_host_tables(const int16_t *lut, CzmTables *t) { czm_build_tables(lut, t); }
extern "C" int czc_host_sizeof_tables(void) { return (int)sizeof(CzmTables); }
// boards [n][90], side [n] -> moves [n][128] (0xFFFF padding), count [n] (-1: refused), flags [n]; want_list = 0: the count /
// flags form of the function (no list), moves stay as they are
extern "C" void czc_host_checks(const CzmTables *t, const uint8_t *boards, const uint8_t *side, int n, int want_list, uint16_t *moves, int *count,
                                uint8_t *flags) {
    for (int i = 0; i < n; ++i) {
        uint32_t w[23];
        unsigned char buf[92];
        memcpy(buf, boards + (size_t)i * 90, 90);
        buf[90] = buf[91] = 0;
        memcpy(w, buf, 92);
        uint32_t scratch[CZK_SCRATCH], pf = 0;
        auto scr = [&scratch](int k) -> uint32_t & { return scratch[k]; };
        if (!want_list) {
            count[i] = czk_position<false, false, true>(w, side[i] ? 1 : 0, *t, scr, [](int, int) {}, [](int, uint32_t) {}, [] {}, &pf);
        } else {
            uint16_t *row = moves + (size_t)i * 128;
            for (int k = 0; k < 128; ++k) row[k] = 0xFFFF;
            int puts = 0;
            count[i] = czk_position<true, false, true>(w, side[i] ? 1 : 0, *t, scr,
                [row, &puts](int k, int label) { if (k >= 0 && k < 128 && row[k] == 0xFFFF) { row[k] = (uint16_t)label; ++puts; } else puts = -1000; },
                [](int, uint32_t) {}, [] {}, &pf);
            if (count[i] >= 0 && puts != count[i]) count[i] = -2000;   // every slot of the list written exactly once
        }
        flags[i] = (uint8_t)pf;
    }
}
