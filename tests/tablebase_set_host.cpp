// tests/tablebase_set_host.cpp — the material key and the directory of a table set (cchess_zero_amd/csrc/cz_tablebase.h:
// cztb_material_key, cztb_desc_key, cztb_set_sort, cztb_set_find — what k_tb_probe_set and cz_tb_set_create run) compiled for
// the HOST, as tests/tablebase_host.cpp compiles the index mapping: this very text, on the CPU.  A stand-alone program with its
// own main, which tests/test_tablebase_set_cpu.py builds plain and with -fsanitize=address,undefined and runs:
//   keys FILE       FILE holds boards of 90 bytes -> one line per board: its key
//   desc SIG ...    -> one line per signature: the key of its descriptor, or "bad <code>"
//   dir SIG ...     the directory cz_tb_set_create would make -> "refused n" / "refused bad SIG" / "refused twice SIG", or the
//                   signatures in directory order on one line and, per signature given, "SIG at PLACE" as cztb_set_find finds
//                   the key of its descriptor among the sorted keys (a key that is none of them must not be found)
// Test infrastructure: nothing in the product path uses it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../cchess_zero_amd/csrc/cz_tablebase.h"

static int cmd_keys(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    uint8_t board[90];
    while (fread(board, 1, 90, f) == 90) {
        uint32_t w[23];
        memset(w, 0, sizeof(w));
        memcpy(w, board, 90);
        printf("%llu\n", (unsigned long long)cztb_material_key(w));
    }
    fclose(f);
    return 0;
}

static int cmd_desc(int n, char **sig) {
    for (int i = 0; i < n; ++i) {
        CztbDesc d;
        const int rc = cztb_parse(sig[i], &d);
        if (rc) printf("bad %d\n", rc);
        else printf("%llu\n", (unsigned long long)cztb_desc_key(d));
    }
    return 0;
}

static int cmd_dir(int n, char **sig) {
    std::vector<uint64_t> keys((size_t)(n > 0 ? n : 1));
    std::vector<int> order((size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) {
        CztbDesc d;
        if (cztb_parse(sig[i], &d)) { printf("refused bad %s\n", sig[i]); return 0; }
        keys[i] = cztb_desc_key(d);
    }
    const int rc = cztb_set_sort(n, keys.data(), order.data());
    if (rc < 0) { printf("refused n\n"); return 0; }
    if (rc > 0) { printf("refused twice %s\n", sig[order[rc - 1]]); return 0; }
    uint64_t skeys[CZTB_SET_MAX];
    for (int i = 0; i < CZTB_SET_MAX; ++i) skeys[i] = i < n ? keys[order[i]] : ~0ull;
    for (int i = 0; i < n; ++i) printf("%s%s", i ? " " : "", sig[order[i]]);
    printf("\n");
    int wrong = 0;
    for (int i = 0; i < n; ++i) {
        const int at = cztb_set_find(skeys, n, keys[i]);
        printf("%s at %d\n", sig[i], at);
        wrong += at < 0 || order[at] != i;
        // the keys next to it belong to nobody unless the directory holds them
        for (int dlt = -1; dlt <= 1; dlt += 2) {
            const uint64_t other = keys[i] + (uint64_t)(int64_t)dlt;
            const int o = cztb_set_find(skeys, n, other);
            wrong += o >= 0 && skeys[o] != other;
        }
    }
    wrong += cztb_set_find(skeys, n, 0ull) >= 0 || cztb_set_find(skeys, n, ~0ull) >= 0 || cztb_set_find(skeys, n, CZTB_KEY_FOREIGN) >= 0;
    printf("%d wrong\n", wrong);
    return wrong ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "keys")) return cmd_keys(argv[2]);
    if (argc >= 2 && !strcmp(argv[1], "desc")) return cmd_desc(argc - 2, argv + 2);
    if (argc >= 2 && !strcmp(argv[1], "dir")) return cmd_dir(argc - 2, argv + 2);
    fprintf(stderr, "usage: %s keys FILE | desc SIG ... | dir SIG ...\n", argv[0]);
    return 2;
}
