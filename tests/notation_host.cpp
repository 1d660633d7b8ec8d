// tests/notation_host.cpp — the token decode of cz_games_read (cchess_zero_amd/csrc/cz_notation.h: czn_pick, on top of
// cz_games.h's czg_step_pick; one lane = one game on the GPU) compiled for the HOST, so that tests/test_notation_host_cpu.py can
// hold the very same text to tests/notation_model.py on the CPU.  The loop around the step restates czg_replay_body's
// (cz_games_body.h) for one game at a time: the board before the move and the list lie in the record's row, and the decode reads
// them there.  Built twice: as a shared library for ctypes, and (-DNOTATION_HOST_MAIN) as a stand-alone program that the test
// builds with -fsanitize=address,undefined and runs over a corpus it writes to files.  Test infrastructure: nothing in the
// product path uses it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../cchess_zero_amd/csrc/cz_notation.h"

enum { REC_BYTES = 608, REC_LABELS = 96, REC_VISITS = 352 };

extern "C" void czn_host_tables(const int16_t *lut, CzmTables *t) { memset(t, 0, sizeof *t); czm_build_tables(lut, t); }
extern "C" int czn_host_sizeof_tables(void) { return (int)sizeof(CzmTables); }
// one candidate against one token, for the tests that walk a position's list themselves: board uint8[90]
extern "C" int czn_host_match(uint32_t tok, int side, int from, int to, const uint8_t *board) {
    uint32_t w[23];
    unsigned char buf[92] = {0};
    memcpy(buf, board, 90);
    memcpy(w, buf, 92);
    const CznToken k = czn_token(tok);
    return czn_match(k, side, from, to, czn_kind_set(k.kind ? (uint32_t)(k.kind + (side ? 7 : 0)) : 0xFFu, [&w](int i) { return w[i]; })) ? 1 : 0;
}

template <int RULES>
static void read_one(const CzmTables &T, const uint16_t *srcdst, const uint8_t *board, int side, const uint32_t *tokens, int stride, int len, int result,
                     long long off, int total, uint8_t *records, int32_t *valid, uint8_t *status, uint8_t *end_flags, uint8_t *final_board,
                     uint8_t *final_side, uint16_t *labels_out) {
    uint32_t w[23] = CZG_START_WORDS;
    if (board) {
        unsigned char buf[92];
        memcpy(buf, board, 90);
        buf[90] = buf[91] = 0;
        memcpy(w, buf, 92);
    }
    uint32_t scratch[CZG_SCRATCH];
    auto scr = [&scratch](int k) -> uint32_t & { return scratch[k]; };
    const bool len_ok = len >= 0 && len <= stride;
    int made = 0, st = len_ok ? CZG_OK : CZG_BAD_LEN, sd = side ? 1 : 0;
    bool stopped = !len_ok;
    if (labels_out) for (int i = 0; i < stride; ++i) labels_out[i] = 0xFFFFu;
    for (int i = 0; len_ok && i < len; ++i) {
        uint32_t row[REC_BYTES / 4];
        memset(row, 0, sizeof row);
        if (!stopped) {
            uint32_t before[23];
            memcpy(before, w, sizeof before);
            memcpy(row, before, 92);   // the board before the move, bytes 88 and 89 too: the decode reads the row
            uint16_t *const lrow = reinterpret_cast<uint16_t *>(row + REC_LABELS / 4);
            const uint32_t tok = tokens[i];
            uint32_t played = tok;
            const CzgStep r = czg_step_pick<RULES>(w, sd, tok, true, T, srcdst, scr, [lrow](int k, int l) { lrow[k & 127] = (uint16_t)l; },
                [&row]() { for (int k = REC_LABELS / 4; k < REC_VISITS / 4; ++k) row[k] = 0xFFFFFFFFu; },
                [&](int n, uint32_t &lab, int &idx) {
                    const int miss = czn_pick(tok, tok >= 65536u, sd, n, lab, idx, [lrow](int j) { return lrow[j & 127]; },
                                              [srcdst](uint32_t l) { return (uint32_t)srcdst[l]; }, [&row](int k) { return row[k]; });
                    played = lab;
                    return miss;
                });
            if (r.status == CZG_OK) {
                row[22] = czg_rec_word22(before[22], sd, r.n);
                row[23] = czg_rec_word23(sd ? -result : result, i);
                for (int k = REC_VISITS / 4; k < REC_BYTES / 4; ++k) row[k] = 0u;
                reinterpret_cast<uint16_t *>(row + REC_VISITS / 4)[r.idx & 127] = 1;
                if (labels_out) labels_out[i] = (uint16_t)played;
                ++made;
                sd ^= 1;
            } else {
                stopped = true;
                st = r.status;
                memset(row, 0, sizeof row);
            }
        }
        const long long at = off + i;
        if (records && at >= 0 && at < total) memcpy(records + (size_t)at * REC_BYTES, row, REC_BYTES);
    }
    *valid = made;
    *status = (uint8_t)st;
    *end_flags = (uint8_t)czg_end_flags(w, sd, true, T, scr);
    if (final_board) memcpy(final_board, w, 90);
    if (final_side) *final_side = (uint8_t)sd;
}

// cz_games_read's arguments, on the host (every array a host array)
extern "C" void czn_host_read(const CzmTables *t, const uint16_t *srcdst, const uint8_t *boards, const uint8_t *side, const uint32_t *tokens, int stride,
                              const int32_t *len, const int8_t *result, int G, int rules, const int32_t *rec_offset, int total, uint8_t *records,
                              int32_t *valid, uint8_t *status, uint8_t *end_flags, uint8_t *final_boards, uint8_t *final_side, uint16_t *labels_out) {
    for (int g = 0; g < G; ++g) {
        const uint8_t *b = boards ? boards + (size_t)g * 90 : nullptr;
        const int sd = side ? side[g] : 0;
        const uint32_t *m = tokens + (size_t)g * stride;
        uint8_t *fb = final_boards ? final_boards + (size_t)g * 90 : nullptr, *fs = final_side ? final_side + g : nullptr;
        uint16_t *lo = labels_out ? labels_out + (size_t)g * stride : nullptr;
        if (rules) read_one<1>(*t, srcdst, b, sd, m, stride, len[g], result[g], rec_offset[g], total, records, valid + g, status + g, end_flags + g, fb, fs, lo);
        else read_one<0>(*t, srcdst, b, sd, m, stride, len[g], result[g], rec_offset[g], total, records, valid + g, status + g, end_flags + g, fb, fs, lo);
    }
}

#ifdef NOTATION_HOST_MAIN
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
template <typename T>
static std::vector<T> as(const std::vector<unsigned char> &v) {
    std::vector<T> o(v.size() / sizeof(T));
    memcpy(o.data(), v.data(), o.size() * sizeof(T));
    return o;
}
// notation_host DIR RULES STRIDE: reads DIR/{lut,srcdst,boards,side,tokens,len,result,offset}, writes DIR/out<RULES>: records (the games' records one
// after the other, as the offsets say), then valid, status, end_flags, final boards, final sides, labels_out
int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s dir rules stride\n", argv[0]); return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const int rules = atoi(argv[2]), stride = atoi(argv[3]);
    const std::vector<int16_t> lut = as<int16_t>(slurp((d + "lut").c_str()));
    const std::vector<uint16_t> srcdst = as<uint16_t>(slurp((d + "srcdst").c_str()));
    const std::vector<uint32_t> tokens = as<uint32_t>(slurp((d + "tokens").c_str()));
    const std::vector<unsigned char> boards = slurp((d + "boards").c_str()), side = slurp((d + "side").c_str());
    const std::vector<int32_t> len = as<int32_t>(slurp((d + "len").c_str())), offset = as<int32_t>(slurp((d + "offset").c_str()));
    const std::vector<int8_t> result = as<int8_t>(slurp((d + "result").c_str()));
    const int G = (int)len.size();
    if (lut.size() != 90 * 90 || srcdst.size() != 2086 || (int)side.size() != G || boards.size() != (size_t)G * 90 || tokens.size() != (size_t)G * stride ||
        (int)offset.size() != G + 1 || (int)result.size() != G) { fprintf(stderr, "bad input sizes\n"); return 2; }
    const int total = offset[G];
    CzmTables *t = new CzmTables;
    czn_host_tables(lut.data(), t);
    std::vector<uint8_t> records((size_t)total * REC_BYTES, 0xA5), status(G), flags(G), fb((size_t)G * 90), fs(G);
    std::vector<int32_t> valid(G);
    std::vector<uint16_t> labels((size_t)G * stride, 0x5A5A);
    czn_host_read(t, srcdst.data(), boards.data(), side.data(), tokens.data(), stride, len.data(), result.data(), G, rules, offset.data(), total,
                  records.data(), valid.data(), status.data(), flags.data(), fb.data(), fs.data(), labels.data());
    delete t;
    FILE *f = fopen((d + "out" + argv[2]).c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write the output\n"); return 2; }
    fwrite(records.data(), 1, records.size(), f);
    fwrite(valid.data(), 4, valid.size(), f);
    fwrite(status.data(), 1, G, f);
    fwrite(flags.data(), 1, G, f);
    fwrite(fb.data(), 1, fb.size(), f);
    fwrite(fs.data(), 1, G, f);
    fwrite(labels.data(), 2, labels.size(), f);
    fclose(f);
    printf("%d games, %d records\n", G, total);
    return 0;
}
#endif
