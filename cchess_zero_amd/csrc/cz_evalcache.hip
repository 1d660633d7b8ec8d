// cz_evalcache.hip — host side of the evaluation cache (layout and device side: cz_evalcache.h): switching the two levels on and
// off, their statistics, and the dumps the tests read.  Every size and offset here comes from the field lists of the header.
#include "cz_internal.h"

#include <string.h>
#include <vector>

namespace {

// the trees' records on the host (synchronises): the cache statistics of a tree live in its CzTreeRec
int download_tree_recs(cz_ctx *c, std::vector<CzTreeRec> &h) {
    h.resize((size_t)(c->G > 0 ? c->G : 0));
    if (h.empty()) return CZ_OK;
    CZ_HIP(hipMemcpyAsync(h.data(), c->t.rec, h.size() * sizeof(CzTreeRec), hipMemcpyDeviceToHost, c->stream));
    CZ_HIP(hipStreamSynchronize(c->stream));
    return CZ_OK;
}

int xcache_stats(cz_ctx *c, unsigned long long *stats, int n) {
    for (int k = 0; k < n; ++k) stats[k] = 0;
    if (!c->t.xc_base) return CZ_OK;
    std::vector<uint32_t> per((size_t)c->max_games * CZX_TREE_STATS);
    CZ_HIP(hipMemcpyAsync(per.data(), czx_tree_stats(c->t), per.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    CZ_HIP(hipStreamSynchronize(c->stream));
    for (size_t g = 0; g < (size_t)c->max_games; ++g)
        for (int k = 0; k < n; ++k) stats[k] += per[g * CZX_TREE_STATS + k];
    return CZ_OK;
}

}  // namespace

extern "C" {

int cz_search_set_eval_cache(cz_ctx *c, int on) {
    CZ_REQUIRE(c, "cz_search_set_eval_cache: null ctx");
    if (on && c->width != 1) { cz_set_error("cz_search_set_eval_cache: needs width 1 (one simulation in flight per tree)"); return CZ_EINVAL; }
    const size_t per = (size_t)c->max_games * CZ_EC_ENTRIES;
    if (on && !c->ec_block) {
        const size_t bytes = per * CZ_EC_ENTRY_BYTES + (size_t)c->max_games * CZ_EC_PEND_BYTES;
        CZ_HIP(hipSetDevice(c->device));
        if (hipMalloc(&c->ec_block, bytes) != hipSuccess) { c->ec_block = nullptr; cz_set_error("cz_search_set_eval_cache: hipMalloc(%zu B) failed", bytes); return CZ_ENOMEM; }
    }
    if (on) {
        char *b = (char *)c->ec_block;
#define CZ_EC_POINT(name, type, n) c->t.ec_##name = (type *)(b + cze_offset(cze::name, per));
        CZ_EC_FIELDS(CZ_EC_POINT)
#undef CZ_EC_POINT
        c->t.pend_board = (uint32_t *)(b + cze_offset(cze::COUNT, per));
        if (!c->t.ec_key_mask) c->t.ec_key_mask = ~0ull;
        // an empty cache: entries of an earlier use would point into trees that no longer exist
        CZ_HIP(hipMemsetAsync(c->t.ec_key, 0, per * sizeof(*c->t.ec_key), c->stream));
        cz_search_clear_cache_stats(c);
        if (c->t.xc_base) CZ_HIP(hipMemsetAsync(c->xc_block, 0, czx_clear_bytes(czx_n(c->t)), c->stream));   // and the cross-tree level
    } else {
#define CZ_EC_POINT(name, type, n) c->t.ec_##name = nullptr;
        CZ_EC_FIELDS(CZ_EC_POINT)
#undef CZ_EC_POINT
        c->t.pend_board = nullptr;
        if (c->xc_block) return cz_search_set_xcache(c, 0);   // the cross-tree level lives behind the per-tree probe
    }
    return CZ_OK;
}

int cz_search_set_xcache(cz_ctx *c, int log2_entries) {
    CZ_REQUIRE(c && (log2_entries == 0 || (log2_entries >= 6 && log2_entries <= 24)), "cz_search_set_xcache: log2_entries must be 0 (off) or 6..24");
    CZ_HIP(hipSetDevice(c->device));
    if (log2_entries == 0 || (c->xc_block && c->xc_log2_entries != log2_entries)) {
        if (c->xc_block) { CZ_HIP(hipStreamSynchronize(c->stream)); (void)hipFree(c->xc_block); }
        c->xc_block = nullptr; c->xc_log2_entries = 0;
        c->t.xc_base = nullptr; c->t.xc_mask = 0;
        if (log2_entries == 0) return CZ_OK;
    }
    if (!c->t.ec_key) { cz_set_error("cz_search_set_xcache: switch the per-tree evaluation cache on first (cz_search_set_eval_cache(ctx, 1))"); return CZ_EINVAL; }
    const size_t n = (size_t)1 << log2_entries;
    if (!c->xc_block) {
        const size_t bytes = czx_block_bytes(n, (size_t)c->max_games);
        if (hipMalloc(&c->xc_block, bytes) != hipSuccess) { c->xc_block = nullptr; cz_set_error("cz_search_set_xcache: hipMalloc(%zu B) failed", bytes); return CZ_ENOMEM; }
        c->xc_log2_entries = log2_entries;
        c->t.xc_base = (char *)c->xc_block;
        c->t.xc_mask = (uint32_t)(n / 64 - 1);
    }
    // an empty table (new weights => remembered evaluations are stale): keys, values and count | ply words (a full bucket's
    // victim is chosen by the ply of every slot: no slot may carry a ply of an earlier use or uninitialised memory)
    CZ_HIP(hipMemsetAsync(c->xc_block, 0, czx_clear_bytes(n), c->stream));
    CZ_HIP(hipMemsetAsync(czx_tree_stats(c->t), 0, (size_t)c->max_games * CZX_TREE_STATS * sizeof(uint32_t), c->stream));
    return CZ_OK;
}
int cz_search_xcache_stats(cz_ctx *c, unsigned long long *stats4) {
    CZ_REQUIRE(c && stats4, "cz_search_xcache_stats: null argument");
    return xcache_stats(c, stats4, 4);
}
int cz_search_xcache_stats5(cz_ctx *c, unsigned long long *stats5) {
    CZ_REQUIRE(c && stats5, "cz_search_xcache_stats5: null argument");
    return xcache_stats(c, stats5, 5);
}
int cz_search_debug_xcache_dump(cz_ctx *c, void *host, size_t bytes) {
    CZ_REQUIRE(c, "cz_search_debug_xcache_dump: null context");
    if (!c->t.xc_base) { cz_set_error("cz_search_debug_xcache_dump: the cross-tree table is off"); return CZ_EINVAL; }
    const size_t n = czx_n(c->t), need = czx_dump_bytes(n);
    if (!host) return (int)n;
    if (bytes < need) { cz_set_error("cz_search_debug_xcache_dump: %zu bytes < %zu", bytes, need); return CZ_EINVAL; }
    CZ_HIP(hipStreamSynchronize(c->stream));
    CZ_HIP(hipMemcpy(host, c->t.xc_base, need, hipMemcpyDeviceToHost));
    return (int)n;
}
int cz_search_debug_eval_cache_dump(cz_ctx *c, int g, unsigned long long *key, int32_t *node, float *value, uint32_t *board,
                                    int32_t *record) {
    CZ_REQUIRE(c && c->G > 0 && g >= 0 && g < c->G, "cz_search_debug_eval_cache_dump: bad tree index");
    if (!c->t.ec_key) { cz_set_error("cz_search_debug_eval_cache_dump: the evaluation cache is off"); return CZ_EINVAL; }
    CZ_HIP(hipStreamSynchronize(c->stream));
    const size_t e0 = (size_t)g * CZ_EC_ENTRIES;
    std::vector<unsigned long long> k(CZ_EC_ENTRIES);
    std::vector<int32_t> nd(CZ_EC_ENTRIES);
    CZ_HIP(hipMemcpy(k.data(), c->t.ec_key + e0, cze::BYTES[cze::key] * CZ_EC_ENTRIES, hipMemcpyDeviceToHost));
    CZ_HIP(hipMemcpy(nd.data(), c->t.ec_node + e0, cze::BYTES[cze::node] * CZ_EC_ENTRIES, hipMemcpyDeviceToHost));
    if (key) memcpy(key, k.data(), cze::BYTES[cze::key] * CZ_EC_ENTRIES);
    if (node) memcpy(node, nd.data(), cze::BYTES[cze::node] * CZ_EC_ENTRIES);
    if (value) CZ_HIP(hipMemcpy(value, c->t.ec_val + e0, cze::BYTES[cze::val] * CZ_EC_ENTRIES, hipMemcpyDeviceToHost));
    if (board) CZ_HIP(hipMemcpy(board, c->t.ec_board + e0 * 12, cze::BYTES[cze::board] * CZ_EC_ENTRIES, hipMemcpyDeviceToHost));
    if (record) {
        // the entry's node as cz_search_tree_dump numbers it: -1 the root, -2 not in the tree
        CzPreorder po;
        if (const int rc = cz_tree_preorder(c, g, po)) return rc;
        std::vector<int32_t> rec((size_t)po.n, -2);
        if (po.root >= 0) rec[po.root] = -1;
        for (size_t r = 0; r < po.node.size(); ++r) rec[po.node[r]] = (int32_t)r;
        for (int i = 0; i < CZ_EC_ENTRIES; ++i) record[i] = (k[i] && nd[i] >= 0 && nd[i] < po.n) ? rec[nd[i]] : -2;
    }
    return CZ_EC_ENTRIES;
}
int cz_search_debug_eval_cache_key_bits(cz_ctx *c, int bits) {
    CZ_REQUIRE(c && (bits == 64 || (bits >= 8 && bits <= 24)), "cz_search_debug_eval_cache_key_bits: bits must be 8..24 or 64");
    // narrowed keys keep the 7-bit bucket field (bits 17..23) plus the bits - 7 lowest bits: entries still spread over the buckets
    c->t.ec_key_mask = bits == 64 ? ~0ull : ((0x7Full << 17) | ((1ull << (bits - 7)) - 1ull));
    return CZ_OK;
}
int cz_search_eval_cache_collisions(cz_ctx *c, unsigned long long *collisions) {
    CZ_REQUIRE(c && collisions, "cz_search_eval_cache_collisions: null argument");
    *collisions = 0;
    std::vector<CzTreeRec> h;
    if (const int rc = download_tree_recs(c, h)) return rc;
    for (const CzTreeRec &r : h) *collisions += r.ec_collisions;
    return CZ_OK;
}
int cz_search_eval_cache_stats(cz_ctx *c, unsigned long long *hits, unsigned long long *lookups) {
    CZ_REQUIRE(c && hits && lookups, "cz_search_eval_cache_stats: null argument");
    *hits = 0; *lookups = 0;
    std::vector<CzTreeRec> h;
    if (const int rc = download_tree_recs(c, h)) return rc;
    for (const CzTreeRec &r : h) { *hits += r.ec_hits; *lookups += r.ec_lookups; }
    return CZ_OK;
}

}  // extern "C"
