// cz_evalcache.h — the two-level evaluation cache of the width-1 search: its memory layout, stated once, and the device side
// of its probes and filings.  Included by cz_internal.h where CzTrees and TreeView are declared; the host side is
// cz_evalcache.hip, the kernels that call the helpers are k_select* and k_expand_backup (cz_search.hip).
//
// The net is a pure function of (board, side to move) and every row of a batch is computed independently of the others, so a
// position that has been evaluated before would get the same priors and value, bit for bit.
//   Per-tree level (cz_search_set_eval_cache): per tree CZ_EC_BUCKETS buckets of 64 entries {Zobrist key of an expanded node's
// position, its node index, the value its evaluation backed up, the position itself}.  The priors are the node's children's P.
// Each tree is touched only by its own wave.
//   Cross-tree level (cz_search_set_xcache): ONE table per context, shared by all of its trees.  An entry cannot lend node
// indices (the lender tree's nodes move at its next re-root), so it is self-contained: key, packed position, the value the
// evaluation backed up, the move count, the <= 128 labels / (src, dst) pairs / priors.  Entries are claimed by k_expand_backup
// with an atomic compare-and-swap on the key — an empty slot of the key's 64-entry bucket, or, when the bucket is full, the
// entry whose position lies DEEPEST in its game (game ply = re-roots of the filing tree + depth of the leaf, kept in the upper
// half of the move-count word) if the new position is shallower: the table converges to the shallowest positions ever
// evaluated — the openings every restarted game walks through again — instead of whatever arrived first.  A filing claims its
// slot by swapping the key to key | CZ_XC_BUSY, writes the payload write-through and only then stores the real key, so a slot
// is never claimed twice before its payload is in memory (xc_file).  k_select (a later launch: the kernel boundary publishes
// the payload) only reads, and verifies the stored position on every hit.  Emptied by the host (keys, values and counts)
// whenever the weights change.
#pragma once

#define CZ_EC_BUCKETS 128
#define CZ_EC_ENTRIES (CZ_EC_BUCKETS * 64)
#ifndef CZ_EC_BUDGET
#define CZ_EC_BUDGET 4   // evaluation-cache hits a tree may complete inside one select launch (its own budget, beside terminal_extra)
#endif
// cross-tree table: the bit that marks an entry whose payload is being written (claimed as key | CZ_XC_BUSY, not yet published);
// no position's key has it (wave_position_key clears it), so a claim still tells the other trees which position it is for
#define CZ_XC_BUSY (1ull << 63)

// ---- layout -----------------------------------------------------------------------------------------------------------
// Both blocks are arrays of fields, field after field: X(name, element type, elements per entry), in memory order.
//   per tree (CzTrees::ec_<name>, [max_games][CZ_EC_ENTRIES] entries), then the pending leaf's packed position per tree
#define CZ_EC_FIELDS(X)                                                                       \
    X(key, unsigned long long, 1) /* 0 = empty */                                             \
    X(node, int32_t, 1)                                                                       \
    X(val, float, 1)                                                                          \
    X(board, uint32_t, 12)        /* wave_pack_board: checked on every hit */
//   cross-tree (czx_<name>(t), n = (xc_mask + 1) * 64 entries behind the ONE pointer CzTrees::xc_base — the kernels are short
//   of scalar registers); CZX_COUNTER_BYTES lie between the keys and the values, the per-tree statistics behind the last field.
//   This is the format cz_search_debug_xcache_dump hands out (include/cchess_hip.h).
#define CZ_XC_FIELDS(X)                                                                       \
    X(key, unsigned long long, 1) /* 0 = empty, key | CZ_XC_BUSY = being written */          \
    X(val, float, 1)                                                                          \
    X(cnt, uint32_t, 1)           /* move count | game ply << 16 */                          \
    X(board, uint32_t, 12)                                                                    \
    X(moves, uint16_t, CZD_MAXMOVES)                                                          \
    X(sd, uint16_t, CZD_MAXMOVES) /* src | dst << 8 */                                        \
    X(P, float, CZD_MAXMOVES)

#define CZ_FIELD_ENUM(name, type, per) name,
#define CZ_FIELD_BYTES(name, type, per) sizeof(type) * (per),
namespace cze { enum Field { CZ_EC_FIELDS(CZ_FIELD_ENUM) COUNT }; constexpr size_t BYTES[] = {CZ_EC_FIELDS(CZ_FIELD_BYTES)}; }
namespace czx { enum Field { CZ_XC_FIELDS(CZ_FIELD_ENUM) COUNT }; constexpr size_t BYTES[] = {CZ_XC_FIELDS(CZ_FIELD_BYTES)}; }
#undef CZ_FIELD_ENUM
#undef CZ_FIELD_BYTES
// bytes per entry of the fields before field f (f = COUNT: of a whole entry)
template <int N> constexpr size_t cz_bytes_before(const size_t (&bytes)[N], int f) {
    size_t s = 0;
    for (int i = 0; i < f; ++i) s += bytes[i];
    return s;
}
constexpr size_t CZ_EC_ENTRY_BYTES = cz_bytes_before(cze::BYTES, cze::COUNT);
constexpr size_t CZ_EC_PEND_BYTES = cze::BYTES[cze::board];   // per tree: the pending leaf's packed position (select -> expand_backup)
constexpr size_t cze_offset(int f, size_t entries) { return entries * cz_bytes_before(cze::BYTES, f); }   // f = COUNT: pend_board

constexpr size_t CZX_ENTRY_BYTES = cz_bytes_before(czx::BYTES, czx::COUNT);
constexpr size_t CZX_COUNTER_BYTES = 64;   // u64 [8] behind the keys: the context-wide counters of the first table; the format keeps their room
constexpr int CZX_TREE_STATS = 8;          // u32 per tree: hits, lookups, written, no room, replaced, 3 spare
constexpr size_t czx_offset(int f, size_t n) { return n * cz_bytes_before(czx::BYTES, f) + (f > czx::key ? CZX_COUNTER_BYTES : 0); }
constexpr size_t czx_dump_bytes(size_t n) { return czx_offset(czx::COUNT, n); }          // every entry: what the dump copies
constexpr size_t czx_clear_bytes(size_t n) { return czx_offset(czx::board, n); }         // keys, counters, values, counts: an empty table
constexpr size_t czx_block_bytes(size_t n, size_t trees) { return czx_dump_bytes(n) + trees * CZX_TREE_STATS * sizeof(uint32_t); }

// the dump format is public (include/cchess_hip.h): per-entry offsets 0, 8, 12, 16, 64, 320, 576 (x n, + 64 behind the keys),
// an entry of 8 + 4 + 4 + 48 + 256 + 256 + 512 = 1088 bytes
static_assert(czx_offset(czx::key, 64) == 0 && czx_offset(czx::val, 64) == 8 * 64 + 64 && czx_offset(czx::cnt, 64) == 12 * 64 + 64 &&
                  czx_offset(czx::board, 64) == 16 * 64 + 64 && czx_offset(czx::moves, 64) == 64 * 64 + 64 &&
                  czx_offset(czx::sd, 64) == 320 * 64 + 64 && czx_offset(czx::P, 64) == 576 * 64 + 64,
              "cross-tree table: field offsets of the documented dump format");
static_assert(CZX_ENTRY_BYTES == 8 + 4 + 4 + 48 + 256 + 256 + 512 && czx_dump_bytes(64) == 64 * CZX_ENTRY_BYTES + 64,
              "cross-tree table: entry and dump size of the documented format");
// per tree: 64 bytes per entry (key 8, node 4, value 4, position 48) and 48 bytes for the pending position
static_assert(cze_offset(cze::key, 1) == 0 && cze_offset(cze::node, 1) == 8 && cze_offset(cze::val, 1) == 12 && cze_offset(cze::board, 1) == 16 &&
                  CZ_EC_ENTRY_BYTES == 64 && CZ_EC_PEND_BYTES == 48,
              "per-tree cache: 64 bytes per entry, 48 per pending leaf");

// cross-tree cache: the arrays inside CzTrees::xc_base
__host__ __device__ __forceinline__ size_t czx_n(const CzTrees &t) { return ((size_t)t.xc_mask + 1) * 64; }
#define CZX_ACCESSOR(name, type, per)                                                                              \
    __host__ __device__ __forceinline__ type *czx_##name(const CzTrees &t) {                                       \
        constexpr size_t per_entry = cz_bytes_before(czx::BYTES, czx::name), fixed = czx_offset(czx::name, 0);     \
        return reinterpret_cast<type *>(t.xc_base + czx_n(t) * per_entry + fixed);                                 \
    }
CZ_XC_FIELDS(CZX_ACCESSOR)
#undef CZX_ACCESSOR
// statistics: PER TREE, [max_games][CZX_TREE_STATS] uint32 behind the entries, updated by the tree's own wave without atomics —
// four counters of the context bumped with same-address atomics by every probe of every tree cost the select launch 95 us of
// its 167 (profiles/r04x_xcache_stats_atomics.txt); cz_search_xcache_stats sums them
__host__ __device__ __forceinline__ uint32_t *czx_tree_stats(const CzTrees &t) {
    return reinterpret_cast<uint32_t *>(t.xc_base + czx_n(t) * CZX_ENTRY_BYTES + CZX_COUNTER_BYTES);
}
enum { CZX_ST_HITS, CZX_ST_LOOKUPS, CZX_ST_WRITTEN, CZX_ST_NO_ROOM, CZX_ST_REPLACED };
__host__ __device__ __forceinline__ uint32_t &xc_stat(const CzTrees &t, int g, int which) { return czx_tree_stats(t)[(size_t)g * CZX_TREE_STATS + which]; }

// ---- device helpers ---------------------------------------------------------------------------------------------------
// forget everything tree g knows (fresh root: reset / reload / re-seed / failed advance)
__device__ __forceinline__ void ec_clear_tree(const CzTrees &t, int g, int tid, int nthreads) {
    if (!t.ec_key) return;
    unsigned long long *k = t.ec_key + (size_t)g * CZ_EC_ENTRIES;
    for (int i = tid; i < CZ_EC_ENTRIES; i += nthreads) k[i] = 0ull;
}

// Zobrist key of the position in LDS: cz_hash without its top bit, which marks "being written" in the cross-tree table
// (CZ_XC_BUSY); 0 is reserved for "empty" in the evaluation cache (a position with key 0 is filed under 1)
__device__ __forceinline__ unsigned long long wave_position_key(const uint8_t *b, int side, const uint64_t *__restrict__ zob, int lane) {
    unsigned long long h = 0ull;
    const int c0 = b[lane];
    if (c0) h = zob[c0 * CZ_NSQ + lane];
    if (lane + 64 < CZ_NSQ) { const int c1 = b[lane + 64]; if (c1) h ^= zob[c1 * CZ_NSQ + lane + 64]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) h ^= __shfl_xor(h, d, 64);
    if (side) h ^= zob[15 * CZ_NSQ];
    // the key is wave-uniform: keep it in scalar registers (the select kernel sits exactly at its 64-VGPR budget)
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)h), hi = __builtin_amdgcn_readfirstlane((uint32_t)(h >> 32));
    h = ((unsigned long long)hi << 32) | lo;
    h &= ~CZ_XC_BUSY;
    return h ? h : 1ull;
}
// write-through store (agent scope, sc1): reaches memory, not only this XCD's L2 — followed by s_waitcnt vmcnt(0), the value is
// in memory before anything stored after the wait (the cross-tree table's payload before its key)
template <typename T> __device__ __forceinline__ void st_through(T *p, T x) {
    __hip_atomic_store((__attribute__((address_space(1))) T *)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ec_bucket(unsigned long long key) { return (int)((key >> 17) & (CZ_EC_BUCKETS - 1)); }
__device__ __forceinline__ uint32_t xc_bucket(unsigned long long key) { return (uint32_t)(key >> 24); }   // cross-tree table: other key bits
// The position itself, packed: 90 squares x 4 bits (piece codes 0..14) in 12 dwords, side to move in the top nibble of the
// last one.  Lane j < 12 packs squares 8j .. 8j+7 (LDS bytes 90..95 of the board are zero).  A cache entry carries this
// image of its node's position and a hit is only taken when it equals the leaf's: the 64-bit key finds the candidate, the
// position decides — a key collision cannot lend a wrong node.
__device__ __forceinline__ uint32_t wave_pack_board(const uint8_t *b, int side, int lane) {
    uint32_t pk = 0u;
    if (lane < 12) {
        const uint32_t w0 = ((const uint32_t *)b)[2 * lane], w1 = ((const uint32_t *)b)[2 * lane + 1];
        pk = (w0 & 15u) | ((w0 >> 4) & 0xF0u) | ((w0 >> 8) & 0xF00u) | ((w0 >> 12) & 0xF000u);
        pk |= ((w1 & 15u) | ((w1 >> 4) & 0xF0u) | ((w1 >> 8) & 0xF00u) | ((w1 >> 12) & 0xF000u)) << 16;
        if (lane == 11) pk |= (uint32_t)side << 28;
    }
    return pk;
}

// The leaf in LDS as the cache knows it: its key (masked by ec_key_mask, never 0; wave-uniform) and its packed position pk
// (lanes 0..11)
__device__ __forceinline__ void ec_leaf_key(const CzTrees &t, const uint8_t *b, int side, const uint64_t *__restrict__ zob, int lane,
                                            unsigned long long &key, uint32_t &pk) {
    key = wave_position_key(b, side, zob, lane) & t.ec_key_mask;
    key = key ? key : 1ull;
    pk = wave_pack_board(b, side, lane);
}

// Per-tree probe of leaf (key, pk) by tree g's wave -> hit; then node = the expanded node of this tree with the leaf's
// position and val = the value its evaluation backed up (neither is touched on a miss).  Counts the lookup, the hit and every
// same-key entry that held another position.  XC: xk = lane's key of the leaf's cross-tree bucket, requested together with
// the tree's own bucket — one wait for both probes (xc_probe takes it).
template <bool XC>
__device__ __forceinline__ bool ec_probe(const CzTrees &t, int g, unsigned long long key, uint32_t pk, int lane, int &node, float &val,
                                         unsigned long long &xk) {
    bool hit = false;
    const size_t eb0 = (size_t)g * CZ_EC_ENTRIES + (size_t)ec_bucket(key) * 64;
    const unsigned long long ek = t.ec_key[eb0 + lane];
    if (XC) xk = czx_key(t)[(size_t)(xc_bucket(key) & t.xc_mask) * 64 + lane];
    const int en = t.ec_node[eb0 + lane];
    const float ev = t.ec_val[eb0 + lane];
    // every entry of the bucket with the leaf's key is a candidate (after a key collision two positions share a key): the
    // stored position decides
    for (unsigned long long m = __ballot(ek == key); m; m &= m - 1ull) {
        const int hl = __ffsll((long long)m) - 1;
        // the candidate's position against the leaf's: 12 lanes, one dword each
        const uint32_t lb = lane < 12 ? t.ec_board[(eb0 + hl) * 12 + lane] : 0u;
        if (__ballot(lb != pk) == 0ull) {
            node = __builtin_amdgcn_readlane(en, hl);
            val = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ev), hl));
            hit = true;
            break;
        }
        if (lane == 0) t.ec_collisions[g] += 1u;   // same key, another position: not this entry
    }
    if (lane == 0) { t.ec_hits[g] += hit ? 1u : 0u; t.ec_lookups[g] += 1u; }
    return hit;
}

// Cross-tree probe (after a per-tree miss): a position ANOTHER tree has had evaluated -> its entry (then val = the value its
// evaluation backed up), or -1.  xk: the bucket's keys as ec_probe<true> requested them.  Entries are self-contained and
// read-only here.  Counts the lookup and the hit in tree g's statistics.
__device__ __forceinline__ long long xc_probe(const CzTrees &t, int g, unsigned long long key, uint32_t pk, unsigned long long xk, int lane,
                                              float &val) {
    long long xe = -1;
    const size_t xb0 = (size_t)(xc_bucket(key) & t.xc_mask) * 64;
    for (unsigned long long m = __ballot(xk == key); m; m &= m - 1ull) {
        const int hl = __ffsll((long long)m) - 1;
        const uint32_t lb = lane < 12 ? czx_board(t)[(xb0 + hl) * 12 + lane] : 0u;
        if (__ballot(lb != pk) == 0ull) { xe = (long long)(xb0 + hl); break; }
    }
    if (xe >= 0) val = czx_val(t)[xe];
    if (lane == 0) { xc_stat(t, g, CZX_ST_LOOKUPS) += 1u; if (xe >= 0) xc_stat(t, g, CZX_ST_HITS) += 1u; }
    return xe;
}

// leaf_node.expand of `leaf` with a lender's labels, (src, dst) pairs and priors: the children of this tree's expanded node
// `node`, or (XC, xe >= 0) the arrays of cross-tree entry xe.  -> false when the node pool has no room: the tree is flagged
// CZ_ST_POOL_EXHAUSTED and nothing is written.
template <bool XC>
__device__ __forceinline__ bool ec_expand_from(const CzTrees &t, const TreeView &v, int g, int leaf, int node, long long xe, int lane) {
    const int scb = (XC && xe >= 0) ? 0 : v.child_begin[node];
    const int n = (XC && xe >= 0) ? (int)(czx_cnt(t)[xe] & 0xFFFFu) : (int)v.child_count[node];
    const int begin = t.n_nodes[g];
    if (begin + n > t.cap) {
        if (lane == 0) t.status[g] |= CZ_ST_POOL_EXHAUSTED;
        return false;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = lane + 64 * r;
        if (i < n) {
            const int c = begin + i;
            if (XC && xe >= 0) {
                const size_t o = (size_t)xe * CZD_MAXMOVES + i;
                v.P[c] = czx_P(t)[o]; v.move[c] = czx_moves(t)[o]; v.sd[c] = czx_sd(t)[o];
            } else {
                v.P[c] = v.P[scb + i]; v.move[c] = v.move[scb + i]; v.sd[c] = v.sd[scb + i];
            }
            v.W[c] = 0.f; v.Q[c] = 0.f; v.N[c] = 0; v.parent[c] = leaf; v.child_begin[c] = -1;
            v.child_count[c] = 0;
        }
    }
    if (lane == 0) { v.child_begin[leaf] = begin; v.child_count[leaf] = (uint16_t)n; t.n_nodes[g] = begin + n; }
    return true;
}

// Per-tree filing (k_expand_backup, after `leaf` got its children): the node now holds the priors of its position (its
// children's P), `val` is what its evaluation backs up.  First empty entry of the key's bucket; a full bucket replaces a
// pseudo-random entry.  -> the pending leaf's packed position (lanes 0..11), for the cross-tree filing.
__device__ __forceinline__ uint32_t ec_file(const CzTrees &t, int g, unsigned long long key, int leaf, float val, int lane) {
    const size_t eb0 = (size_t)g * CZ_EC_ENTRIES + (size_t)ec_bucket(key) * 64;
    const unsigned long long ek = t.ec_key[eb0 + lane];
    // already remembered?  Only an entry with this key AND this position counts (the lookup may have been skipped by its
    // per-launch budget); a same-key entry holding ANOTHER position — a key collision — does not keep this one out
    bool have = false;
    const uint32_t mine = lane < 12 ? t.pend_board[(size_t)g * 12 + lane] : 0u;
    for (unsigned long long m = __ballot(ek == key); m && !have; m &= m - 1ull) {
        const int hl = __ffsll((long long)m) - 1;
        const uint32_t lb = lane < 12 ? t.ec_board[(eb0 + hl) * 12 + lane] : 0u;
        have = __ballot(lb != mine) == 0ull;
    }
    if (!have) {
        const unsigned long long em = __ballot(ek == 0ull);
        int slot = em ? __ffsll((long long)em) - 1 : (int)((key >> 40) & 63);
        if (lane == slot) { t.ec_key[eb0 + lane] = key; t.ec_node[eb0 + lane] = leaf; t.ec_val[eb0 + lane] = val; }
        if (lane < 12) t.ec_board[(eb0 + slot) * 12 + lane] = t.pend_board[(size_t)g * 12 + lane];
    }
    return mine;
}

// Cross-tree filing (k_expand_backup, behind ec_file): file the evaluation of the pending leaf — key, packed position `mine`,
// value `val`, its n children at node `begin` of the view — for the OTHER trees as well, in an empty slot of the key's bucket,
// or in place of the entry deepest in its game.  The claim protocol, top to bottom:
//   1. nothing to do if the bucket already shows this key, published or claimed;
//   2. claim a slot: compare-and-swap its key (empty, or the victim's) to key | CZ_XC_BUSY;
//   3. store the payload (ply included) write-through, and drain: s_waitcnt vmcnt(0);
//   4. only then store the real key.
// So no two trees of a launch hold one slot at once, and a later claim of the slot (which has to find the real key) writes
// after this payload is in memory: the XCDs' L2s are not coherent with each other, and the plain stores of two claimants could
// reach memory in either order — a key and board of one position with the labels, priors or count of another.  Two trees
// expanding the same position in this launch: one files it, the other finds the key, claimed or published (or loses the swap
// to it), and leaves.  Readers are the select kernels of later launches (the kernel boundary publishes the payload); they
// never match a claimed key, and none is left once this launch has ended.
__device__ __forceinline__ void xc_file(const CzTrees &t, const TreeView &v, int g, unsigned long long key, uint32_t mine, int begin, float val,
                                        int lane) {
    const size_t xb0 = (size_t)(xc_bucket(key) & t.xc_mask) * 64;
    const unsigned long long xk = czx_key(t)[xb0 + lane];
    const unsigned long long xm = __ballot(xk == 0ull);
    if (__ballot((xk & ~CZ_XC_BUSY) == key) != 0ull) return;
    // this position's game ply: re-roots of the tree + levels below the root (the priority of the entry: low = shared)
    const uint32_t myply = (uint32_t)min((int)t.root_ply[g] + (int)t.pend_depth[g], 0xFFFF);
    int slot = 0, won = 0, dup = 0;
    if (xm) {
        // the first empty slot at or behind a key-dependent position: trees filing different positions into one bucket in
        // the same launch do not all go for slot 0; a tree that loses the swap to ANOTHER position tries the next empty
        // slot, up to three times; losing it to the SAME position means it is filed
        const int rot = (int)((key >> 40) & 63);
        unsigned long long xr = rot ? (xm >> rot) | (xm << (64 - rot)) : xm;
        for (int attempt = 0; attempt < 3 && xr && !won && !dup; ++attempt) {
            slot = (__ffsll((long long)xr) - 1 + rot) & 63;
            xr &= xr - 1ull;
            unsigned long long seen = 0ull;
            if (lane == 0) seen = atomicCAS(&czx_key(t)[xb0 + slot], 0ull, key | CZ_XC_BUSY);
            seen = __shfl(seen, 0, 64);
            won = seen == 0ull ? 1 : 0;
            dup = (seen & ~CZ_XC_BUSY) == key ? 1 : 0;
        }
    } else {
        // full bucket: the entry deepest in its game makes room if this position is shallower.  A slot another tree of this
        // launch is writing (CZ_XC_BUSY set: its count word is not this key's) is no candidate.  One attempt: a lost swap
        // drops the filing.
        const uint32_t ep = (xk & CZ_XC_BUSY) ? 0u : czx_cnt(t)[xb0 + lane] >> 16;
        uint32_t best = (ep << 6) | (uint32_t)lane;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
        if ((best >> 6) > myply) {
            slot = (int)(best & 63u);
            const unsigned long long old = __shfl(xk, slot, 64);
            unsigned long long seen = 0ull;
            if (lane == 0) seen = atomicCAS(&czx_key(t)[xb0 + slot], old, key | CZ_XC_BUSY);
            seen = __shfl(seen, 0, 64);
            won = seen == old ? 1 : 0;
            if (won && lane == 0) xc_stat(t, g, CZX_ST_REPLACED) += 1u;
        }
    }
    if (won) {
        const size_t e = xb0 + slot;
        const int n = t.pend_nmoves[g];   // the children k_expand_backup has just written: lane l re-reads exactly the elements lane l wrote
        if (lane < 12) st_through(&czx_board(t)[e * 12 + lane], mine);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = lane + 64 * r;
            if (i < n) {
                st_through(&czx_P(t)[e * CZD_MAXMOVES + i], v.P[begin + i]);
                st_through(&czx_moves(t)[e * CZD_MAXMOVES + i], v.move[begin + i]);
                st_through(&czx_sd(t)[e * CZD_MAXMOVES + i], v.sd[begin + i]);
            }
        }
        if (lane == 0) { st_through(&czx_val(t)[e], val); st_through(&czx_cnt(t)[e], (uint32_t)n | (myply << 16)); }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the whole payload is in memory ...
        if (lane == 0) {                                    // ... before the slot shows its key
            __hip_atomic_store(&czx_key(t)[e], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            xc_stat(t, g, CZX_ST_WRITTEN) += 1u;
        }
    } else if (!dup && lane == 0) {
        xc_stat(t, g, CZX_ST_NO_ROOM) += 1u;   // filings that found no room (deeper than everything in a full bucket, or lost every swap)
    }
}
