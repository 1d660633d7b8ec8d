// cz_internal.h — context layout and helpers shared by the libcchess_hip translation units.
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/cchess_hip.h"
#include "cz_device.h"
#include "cz_rootrules.h"

// ---- error plumbing -------------------------------------------------------------------------
void cz_set_error(const char *fmt, ...);
#define CZ_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            cz_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return CZ_EHIP;                                                                       \
        }                                                                                         \
    } while (0)
#define CZ_REQUIRE(cond, msg)                                \
    do {                                                     \
        if (!(cond)) { cz_set_error("%s", msg); return CZ_EINVAL; } \
    } while (0)

// ---- carving one device allocation into arrays (base NULL: only the size, in off) --------------
struct Carver {
    char *base;
    size_t off = 0;
    template <typename T> T *take(size_t n) {
        T *p = base ? (T *)(base + off) : nullptr;
        off = (off + n * sizeof(T) + 255) / 256 * 256;
        return p;
    }
};
// One device allocation laid out by lay(Carver &), which takes its arrays: lay runs once on a NULL Carver for the size (the
// pointers it stores are NULL then) and once on the block.  *block is allocated here unless it already is; zero: all of it is
// cleared, in stream order; who: the API call the error text names.  After an error lay's pointers are not to be used, and
// *block, if it is set, stays the caller's to free.
template <typename Lay>
inline int carve_alloc(void **block, hipStream_t stream, bool zero, const char *who, Lay lay) {
    Carver sizing{nullptr};
    lay(sizing);
    if (!*block && hipMalloc(block, sizing.off) != hipSuccess) {
        *block = nullptr;
        cz_set_error("%s: hipMalloc(%zu B) failed", who, sizing.off);
        return CZ_ENOMEM;
    }
    if (zero) CZ_HIP(hipMemsetAsync(*block, 0, sizing.off, stream));
    Carver k{(char *)*block};
    lay(k);
    return CZ_OK;
}

// ---- host tables (cz_tables.hip) --------------------------------------------------------------
struct CzHostTables {
    char labels[CZ_NLABELS * 5];
    int16_t lut[CZ_NSQ * CZ_NSQ];
    int16_t unflip[CZ_NLABELS];
    int16_t mirror[CZ_NLABELS];   // the label of the move mirrored across the e-file (an involution; cz_mirror_table)
    uint16_t srcdst[CZ_NLABELS];
    uint64_t zob[15 * CZ_NSQ + 1];  // [15*90] = side key
};
const CzHostTables &cz_host_tables();

#define CZ_PATH_MAX 32   // deeper paths fall back to the parent walk

// ---- tree storage: structure-of-arrays, one fixed-capacity pool per tree -----------------------
// A node is the edge into it plus its expansion record (the reference's leaf_node, main.py:93-103,
// minus the eagerly materialised state string, quirk Q8).  Children of a node are contiguous, so a
// wave scores up to 128 siblings with three coalesced loads (Q, P, N).  Nodes are allocated in expansion
// order, so every child has a larger index than its parent — cz_search_advance relies on that to compact
// the kept subtree IN PLACE (one pool per tree, no spare pool).
struct CzPool {
    float *P, *W, *Q;
    int32_t *N, *parent, *child_begin;
    uint16_t *child_count, *move;
    uint16_t *sd;   // src | dst << 8 of `move` (k_select applies the move without the label -> (src, dst) table round trip)
};

// cz_selfplay_set_resign: what resignation keeps per slot — an allocation of its own (cz_ctx::sp_resign_block); its counters are
// slots of CzSelfplay::stats.
// game_no == NULL: the setter has not run since cz_selfplay_begin, and no kernel does anything for it.
struct CzSpResign {
    float threshold;             // a mover whose root value (wave_root_value) is below it resigns; NaN: no ply is judged
    int min_ply;                 // plies of a game before the first judged one
    double playon_fraction;      // a game plays on iff uniform53(seed, slot, game_no) < playon_fraction
    unsigned long long seed;
    uint32_t *game_no;           // [max_games] games the slot has started before the one in progress
    uint8_t *playon;             // [max_games] the game in progress plays on: it is judged, counted, and never resigned
    float *minq;                 // [max_games][2] lowest judged root value of red / black in the game in progress; 2.0: none yet
    uint8_t *would;              // [max_games] play-on game: 0, or 1 + the side that first crossed the threshold
    uint8_t *resigned;           // [max_games] the last choose resigned the game (k_sp_adjudicate ends it)
};
__device__ __forceinline__ bool sp_plays_on(const CzSpResign &rs, int g, uint32_t game_no) {
    return uniform53(splitmix64(rs.seed ^ splitmix64(((unsigned long long)g << 32) | (unsigned long long)game_no))) < rs.playon_fraction;
}

// Every counter of self-play is a slot of CzSelfplay::stats, cleared by cz_selfplay_begin: the public CZ_SP_NSTATS
// (cz_selfplay_stats), then what the other four getters copy out, each a slice in its own order
enum CzSpSlot {
    CZ_SP_MATES = CZ_SP_NSTATS, CZ_SP_REPETITIONS, CZ_SP_PERPETUALS,              // cz_selfplay_rules_stats
    CZ_SP_CHASES,                                                                   // cz_selfplay_chase_stats
    CZ_SP_TABLEBASE,                                                                // cz_selfplay_tablebase_stats
    CZ_SP_RESIGNED, CZ_SP_PLAYON_GAMES, CZ_SP_PLAYON_WOULD, CZ_SP_PLAYON_FALSE,   // cz_selfplay_resign_stats
    CZ_SP_RESIGN_HIST,   // its 64 bins: lowest root values of the sides that did not lose a play-on game, 1/32 each over [-1, 1)
    CZ_SP_AVOIDED = CZ_SP_RESIGN_HIST + 64, CZ_SP_FORCED_REPETITIONS,               // cz_selfplay_avoid_stats
    CZ_SP_NSLOTS
};

// cz_selfplay_*: per game slot, the (s, pi, z) records of the game in progress (cchess_main.selfplay keeps
// states / mcts_probs / current_players lists, main.py:1496-1518) and the counters of finished games
struct CzSelfplay {
    int max_plies;               // history capacity per game; a game reaching it is adjudicated a draw
    uint8_t *hist;               // [max_games][max_plies][CZ_REC_BYTES]
    int32_t *ply;                // [max_games] plies recorded for the game in progress
    uint8_t *stalled;            // [max_games] the last choose found no root child (node pool exhausted at the root)
    uint8_t *active;             // [max_games] 0 = parked (finished, not re-seeded)
    uint8_t *start_board;        // [max_games][96] position every new game of the slot starts from
    uint8_t *start_side;         // [max_games]
    int32_t *start_rr;           // [max_games]
    long long *stats;            // [CZ_SP_NSLOTS] (CzSpSlot)
    // cz_selfplay_set_rules(1): what the rules at the root keep beside the games (cz_rootrules.h); the chase part is an allocation
    // of its own (CzRootHost), NULL while cz_selfplay_set_chase is off
    CzRootRules rr;
    // cz_selfplay_set_tablebase: an allocation of its own (CzRootHost).  tb_value NULL: no set is attached, nothing is probed
    int16_t *tb_value;           // [max_games] the table set's value of every slot's root position after the move (k_tb_probe_set)
    CzSpResign rs;               // cz_selfplay_set_resign
};
__device__ __forceinline__ void sp_count(const CzSelfplay &sp, int slot, unsigned long long n = 1ull) {
    atomicAdd((unsigned long long *)&sp.stats[slot], n);
}

// Per-tree scalars: ONE 64-byte record per tree instead of sixteen arrays.  A wave owns a tree, so what it reads at entry
// (root, counters, status) and leaves behind (the pending leaf) is one cache line, and the kernels hold one base pointer
// instead of sixteen (the select kernels spilled 30-60 SGPRs keeping the array bases alive).  Kernel code keeps the array
// syntax — t.status[g] — through CzRecField: every field of the union below IS the record pointer plus a constant offset.
struct CzTreeRec {
    int32_t root_rr, root_node, n_nodes, status;      //  0
    int32_t sims;                                     // 16
    int16_t last_depth;                               // 20  depth of the last simulation (statistics)
    uint16_t root_ply;                                // 22  re-roots since the tree was (re)set: the root's ply in its game (cross-tree cache priority)
    int32_t pend_kind, pend_leaf;                     // 24  pending leaf between select and expand_backup (width 1)
    float pend_value;                                 // 32
    int32_t pend_depth;                               // 36  levels of the pending path (pend_path)
    uint32_t ec_hits, ec_lookups;                     // 40  evaluation cache statistics of the tree
    unsigned long long pend_key;                      // 48  Zobrist key of the pending leaf (evaluation cache)
    uint16_t pend_nmoves;                             // 56
    uint8_t root_side, pend_side;                     // 58
    uint32_t ec_collisions;                           // 60  key matches whose stored position differed (taken as misses)
};
static_assert(sizeof(CzTreeRec) == 64, "CzTreeRec is one 64-byte line per tree");

template <typename T, int OFF>
struct CzRecField {
    char *base;
    __host__ __device__ __forceinline__ T &operator[](int g) const { return *reinterpret_cast<T *>(base + (size_t)g * sizeof(CzTreeRec) + OFF); }
};
#define CZ_REC_FIELD(type, name) CzRecField<type, offsetof(CzTreeRec, name)> name

struct CzTrees {
    CzPool pool;         // [max_games * cap]
    int cap;
    int words;           // ceil(cap / 64): 64-node words of the advance bitmap
    unsigned long long *mark_bits;   // [max_games][words] k_advance: which nodes of the tree are kept
    uint32_t *mark_rank;             // [max_games][words] kept nodes before the word = new index of its first kept node
    int32_t *adv_list, *adv_cnt;     // [max_games], [1]  k_advance_list: the trees that move at this cz_search_advance
    uint8_t *root_board; // [max_games][96]
    union {              // [max_games] records; t.<field>[g] addresses rec[g].<field>
        CzTreeRec *rec;
        CZ_REC_FIELD(int32_t, root_rr); CZ_REC_FIELD(int32_t, root_node); CZ_REC_FIELD(int32_t, n_nodes);
        CZ_REC_FIELD(int32_t, status); CZ_REC_FIELD(int32_t, sims); CZ_REC_FIELD(int16_t, last_depth); CZ_REC_FIELD(uint16_t, root_ply);
        CZ_REC_FIELD(int32_t, pend_kind); CZ_REC_FIELD(int32_t, pend_leaf); CZ_REC_FIELD(float, pend_value);
        CZ_REC_FIELD(int32_t, pend_depth); CZ_REC_FIELD(uint32_t, ec_hits); CZ_REC_FIELD(uint32_t, ec_lookups); CZ_REC_FIELD(uint32_t, ec_collisions);
        CZ_REC_FIELD(unsigned long long, pend_key); CZ_REC_FIELD(uint16_t, pend_nmoves);
        CZ_REC_FIELD(uint8_t, root_side); CZ_REC_FIELD(uint8_t, pend_side);
    };
    uint16_t *pend_moves;             // [max_games * width][128] legal moves of the pending leaves
    // the selected path of the pending simulation (width 1): node index per level below the root, so that the backup
    // updates all levels in parallel instead of chasing parent pointers (one dependent round trip per level)
    int32_t *pend_path;               // [max_games][CZ_PATH_MAX]
    // pending leaves of the width > 1 kernels (k_select_k / k_expand_backup_k), slot = tree * width + j
    int32_t *pk_kind, *pk_leaf;       // [max_games * width]
    float *pk_value;
    uint8_t *pk_side;
    uint16_t *pk_nmoves;
    // evaluation cache (cz_evalcache.h: what it is, its layout, the kernels' helpers).  Per-tree level, cz_search_set_eval_cache:
    unsigned long long *ec_key;       // [max_games][CZ_EC_ENTRIES]  0 = empty      (NULL: cache off)
    int32_t *ec_node;                 // [max_games][CZ_EC_ENTRIES]
    float *ec_val;                    // [max_games][CZ_EC_ENTRIES]
    uint32_t *ec_board;               // [max_games][CZ_EC_ENTRIES][12] the entry's position, packed (wave_pack_board): checked on every hit
    uint32_t *pend_board;             // [max_games][12] packed position of the pending leaf (select -> expand_backup)
    unsigned long long ec_key_mask;   // ~0; tests narrow it (cz_search_debug_eval_cache_key_bits) to force key collisions
    // cross-tree level, cz_search_set_xcache: ONE table per context behind ONE base pointer, its arrays through czx_*
    char *xc_base;                    // NULL: off
    uint32_t xc_mask;                 // buckets - 1 (a power of two); a bucket = 64 consecutive entries
    // compact evaluation batches (cz_search_select_compact): row of the step's leaf in planes / z / value, or -1
    int32_t *slot_of;                 // [max_games]
    int32_t *evcnt;                   // [2] rows handed out this step / next step (ping-pong, zeroed one step ahead)
    unsigned long long *evtotal;      // [2] rows evaluated, steps: running totals for the flop accounting
};

// The rules at the root and the table set of one consumer, host side: the match embeds one (cz_match), self-play one (cz_ctx).  The
// device view — rr (the fold is rr->fold) and tb_value — stays inside the consumer's kernel-argument struct; the functions on
// this one (cz_root_*, below) are the bodies of both consumers' setters and getters.
struct cz_ctx;
struct CzRootHost {
    // the consumer's contract (cz_root_begin): the names its error texts speak of, and where the two consumers differ
    const char *api, *handle, *since;   // "cz_match" / "cz_selfplay", "match" / "ctx", where the consumer's history starts
    bool rules_between_plies;   // the match: the rules may change between two plies, the first choose freezes only the fold and the chase rule
    bool owns_rules_part;       // the match: rr's arrays other than the chase part are a zeroed allocation of the first set_rules(1);
                                // self-play's live in sp_block and are k_sp_seed's to initialise
    bool rezero_chase;          // self-play: the chase rings are cleared at every switching on; the match's once, when they are made
    cz_ctx *c;                  // whose stream and device
    int G;                      // slots the arrays are carved for
    CzRootRules *rr;
    int16_t **tb_value;
    // the state
    int rules, chase;           // 0 king capture / 1 xiangqi; 1: perpetual chase is judged too (needs a fold); the avoid switch is rr->avoid
    bool chosen;                // a choose has run
    cz_tb_set *tb;              // the attached table set (not owned; held), or NULL
    void *rules_block, *chase_block, *tb_block;   // rr's two parts and tb_value, made at the first switching on, kept until cz_root_free
};

// the kernel families of cz_conv.hip that opt in to dynamic LDS once per context, both dtypes of a family together
enum CzLdsFamily { CZ_LDS_CONV, CZ_LDS_TOWER, CZ_LDS_SPLIT, CZ_LDS_MX, CZ_LDS_NFAMILIES };

struct cz_ctx {
    int device;
    hipStream_t stream;
    int max_games, cap, G;
    CzTables tab;      // device tables
    void *tab_block;   // single allocation behind `tab`
    const int16_t *tab_mirror;   // [2086] device copy of CzHostTables::mirror, in tab_block (cz_records_expand alone reads it)
    CzTrees t;
    void *tree_block;  // single allocation behind the per-tree arrays
    void *pool_block;
    bool adv_attr_set;   // dynamic-LDS opt-in of k_advance_lds done
    bool adv_force_global;   // cz_search_debug_advance_in_global_memory (tests): take the path of pools whose bitmap exceeds LDS
    bool lds_opt_in[CZ_LDS_NFAMILIES];   // dynamic-LDS opt-in of an MFMA kernel family done for this device (cz_conv.hip)
    int width;         // simulations in flight per tree the pending arrays are sized for (cz_search_set_width)
    void *pend_block;  // separate allocation of the pending arrays when width > 1
    int terminal_extra;   // cz_search_set_terminal_extra: terminal simulations a tree may complete inside one select launch
    int sim_target;    // cz_search_set_sim_target: completed simulations per tree a k > 1 search stops at (0: no limit)
    int step_parity;   // which evcnt entry the current compact step uses
    const int32_t *batch_count;  // cz_set_batch_count: device row count bounding the net launches, or NULL
    void *xc_block;      // cz_search_set_xcache: the cross-tree table's allocation
    int xc_log2_entries;
    const struct CzmTables *mask_tab;  // cz_maskgen.h tables on the device (k_movegen_mask)
    unsigned long long *clock_probe;  // cz_set_clock_probe: [clock_probe_wgs][4] stamps written by the trunk kernels, or NULL
    int clock_probe_wgs, clock_probe_last_grid;
    CzSelfplay sp;     // cz_selfplay_begin
    void *sp_block;    // NULL: no cz_selfplay_begin yet
    CzRootHost sp_root;      // the rules at the root of self-play and its table set, over sp.rr and sp.tb_value
    void *sp_resign_block;   // cz_selfplay_set_resign: allocated by its first call, sp.rs points into it while resignation is set
    void *ec_block;    // cz_search_set_eval_cache
};

// ---- device helpers shared by cz_search.hip / cz_selfplay.hip / cz_match.hip ----------------------
struct TreeView {
    float *P, *W, *Q;
    int32_t *N, *parent, *child_begin;
    uint16_t *child_count, *move;
    uint16_t *sd;   // src | dst << 8 of `move` (k_select applies the move without the label -> (src, dst) table round trip)
};

__device__ __forceinline__ TreeView view_of(const CzTrees &t, int g) {
    const CzPool &p = t.pool;
    const size_t base = (size_t)g * (size_t)t.cap;
    TreeView v;
    v.P = p.P + base; v.W = p.W + base; v.Q = p.Q + base;
    v.N = p.N + base; v.parent = p.parent + base; v.child_begin = p.child_begin + base;
    v.child_count = p.child_count + base; v.move = p.move + base; v.sd = p.sd + base;
    return v;
}

__device__ __forceinline__ void init_root(TreeView v, int idx) {
    v.P[idx] = 1.0f;  // p_ = 0.75 + 0.25 * dirichlet([0.3]) == 1 (quirk Q4), main.py:238
    v.W[idx] = 0.f; v.Q[idx] = 0.f; v.N[idx] = 0; v.parent[idx] = -1; v.child_begin[idx] = -1;
    v.child_count[idx] = 0; v.move[idx] = 0xFFFF; v.sd[idx] = 0;
}

#include "cz_evalcache.h"   // the evaluation cache: layout, czx_* accessors, ec_* / xc_* device helpers

// ---- a game at a root (the bench loop of cz_search.hip, cz_selfplay.hip, cz_match.hip) -----------
// MCTS_tree.reload (main.py:255-259): a fresh, unexpanded root for tree g on the position the root has, by one wave64.
// This is the whole list of what a fresh root owns besides its position: the counters, the pending leaf, node 0 and an
// empty evaluation cache.  Of the pending leaf only pend_kind = 0 is ever observed (k_expand_backup returns on it before
// it reads the other four, and select_body writes all five together); they are cleared with it so that the record of a
// fresh root does not depend on the tree's past.
__device__ __forceinline__ void fresh_root(const CzTrees &t, int g, int lane) {
    if (lane == 0) {
        t.root_node[g] = 0; t.n_nodes[g] = 1; t.status[g] = 0; t.sims[g] = 0; t.last_depth[g] = 0; t.root_ply[g] = 0;
        t.pend_kind[g] = 0; t.pend_leaf[g] = 0; t.pend_value[g] = 0.f; t.pend_side[g] = 0; t.pend_nmoves[g] = 0;
        init_root(view_of(t, g), 0);
    }
    ec_clear_tree(t, g, lane, 64);
}
// ... on position i of the caller's arrays: the squares boards[i * stride + 0 .. 89] (stored as the 96-byte root board, padding 0),
// the mover side[i], the restrict round rr[i] (rr == nullptr: 0).  The arrays, not their values: only lane 0 reads side and rr.
__device__ __forceinline__ void fresh_root(const CzTrees &t, int g, int lane, const uint8_t *__restrict__ boards, int stride,
                                           const uint8_t *__restrict__ side, const int32_t *__restrict__ rr, int i) {
    for (int j = lane; j < CZD_BOARD_LDS; j += 64)
        t.root_board[(size_t)g * CZD_BOARD_LDS + j] = j < CZ_NSQ ? boards[(size_t)i * stride + j] : (uint8_t)0;
    if (lane == 0) { t.root_side[g] = side[i] ? 1 : 0; t.root_rr[g] = rr ? rr[i] : 0; }
    fresh_root(t, g, lane);
}

// check_end (main.py:1380-1392) on a 96-byte board, by one wave64: is the red king ('K' = 1) / the black king ('k' = 8) gone
__device__ __forceinline__ void wave_kings_missing(const uint8_t *board, int lane, bool &Kmiss, bool &kmiss) {
    const int c0 = board[lane], c1 = (lane + 64 < CZ_NSQ) ? board[lane + 64] : 0;
    Kmiss = __ballot(c0 == 1 || c1 == 1) == 0ull;
    kmiss = __ballot(c0 == 8 || c1 == 8) == 0ull;
}
// the side code of the winner when a king is gone: 'K' missing -> black = 1, 'k' missing -> red = 0 (main.py:1384-1389, 1534-1537)
__device__ __forceinline__ int king_capture_winner(bool Kmiss) { return Kmiss ? 1 : 0; }
// check_end's tie: 60 plies without a capture (main.py:1388-1390)
__device__ __forceinline__ bool restrict_round_draw(int rr) { return rr >= 60; }

// root.child.items() (main.py:1339): the root's n children start at node cb of the view; n = 0 for an unexpanded root
__device__ __forceinline__ void root_children(const CzTrees &t, int g, const TreeView &v, int &cb, int &n) {
    const int root = t.root_node[g];
    cb = v.child_begin[root];
    n = cb < 0 ? 0 : (int)v.child_count[root];
}
// the mover has no child to play: the node pool was exhausted at the root, or the rules kernels overflowed (the reference
// has no node limit, so it has no such case); the driver's adjudication ends the game
__device__ __forceinline__ bool root_cannot_move(const CzTrees &t, int g, int n) {
    return n == 0 || (t.status[g] & (CZ_ST_NO_MOVES | CZ_ST_MOVE_OVERFLOW)) != 0;
}

// How the game at a root ended: `how` is 0 while it goes on, else the CZ_MATCH_* code (include/cchess_hip.h) of the ending, for
// every driver; `loser` the side code of the side that lost, -1 for a draw, an aborted game and a game that goes on.
struct CzGameEnd { int how, loser; };
// THE PRECEDENCE OF THE ENDINGS, at rule level LEVEL, on slot g after its choose and advance, by one wave64: the verdict of the
// repetition rule the choose left in rr.rep[g] (with CZ_REP_BY_CHASE: a chase) > a mated mover (rr.mated[g]) > a resignation >
// an aborted game > a table's value of the position after the move (CZ_MATCH_TABLEBASE) > check_end (main.py:1380-1392: a king is
// gone, then 60 plies without a capture) > the driver's ply cap.
// The first three were found by the choose on the root it then left untouched, so the side to move (root_side) is the mover that
// loses a mate or a resignation; `resigned` and `aborted` are the caller's own.  rr is not read below CZ_RULES_KINGSAFE.
// tb: what the attached table set answers for the root position (k_tb_probe_set), from the side to move's view — CZ_TB_MISS when no
// set is attached, for a slot that did not just move, and from the bench driver.  A covered value (neither CZ_TB_MISS nor
// CZ_TB_ILLEGAL) ends the game: tb > 0 the side to move wins, tb < 0 it loses, 0 a draw.  It stands in front of the no-capture
// counter and the ply cap because a forced mate is a mate whatever they say (the tables' own stance), and behind the endings the
// choose found because those were found on the root that was then not left: the table judges the position AFTER a move.
template <int LEVEL>
__device__ __forceinline__ CzGameEnd wave_game_end(const CzRootRules &rr, int g, bool resigned, bool aborted, int tb, const uint8_t *root_board,
                                                   int root_rr, int root_side, int ply, int max_plies, int lane) {
    int verdict = CZ_REP_NONE;
    bool by_chase = false;
    if constexpr (LEVEL >= CZ_RULES_REPETITION) verdict = rr.rep[g];
    if constexpr (LEVEL >= CZ_RULES_CHASE) { by_chase = (verdict & CZ_REP_BY_CHASE) != 0; verdict &= ~CZ_REP_BY_CHASE; }
    bool Kmiss, kmiss;
    wave_kings_missing(root_board, lane, Kmiss, kmiss);
    if (verdict == CZ_REP_DRAW) return {CZ_MATCH_REPETITION, -1};
    if (verdict != CZ_REP_NONE) return {by_chase ? CZ_MATCH_CHASE : CZ_MATCH_PERPETUAL, verdict == CZ_REP_RED_LOSES ? 0 : 1};
    if (LEVEL >= CZ_RULES_KINGSAFE && rr.mated[g]) return {CZ_MATCH_MATE, root_side};
    if (resigned) return {CZ_MATCH_RESIGN, root_side};
    if (aborted) return {CZ_MATCH_ABORTED, -1};
    if (tb != CZ_TB_MISS && tb != CZ_TB_ILLEGAL) return {CZ_MATCH_TABLEBASE, tb > 0 ? 1 - root_side : (tb < 0 ? root_side : -1)};
    if (Kmiss || kmiss) return {CZ_MATCH_KING, 1 - king_capture_winner(Kmiss)};
    if (restrict_round_draw(root_rr)) return {CZ_MATCH_RR60, -1};
    if (ply >= max_plies) return {CZ_MATCH_PLY_CAP, -1};
    return {0, -1};
}

// ---- move choice at a root (k_pick_ready, k_lines, and k_sp_choose / k_match_choose behind wave_choose_prologue) ----
// The candidates of a choice at a root, in generation order, by one wave64: the root's n <= CZD_MAXMOVES children at cb, or —
// mask != NULL ([CZ_MASK_WORDS]: the king-safe set of cz_movegen_kingsafe under rules = 1, root_allowed of cz_search_lines) —
// those of them whose label has its bit set, compacted.  N[r] / at[r] = the visit count / the index among the root's children
// of candidate lane + 64 r (0 past the last) -> their number.  sN / sI (LDS, CZD_MAXMOVES ints each): the same lists visible to
// every lane on return; the compaction goes through them, so a mask needs them, and all children without them (k_pick_ready,
// the king-capture choosers) cost no LDS and no barrier.
__device__ __forceinline__ int wave_root_candidates(const TreeView &v, int cb, int n, const uint32_t *__restrict__ mask, int lane, int N[2],
                                                    int at[2], int *sN, int *sI) {
    bool ok[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = lane + 64 * r;
        N[r] = 0; at[r] = 0;
        ok[r] = i < n;
        if (mask) {
            const uint32_t mv = ok[r] ? v.move[cb + i] : 0xFFFFu;
            ok[r] = mv < CZ_NLABELS && ((mask[mv >> 5] >> (mv & 31)) & 1u) != 0u;
        }
        if (ok[r]) { N[r] = v.N[cb + i]; at[r] = i; }
    }
    if (!sN) return n;
    // candidate j is the j-th child that is ok (without a mask: child j)
    const unsigned long long b0 = __ballot(ok[0]), b1 = __ballot(ok[1]), below = (1ull << lane) - 1ull;
    const int to[2] = {(int)__popcll(b0 & below), (int)(__popcll(b0) + __popcll(b1 & below))};
    n = __popcll(b0) + __popcll(b1);
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (ok[r]) { sN[to[r]] = N[r]; sI[to[r]] = at[r]; }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = lane + 64 * r;
        N[r] = i < n ? sN[i] : 0; at[r] = i < n ? sI[i] : 0;
    }
    return n;
}

// get_action in its T -> 0 limit (main.py:1332-1341): the first maximum of N over a root's n <= 128 children, in generation
// order (Python max() over root.child.items()) — N[r] is the visit count of child lane + 64 r; the index is wave-uniform
__device__ __forceinline__ int wave_most_visited(const int N[2], int n, int lane) {
    int bn = -1, bi = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (lane + 64 * r < n && N[r] > bn) { bn = N[r]; bi = lane + 64 * r; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int on = __shfl_xor(bn, d, 64), oi = __shfl_xor(bi, d, 64);
        if (on > bn || (on == bn && oi < bi)) { bn = on; bi = oi; }
    }
    return bi;
}

// The value a mover resigns on (cz_selfplay_set_resign, cz_match_set_resign): Q of the most visited candidate — the child
// wave_most_visited picks among the n candidates, N[r] / at[r] the visit count / the index among the root's children (at cb) of
// candidate lane + 64 r.  Q as the pool holds it, in the sign PUCT maximises: larger is better for the mover, a child that
// takes the king reads +1.  -> that child has a visit (a root value exists); q is wave-uniform
__device__ __forceinline__ bool wave_root_value(const TreeView &v, int cb, const int N[2], const int at[2], int n, int lane, float &q) {
    const int best = wave_most_visited(N, n, lane);
    const int bn = __shfl(best < 64 ? N[0] : N[1], best & 63, 64);
    const int bi = __shfl(best < 64 ? at[0] : at[1], best & 63, 64);
    q = v.Q[cb + bi];
    return bn > 0;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = fmax(x, __shfl_xor(x, d, 64));
    return x;
}
__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
    double x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// probs = softmax(1.0 / temperature * np.log(visits)), main.py:1341, over the n <= 128 children of a root: N[r] is the
// visit count of child lane + 64 r (0 past n).  log(0) = -inf -> probability 0; with no visit at all (zero playouts)
// the reference's softmax is NaN and np.random.choice raises: every child gets 1 / n.  pi[r] = 0 past n.
__device__ __forceinline__ void wave_visit_policy(const int N[2], int n, double inv_temp, int lane, double pi[2]) {
    double x[2], e[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = lane + 64 * r;
        x[r] = (i < n && N[r] > 0) ? inv_temp * log((double)N[r]) : -INFINITY;
    }
    const double m = wave_max(fmax(x[0], x[1]));
#pragma unroll
    for (int r = 0; r < 2; ++r) e[r] = (x[r] == -INFINITY || m == -INFINITY) ? 0.0 : exp(x[r] - m);
    const double se = wave_sum(e[0] + e[1]);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = lane + 64 * r;
        pi[r] = se > 0.0 ? e[r] / se : (i < n ? 1.0 / (double)n : 0.0);
    }
}

// np.random.choice(actions, p = ...) given its uniform u in [0, 1): inverse CDF over the children in generation order
// (p[r] of child lane + 64 r) -> the child index, wave-uniform
__device__ __forceinline__ int wave_pick_inverse_cdf(const double p[2], double u, int lane) {
    const double c0 = wave_incl_scan(p[0], lane);
    const double t0 = __shfl(c0, 63, 64);
    const double c1 = t0 + wave_incl_scan(p[1], lane);
    const double total = __shfl(c1, 63, 64);
    const double target = u * total;
    const unsigned long long h0 = __ballot(p[0] > 0.0 && c0 > target), h1 = __ballot(p[1] > 0.0 && c1 > target);
    int pick;
    if (h0) pick = __ffsll((long long)h0) - 1;
    else if (h1) pick = 64 + __ffsll((long long)h1) - 1;
    else {   // rounding at the upper end: the last child with a positive probability
        const unsigned long long q1 = __ballot(p[1] > 0.0), q0 = __ballot(p[0] > 0.0);
        pick = q1 ? 127 - __clzll((long long)q1) : (q0 ? 63 - __clzll((long long)q0) : 0);
    }
    return pick;
}

// ---- host functions of cz_search.hip that a second file calls -------------------------------------
// a tree's records in pre-order (cz_search_tree_dump; the second caller is cz_search_debug_eval_cache_dump, cz_evalcache.hip)
struct CzPreorder {
    int32_t n, root;                      // the tree's node count; its root node, -1 if that is no node of the tree
    std::vector<int32_t> child_begin;     // [n] the expansion records as downloaded
    std::vector<uint16_t> child_count;    // [n]
    std::vector<int32_t> node, depth;     // [records] record k is node[k], depth[k] levels below the root's children
};
int cz_tree_preorder(cz_ctx *c, int g, CzPreorder &out);   // after a stream synchronise
// every tree's evaluation-cache counters (CzTreeRec::ec_*) back to 0, in stream order: cz_search_set_eval_cache (cz_evalcache.hip)
int cz_search_clear_cache_stats(cz_ctx *c);

// ---- table sets (cz_tablebase.hip, cz_tablebase_set.hip; the consumers are cz_selfplay.hip and cz_match.hip) ----
struct CztbDesc;
// the signature -> its descriptor, or CZ_EINVAL with `who` in the text
int tb_desc(const char *who, const char *signature, CztbDesc *d);
// One k_tb_probe_set launch: position i < G is the 90 bytes at boards + i * board_stride and the byte side[i * side_stride].
// board_stride 90: boards at any address (cz_tb_set_probe); otherwise a multiple of 16 with 16-byte aligned boards, each lane
// reading its own row — the trees' root boards in place (CZD_BOARD_LDS apart, the sides inside the 64-byte tree records).
// moved [G] or NULL: position i is probed only when moved[i] is a label (< CZ_NLABELS), and answers CZ_TB_MISS otherwise.
int cz_tb_set_probe_strided(cz_ctx *c, const cz_tb_set *set, const uint8_t *boards, int board_stride, const uint8_t *side, int side_stride,
                            const uint16_t *moved, int G, int16_t *value, int32_t *which);
// a consumer takes / gives back its hold on a set: cz_tb_set_destroy refuses a set that is held
void cz_tb_set_hold(cz_tb_set *set, int delta);
// what both consumers' setters ask of a set and of their rule level: CZ_EINVAL with api ("cz_selfplay" / "cz_match") in the text
int cz_tb_set_attachable(const char *api, const char *handle, const cz_ctx *c, const cz_tb_set *set, int rules);

// ---- the rules at the root, host side (cz_rootrules.h; cz_match.hip, cz_selfplay.hip) ----
// the arrays of G slots inside the carver's allocation: the chase rings (chase_part), or everything else
inline void carve_root_rules(Carver &k, CzRootRules &rr, size_t G, bool chase_part) {
    if (chase_part) {
        rr.ring_chase = k.take<uint64_t>(G * 64 * 4);
        rr.root_chase = k.take<uint64_t>(G * 4);
        return;
    }
    rr.board = k.take<uint8_t>(G * CZ_NSQ);
    rr.side = k.take<uint8_t>(G);
    rr.safe = k.take<uint32_t>(G * CZ_MASK_WORDS);
    rr.mated = k.take<uint8_t>(G);
    rr.ring_key = k.take<uint64_t>(G * 64);
    rr.ring_check = k.take<uint8_t>(G * 64);
    rr.rep = k.take<uint8_t>(G);
    rr.flags = k.take<uint8_t>(G);
    rr.root_key = k.take<uint64_t>(G);
    rr.slot_ply = k.take<int32_t>(G);
    rr.slot_rr = k.take<int32_t>(G);
    rr.avoid_sum = k.take<uint8_t>(G);
}

// Between a consumer's root gather (wave_gather_root) and its choose kernel, level >= CZ_RULES_KINGSAFE: the king-safe sets of
// the G root positions; from CZ_RULES_REPETITION their check flags and keys; at CZ_RULES_CHASE their chase records.  Through
// the public entry points: their checks hold for a carved rr (every array set at the level that reads it, 256-byte aligned).
inline int czk_root_rules_prepare(cz_ctx *c, const CzRootRules &rr, int G, int level) {
    int rc = cz_movegen_kingsafe(c, rr.board, rr.side, G, nullptr, nullptr, rr.safe, level >= CZ_RULES_REPETITION ? rr.flags : nullptr, 0);
    if (rc == CZ_OK && level >= CZ_RULES_REPETITION) rc = cz_hash(c, rr.board, rr.side, G, rr.root_key);
    if (rc == CZ_OK && level >= CZ_RULES_CHASE) rc = cz_threats(c, rr.board, rr.side, G, rr.root_chase);
    return rc;
}

// The order a consumer's three setters keep — rules before the fold, the fold before the chase rule, off in the reverse order,
// nothing after the first choose (started), no rules 0 under an attached table set (tablebase) — for the call `what` with argument `value` on a consumer in state (rules, fold,
// chase).  api ("cz_match" / "cz_selfplay") and handle ("match" / "ctx") are the names the error texts speak of, since: where
// the consumer's history starts.
enum CzRuleSetter { CZ_SET_RULES, CZ_SET_REPETITION, CZ_SET_CHASE, CZ_SET_AVOID };
inline int cz_root_rules_order(const char *api, const char *handle, const char *since, int what, int value, int rules, int fold, int chase,
                               bool started, bool tablebase = false, int avoid = 0) {
    const std::string a(api), h(handle), late = "before the first " + a + "_choose only (";
    std::string e;
    if (what == CZ_SET_RULES) {
        if (value != 0 && value != 1) e = a + "_set_rules: rules 0 (king capture) or 1 (xiangqi)";
        else if (started) e = a + "_set_rules: " + late + "a game is played under one set of rules)";
        else if (value == 0 && fold != 0) e = a + "_set_rules: the repetition rule needs rules 1: " + a + "_set_repetition(" + h + ", 0) first";
        else if (value == 0 && tablebase) e = a + "_set_rules: the table set needs rules 1: " + a + "_set_tablebase(" + h + ", NULL) first";
    } else if (what == CZ_SET_REPETITION) {
        if (value != 0 && (value < 2 || value > 8)) e = a + "_set_repetition: fold 0 (off) or 2..8";
        else if (started) e = a + "_set_repetition: " + late + since + ")";
        else if (value != 0 && rules != 1) e = a + "_set_repetition: " + a + "_set_rules(" + h + ", 1) first (the check flags are the king-safe pass's)";
        else if (value == 0 && chase != 0) e = a + "_set_repetition: the chase rule needs a fold: " + a + "_set_chase(" + h + ", 0) first";
        else if (value == 0 && avoid != 0) e = a + "_set_repetition: the avoid step needs a fold: " + a + "_set_avoid(" + h + ", 0) first";
    } else if (what == CZ_SET_AVOID) {
        if (value != 0 && value != 1) e = a + "_set_avoid: on 0 or 1";
        else if (started) e = a + "_set_avoid: " + late + since + ")";
        else if (value != 0 && fold == 0) e = a + "_set_avoid: " + a + "_set_repetition(" + h + ", fold) first (a move is judged by the repetition rule)";
    } else {
        if (value != 0 && value != 1) e = a + "_set_chase: on 0 or 1";
        else if (started) e = a + "_set_chase: " + late + since + ")";
        else if (value != 0 && fold == 0) e = a + "_set_chase: " + a + "_set_repetition(" + h + ", fold) first (a chase is judged on a repeated position)";
    }
    if (e.empty()) return CZ_OK;
    cz_set_error("%s", e.c_str());
    return CZ_EINVAL;
}

// ---- one consumer's rules at the root and table set (CzRootHost): what the public setters and getters of both call ----
// A consumer starts (cz_match_create, cz_selfplay_begin): its contract — the first ten fields of `contract` —, rules, fold and
// chase off, nothing chosen, no set attached; the blocks it has stay for the next switching on.
inline void cz_root_begin(CzRootHost &h, CzRootHost contract) {
    cz_tb_set_hold(h.tb, -1);
    contract.rules_block = h.rules_block; contract.chase_block = h.chase_block; contract.tb_block = h.tb_block;
    h = contract;
    h.rr->fold = 0;
    h.rr->avoid = 0;
    *h.tb_value = nullptr;
}
inline int cz_root_order(const CzRootHost &h, int what, int value) {
    return cz_root_rules_order(h.api, h.handle, h.since, what, value, h.rules, h.rr->fold, h.chase,
                               h.chosen && !(what == CZ_SET_RULES && h.rules_between_plies), h.tb != nullptr, h.rr->avoid);
}
// one part of rr (carve_root_rules) in a zeroed allocation of its own, for the setter `_set_<what>`
inline int cz_root_carve(CzRootHost &h, void **block, bool chase_part, const char *what) {
    return carve_alloc(block, h.c->stream, true, (std::string(h.api) + "_set_" + what).c_str(),
                       [&](Carver &k) { carve_root_rules(k, *h.rr, (size_t)h.G, chase_part); });
}
inline int cz_root_set_rules(CzRootHost &h, int rules) {
    if (const int rc = cz_root_order(h, CZ_SET_RULES, rules)) return rc;
    if (rules == 1 && h.owns_rules_part && !h.rules_block) {
        if (const int rc = cz_root_carve(h, &h.rules_block, false, "rules")) return rc;
    }
    h.rules = rules;
    return CZ_OK;
}
inline int cz_root_set_repetition(CzRootHost &h, int fold) {
    if (const int rc = cz_root_order(h, CZ_SET_REPETITION, fold)) return rc;
    h.rr->fold = fold;
    return CZ_OK;
}
inline int cz_root_set_chase(CzRootHost &h, int on) {
    if (const int rc = cz_root_order(h, CZ_SET_CHASE, on)) return rc;
    if (on && (h.rezero_chase || !h.chase_block)) {
        if (const int rc = cz_root_carve(h, &h.chase_block, true, "chase")) return rc;
    }
    h.chase = on;
    return CZ_OK;
}
inline int cz_root_set_avoid(CzRootHost &h, int on) {
    if (const int rc = cz_root_order(h, CZ_SET_AVOID, on)) return rc;
    h.rr->avoid = on;
    return CZ_OK;
}
// The avoid step (cz_repmoves.hip): one launch of wave_repetition_moves over the G slots' rings, between the root pass and
// the choose kernel; rr.safe becomes the set without the moves that lose by repetition, rr.avoid_sum what happened.
int czv_root_avoid(cz_ctx *c, const CzRootRules &rr, int G, int chase);
// the device pointers of the rings, owned by the consumer; CZ_EINVAL while the rule is off
inline int cz_root_history(const CzRootHost &h, const uint64_t **keys, const uint8_t **checks) {
    if (h.rr->fold == 0) { cz_set_error("%s_history: %s_set_repetition first", h.api, h.api); return CZ_EINVAL; }
    if (keys) *keys = h.rr->ring_key;
    if (checks) *checks = h.rr->ring_check;
    return CZ_OK;
}
inline int cz_root_chase_history(const CzRootHost &h, const uint64_t **chase) {
    if (h.chase == 0) { cz_set_error("%s_chase_history: %s_set_chase first", h.api, h.api); return CZ_EINVAL; }
    if (chase) *chase = h.rr->ring_chase;
    return CZ_OK;
}
// attaches `set` (NULL: detaches): what cz_tb_set_attachable asks, tb_value [G] in an allocation made once, the holds
inline int cz_root_set_tablebase(CzRootHost &h, cz_tb_set *set) {
    if (const int rc = cz_tb_set_attachable(h.api, h.handle, h.c, set, h.rules)) return rc;
    *h.tb_value = nullptr;
    if (set) {
        const int rc = carve_alloc(&h.tb_block, h.c->stream, false, (std::string(h.api) + "_set_tablebase").c_str(),
                                   [&](Carver &k) { *h.tb_value = k.take<int16_t>((size_t)h.G); });
        if (rc != CZ_OK) { *h.tb_value = nullptr; return rc; }
    }
    cz_tb_set_hold(set, 1);
    cz_tb_set_hold(h.tb, -1);
    h.tb = set;
    return CZ_OK;
}
// In front of an adjudicate kernel: the attached set's value of the G root positions of h.c's trees after the move, read in
// place — boards 96 bytes apart, sides in the tree records — into tb_value.  Nothing without a set.
inline int cz_root_probe(const CzRootHost &h, const uint16_t *played, int G) {
    if (!h.tb || !*h.tb_value) return CZ_OK;
    const CzTrees &t = h.c->t;
    return cz_tb_set_probe_strided(h.c, h.tb, t.root_board, CZD_BOARD_LDS, &t.root_side[0], (int)sizeof(CzTreeRec), played, G, *h.tb_value, nullptr);
}
inline int cz_root_level(const CzRootHost &h) { return cz_rules_level(h.rules, h.rr->fold, h.chase); }
// A consumer's choose over G slots.  From CZ_RULES_KINGSAFE: gather(), its launch of the kernel that copies every slot's root
// position out (wave_gather_root), then what the rules need of them; then choose(L), its launch of the choose kernel at level L.
template <typename Gather, typename Choose>
inline int cz_root_choose(CzRootHost &h, int G, Gather gather, Choose choose) {
    h.chosen = true;
    const int level = cz_root_level(h);
    if (level >= CZ_RULES_KINGSAFE) {
        gather();
        CZ_HIP(hipGetLastError());
        if (const int rc = czk_root_rules_prepare(h.c, *h.rr, G, level)) return rc;
        if (h.rr->avoid && level >= CZ_RULES_REPETITION)
            if (const int rc = czv_root_avoid(h.c, *h.rr, G, h.chase)) return rc;
    }
    cz_by_rules_level(level, choose);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
// A consumer's adjudicate: the probe, then adjudicate(L), its launch of the adjudicate kernel at level L
template <typename Adjudicate>
inline int cz_root_adjudicate(const CzRootHost &h, const uint16_t *played, int G, Adjudicate adjudicate) {
    if (const int rc = cz_root_probe(h, played, G)) return rc;
    cz_by_rules_level(cz_root_level(h), adjudicate);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
// the hold on the set and the blocks (the set itself is the caller's)
inline void cz_root_free(CzRootHost &h) {
    cz_tb_set_hold(h.tb, -1);
    for (void *b : {h.rules_block, h.chase_block, h.tb_block})
        if (b) (void)hipFree(b);
}
