/*
 * cchess_hip.h — C-ABI of libcchess_hip.so: the MI355X (gfx950) hot path of cchess-zero.
 *
 * The reference (chengstone/cchess-zero) is pure Python and has no FFI layer; its boundary
 * for this path is the class surface of main.py.  Each entry point below names the
 * reference interface it replaces (file:line, relative to the reference repo).  The Python
 * façade that keeps the reference's class/CLI names (main.py, policy_value_network.py at the
 * repo root of this project) binds exactly these symbols through ctypes — see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative CZ_E* code on failure;
 *     cz_last_error() returns a thread-local message for the last failure.
 *   - cz_ctx owns one HIP device, one stream and all device buffers of G game trees.  A ctx is
 *     not thread-safe; distinct ctxs are independent (one per GPU / process).
 *   - all array arguments are DEVICE pointers (e.g. torch tensors' data_ptr()); they are
 *     borrowed for the duration of the enqueued work, never freed by the library.  Work is
 *     enqueued on the ctx stream (cz_set_stream) and is asynchronous; cz_synchronize waits.
 *     cz_malloc/cz_upload/cz_download exist for callers without a tensor library.
 *
 * Data formats (shared with the CPU oracle, oracle/cchess_oracle.h)
 *   board   uint8[90], sq = y*9 + x; y = rank 0..9 (rank 0 = first row of the reference's
 *           state string = red / upper-case / 'w' home, main.py:585), x = file 'a'..'i'.
 *           code 0 = empty, 1..14 = 1 + index in pieces_order "KARBNPCkarbnpc" (main.py:208).
 *   side    uint8: 0 = 'w' (red, upper case) to move, 1 = 'b' (black).
 *   label   uint16 index into the 2086-entry move vocabulary labels_array (main.py:30-65,211).
 *   planes  [G][9][10][C] (C >= 14), element (h,w,c) = 1 iff the side-to-move-canonical board
 *           has piece code c+1 on cell h*9+w — the reference's 9-stride quirk (SURVEY Q1,
 *           main.py:547-557) is reproduced; channels >= 14 are zero padding.
 */
#ifndef CCHESS_HIP_H
#define CCHESS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CZ_NLABELS 2086
#define CZ_MAXMOVES 128
#define CZ_NSQ 90
#define CZ_MASK_WORDS 66 /* ceil(2086/32) */

#define CZ_OK 0
#define CZ_EINVAL (-1)
#define CZ_EHIP (-2)
#define CZ_ENOMEM (-3)

#define CZ_F32 0
#define CZ_BF16 1
#define CZ_F16 2 /* IEEE half: accepted where planes are written (cz_encode_planes, cz_search_select[_k]) */

/* status bits reported by cz_search_status */
#define CZ_ST_POOL_EXHAUSTED 1 /* node pool of the tree is full: expansion skipped */
#define CZ_ST_NO_MOVES 2       /* an expanded node with zero legal moves was selected (reference raises, quirk Q7) */
#define CZ_ST_MOVE_OVERFLOW 4  /* > 128 moves or a move without a label */
#define CZ_ST_BAD_ADVANCE 8    /* played move is not a child of the root (reference: KeyError) */

/* One self-play training record (cz_selfplay_*): the tuple cchess_main.selfplay appends per ply (main.py:1504-1518) in
 * packed form.  board = root position BEFORE the move in real coordinates (the canonical, side-to-move-first state of
 * the reference is try_flip of it for black, main.py:1505), side = mover, count = number of root children,
 * z = game result from the mover's point of view (main.py:1533-1544), labels/visits = the root's children in generation
 * order (root.child.items(), main.py:1339) with their visit counts N — pi = softmax(1/T * log(visits)) (main.py:1341) is
 * recomputed from them on the host in float64, bit for bit.  Unused label slots hold 0xFFFF, unused visits 0. */
#define CZ_REC_BYTES 608
#define CZ_REC_SIDE 90    /* uint8 */
#define CZ_REC_COUNT 91   /* uint8 */
#define CZ_REC_Z 92       /* int8: +1 / -1 / 0 */
#define CZ_REC_FLAGS 93   /* uint8: bit 0 = a visit count saturated at 65535 */
#define CZ_REC_PLY 94     /* uint16: index of the ply in its game */
#define CZ_REC_LABELS 96  /* uint16[128] */
#define CZ_REC_VISITS 352 /* uint16[128] */
/* cz_selfplay_stats slots */
#define CZ_SP_NSTATS 8
#define CZ_SP_GAMES 0      /* games finished (including stalled ones) */
#define CZ_SP_RED_WINS 1   /* 'k' captured: "w" wins */
#define CZ_SP_BLACK_WINS 2 /* 'K' captured: "b" wins */
#define CZ_SP_DRAWS 3      /* restrict_round >= 60 (main.py:1542) or the history capacity reached */
#define CZ_SP_PLIES 4      /* records handed to the ring */
#define CZ_SP_STALLED 5    /* games dropped because the root had no child to play (node pool exhausted) */
#define CZ_SP_DROPPED 6    /* records dropped because the ring was full */
#define CZ_SP_SIMS 7       /* simulations of the searches behind the moves played so far */

typedef struct cz_ctx cz_ctx;

const char *cz_last_error(void);
/* host utility: CRC-32C (Castagnoli) of a host buffer — the checksum of the reference's tf.train.Saver checkpoint files
 * (policy_value_network.py:148,176-184), read and written by cchess_zero_amd/tf_checkpoint.py */
unsigned int cz_crc32c(const void *data, size_t n);
int cz_version(void);

/* ---- static tables (host pointers, valid for the process lifetime) --------------------------
 * replaces: create_uci_labels / labels_array / label2i / unflipped_index, main.py:23-65,211-217.
 *   lut90x90[src*90+dst] -> label or -1;  unflip2086[i] = unflipped_index[i];
 *   labels = 2086 x 5 chars ("a0a1\0");   srcdst[i] = src | dst << 8. */
int cz_tables(const int16_t **lut90x90, const int16_t **unflip2086, const char **labels,
              const uint16_t **srcdst);
/* The left-right symmetry of the board on the move vocabulary (host pointer, valid for the process lifetime; the reference has
 * no such table): mirror2086[i] = the label of move i with both files mirrored across the e-file (a..i -> i..a, ranks
 * unchanged), looked up through the 90x90 LUT like unflip2086.  A permutation and an involution; its 90 fixed points are the
 * vertical moves on the e-file; it commutes with unflip2086. */
int cz_mirror_table(const int16_t **mirror2086);
/* Zobrist keys used by cz_hash / cz_apply_move: keys[15][90] (row 0 unused), side key.
 * The reference has no state hash (identity = the state string); this format is ours. */
int cz_zobrist(const uint64_t **keys15x90, uint64_t *side_key);

/* ---- context ------------------------------------------------------------------------------
 * replaces: cchess_main.__init__ building GameBoard + MCTS_tree, main.py:1140-1144. */
int cz_create(int device, int max_games, int max_nodes_per_tree, cz_ctx **out);
void cz_destroy(cz_ctx *);
int cz_set_stream(cz_ctx *, void *hip_stream /* hipStream_t, NULL = default stream */);
int cz_synchronize(cz_ctx *);
int cz_malloc(cz_ctx *, size_t bytes, void **dptr);
int cz_free(cz_ctx *, void *dptr);
int cz_upload(cz_ctx *, void *dst_device, const void *src_host, size_t bytes);
int cz_download(cz_ctx *, void *dst_host, const void *src_device, size_t bytes);

/* ---- rules kernels (stand-alone, G positions per launch) -----------------------------------
 * K1  replaces GameBoard.get_legal_moves, main.py:743-1109.
 *     moves [G][128] labels in the reference's generation order (0xFFFF padding), count [G];
 *     mask [G][66] 2086-bit legality mask (bit i of word i/32).  moves or mask may be NULL.
 *     Alignment: `moves` must be 16-byte aligned (the list rows leave as 16-byte stores; CZ_EINVAL otherwise); boards, side,
 *     count and mask may sit at any byte / element address (unaligned inputs take a slower staging path).
 *     A board this library cannot be asked about answers count 0xFFFF (its list / mask row is undefined): more than 16 pieces of
 *     the side to move, more of a kind than a Xiangqi set holds (3 rooks / cannons / knights / advisors / bishops, 6 pawns, 2
 *     kings of the side to move — the one-lane-per-position generators take a kind's squares as the lowest and highest of its
 *     set), or an advisor / bishop step the 2086-label vocabulary has no label for. */
int cz_movegen(cz_ctx *, const uint8_t *boards, const uint8_t *side, int G, uint16_t *moves,
               uint16_t *count, uint32_t *mask);
/*     cz_movegen_ex: the same with flags.  CZ_MOVES_NO_PAD: row g of `moves` is written up to count[g] only (in 16-byte pieces; the
 *     labels behind count[g] are UNDEFINED, not 0xFFFF) — the padding is two thirds of a row (~40 moves per position, main.py:743)
 *     and was 1.97x the ordered kernel's algorithmic HBM traffic; a caller that reads rows up to `count`, as every consumer of
 *     get_legal_moves' list does, loses nothing.  flags = 0 is cz_movegen.
 *     The count-0xFFFF restriction above is the stand-alone kernels' only: the generator INSIDE the search (k_select, lane =
 *     piece, csrc/cz_device.h) generates moves for any board the reference's get_legal_moves does. */
#define CZ_MOVES_NO_PAD 1
int cz_movegen_ex(cz_ctx *, const uint8_t *boards, const uint8_t *side, int G, uint16_t *moves,
                  uint16_t *count, uint32_t *mask, int flags);
/* K1s KING-SAFE move generation.  No reference function: the reference plays king-capture games and its get_legal_moves
 *     (main.py:743-1109, the generator this entry point filters) lets a side leave its king attacked.  Here a side is
 *     ATTACKED when it has a king and the other side has a pseudo-legal move onto the king's square — the flying general
 *     (main.py:1097-1107) is such a move — and a pseudo-legal move is KING-SAFE when the mover is not attacked after it (one
 *     rule, also for a move that takes the king and for a board without the mover's king: every move is safe there).
 *     moves [G][128]: the king-safe moves in get_legal_moves' order (0xFFFF padding; CZ_MOVES_NO_PAD as in cz_movegen_ex);
 *     count [G]: their number; mask [G][66]: their set; pos_flags [G]: CZ_POS_*.  Any of the four may be NULL; with only
 *     pos_flags (and / or count) this is the "in check?" query and neither list nor set rows are built.
 *     Alignment as for cz_movegen: `moves` 16-byte aligned, everything else at any address.  A board cz_movegen answers with
 *     count 0xFFFF answers count 0xFFFF here too (its rows are undefined, its flags 0).  Repetition and perpetual check
 *     are judged by cz_repetition below, on a game's history; perpetual chase by cz_threats and cz_repetition_chase. */
#define CZ_POS_IN_CHECK 1        /* the side to move is attacked */
#define CZ_POS_CAN_TAKE_KING 2   /* the other side is attacked: the side to move can take its king */
#define CZ_POS_NO_SAFE_MOVE 4    /* no king-safe move: checkmate or stalemate, both lost in Xiangqi */
int cz_movegen_kingsafe(cz_ctx *, const uint8_t *boards, const uint8_t *side, int G, uint16_t *moves, uint16_t *count,
                        uint32_t *mask, uint8_t *pos_flags, int flags);
/* K1c CHECKING MOVES: the king-safe moves of cz_movegen_kingsafe that GIVE CHECK — after the move the other side is attacked
 *     (the definition above) — in the same order, the other moves taken out.  What a continuous-check mate search expands an
 *     attacker's position by, without making the ~40 children and asking each whether it is in check.
 *     moves [G][128], count [G]: that list (0xFFFF padding; CZ_MOVES_NO_PAD as in cz_movegen_ex) and its length; pos_flags [G]:
 *     the POSITION's CZ_POS_* exactly as cz_movegen_kingsafe writes them — CZ_POS_NO_SAFE_MOVE speaks of all king-safe moves,
 *     not of the checks.  A move that takes the other king gives no check (a side without a king is not attacked).  Any of
 *     the three may be NULL, not all; `moves` 16-byte aligned; a refused board answers count 0xFFFF and flags 0. */
int cz_movegen_checks(cz_ctx *, const uint8_t *boards, const uint8_t *side, int G, uint16_t *moves, uint16_t *count,
                      uint8_t *pos_flags, int flags);
/* K1r REPETITION AND PERPETUAL CHECK on G game records that the caller keeps.  No reference function: the reference's games
 *     have no repetition rule.  A game's history is the sequence of its positions: position i is the position after i plies
 *     (position 0 is the opening), with key[i] = its cz_hash (board and side to move; equal keys are taken as equal positions)
 *     and in_check[i] != 0 when the side to move at i is attacked (CZ_POS_IN_CHECK).  Let n be the current position and w how
 *     far back to look:
 *       1. the earlier occurrences are the i with n - w <= i < n and key[i] == key[n];
 *       2. with fewer than fold - 1 of them there is no verdict;
 *       3. otherwise j is the (fold - 1)-th most recent of them, and the cycle is the positions j + 1 .. n;
 *       4. side X checked perpetually when every position of the cycle with side 1 - X to move — the positions X's moves
 *          led to — has in_check set, and there is at least one such position;
 *       5. exactly one side checked perpetually: that side loses; neither or both: a draw.
 *     Perpetual CHASE is not judged by this call: a chase that repeats is a draw here (cz_repetition_chase below judges it).
 *     keys uint64 [G][stride], in_check uint8 [G][stride]: position i of game g at g * stride + i; len int32 [G]: 1 <= len[g] <=
 *     stride, the current position is len[g] - 1 (a length outside that range answers CZ_REP_NONE / -1: nothing is read);
 *     window int32 [G]: w, clamped to 0 .. len[g] - 1, or NULL = every earlier position; side uint8 [G]: the side to move in the
 *     current position (the earlier sides follow by parity); 2 <= fold <= 8 (3: the usual threefold rule).
 *     verdict uint8 [G] out: CZ_REP_*; first int32 [G] out (may be NULL): j, or -1 without a verdict.  One wave per game, the
 *     history in chunks of 64 positions, most recent first.  All device arrays, at any address their element type allows. */
#define CZ_REP_NONE 0          /* fewer than fold occurrences inside the window */
#define CZ_REP_DRAW 1          /* repeated; neither side, or both, checked with every move of the cycle */
#define CZ_REP_RED_LOSES 2     /* red checked with every move of the cycle, black did not */
#define CZ_REP_BLACK_LOSES 3   /* black checked with every move of the cycle, red did not */
int cz_repetition(cz_ctx *, const uint64_t *keys, const uint8_t *in_check, int stride, const int32_t *len, const int32_t *window,
                  const uint8_t *side, int G, int fold, uint8_t *verdict, int32_t *first);
/* K1t THREATS: the attack-and-protection analysis of the perpetual-chase rule.  No reference function.  s is the side to
 *     move (the possible victim), X = 1 - s the side that just moved.  Square t is THREATENED when it holds a piece of s and
 *     some pseudo-legal move a -> t of X on this board (cz_movegen's list for X) passes all of:
 *       1. the attacker on a is a rook, cannon, knight, advisor or bishop (kings and pawns may chase freely);
 *       2. the victim on t is not the king and not a pawn on its own side of the river (a crossed pawn counts);
 *       3. the capture is king-safe for X (cz_movegen_kingsafe's rule: a pinned piece threatens nothing);
 *       4. it is no exchange offer: attacker and victim are of one kind and s has the pseudo-legal move t -> a;
 *       5. the victim is not protected, unless it is worth more than the attacker (R 3, N = C 2, A = B = P 1).  PROTECTED:
 *          after a x t, s has a pseudo-legal move onto t — pseudo-legal on purpose (a pinned protector protects): this is
 *          the library's definition.
 *     chase uint64 [G][4] out, 8-byte aligned: words 0, 1 the threatened set (bit q of word 0 = square q < 64, bit q - 64 of
 *     word 1 = square 64 .. 89), words 2, 3 the squares of the side to move in the same layout: a position's CHASE RECORD.  A
 *     board cz_movegen refuses for either side (not a Xiangqi set, an advisor / bishop step without a label) answers four
 *     zero words.  boards and side at any address.  One lane per position. */
int cz_threats(cz_ctx *, const uint8_t *boards, const uint8_t *side, int G, uint64_t *chase);
/* K1c REPETITION, PERPETUAL CHECK AND PERPETUAL CHASE: cz_repetition (same records, lengths, windows, fold and refusals; its
 *     steps 1 - 5) with the chase record of every position beside its key, chase uint64 [G][stride][4] (cz_threats):
 *       6. exactly one side checked perpetually: cz_repetition's verdict, cause CZ_CAUSE_CHECK — perpetual check outranks a
 *          chase by the other side; both sides checked perpetually: a draw;
 *       7. otherwise side X CHASES perpetually when one and the same piece of 1 - X is threatened in every position of the cycle
 *          that X's moves led to (at least one).  The piece is followed from such a position to the next by the one "from" and
 *          one "to" square in which the squares of 1 - X differ (a cycle holds no capture; records that differ in another way
 *          follow nothing).  A threat that merely stands while X moves something else counts: the rule looks at the position
 *          after each of X's moves;
 *       8. exactly one side chases perpetually: that side loses, cause CZ_CAUSE_CHASE; neither or both: a draw.
 *     NOT judged: a cycle that mixes checks and chases move by move is a draw, and two pieces of one kind that swap places over
 *     a cycle are not told apart.
 *     verdict uint8 [G] out: CZ_REP_*; first int32 [G] out (may be NULL) as in cz_repetition; cause uint8 [G] out (may be NULL):
 *     CZ_CAUSE_* (NONE without a verdict and for a draw). */
#define CZ_CAUSE_NONE 0
#define CZ_CAUSE_CHECK 1
#define CZ_CAUSE_CHASE 2
int cz_repetition_chase(cz_ctx *, const uint64_t *keys, const uint8_t *in_check, const uint64_t *chase, int stride, const int32_t *len,
                        const int32_t *window, const uint8_t *side, int G, int fold, uint8_t *verdict, int32_t *first, uint8_t *cause);
/* K1m REPETITION VERDICTS ON MOVES: what cz_repetition_chase WOULD answer after every king-safe move of G positions, and after
 *     every king-safe reply to it — the lookahead of a mover who does not want to lose by repetition.  No new rule: every
 *     verdict is that call's on the record extended by the new position's cz_hash, CZ_POS_IN_CHECK flag and cz_threats record.
 *     boards [G][90], side [G]: the current positions.  keys, in_check, chase, stride, len, window, fold: the games' records
 *     exactly as cz_repetition_chase takes them, the current position being position len[g] - 1 OF THE RECORD (its key, flag
 *     and chase record are read there, not computed); chase == NULL: no chase rule, as cz_repetition (a loss then has cause
 *     CZ_CAUSE_CHECK).  window[g] (NULL: every earlier position) is the current position's window w.
 *       CANDIDATE j is the j-th king-safe move of the current position, in cz_movegen_kingsafe's order; it makes position len.
 *         Its window is 0 after a capture, else min(w + 1, len).
 *       A REPLY is a king-safe move of the position after the candidate; it makes position len + 1, its window by the same step.
 *       A candidate is LOSING when its own verdict is a loss for the mover, or its own verdict is CZ_REP_NONE and some reply's
 *         verdict is a loss for the mover.
 *     Outputs, each NULL or (not all NULL):
 *       moves uint16 [G][128] (16-byte aligned, CZ_EINVAL otherwise), count uint16 [G]: the king-safe list as
 *         cz_movegen_kingsafe writes it (0xFFFF padding);
 *       verdict uint8 [G][128]: CZ_REP_* | CZ_CAUSE_* << 4 of the position after candidate j (0 behind the list);
 *       reply uint16 [G][128], reply_verdict uint8 [G][128]: the first king-safe reply to candidate j, in generation order,
 *         whose verdict is a loss for the mover, and that verdict; 0xFFFF / 0 when there is none;
 *       allowed uint32 [G][66]: the king-safe set without the losing candidates — or the whole king-safe set when every
 *         candidate is losing: a forced loss is still a move;
 *       summary uint8 [G]: CZ_REPMOVES_* below.
 *     A board cz_movegen_kingsafe refuses answers count 0xFFFF and zeros in every other row.  A length outside 1 .. stride
 *     reads nothing of the record: the list and the whole set, no verdict.  G == 0: CZ_OK, no launch.  One launch, one wave
 *     per game, a pure function of the input; no position it makes is written to memory. */
#define CZ_REPMOVES_REMOVED 1      /* some candidate is losing and was taken out of allowed */
#define CZ_REPMOVES_FORCED 2       /* every candidate is losing (at least one): allowed is the king-safe set */
#define CZ_REPMOVES_OPP_LOSES 4    /* some candidate's own verdict is a loss for the opponent */
int cz_repetition_moves(cz_ctx *, const uint8_t *boards, const uint8_t *side, const uint64_t *keys, const uint8_t *in_check,
                        const uint64_t *chase, int stride, const int32_t *len, const int32_t *window, int G, int fold, uint16_t *moves,
                        uint16_t *count, uint8_t *verdict, uint16_t *reply, uint8_t *reply_verdict, uint32_t *allowed, uint8_t *summary);
/* K2  replaces GameBoard.sim_do_action (main.py:647-702), is_kill_move (:226) and the king test
 *     (:409-413).  Updates boards/side in place.  hash: in/out incremental Zobrist (may be NULL);
 *     captured [G] = captured piece code or 0; terminal [G]: bit0 'K' missing, bit1 'k' missing.
 *     move_label 0xFFFF leaves the game untouched. */
int cz_apply_move(cz_ctx *, uint8_t *boards, uint8_t *side, const uint16_t *move_label, int G,
                  uint64_t *hash, uint8_t *captured, int8_t *terminal);
int cz_hash(cz_ctx *, const uint8_t *boards, const uint8_t *side, int G, uint64_t *hash);
/* K2s SUCCESSORS: every position one move away from G positions.  No reference function (the reference plays one move per
 *     game, sim_do_action, main.py:647-702); the move is made as cz_apply_move makes it.
 *     moves [G][128]: a move list as cz_movegen / cz_movegen_ex / cz_movegen_kingsafe write it, padded or CZ_MOVES_NO_PAD; the
 *     kernel generates no move itself, so pseudo-legal and king-safe lists serve alike.  offsets int32 [G + 1]: the exclusive
 *     prefix sum of the per-position counts, offsets[G] == total — the only source of how many children a parent has: parent
 *     g has offsets[g + 1] - offsets[g] of them, 0 .. 128 (the caller gives a board with count 0xFFFF none).
 *     Child offsets[g] + j is parent g after moves[g][j], in list order: the output is a pure function of the input (no
 *     atomics).  Per child: out_boards [total][90]; out_side = 1 - the parent's side; out_captured = the piece code taken or
 *     0, as cz_apply_move reports it; out_parent int32 = g; out_label = the move.  Every output but out_boards may be NULL.  A
 *     label >= 2086 in the list leaves the child the parent's board (captured 0).
 *     Alignment: out_boards must be 16-byte aligned (the children leave as 16-byte stores; CZ_EINVAL otherwise); everything
 *     else may sit at any address its element type allows.  G == 0 or total == 0: CZ_OK, no launch.  Offsets outside
 *     [0, total] are clamped: no access leaves the arrays whatever they hold. */
int cz_successors(cz_ctx *, const uint8_t *boards, const uint8_t *side, int G, const uint16_t *moves /* [G][128] */,
                  const int32_t *offsets /* [G + 1] */, int total, uint8_t *out_boards /* [total][90] */, uint8_t *out_side,
                  uint8_t *out_captured, int32_t *out_parent, uint16_t *out_label);
/* K2m MATE BACKUP: the AND/OR step of a forced-mate search over the child ranges cz_successors lays out.  dist is the number
 *     of plies until the defender is mated, CZ_MATE_NONE = not proven.  Parent g has the children offsets[g] .. offsets[g + 1]
 *     - 1 (0 .. 128 of them), child c the distance child_dist[c], the move child_label[c] that leads to it and, for W > 0, its
 *     own line child_pv[c][0 .. W) (0xFFFF behind its end).
 *       mode 0, the attacker to move (OR):  out_dist[g] = 1 + the minimum over the proven children; CZ_MATE_NONE when none is
 *               proven or there is no child;
 *       mode 1, the defender to move (AND): 0 without children (no king-safe move: mated, and stalemate loses too);
 *               CZ_MATE_NONE when any child is not proven; else 1 + the maximum.
 *     The best child is the FIRST in list order that attains the minimum / maximum.  out_pv[g][0 .. W]: its label, then its
 *     child_pv row; all 0xFFFF when out_dist[g] is 0 or CZ_MATE_NONE.  A child_dist outside 0 .. CZ_MATE_NONE - 1 counts as not
 *     proven.  Offsets outside [0, total] are clamped as in cz_successors: no access leaves the arrays whatever they hold.
 *     0 <= W <= CZ_MATE_MAX_LINE; total == 0 is served (every parent is childless), G == 0 is CZ_OK without a launch. */
#define CZ_MATE_NONE 0x7FFF
#define CZ_MATE_MAX_LINE 255
int cz_mate_backup(cz_ctx *, const int32_t *offsets /* [G + 1] */, int G, int total, const int16_t *child_dist /* [total] */,
                   const uint16_t *child_label /* [total] */, const uint16_t *child_pv /* [total][W], NULL when W == 0 */, int W,
                   int mode, int16_t *out_dist /* [G] */, uint16_t *out_pv /* [G][W + 1] */);
/* K2t TABLEBASES: the exact value of every position of a material class, by retrograde analysis.  No reference function.
 *   SIGNATURE  a C string such as "KR-KAA": red pieces, '-', black pieces.  Letters from KRNCPAB, in that order within a side,
 *     so K is first; each side has exactly one K, at most two each of R N C A B and at most five P.  Each letter is a SLOT,
 *     numbered left to right: in KR-KAA the slots are K, R, k, a, a.
 *   DOMAINS  the squares a slot may stand on, in ascending square order (sq = 9 y + x, red at home on ranks 0-2): K the 9 palace
 *     squares; A 3, 5, 13, 21, 23; B 2, 6, 18, 22, 26, 38, 42; P 55 squares — files a, c, e, g, i of ranks 3 and 4 and every
 *     square of ranks 5-9; R, N, C all 90.  A black piece's domain is the red one with y -> 9 - y, sorted ascending again.
 *   INDEX  index = 2 * mixed_radix(d0, d1, ...) + side: slot 0 is the most significant digit, d_i the place of slot i's square in
 *     its domain, side 0 for red to move; entries = 2 * the product of the domain sizes.  A signature with more than 2^31 - 1
 *     entries (or more than 10 slots, which has more) is refused.  Two equal pieces give two indices for one position; both
 *     hold the same value — the redundancy is accepted — and cz_tb_probe reads the one that puts the k-th of equal pieces in
 *     ascending square order on their k-th slot.  Mirror symmetry is not exploited.
 *   VALUE  int16, from the side to move's view, plies(v) = |v| - 1:
 *       0                 a draw: neither side can force mate;
 *       v > 0             the mover mates in v - 1 plies (an odd count, v is even);
 *       v < 0             the mover is mated in -v - 1 plies (an even count); -1: no king-safe move now — stalemate loses, as
 *                         in CZ_POS_NO_SAFE_MOVE;
 *       CZ_TB_ILLEGAL     the index has no position: two slots share a square, cz_movegen_kingsafe refuses the board, or the
 *                         mover can take the king (CZ_POS_CAN_TAKE_KING);
 *       CZ_TB_UNKNOWN     during a build only;
 *       CZ_TB_MISS        cz_tb_probe's answer for a board whose pieces are not the signature's.
 *     A win's ply count is the distance of the forced-mate search over all king-safe moves (cz_mate_backup's dist).
 *     Repetition, perpetual check and chase, and any move limit are NOT part of the table: a forced mate is a mate.
 *   THE BUILD  cz_tb_pass is one pass over every index of one table, in ONE launch, in place.
 *     pass 0: every index becomes CZ_TB_ILLEGAL, -1 (no king-safe move) or CZ_TB_UNKNOWN.
 *     pass d >= 1: every CZ_TB_UNKNOWN index walks its king-safe list; the child of a move is found arithmetically from the
 *       parent's digits (the slot on `from` gets the digit of `to`, the side flips; a move that takes the piece of slot j drops
 *       digit j and indexes sub[j], the table of the signature without that letter, which keeps the slot order) and its value u
 *       is read; u is settled below d when it is no CZ_TB_UNKNOWN and plies(u) < d.  Some child u < 0 settled below d:
 *       v = min plies(u) + 2, a win.  Otherwise every child u > 0 settled below d: v = -(max plies(u) + 2), a loss (a child
 *       that is a draw or unknown prevents it).  Otherwise the index stays CZ_TB_UNKNOWN.
 *     Values written in pass d have plies == d and a reader of the same launch treats them as not settled, so the result does
 *     not depend on which stores a reader sees: no synchronisation between workgroups.  *decided (device memory, the caller
 *     clears it) grows by the number of indices the pass decided.
 *     STOPPING is the caller's: with S the largest plies in any sub[j] (-1 if none is decided), the build ends after the first
 *     pass d >= 1 that decides nothing AND has d >= S + 1 — a capture into a sub-table entry lost in 12 plies settles its parent
 *     at pass 13, whatever passes 1-12 did in this table — and then CZ_TB_UNKNOWN becomes 0.  Sub-tables are finished tables.
 *   sub is a HOST array of n_slots DEVICE pointers, NULL for the kings' slots — the one host array in this ABI; it is read
 *     during the call only.  Pass 0 reads no sub-table and takes sub == NULL.
 *   cz_tb_probe: G boards [G][90] and sides -> value [G] and, when index is not NULL, index [G] (-1 without one).  A board
 *     whose multiset of pieces is not the signature's answers CZ_TB_MISS and nothing of the table is read; one with a piece
 *     outside its domain answers CZ_TB_ILLEGAL.  boards at any address: 16-byte aligned boards are staged with 16-byte loads,
 *     others byte by byte.
 *   cz_tb_boards: indices int32 [G] -> boards [G][90] (16-byte stores: boards must be 16-byte aligned, CZ_EINVAL otherwise) and
 *     side [G].  An index whose slots overlap gives an EMPTY board with the index's side; one outside 0 .. entries - 1 an empty
 *     board and side 0.
 *   All: CZ_EINVAL for a string that is no signature, a NULL context or array; G == 0 is CZ_OK without a launch.
 *   cz_tb_entries: host only — the number of entries and slots of a signature. */
#define CZ_TB_ILLEGAL (-32768)
#define CZ_TB_UNKNOWN 32767
#define CZ_TB_MISS 32766
#define CZ_TB_MAX_SLOTS 10
int cz_tb_entries(const char *signature, long long *entries, int *n_slots);
int cz_tb_pass(cz_ctx *, const char *signature, int16_t *table /* [entries] */, const int16_t *const *sub /* host [n_slots] */,
               int pass, unsigned long long *decided);
int cz_tb_probe(cz_ctx *, const char *signature, const int16_t *table /* [entries] */, const uint8_t *boards /* [G][90] */,
                const uint8_t *side, int G, int16_t *value /* [G] */, int32_t *index /* [G] or NULL */);
int cz_tb_boards(cz_ctx *, const char *signature, const int32_t *index /* [G] */, int G, uint8_t *boards /* [G][90] */,
                 uint8_t *side);
/* TABLE SETS: several finished tables behind one handle, probed by ONE launch whatever the positions' material — what a loop
 *   that must not wait for the host every ply needs (cz_selfplay_set_tablebase, cz_match_set_tablebase).
 *   THE MATERIAL KEY of a board: the sum over the piece codes c = 1 .. 14 of min(count of c, 7) << 3 c, and bit 45 when any byte
 *     is no piece code.  Two boards have one key iff they hold the same pieces; a signature's key is that of all its boards.
 *   cz_tb_set_create: n signatures and their tables (DEVICE pointers, the caller's, which must outlive the set) -> a directory in
 *     device memory: the keys sorted ascending, beside each its descriptor, its table and its place in the order given.
 *     1 <= n <= CZ_TB_SET_MAX: the kernel keeps the sorted keys in LDS (2 KB) and finds a board's entry by a binary search of
 *     eight steps there, and 256 is also the most a closure can hold — a signature has at most eight letters that are no king,
 *     each present or taken.  CZ_EINVAL: n outside that range, a string that is no signature (cz_tb_entries' text), a
 *     signature given twice, a table pointer that is NULL or odd.
 *   cz_tb_set_probe: G boards [G][90] and sides -> value [G], exactly what cz_tb_probe answers under the one signature of the
 *     set that has the board's pieces — the table's value, or CZ_TB_ILLEGAL for a piece outside its domain — and CZ_TB_MISS when
 *     no signature of the set has them; which [G] (may be NULL): the place of that signature in cz_tb_set_create's order, -1 for
 *     a miss.  A board of more than CZ_TB_MAX_SLOTS pieces is a miss before anything is looked up.  boards at any address, as
 *     for cz_tb_probe; G == 0 is CZ_OK without a launch.
 *   cz_tb_set_destroy: CZ_EINVAL while a self-play context or a match holds the set (detach it there first, or destroy the
 *     match); NULL is CZ_OK. */
#define CZ_TB_SET_MAX 256
typedef struct cz_tb_set cz_tb_set;
int cz_tb_set_create(cz_ctx *, int n, const char *const *signatures /* host [n] */, const int16_t *const *tables /* host [n] of device pointers */,
                     cz_tb_set **out);
int cz_tb_set_destroy(cz_tb_set *);
int cz_tb_set_probe(cz_ctx *, const cz_tb_set *, const uint8_t *boards /* [G][90] */, const uint8_t *side, int G, int16_t *value /* [G] */,
                    int32_t *which /* [G] or NULL */);
/* BOOK: an opening book from recorded games.  No reference function: the reference has no book.  A book is a table of entries
 *   (key, label) -> games, wins, draws in the CALLER'S device arrays bkey u64 [E], blabel u16 [E], bgames u32 [E] (wins and draws
 *   never reach a kernel), ascending by key as unsigned 64-bit, then by label, one entry per pair.  There is no handle.
 *   THE CANONICAL KEY of a position: k = cz_hash(board, side), k' = cz_hash of the board with its files reversed (cell (r, f)
 *     from (r, 8 - f)), same side; key = min(k, k') as unsigned.  The position is MIRRORED when k' < k and SELF-MIRROR when
 *     k' == k (the opening position is).  `mirrored` bytes: 0 as it is, 1 mirrored, 2 self-mirror.  A byte above 14 hashes as
 *     an empty square, as in cz_hash.
 *   THE CANONICAL LABEL of a move played there: cz_mirror_table[label] in a mirrored position, min(label, mirror[label]) in a
 *     self-mirror one (h2e2 and b2e2 from the opening position are one entry), the label itself otherwise.
 *   cz_book_keys: G boards [G][90] and sides -> key [G] and, unless NULL, mirrored [G].  boards at any address, as cz_tb_probe.
 *   cz_book_entries: n packed CZ_REC_* records (16-byte aligned) -> per record its canonical key, the canonical label of the
 *     move played — the label at the FIRST maximum of the first `count` visits (count above 128 is taken as 128) — and
 *     outcome 0 / 1 / 2: the mover won (z > 0) / drew (z == 0) / lost.  A record with ply >= max_ply (max_ply > 0; 0: no bound)
 *     or count == 0 is SKIPPED: outcome 255, label 0xFFFF; its key is written all the same.
 *   cz_book_probe: per position the canonical key and an unsigned binary search of bkey: first [G] the first entry of that key
 *     and count [G] how many follow it (the position's entries are first .. first + count - 1), or first -1 / count 0.
 *     E == 0 is a legal, empty book (bkey may be NULL).
 *   cz_book_choose: probe and pick in one launch.  An entry is ELIGIBLE when games >= max(min_games, 1) and its label, translated
 *     to the position's OWN orientation (mirror[label] for a mirrored position, the label itself otherwise), is set in
 *     allowed [G][66] (bit l & 31 of word l >> 5, as cz_movegen's mask; NULL: every label).  mode 0: the eligible entry with the
 *     most games, the first of equals in entry order.  mode 1: in proportion to games, in integers: T the sum over the eligible
 *     entries (the caller keeps the sum of games over one position below 2^32), t = ((uint64) rnd[g] * T) >> 32, the first
 *     eligible entry whose running sum exceeds t.  played [G]: the move in the position's own orientation, 0xFFFF when nothing
 *     is eligible; index [G] (may be NULL): the chosen entry, or -1.  A stored label >= 2086 is never eligible.
 *   All: G == 0 / n == 0 is CZ_OK without a launch.  CZ_EINVAL: a NULL context or required array, negative G / n / E / max_ply
 *     / min_games, mode outside 0 .. 1, mode 1 without rnd, a u64 array not 8-byte, a u32 / i32 array not 4-byte, a u16 array
 *     not 2-byte aligned, records not 16-byte aligned. */
int cz_book_keys(cz_ctx *, const uint8_t *boards /* [G][90] */, const uint8_t *side, int G, uint64_t *key /* [G] */,
                 uint8_t *mirrored /* [G] or NULL */);
int cz_book_entries(cz_ctx *, const uint8_t *records /* [n][CZ_REC_BYTES] */, int n, int max_ply, uint64_t *key /* [n] */,
                    uint16_t *label /* [n] */, uint8_t *outcome /* [n] */);
int cz_book_probe(cz_ctx *, int E, const uint64_t *bkey /* [E] */, const uint8_t *boards /* [G][90] */, const uint8_t *side, int G,
                  int32_t *first /* [G] */, int32_t *count /* [G] */, uint8_t *mirrored /* [G] */);
int cz_book_choose(cz_ctx *, int E, const uint64_t *bkey /* [E] */, const uint16_t *blabel /* [E] */, const uint32_t *bgames /* [E] */,
                   const uint8_t *boards /* [G][90] */, const uint8_t *side, const uint32_t *allowed /* [G][66] or NULL */, int G,
                   int min_games, int mode, const uint32_t *rnd /* [G], mode 1 */, uint16_t *played /* [G] */,
                   int32_t *index /* [G] or NULL */);
/* K3  replaces MCTS_tree.generate_inputs = try_flip + state_to_positions, main.py:531-574.
 *     planes [G][9][10][channels] of dtype CZ_F32 / CZ_BF16.  quirk_q1 = 1 reproduces the
 *     reference bit for bit; 0 gives the transposed encoding its shapes suggest. */
int cz_encode_planes(cz_ctx *, const uint8_t *boards, const uint8_t *side, int G, void *planes,
                     int dtype, int channels, int quirk_q1);
/* Record expansion  replaces the host side of cchess_main.run's data_buffer.extend (main.py:1234-1240) for packed records: n
 *     CZ_REC_* records on the device -> the training tuples, planes [n][9][10][14] f32 (generate_inputs of the record's board
 *     for its mover, quirk Q1), pi [n][2086] f32 (softmax(1 / temperature * log(visits)) in float64 — get_action's expression,
 *     main.py:1341; no visit at all: 1 / count each — rounded to float32 and scattered over the children's labels in canonical
 *     orientation, main.py:1507-1512; 0 elsewhere; count 0: a zero row), z [n] f32.  mirror [n] (device; NULL = none): a record
 *     with mirror[i] != 0 is expanded as its LEFT-RIGHT MIRROR IMAGE — the board read with its files reversed (cell (rank, f)
 *     from (rank, 8 - f)) and every label mapped through cz_mirror_table — an equally valid sample of the same game.  The
 *     mirror acts before try_flip / unflip and the encoding; it is not a flip of the plane tensor (the planes are read with a
 *     9-stride).  The children of a mirrored record stay in the order they were generated for the unmirrored board.
 *     Every element of planes, pi and z is written exactly once.  Records from anywhere are safe: a count above 128 is taken
 *     as 128, a label >= 2086 has no cell in pi (its visits still count in the softmax), nothing outside the n records and the
 *     three output arrays is touched.  n == 0: CZ_OK, no launch.  CZ_EINVAL: n < 0, temperature <= 0, a NULL output, records
 *     or planes or z not 4-byte aligned, pi not 8-byte aligned. */
int cz_records_expand(cz_ctx *, const uint8_t *records /* [n][CZ_REC_BYTES], device */, int n,
                      const uint8_t *mirror /* [n] 0/1, or NULL = none */, double temperature,
                      float *planes /* [n][9][10][14] */, float *pi /* [n][2086] */, float *z /* [n] */);
/* Game replay: G RECORDED GAMES (move lists) -> CZ_REC_* records, one launch.  No reference function: the reference learns
 *     from its own self-play only (cchess_main.selfplay, main.py:1493-1554) and never reads a game back.
 *     Game g starts from start_boards[g] / start_side[g] (NULL: the opening position, main.py:585 / red to move) and is given
 *     len[g] moves, moves[g * stride + i] the label of ply i.  At ply i the LEGAL LIST of the position is, for rules = 0, the
 *     pseudo-legal list of cz_movegen, in the reference's order; for rules = 1, the king-safe list of cz_movegen_kingsafe, in
 *     the same order.  If the move is in that list, record rec_offset[g] + i is written and the move is made exactly as
 *     cz_apply_move makes it.  The record is one that cz_records_expand takes as it is: the board BEFORE the move, the side
 *     to move, count and labels = the legal list, visits = 1 at the played child and 0 elsewhere (pi is one-hot at any
 *     temperature), z = result[g] for a red-to-move record and -result[g] for a black one (the mover's view, as self-play
 *     writes it), ply = i, flags = 0, unused label slots 0xFFFF and unused visits 0.
 *     The replay of a game STOPS at the first ply whose move cannot be made.  valid[g]: the plies made.  status[g], the
 *     tests in this order:
 *       CZ_GAME_BAD_LEN    len[g] is outside 0 .. stride: nothing is read, valid[g] = 0, no record is written;
 *       CZ_GAME_BAD_BOARD  the stand-alone generators refuse the position of that ply (count 0xFFFF);
 *       CZ_GAME_AFTER_END  a move was given in a position with a king missing or, under rules = 1, without a king-safe move;
 *       CZ_GAME_ILLEGAL    the label is not in the list (a label >= 2086, 0xFFFF included, never is);
 *       CZ_GAME_OK         all len[g] plies were made.
 *     The records of the plies given but not made, valid[g] .. len[g] - 1, are written as CZ_REC_BYTES zero bytes, so that a
 *     caller can compact by a mask: every byte of records rec_offset[g] .. rec_offset[g] + len[g] - 1 is written exactly once
 *     and nothing else of `records` is touched.  The caller keeps the games' ranges disjoint; a record index outside
 *     [0, total) is not written: no access leaves the arrays whatever they hold.
 *     end_flags[g]: the position after valid[g] plies — its CZ_POS_* bits as cz_movegen_kingsafe reports them (at both rule
 *     levels; 0 for a board it refuses), CZ_GAME_RED_KING_GONE, CZ_GAME_BLACK_KING_GONE.  final_boards [G][90] / final_side
 *     [G] (may be NULL): that position.  records may be NULL (legality, counts and the final positions alone).
 *     One lane per game, the board in registers from ply to ply; a wave of 64 games runs as long as its longest game: sort
 *     the games by length and let rec_offset put the records in the order wanted.
 *     G == 0: CZ_OK, no launch.  CZ_EINVAL: a NULL moves, len, result, rec_offset, valid, status or end_flags; stride < 0 or
 *     > 65535 (ply is 16 bits); total < 0; rules outside 0 .. 1; records not 16-byte aligned; final_boards without
 *     final_side.  Everything else at any address its element type allows. */
#define CZ_GAME_OK 0
#define CZ_GAME_ILLEGAL 1
#define CZ_GAME_AFTER_END 2
#define CZ_GAME_BAD_BOARD 3
#define CZ_GAME_BAD_LEN 4
#define CZ_GAME_RED_KING_GONE 16    /* end_flags: no 'K' on the board */
#define CZ_GAME_BLACK_KING_GONE 32  /* end_flags: no 'k' on the board */
int cz_games_replay(cz_ctx *, const uint8_t *start_boards /* [G][90] or NULL: the opening position */,
                    const uint8_t *start_side /* [G] or NULL: red */, const uint16_t *moves /* [G][stride] labels */, int stride,
                    const int32_t *len /* [G], 0..stride */, const int8_t *result /* [G]: +1 red won, -1 black won, 0 draw */, int G,
                    int rules /* 0 capture, 1 king-safe */, const int32_t *rec_offset /* [G] */, int total,
                    uint8_t *records /* [total][CZ_REC_BYTES] or NULL */, int32_t *valid /* [G] */, uint8_t *status /* [G] */,
                    uint8_t *end_flags /* [G] */, uint8_t *final_boards /* [G][90] or NULL */, uint8_t *final_side /* [G] or NULL */);
/* Game replay from TOKENS: cz_games_replay for games written in WXF / Chinese notation.  Such a move ("C2=5", 炮二平五) has
 *     no coordinates; it is read against the position it is played in, inside the replay.  Everything not said here is as in
 *     cz_games_replay: records, the order of the tests, zero records for plies given but not made, end_flags, G == 0.
 *     tokens[g * stride + i] is one uint32.  Below 65536 it is a move label and is used as cz_games_replay uses it (label and
 *     notation games go through one launch).  Otherwise it is four bytes, least significant first, b0 b1 b2 b3:
 *       b0  a kind out of K A E H R C P, or a file digit 1-9: the mover's pawn on that file (b1 is then an ordinal);
 *       b1  the source: a file digit 1-9, or an ordinal on the file: + frontmost, - rearmost, a-e the 1st .. 5th from the front;
 *       b2  + forward, - backward, = sideways;      b3  a digit 1-9.
 *     With x = 0..8 the files a..i and y = 0 red's back rank, the file number of x is 9 - x for red and x + 1 for black, and
 *     forward is +y for red, -y for black.  A move from -> to of the ply's legal list MATCHES the token when
 *       the mover's piece on `from` is of the token's kind (b0 a digit: a pawn, and the file of `from` is that digit);
 *       source, a digit: `from` is on that file, however many of the kind stand there; an ordinal: at least two of the
 *         mover's pieces of that kind stand on `from`'s file and `from` is the one the ordinal names;
 *       move: R C P K with + / -: same file, that direction, |dy| == b3; any kind with =: dy == 0 and the file of `to` is b3;
 *         H E A with + / -: dy in that direction and the file of `to` is b3; H E A never match =.
 *     Exactly one match: that move is made.  None: CZ_GAME_ILLEGAL.  Two or more: CZ_GAME_AMBIGUOUS, tested where ILLEGAL
 *     is; the game stops there as for any other status.  Any 32-bit value is safe: bytes outside the alphabet (and b0 a digit
 *     with b1 a digit) match nothing, and no token value indexes anything.
 *     labels_out [G][stride] (may be NULL): the label each made ply decoded to, 0xFFFF everywhere else; every element is
 *     written exactly once.
 *     CZ_EINVAL as cz_games_replay's (tokens for moves), and tokens not 4-byte or labels_out not 2-byte aligned. */
#define CZ_GAME_AMBIGUOUS 5
int cz_games_read(cz_ctx *, const uint8_t *start_boards, const uint8_t *start_side, const uint32_t *tokens /* [G][stride] */, int stride,
                  const int32_t *len, const int8_t *result, int G, int rules, const int32_t *rec_offset, int total, uint8_t *records,
                  int32_t *valid, uint8_t *status, uint8_t *end_flags, uint8_t *final_boards, uint8_t *final_side,
                  uint16_t *labels_out /* [G][stride] or NULL */);

/* ---- lock-step search over G trees, one wavefront per tree ---------------------------------
 * replaces: MCTS_tree.__init__/reload (main.py:235-259): fresh, unexpanded roots. */
int cz_search_reset(cz_ctx *, const uint8_t *root_boards, const uint8_t *root_side,
                    const int32_t *restrict_round /* may be NULL = 0 */, int G);
/* replaces: MCTS_tree.reload / GameBoard.reload when a game is over (main.py:255-258,604-608,1494,1552): the trees g with
 *   which[g] != 0 start afresh (unexpanded root, no simulations) from root_boards[g] / root_side[g] / restrict_round[g]
 *   ([G] arrays like cz_search_reset's; restrict_round may be NULL = 0); every other tree is left untouched. */
int cz_search_reload(cz_ctx *, const uint8_t *which, const uint8_t *root_boards, const uint8_t *root_side,
                     const int32_t *restrict_round);
/* K4 (+K1,K2,K3 on the leaf)  replaces one start_tree_search descent, main.py:350-418
 *   (select_new :158, get_Q_plus_U_new :108-116, kill-move/restrict_round :393-396, terminal
 *   tests :409-416, generate_inputs :362, get_legal_moves :374) with search_threads = 1.
 *   mode 0: root expansion only (MCTS_tree.main, main.py:475-487); mode 1: one simulation.
 *   active [G] (may be NULL): trees with 0 idle this step.
 *   leaf_planes [G][9][10][channels]; needs_eval [G] = 1 where the net must be evaluated. */
int cz_search_select(cz_ctx *, int mode, const uint8_t *active, void *leaf_planes, int dtype,
                     int channels, uint8_t *needs_eval);
/* K5+K6  replaces leaf_node.expand (main.py:175-187) with flip_policy (:1153-1155) and
 *   back_up_value (:189-194) along the unwind (:426-435), including the float32 effect of the
 *   virtual-loss add/remove (:403-404,426-427).  logits [G][2086], value [G] of `dtype`. */
int cz_search_expand_backup(cz_ctx *, const void *logits, const void *value, int dtype);

/* cz_search_expand_backup with the policy FC (policy_value_network.py:62-63) folded in: instead of a full logits row
 * per tree it takes the head-conv outputs z [G][90][3] f32 (cz_net_trunk_*), the FC weight pfc_w [2086][180] f32
 * (row = label, torch / "out,in" layout; the reference stores [in,out]) and bias pfc_b [2086], and evaluates the FC
 * only for the <= 128 labels each expansion reads (leaf_node.expand gathers action_probs[label2i[action]], main.py:
 * 179-181).  The float32 evaluation order of the 180-term dot product is fixed and documented at k_expand_backup
 * (cz_search.hip) so that a CPU restatement reproduces the priors bit for bit (tests/test_hip_search.py).
 * value [G] f32.  Pairs with cz_search_select (one simulation per tree). */
int cz_search_expand_backup_fc(cz_ctx *, const float *z, const float *value, const float *pfc_w, const float *pfc_b,
                               int compact /* 1: z / value rows are the ones cz_search_select_compact handed out */);

/* Compact evaluation batches.  Terminal and drawn leaves (main.py:409-416) and parked trees need no net evaluation — the
 * reference never calls forward() for them — so cz_search_select_compact writes the leaf planes of the trees that DO
 * need one to consecutive rows 0 .. n-1 of leaf_planes (rows are handed out by an atomic counter; which tree gets
 * which row is irrelevant because every row of the net is computed independently).  *slot_of -> device int32 [G]: the
 * row of tree g's leaf or -1; *n_rows -> device int32: n for this step (valid until the step after the next).  Pass
 * n_rows to cz_set_batch_count so that the following cz_net_trunk_bf16 / cz_net_trunk_f16 / cz_fc_heads_f32 launches
 * stop after n rows (whole workgroups beyond them return at once; no host synchronisation), then call
 * cz_search_expand_backup_fc(..., compact = 1).  cz_search_eval_totals returns the running totals of rows evaluated
 * and of compact steps (synchronises the stream): the flop accounting of a benchmark. */
int cz_search_select_compact(cz_ctx *, int mode, const uint8_t *active, void *leaf_planes, int dtype, int channels,
                             const int32_t **slot_of, const int32_t **n_rows);
int cz_set_batch_count(cz_ctx *, const int32_t *n_rows_dev /* or NULL: every row of B */);
int cz_search_eval_totals(cz_ctx *, unsigned long long *rows, unsigned long long *steps);
/* k simulations in flight per tree and step, with the reference's virtual loss (N += 3, W -= 3 while in flight):
 * replaces the `search_threads` coroutines of MCTS_tree (asyncio.Semaphore(search_threads), main.py:250,337-348,
 * virtual loss :231,403-404,426-427, now_expanding :354-360).  cz_search_set_width sizes the pending-leaf arrays
 * (1 <= width <= 64, default 1; call before the search loop).  leaf_planes / needs_eval / logits / value then have
 * G*k rows, slot g*k + j = j-th descent of tree g; slots a tree does not use have needs_eval = 0.  k = 1 is
 * arithmetically identical to cz_search_select / cz_search_expand_backup. */
int cz_search_set_width(cz_ctx *, int width);
/* cz_search_set_sim_target: with k > 1 a tree stops issuing descents once `target` simulations (counted since the last
 * cz_search_reset / cz_search_advance, cz_search_status `sims`) are completed or in flight, so that a search of
 * ceil(playouts / k) + a few steps ends with EXACTLY `playouts` simulations per tree like MCTS_tree.main (main.py:489-493:
 * `playouts` coroutines, at most search_threads of them in flight).  0 = no limit (default). */
int cz_search_set_sim_target(cz_ctx *, int target);
/* cz_search_set_terminal_extra: a simulation that ends on a king capture or on the 60-ply rule needs no net evaluation
 * (main.py:409-416 returns before push_queue).  With n > 0, cz_search_select[_compact] completes up to n such simulations
 * per tree inside the launch (value backed up along the path, simulation counted) and goes on to the next descent, so that
 * every tree presents a leaf that DOES need the net: a lock-step then completes 1 / (1 - f) simulations per net row.
 * Simulations of one tree stay strictly sequential: the tree after N simulations is bit-identical to the n = 0 schedule.
 * Use cz_search_set_sim_target (also honoured by cz_search_select) to stop every tree at exactly N.  Default 0. */
int cz_search_set_terminal_extra(cz_ctx *, int n);
/* Evaluation cache (off by default; width 1 only).  The net is a pure function of (board, side to move) and this library
 *   computes every row of a batch independently of the others, so a position a tree has evaluated before would get the
 *   same priors and value again, bit for bit (the reference re-evaluates it: transpositions are separate nodes,
 *   main.py:357-384).  With the cache on, every expanded node is remembered under the 64-bit Zobrist key of its position
 *   (cz_zobrist; per tree 128 buckets x 64 entries of {key, node, value, the position itself packed into 48 bytes} =
 *   512 KB); a leaf whose key is found AND whose position equals the stored one is expanded inside the select launch from
 *   the remembered node's children (labels, priors) and backed up with the remembered value — no net row.  The key only
 *   finds the candidate, the position decides: a key collision is a miss (counted), never a wrong node.  Up to 4 hits
 *   complete per tree and launch, a budget of their own beside cz_search_set_terminal_extra (the cache works with
 *   terminal_extra = 0).  Trees are identical with the cache on or off; entries follow their nodes through
 *   cz_search_advance and are dropped with them.  Turning it on empties it.
 *   cz_search_eval_cache_stats: hits / lookups summed over the trees since the cache was turned on (synchronises);
 *   cz_search_eval_cache_collisions: key matches refused because the stored position differed;
 *   cz_search_debug_eval_cache_key_bits (tests): keys narrowed to 8..24 bits so that collisions DO occur (64 = full). */
int cz_search_set_eval_cache(cz_ctx *, int on);
int cz_search_eval_cache_stats(cz_ctx *, unsigned long long *hits, unsigned long long *lookups);
int cz_search_eval_cache_collisions(cz_ctx *, unsigned long long *collisions);
int cz_search_debug_eval_cache_key_bits(cz_ctx *, int bits);
/* Cross-tree level of the evaluation cache (needs cz_search_set_eval_cache(ctx, 1)): one table of 2^log2_entries self-contained,
 * entries (key, packed position, value, the <= 128 labels and priors: 1088 bytes each) shared by all trees of the
 * context — in self-play from the start position the games share their openings, and the reference evaluates the same position
 * once per game (main.py:357-384).  A leaf whose position ANY tree has evaluated is expanded inside the select launch from the
 * remembered row, verified against the stored position; trees stay bit-identical (the net's row for a position does not depend
 * on the tree it is asked for).  log2_entries 0 frees the table; calling it again (or cz_search_set_eval_cache(ctx, 1)) empties
 * it — do so whenever the weights change.  Round 6: a FULL bucket is no longer closed — the entry whose position lies deepest in
 * its game (re-roots of the filing tree + depth of the leaf) is replaced when the new position is shallower, so the table converges
 * to the openings every restarted game walks through again.  A filing claims its slot by swapping in its key with the top bit
 * set (the bit no position's key has: keys are cz_hash without it), writes the entry through to memory and only then stores
 * the real key: two trees of one launch never write one entry at once, no entry mixes two positions, and a tree filing a
 * position another tree is still writing leaves it to that one.  Emptying the
 * table clears keys, values and counts.  stats4: hits, lookups, entries written, filings that found no room
 * (a full bucket of shallower positions, or every swap lost to another tree of the launch); stats5 adds: entries that replaced
 * a deeper one (included in `written`). */
int cz_search_set_xcache(cz_ctx *, int log2_entries);
int cz_search_xcache_stats(cz_ctx *, unsigned long long *stats4);
int cz_search_xcache_stats5(cz_ctx *, unsigned long long *stats5);
/* tests: cz_search_advance runs one compaction with the kept-node bitmap of a tree in LDS when it fits (12 bytes per 64 nodes)
 * and in global memory otherwise; on != 0 forces the global-memory home so that it is exercised at test sizes. */
int cz_search_debug_advance_in_global_memory(cz_ctx *, int on);
/* tests: read the caches back (synchronise the stream).
 *   cz_search_debug_xcache_dump: the whole cross-tree block, n * 1088 + 64 bytes for n entries, in the table's own layout:
 *     key u64 [n] | 64 bytes | value f32 [n] | count | ply << 16 u32 [n] | packed position u32 [n][12] | labels u16 [n][128] |
 *     (src | dst << 8) u16 [n][128] | priors f32 [n][128].  Key 0 = empty.  host NULL: only returns n.  Returns n, or an error
 *     when the table is off or `bytes` is short.
 *   cz_search_debug_eval_cache_dump: tree g's per-tree entries (8192 = 128 buckets x 64): key, node, value, packed position
 *     [8192][12]; record[i] = the node's index in cz_search_tree_dump's pre-order records, -1 for the root, -2 when the node
 *     is not in the tree (or the entry is empty).  Any array may be NULL.  Returns 8192. */
int cz_search_debug_xcache_dump(cz_ctx *, void *host, size_t bytes);
int cz_search_debug_eval_cache_dump(cz_ctx *, int g, unsigned long long *key, int32_t *node, float *value, uint32_t *board,
                                    int32_t *record);
int cz_search_select_k(cz_ctx *, int mode, int k, const uint8_t *active, void *leaf_planes, int dtype,
                       int channels, uint8_t *needs_eval);
int cz_search_expand_backup_k(cz_ctx *, int k, const void *logits, const void *value, int dtype);
/* replaces: reading root.child.items() in get_action, main.py:1339 (+ MCTS_tree.Q :261).
 *   arrays [G][128] (any may be NULL), count [G]. */
int cz_search_root_stats(cz_ctx *, uint16_t *move_label, int32_t *N, float *Q, float *P, float *W,
                         uint16_t *count);
/* Principal variations: for every tree, n_lines lines of at most max_len moves read from the tree as it stands (read-only; call
 *   it between complete lock-steps, as cz_search_root_stats: with width > 1 a pending descent still carries its virtual loss).
 *   root_allowed [G][CZ_MASK_WORDS] (a move set as cz_movegen_kingsafe writes it) or NULL; moves / visits / q [G][n_lines][max_len]
 *   (any may be NULL), len [G][n_lines]; all device memory.  1 <= n_lines <= 128, 1 <= max_len <= 64, CZ_EINVAL otherwise.
 *   Candidates of tree g: the root's children, in generation order, whose label has its bit set in root_allowed[g] (NULL: all of
 *   them) - the list cz_match_choose / cz_selfplay_choose choose from under rules 1.  Line j starts at the candidate of rank j
 *   under "more visits first, earlier in generation order first among equals": line 0's first move is the greedy move of
 *   cz_search_pick_ready / cz_match_choose.  A candidate without a visit still gives a line of length 1; j >= the number of
 *   candidates gives len 0, as does every line of an unexpanded root or a root without children.  From the node just appended,
 *   while it is expanded and the line is shorter than max_len, the line takes the first maximum of N over its children and stops,
 *   without appending it, when that child has no visit.  Entry i < len: moves = the child's label (board coordinates at every
 *   depth), visits = its N, q = its Q as the pool holds it, bit for bit, in the sign the search maximises for the mover at that
 *   node's parent.  Entries i >= len: 0xFFFF, 0, 0.0f - every element of every output array is written. */
int cz_search_lines(cz_ctx *, const uint32_t *root_allowed, int n_lines, int max_len, uint16_t *moves, int32_t *visits, float *q,
                    uint16_t *len);
/* K7  replaces MCTS_tree.update_tree (main.py:272-276) + the board bookkeeping of selfplay
 *   (:1522-1528): re-root on the played child keeping its subtree (compacted in place: one node
 *   pool per tree); clears CZ_ST_POOL_EXHAUSTED.  played_label 0xFFFF leaves the tree untouched. */
int cz_search_advance(cz_ctx *, const uint16_t *played_label);
/* greedy re-rooting driver (device arrays, no host round trip; bench.py's search loop, "play the strongest move" loops)
 * replaces: get_action in its temperature -> 0 limit (main.py:1332-1341, default temperature 1e-3: softmax(log(visits)/T)
 *   puts all mass on the most visited child; first maximum in generation order like Python's max()) for the trees whose
 *   search is complete.  A tree is READY when it has completed sim_threshold[g] simulations since its last reset /
 *   advance or its node pool is full: played[g] = label of its most visited root child (0xFFFF: not ready, or no child),
 *   ready[g] = 1 / 0 (may be NULL), sim_threshold[g] = next_threshold, *banked_sims += its simulation count (device
 *   scalar, may be NULL).  Follow with cz_search_advance(played) and cz_search_reload_finished. */
int cz_search_pick_ready(cz_ctx *, int32_t *sim_threshold /*[G] in/out*/, int next_threshold, uint16_t *played /*[G]*/,
                         uint8_t *ready /*[G]*/, unsigned long long *banked_sims);
/* replaces: check_end + reload after the move (main.py:1380-1392 king gone / restrict_round >= 60; :255-258,604-608):
 *   the READY trees whose game is now over — or that had no move to play — start afresh from root_boards[g] /
 *   root_side[g] / restrict_round[g] (may be NULL = 0) like cz_search_reload; *reloaded (device scalar, may be NULL)
 *   counts them. */
int cz_search_reload_finished(cz_ctx *, const uint8_t *ready, const uint16_t *played, const uint8_t *root_boards,
                              const uint8_t *root_side, const int32_t *restrict_round, unsigned long long *reloaded);
int cz_search_status(cz_ctx *, int32_t *status, int32_t *nodes_used, int32_t *sims,
                     int32_t *last_depth); /* device [G] arrays, any may be NULL */
int cz_search_root_state(cz_ctx *, uint8_t *boards, uint8_t *side, int32_t *restrict_round);
/* parity/debug: pre-order dump of tree g into HOST memory; record = 7 int32
 *   {depth, label, N, bits(W), bits(Q), bits(P), child_count or -1}.  Returns the record count
 *   (>= 0; at most max_records are written) or a negative error. */
int cz_search_tree_dump(cz_ctx *, int g, int32_t *host_out, int max_records);

/* ---- device-resident self-play bookkeeping (one wave per game; no host round trip per ply) ------------------------
 * replaces: cchess_main.get_action (main.py:1332-1358) and the per-ply / end-of-game bookkeeping of cchess_main.selfplay
 * (:1493-1554) for the G games of the ctx at once.  One ply of every game =
 *     cz_search_select/expand_backup... (the playouts; pass cz_selfplay_active as the select `active` mask)
 *     cz_selfplay_choose      pi from the root visits, the sampled move, the (s, pi) record of the ply
 *     cz_search_advance       update_tree + board bookkeeping with the chosen moves
 *     cz_selfplay_adjudicate  game end tests on the new positions, z for the finished games' records, re-seed
 *     cz_selfplay_flush       finished games' records -> the caller's record ring
 * cz_selfplay_begin (after cz_search_reset): allocates the per-slot histories [G][max_plies] records and makes the
 *   given positions (NULL: the trees' current roots) the ones every new game of a slot starts from; zeroes the statistics.
 *   A game that reaches max_plies plies is adjudicated a draw (the reference has no such limit; its games end by the
 *   60-ply no-capture rule).
 * cz_selfplay_choose: gamma [G][128] f32 Gamma(0.3, 1) variates (normalised per game = Dirichlet(0.3), main.py:1346) or
 *   NULL, u [G] f32 uniforms in [0, 1), forced [G] labels overriding the sampled move (0xFFFF = none; NULL) for replaying
 *   recorded games; temperature as in get_action; noise_eps = 0.25 when exploring, 0 otherwise.  min_sims = 0: every
 *   active game moves (lock-step plies); min_sims > 0: only the games whose current search has completed that many
 *   simulations (or whose tree cannot go on) move — asynchronous plies, every game at its own pace.  played [G] out
 *   (0xFFFF for parked games, for games that do not move now and for games whose root has no child).
 * cz_selfplay_adjudicate: reseed != 0: a finished slot starts a new game at once; 0: it is parked (cz_selfplay_active
 *   turns 0).  played: the array cz_selfplay_choose filled (slots that did not move are skipped) or NULL (all slots).
 *   fin_n [G] out: records the finished game contributes (0 otherwise).
 * cz_selfplay_flush: offset [G] int64 = first ring index (before the modulo) of each finished game, i.e. an exclusive
 *   prefix sum of fin_n on top of the running cursor, computed by the caller; ring [ring_records][CZ_REC_BYTES];
 *   read_cursor: device int64 the caller advances after draining (records that would overwrite undrained ones are
 *   dropped and counted), or NULL.
 * cz_selfplay_stats: device int64 [CZ_SP_NSTATS] <- running totals. */
int cz_selfplay_begin(cz_ctx *, int max_plies, const uint8_t *start_boards, const uint8_t *start_side,
                      const int32_t *start_rr);
int cz_selfplay_active(cz_ctx *, const uint8_t **active_dev /* [G] */);
int cz_selfplay_choose(cz_ctx *, const float *gamma, const float *u, const uint16_t *forced, double temperature,
                       float noise_eps, int min_sims, uint16_t *played);
int cz_selfplay_adjudicate(cz_ctx *, int reseed, const uint16_t *played, int32_t *fin_n);
int cz_selfplay_flush(cz_ctx *, const int32_t *fin_n, const long long *offset, uint8_t *ring, long long ring_records,
                      const long long *read_cursor);
int cz_selfplay_stats(cz_ctx *, long long *stats_dev);
/* cz_selfplay_set_rules: 0 = king capture (the default: the reference's games, everything above, launch for launch), 1 = xiangqi,
 *   as cz_match_set_rules.  The rules act AT THE ROOT ONLY: the search below it is untouched, so the trees stay the reference's
 *   (in the tree a mate is a king capture two plies down, which the search already sees).  With 1, cz_selfplay_choose first
 *   computes the king-safe set (cz_movegen_kingsafe) of every active slot's root position and then does everything above ON
 *   THE ROOT CHILDREN WHOSE MOVE IS IN THAT SET, compacted in generation order: pi = softmax(log N / T) over them alone, the noise
 *   of compacted child j is gamma[g][j] (a Dirichlet over len(probs) entries), the same inverse CDF with u[g], and the record holds
 *   only them (labels / visits in generation order, count = their number, padding 0xFFFF / 0): pi has no mass on a move that
 *   leaves the king en prise (when every simulation went to children outside the set, the record's visits are all 0: the move
 *   is picked uniformly among them, as for a root without a visit).  A forced label is played as given.  A root with children, none of them king-safe: played = 0xFFFF,
 *   no record, and cz_selfplay_adjudicate ends the game as a loss for the side to move (checkmate or stalemate), z = +1 / -1 as for
 *   a king capture, fin_n = min(plies played, max_plies).  A root without children stalls as above.
 *   Both setters: after cz_selfplay_begin — which returns the context to rules 0, fold 0 and zeroes the counters below and the
 *   rings — and before the first cz_selfplay_choose that follows it; CZ_EINVAL otherwise.
 * cz_selfplay_set_repetition: fold 0 = no repetition rule (the default), 2 <= fold <= 8 = a game ends when its position occurs
 *   for the fold-th time (cz_repetition's rule, as cz_match_set_repetition; 3 is the usual value).  Needs cz_selfplay_set_rules(ctx,
 *   1) first — the check flags are the king-safe pass's; cz_selfplay_set_rules(ctx, 0) is refused while the fold is not 0.  With
 *   it, cz_selfplay_choose also takes every root position's CZ_POS_* flags and cz_hash, writes them into the slot's ring of 64
 *   positions at entry ply & 63 (after the parked / min_sims / stalled tests, every index masked) and evaluates the rule with
 *   w = min(restrict_round of the root, ply, 63): w <= ply keeps every read inside the slot's current game, so a re-seeded slot
 *   never reads its previous game's ring.  Order: stalled, then repetition, then mate.  On a verdict played = 0xFFFF, no record is
 *   written, the ply stays, and cz_selfplay_adjudicate — before the mate and before every test above, also for a slot its `played`
 *   argument would skip — ends the game: CZ_REP_DRAW a draw (z = 0, CZ_SP_DRAWS), CZ_REP_RED_LOSES / CZ_REP_BLACK_LOSES a loss for
 *   that side (z as for a king capture, CZ_SP_BLACK_WINS / CZ_SP_RED_WINS); fin_n = min(plies played, max_plies).
 * cz_selfplay_history: the device pointers of the two rings, owned by the context — keys uint64 [G][64], checks uint8 [G][64]:
 *   position i of the game in slot g at [g][i & 63]; either may be NULL.  CZ_EINVAL while the repetition rule is off.
 * cz_selfplay_rules_stats: device int64 [3] <- games ended by mate, by a repetition draw, by perpetual check since
 *   cz_selfplay_begin.  They are counted in the cz_selfplay_stats slots too (wins / draws, games, plies).
 * cz_selfplay_set_chase: 0 = perpetual chase is not judged (the default: everything above, launch for launch and byte for
 *   byte), 1 = it is, as cz_match_set_chase.  Needs a non-zero fold (CZ_EINVAL otherwise; cz_selfplay_set_repetition(ctx, 0) is
 *   refused while it is on) and is set like the other two, between cz_selfplay_begin — which switches it off — and the first
 *   cz_selfplay_choose.  With it, cz_selfplay_choose also takes every root position's chase record (one cz_threats launch on
 *   the boards it already copies out), writes it into a third ring, chase uint64 [G][64][4], at entry ply & 63, and evaluates
 *   cz_repetition_chase's rule instead of cz_repetition's: a repetition that cz_repetition calls a draw is a loss for the
 *   side that alone chased one piece with every move of the cycle — z as for perpetual check.  Such a game counts in
 *   cz_selfplay_chase_stats and NOT among cz_selfplay_rules_stats' perpetuals (whose signature and meaning stay).
 * cz_selfplay_chase_history: the device pointer of the third ring; CZ_EINVAL while the rule is off.
 * cz_selfplay_chase_stats: device int64 [1] <- games ended by perpetual chase since cz_selfplay_begin (0 while the rule is
 *   off). */
int cz_selfplay_set_rules(cz_ctx *, int rules);
int cz_selfplay_set_repetition(cz_ctx *, int fold);
int cz_selfplay_history(cz_ctx *, const uint64_t **keys, const uint8_t **checks);
int cz_selfplay_rules_stats(cz_ctx *, long long *stats_dev /* [3]: mates, repetitions, perpetuals */);
int cz_selfplay_set_chase(cz_ctx *, int on);
int cz_selfplay_chase_history(cz_ctx *, const uint64_t **chase);
int cz_selfplay_chase_stats(cz_ctx *, long long *stats_dev /* [1]: chases */);
/* cz_selfplay_set_resign: resignation (AlphaGo Zero's), at every rule level.  threshold NaN = off (the default: everything above,
 *   launch for launch and byte for byte).  THE VALUE A MOVER RESIGNS ON is the Q of its most visited candidate child — the first
 *   maximum of N in generation order, as cz_match_choose's greedy pick; under rules 1 among the king-safe children the move is
 *   chosen from — read from the tree as it is, in the sign the search maximises: larger is better for the mover, a child that takes
 *   the king reads +1.  A ply is judged when that child has a visit, ply >= min_ply and no forced label is played; the mover
 *   resigns when Q < threshold, a float32 compare with no arithmetic on Q (cz_search_root_stats' Q reproduces it exactly).
 *   Order in cz_selfplay_choose: stalled, repetition, mate, then this, then the pick.  On a resignation played = 0xFFFF, no
 *   record is written, the ply stays, and cz_selfplay_adjudicate — behind the verdict and the mate, before every other test, also
 *   for a slot its `played` argument would skip — ends the game as a loss for the side to move: z as for a king capture,
 *   fin_n = min(plies played, max_plies), counted in CZ_SP_GAMES, the winner's wins and CZ_SP_PLIES.
 *   PLAY-ON GAMES measure what resignation costs: game number n of slot g (0 for the slot's first game, + 1 at every re-seed)
 *   plays on iff (splitmix64(seed ^ splitmix64(g << 32 | n)) >> 11) * 2^-53 < playon_fraction (0 <= playon_fraction <= 1).  Such a
 *   game never resigns; it notes the side that first crossed the threshold and is played out.  Every game keeps the lowest judged
 *   value of each side.  When a play-on game ends (unless it stalled): playon_games + 1; if a side crossed, playon_would_resign
 *   + 1, and if that side then won or drew, playon_false_positives + 1; and for each side that did not lose and was judged at all,
 *   its lowest value q goes into the histogram at bin clamp((int)floorf((q + 1.0f) * 32.0f), 0, 63): 64 bins of 1/32 over [-1, 1)
 *   — the values a threshold must stay below to spare those sides.
 *   The first call after cz_selfplay_begin (which switches resignation off and zeroes the counters) allocates and zeroes the state,
 *   draws every slot's game 0 and may come at any time; seed is taken then.  A later call only changes threshold, min_ply and
 *   playon_fraction — the game numbers, the games' state and the counters stay, so a threshold can be retuned between batches; with
 *   NaN no ply is judged until the next call.  playon_fraction applies from the slots' next games.
 * cz_selfplay_resign_stats: device int64 [4] <- games resigned, play-on games finished, those in which a side crossed the
 *   threshold, those of them that side did not lose; device int64 [64] <- the histogram (may be NULL).  Zeros while off. */
int cz_selfplay_set_resign(cz_ctx *, float threshold, int min_ply, double playon_fraction, unsigned long long seed);
/* cz_selfplay_set_tablebase: NULL = no game is adjudicated from a table (the default: everything above, launch for launch and
 *   byte for byte), a cz_tb_set = cz_selfplay_adjudicate first probes the set on every slot's root position AFTER the move — one
 *   launch on the trees' boards in place, nothing goes through the host — and a slot that just moved into a position the set
 *   covers (a value that is neither CZ_TB_MISS nor CZ_TB_ILLEGAL) ends its game there: value > 0 the side to move wins, < 0 it
 *   loses, 0 a draw; z of every record as for a king capture, fin_n = min(plies played, max_plies), counted in CZ_SP_GAMES,
 *   RED_WINS / BLACK_WINS / DRAWS, CZ_SP_PLIES and cz_selfplay_tablebase_stats; the slot re-seeds as after any ending.  Place
 *   among the endings: behind the repetition verdict, the mate, the resignation and the aborted game — found by the choose on
 *   a root that was then not left —, in front of the king test, the 60-ply rule and the ply cap: a forced mate is a mate
 *   whatever the no-capture counter says.  Play-on games of the resignation measurement end here like any other game.
 *   A table holds values under Xiangqi rules, so the set needs cz_selfplay_set_rules(ctx, 1): CZ_EINVAL under rules 0, and
 *   cz_selfplay_set_rules(ctx, 0) is refused while a set is attached.  Unlike the rule setters it may be called between any two
 *   plies — it judges positions, it keeps no history.  cz_selfplay_begin detaches the set.  The set must be the context's device's.
 *   A game whose START position is covered plays one ply first (adjudication follows a move).  A capture that leaves the set
 *   goes on, and the game is judged again after its next move.  A table draw is a draw even where the repetition or chase
 *   rules would later have punished a side; nothing is probed inside the search tree.
 * cz_selfplay_tablebase_stats: device int64 [1] <- games adjudicated from a table since cz_selfplay_begin (0 before a set was
 *   ever attached). */
int cz_selfplay_set_tablebase(cz_ctx *, cz_tb_set *set /* NULL = off */);
int cz_selfplay_tablebase_stats(cz_ctx *, long long *stats_dev /* [1]: games adjudicated */);
int cz_selfplay_resign_stats(cz_ctx *, long long *stats_dev /* [4]: resigned, playon_games, playon_would_resign, playon_false_positives */,
                             long long *hist_dev /* [64], may be NULL */);

/* ---- device-resident evaluation matches between two players (one wave per game slot; no host round trip per ply) -------
 * replaces: cchess_main.policy_evaluate (main.py:1207-1222, commented out in the reference) — many games of player A
 * against player B, both colours, for the G slots of two contexts at once.  Each player has its own cz_ctx (trees, net,
 * playout budget); slot g of both contexts belongs to the same game.  One ply of every game =
 *     cz_search_select/expand_backup... on A's context with mask cz_match_active(A), the same on B's with its mask
 *     cz_match_choose        the mover's move on the mover's tree (get_action, main.py:1332-1341), logged per game
 *     cz_search_advance      on BOTH contexts with the same `played`: the mover re-roots on its child; the other player's
 *                            tree keeps its subtree for the move if it has one (update_tree after the opponent's move,
 *                            main.py:272-276), else starts a fresh root on the new position
 *     cz_match_adjudicate    check_end (main.py:1380-1392) and the match's own endings; the slot's next game
 * cz_match_create (after cz_search_reset of both contexts to the same G, bound to the same stream): a queue of
 *   n_games = 2 n_openings games; game i plays opening i / 2 (boards [n][90], side [n], rr [n] or NULL = 0, device arrays)
 *   with player A red when i is even.  Slot g starts game g; a slot whose game ends takes the next game of the queue at
 *   once, or parks (both trees keep a fresh root with no simulation; neither mask names it).  pair_base / pair_stride: the
 *   GLOBAL index of local opening p is pair_base + pair_stride p (several ranks share one match; 0 / 1 otherwise).
 *   A game ends when a king is missing, when restrict_round reaches 60, at max_plies plies (a draw), or when the mover has
 *   no child to play (node pool exhausted at the root, or a rules overflow: CZ_MATCH_ABORTED, not scored).
 * cz_match_active: player 0 = A, 1 = B -> device uint8 [G] mask "this player is to move in slot g and the game is live",
 *   the `active` argument of that player's cz_search_select.
 * cz_match_choose: greedy — the first maximum of N in generation order (get_action's T -> 0 limit, as
 *   cz_search_pick_ready) — or, for the first sample_plies plies of a game, sampled from softmax(log N) (temperature 1,
 *   no Dirichlet noise: select_move -> get_action(state, 1), main.py:1123,1433-1435) by inverse CDF with the uniform
 *   u = (splitmix64(seed ^ splitmix64(game << 16 | ply)) >> 11) * 2^-53 of the GLOBAL game index: a game's moves do not
 *   depend on the slot it ran in, on G or on the rank.  played [G] out (0xFFFF: parked, or no child to play).
 * cz_match_adjudicate: after both advances; clears the follower's CZ_ST_BAD_ADVANCE (its fresh root is no error); the
 *   mover's is an abort.
 * cz_match_results: device arrays owned by the match — result int8 [n_games] (+1 / 0 / -1 from A's point of view),
 *   a_red uint8 [n_games], plies int32 [n_games], reason uint8 [n_games] (CZ_MATCH_*, 0 = not finished), moves uint16
 *   [n_games][max_plies] (0xFFFF past the game's end), slot_game int32 [G] (the game of each slot, -1 = parked); any may be NULL.
 * cz_match_finished: synchronises the stream; host <- games finished, simulations of the searches whose move was chosen. */
#define CZ_MATCH_KING 1      /* a king was captured */
#define CZ_MATCH_RR60 2      /* 60 plies without a capture: a draw (main.py:1390) */
#define CZ_MATCH_PLY_CAP 3   /* max_plies plies: a draw (the reference has no such limit) */
#define CZ_MATCH_ABORTED 4   /* the mover had no child to play: not scored */
#define CZ_MATCH_MATE 5      /* rules = 1: the mover had no king-safe move (checkmate or stalemate): it loses */
#define CZ_MATCH_REPETITION 6   /* cz_match_set_repetition: the position occurred for the fold-th time: a draw */
#define CZ_MATCH_PERPETUAL 7    /* ... and one side alone checked with every move of the cycle: that side loses */
#define CZ_MATCH_CHASE 9        /* cz_match_set_chase: ... neither side checked so, and one side alone chased one piece with every
                                   move of the cycle: that side loses (8 is not assigned) */
#define CZ_MATCH_RESIGN 10      /* cz_match_set_resign: the mover's root value was below the threshold: it loses */
#define CZ_MATCH_TABLEBASE 11   /* cz_match_set_tablebase: the position after the move is in a table: its value is the result */
typedef struct cz_match cz_match;
int cz_match_create(cz_ctx *a, cz_ctx *b, const uint8_t *open_boards, const uint8_t *open_side, const int32_t *open_rr,
                    int n_openings, long long pair_base, long long pair_stride, int max_plies, cz_match **out);
void cz_match_destroy(cz_match *);
/* cz_match_set_rules: 0 = king capture (the default: the reference's games, everything above), 1 = xiangqi.  With 1,
 *   cz_match_choose first computes the king-safe set (cz_movegen_kingsafe) of every live slot's root position and then chooses
 *   as above AMONG THE ROOT CHILDREN WHOSE MOVE IS IN THAT SET, in generation order: greedy = the first maximum of N over them
 *   (a king-safe child with N = 0 is eligible), sampled = softmax(log N) over them alone with the same uniform.  A root with
 *   children, none of them king-safe: played = 0xFFFF, and cz_match_adjudicate ends the game with CZ_MATCH_MATE — a loss for
 *   the mover, plies = the plies actually played — before it looks at anything else.  A root without children aborts as above. */
int cz_match_set_rules(cz_match *, int rules);
/* cz_match_set_repetition: fold 0 = no repetition rule (the default: everything above, launch for launch), 2 <= fold <= 8 =
 *   a game ends when its position occurs for the fold-th time (cz_repetition's rule; 3 is the usual value).  Needs
 *   cz_match_set_rules(match, 1) first — the check flags are the king-safe pass's — and is refused (CZ_EINVAL) under rules 0
 *   and once a cz_match_choose has run on the match (a history recorded from mid-game would be wrong); cz_match_set_rules(match,
 *   0) is refused while the fold is not 0.  With it, cz_match_choose also takes every root position's CZ_POS_* flags and cz_hash,
 *   writes them into the slot's ring of 64 positions at entry ply & 63 (every ring index is masked; a parked slot returns
 *   before it touches the ring) and evaluates the rule with w = min(restrict_round of the root, ply, 63): a capture makes the
 *   earlier positions unreachable, w <= ply keeps every read inside the slot's current game (no reset when a slot takes its
 *   next game), and restrict_round is below 60 in every live game.  Order: a root without children aborts as above, then
 *   repetition, then mate (a repeated position was moved from before: the two cannot both hold).  On a verdict played =
 *   0xFFFF, no move is logged, the ply is not advanced, and cz_match_adjudicate ends the game before it looks at anything else:
 *   CZ_MATCH_REPETITION (result 0) or CZ_MATCH_PERPETUAL (result -1 when the losing side is A's colour in that game, else +1),
 *   plies = the plies actually played.
 * cz_match_history: the device pointers of the two rings, owned by the match — keys uint64 [G][64], checks uint8 [G][64]:
 *   position i of the game in slot g at [g][i & 63]; either may be NULL.  CZ_EINVAL while the repetition rule is off.
 * cz_match_set_chase: 0 = perpetual chase is not judged (the default: everything above, launch for launch), 1 = it is.  Needs
 *   a non-zero fold (CZ_EINVAL otherwise), is set before the first cz_match_choose, and cz_match_set_repetition(match, 0) is
 *   refused while it is on.  With it, cz_match_choose adds one cz_threats launch on the root boards it already copies out,
 *   writes every root position's chase record into a third ring, chase uint64 [G][64][4], at entry ply & 63, and evaluates
 *   cz_repetition_chase's rule with the same window: a verdict whose cause is CZ_CAUSE_CHASE ends the game as CZ_MATCH_CHASE, a
 *   scored game like CZ_MATCH_PERPETUAL (result -1 when the chaser is A's colour in that game, else +1); every other verdict
 *   ends it as before.
 * cz_match_chase_history: the device pointer of the third ring, owned by the match; CZ_EINVAL while the rule is off.
 * cz_match_set_resign: threshold NaN = nobody resigns (the default: everything above, launch for launch).  Otherwise both
 *   players resign on their own tree's value, the one cz_selfplay_set_resign describes: from ply min_ply of a game on, in sampled
 *   plies too, a mover whose most visited candidate child has a visit and Q < threshold resigns — after the repetition verdict
 *   and the mate, before the choice: played = 0xFFFF, no move is logged, the ply is not advanced, and cz_match_adjudicate ends the
 *   game as CZ_MATCH_RESIGN, a scored loss for the mover, behind CZ_MATCH_REPETITION / _PERPETUAL / _CHASE and CZ_MATCH_MATE and
 *   before CZ_MATCH_ABORTED.  There is no play-on fraction: a match measures strength, not the threshold.  May change between
 *   two plies. */
int cz_match_set_resign(cz_match *, float threshold, int min_ply);
/* cz_match_set_tablebase: NULL = off (the default: everything above, launch for launch), a cz_tb_set = cz_match_adjudicate first
 *   probes the set on every slot's position after the move (one launch, on the trees' boards in place) and a slot that just
 *   moved into a covered position ends its game as CZ_MATCH_TABLEBASE, a scored game: the table's value is from the side to
 *   move's view, result -1 when the losing side is A's colour in that game, +1 when it is B's, 0 for a table draw; plies = the
 *   plies played.  Place among the endings, the rule level it needs (cz_match_set_rules(match, 1); CZ_EINVAL otherwise, and
 *   cz_match_set_rules(match, 0) is refused while a set is attached), the opening that is itself covered (one ply is played
 *   first), the capture that leaves the set and what is not covered: as cz_selfplay_set_tablebase.  May change between two
 *   plies.  cz_match_destroy gives the set back. */
int cz_match_set_tablebase(cz_match *, cz_tb_set *set /* NULL = off */);
int cz_match_set_repetition(cz_match *, int fold);
int cz_match_history(cz_match *, const uint64_t **keys, const uint8_t **checks);
int cz_match_set_chase(cz_match *, int on);
/* THE AVOID STEP (off by default: the launches and outputs are those without it).  cz_match_set_avoid(match, 1) — after
 *   cz_match_set_repetition, before the first cz_match_choose, off again before the fold goes — makes cz_match_choose run one more
 *   launch between the root pass and the choice: cz_repetition_moves' kernel over the slots' rings (windows as the rule's own,
 *   min(root_rr, ply, 63), never past 63; with cz_match_set_chase the chase rule too), and the candidates of the choice are its
 *   `allowed`: the king-safe root children without the moves that lose by repetition, themselves or by a reply.  A mover whose
 *   every move loses chooses among all king-safe moves; "mated" still means no king-safe move.  cz_match_avoid_stats: the plies at
 *   which a move was removed and the plies at which every move lost, over the moves chosen so far (synchronises).
 *   cz_selfplay_set_avoid / cz_selfplay_avoid_stats (long long [2], device): the same for self-play, where pi, the noise and the
 *   record of a ply run over the candidates that are left. */
int cz_match_set_avoid(cz_match *, int on);
int cz_match_avoid_stats(cz_match *, int32_t *avoided, int32_t *forced);
int cz_selfplay_set_avoid(cz_ctx *, int on);
int cz_selfplay_avoid_stats(cz_ctx *, long long *stats_dev /* [2] */);
int cz_match_chase_history(cz_match *, const uint64_t **chase);
int cz_match_active(cz_match *, int player, const uint8_t **mask_dev);
int cz_match_choose(cz_match *, int sample_plies, unsigned long long seed, uint16_t *played);
int cz_match_adjudicate(cz_match *, const uint16_t *played);
int cz_match_results(cz_match *, const int8_t **result, const uint8_t **a_red, const int32_t **plies, const uint8_t **reason,
                     const uint16_t **moves, const int32_t **slot_game);
int cz_match_finished(cz_match *, int32_t *finished, unsigned long long *sims);

/* ---- N1: policy/value network kernels ---------------------------------------------------------
 * One residual-tower layer: 3x3 SAME convolution 128->128 over [B][9][10] boards, NHWC bf16, with the
 * (BN-folded) bias, optional residual add and optional ReLU fused in.
 * replaces: tf.layers.conv2d(128,3,'SAME') + tf.contrib.layers.batch_norm(center=False) [+ tf.add(orig,.)]
 *           + tf.nn.relu, policy_value_network.py:45-47 and residual_block :151-162.
 *   in, residual, out : [B][90][128] bf16 (residual may be NULL; out must not alias in)
 *   wpk  : [9 taps = dy*3+dx][16 = ci/8][128 co][8 = ci%8] bf16, BN scale folded in (net.py packs it)
 *   bias : [128] float32, BN folded */
int cz_conv3x3_c128_bf16(cz_ctx *, const void *in, const void *wpk, const float *bias,
                         const void *residual, void *out, int B, int relu);

/* The whole residual tower (nblocks x [conv3x3+BN+ReLU, conv3x3+BN, add, ReLU]) in ONE launch:
 * activations stay in LDS across all 2*nblocks layers, only `in` and `out` touch HBM.
 * replaces: the `for _ in range(res_block_nums): residual_block(...)` loop, policy_value_network.py:50-53,151-162.
 *   in, out : [B][90][128] bf16 (may alias)
 *   wpk  : [2*nblocks][9][16][128][8] bf16 (layer-major, same per-layer packing as cz_conv3x3_c128_bf16)
 *   bias : [2*nblocks][128] float32 */
int cz_tower_c128_bf16(cz_ctx *, const void *in, const void *wpk, const float *bias, void *out, int B,
                       int nblocks);
/* Same launch with the two head 1x1 convolutions fused in (conv1x1 128->2 policy, 128->1 value, BN folded,
 * ReLU; policy_value_network.py:57-59,68-70), computed from the LDS-resident trunk:
 *   head_w [3][128] f32 (rows: policy ch0, policy ch1, value), head_b [3] f32,
 *   head_out [B][90][3] f32 (post-ReLU; [:, :, 0:2] flattens to the 180 policy-FC inputs in the reference's
 *   (h, w, c) order, [:, :, 2] to the 90 value-FC inputs).  trunk_out may be NULL (trunk never leaves the CU). */
int cz_tower_heads_c128_bf16(cz_ctx *, const void *in, const void *wpk, const float *bias, void *trunk_out,
                             const float *head_w, const float *head_b, float *head_out, int B, int nblocks);

/* Input planes to head-conv outputs in ONE launch: conv3x3(14->128)+BN+ReLU (policy_value_network.py:45-47),
 * the residual tower and (optionally) the head 1x1 convolutions.
 *   planes16 : [B][90][16] bf16 — the K3 encoding with channels = 16 (14 planes + 2 zero channels), e.g. written by
 *              cz_search_select(..., CZ_BF16, 16, ...)
 *   w0 : [9 taps][2 = ci/8][128 co][8 = ci%8] bf16 (input channels 14,15 zero), b0 : [128] f32, BN folded
 *   other arguments as cz_tower_heads_c128_bf16; trunk_out and head_out may each be NULL (not both). */
int cz_net_trunk_bf16(cz_ctx *, const void *planes16, const void *w0, const float *b0, const void *wpk,
                      const float *bias, void *trunk_out, const float *head_w, const float *head_b,
                      float *head_out, int B, int nblocks);

/* cz_net_trunk_bf16 with IEEE fp16 activations and weights (fp32 accumulate): the reference's "19-block net fp16"
 * configuration (BASELINE.json configs[4]).  Same argument layout; planes16, w0, wpk and trunk_out hold fp16. */
int cz_net_trunk_f16(cz_ctx *, const void *planes16, const void *w0, const float *b0, const void *wpk,
                     const float *bias, void *trunk_out, const float *head_w, const float *head_b,
                     float *head_out, int B, int nblocks);

/* The STRICT-precision form of cz_net_trunk_*: every weight and every stored activation is carried as hi + lo, two values
 * of `halves_dtype` (CZ_F16: 22 significant bits, CZ_BF16: 16), and every product is three MFMAs (hi*hi + hi*lo + lo*hi,
 * fp32 accumulate) — the engine that meets north_star's "policy/value outputs within 1e-3 of fp32" for the reference's
 * fp32 sess.run (policy_value_network.py:202-214) also on trained (peaked) weights and at 19 blocks, at a third of the
 * 16-bit kernels' rate.
 *   planes16 : [B][90][16] of halves_dtype (0/1 planes are exact: the same buffer cz_search_select writes)
 *   w0   : [9 taps][hi, lo][2 = ci/8][128 co][8 = ci%8], b0 [128] f32
 *   wpk  : [2*nblocks][9 taps][4 = 32-channel quarter of the tap][hi, lo][4 = ci/8][128 co][8] (16 KB per quarter: one
 *          LDS-DMA slab), bias [2*nblocks][128] f32; BN folded; hi = rn(w), lo = rn(w - hi) (net.py packs it)
 *   trunk_out : [B][90][128] FLOAT32 (hi + lo) or NULL; head_w / head_b / head_out as cz_net_trunk_bf16. */
int cz_net_trunk_split(cz_ctx *, const void *planes16, const void *w0, const float *b0, const void *wpk,
                       const float *bias, float *trunk_out, const float *head_w, const float *head_b,
                       float *head_out, int B, int nblocks, int halves_dtype);

/* The strict-precision trunk at half the matrix work (round 5; k_trunk_mx_c128, csrc/cz_trunk_mx.h): a*w = a_hi*w_hi on fp16
 * MFMAs + BOTH cross terms (a_hi*w_lo + a_lo*w_hi) of 32 input channels on ONE block-scaled fp6 MFMA
 * (v_mfma_scale_f32_32x32x64_f8f6f4, E2M3 operands, one E8M0 scale per cell / output channel and 16 input channels):
 * 1.5 instead of 3 fp16-MFMA-equivalents per product, the cross terms to 4 significant bits per operand (~2^-16 of a product).
 * Replaces the same fp32 sess.run (policy_value_network.py:202-214); |dlogit|, |dvalue| <= 1e-3 against it on trained-like
 * weights up to 8 blocks with a factor of two to spare, at the edge of 1e-3 at 19 (tests/test_net.py, tests/mxemu.py is its CPU
 * emulation).  Which of this and cz_net_trunk_split a net runs is MEASURED on its live weights by the host side (precision
 * "strict", cchess_zero_amd/net.py: strict_check), not decided by depth.
 *   planes16 : [B][90][16] fp16; w0 / b0 : as cz_net_trunk_split with CZ_F16 (the first layer is two fp16 MFMAs per tap)
 *   wpk  : [2*nblocks][9 taps][4 quarters][16384 bytes]: per 32-input-channel quarter of a tap (one LDS-DMA slab)
 *          [fp16 w_hi: 4 = ci/8][128 co][8] (8192 B) [fp6 blocks, first 16 bytes: 2 halves][128 co][16] (4096 B)
 *          [last 8 bytes: 2][128 co][8] (2048 B) [E8M0 scale in byte 0 of a dword: 2][128 co] (1024 B) [1024 B unused];
 *          block (co, half h) = 32 six-bit slots, slot 2j = q6(2^11 w_lo[c_j]), slot 2j+1 = q6(w_hi[c_j]),
 *          c_j = 32 quarter + 8 (j / 4) + 4 h + j % 4, under 2^(exponent(max |w_hi|) - 2); the stored byte is that exponent
 *          - 11 (cchess_zero_amd/net.py: mx_pack_layer); 16-byte aligned.  bias [2*nblocks][128] f32, BN folded.
 *   trunk_out : [B][90][128] FLOAT32 or NULL; head_w / head_b / head_out as cz_net_trunk_bf16. */
int cz_net_trunk_mx(cz_ctx *, const void *planes16, const void *w0, const float *b0, const void *wpk,
                    const float *bias, float *trunk_out, const float *head_w, const float *head_b,
                    float *head_out, int B, int nblocks);

/* Measurement hook for bench.py (roofline.effective_clock_GHz): while buf_dev is set, every workgroup w of the following
 * cz_net_trunk_* launches (grids up to max_workgroups) writes buf_dev[4w .. 4w+3] = {shader-clock cycle counter at its start,
 * at the end of its last layer, 100 MHz reference clock at the same two points}: cycles / (ticks * 10 ns) is the clock the
 * kernel really ran at under the chip's power governor.  NULL switches it off (the default; one uniform branch per
 * workgroup).  cz_clock_probe_last_grid: workgroups of the last probed launch. */
int cz_set_clock_probe(cz_ctx *, unsigned long long *buf_dev, int max_workgroups);
int cz_clock_probe_last_grid(cz_ctx *);

/* Measurement: back-to-back v_mfma_f32_32x32x16 (dtype CZ_BF16 | CZ_F16) on register operands, two waves per SIMD, every CU:
 * the practical MFMA ceiling of this chip under its power governor, measured in the bench run itself (tools/mfma_peak.hip
 * is the stand-alone form).  data: 0 dense random operands, 1 zeros, 2 random with half the elements zero; iters x 48
 * MFMAs per wave.  *tflops, *ms: dense-equivalent TFLOP/s and duration of the (second) launch.  Synchronises the stream. */
int cz_probe_mfma_peak(cz_ctx *, int dtype, int data, int iters, double *tflops, double *ms);

/* The three fully connected layers behind the head convolutions (policy_value_network.py:62-63,72-74): policy FC
 * 180 -> 2086 (raw logits) and value FC 90 -> 256, ReLU, FC 256 -> 1, tanh, from the head conv outputs
 * z [B][90][3] f32 as cz_net_trunk_bf16 / cz_tower_heads_c128_bf16 leave them (flatten order (h,w,c)).
 *   pfc_w_hi, pfc_w_lo : policy FC weight split into bf16 hi + lo parts (w ~= hi + lo), each packed in MFMA
 *                        fragment order [66 = label/32][12 = k/16][64 lanes][8] bf16 with
 *                        element = W[label = tile*32 + (lane & 31)][k = kblock*16 + (lane >> 5)*8 + j], zero padded
 *   pfc_b [2086] f32;  v1_wt [90][256] f32 (value FC1 weight, input-major);  v1_b [256];  v2_w [256];  v2_b [1]
 *   logits [B][2086] f32, value [B] f32 (either may be NULL to skip that head). */
int cz_fc_heads_f32(cz_ctx *, const float *z, const void *pfc_w_hi, const void *pfc_w_lo, const float *pfc_b,
                    const float *v1_wt, const float *v1_b, const float *v2_w, const float *v2_b,
                    float *logits, float *value, int B);

#ifdef __cplusplus
}
#endif
#endif
