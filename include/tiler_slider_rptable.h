/*
 * tiler_slider_rptable.h — C-ABI of the reach policy tables (lib/libtiler_slider_rptable.so).
 *
 * ts_ptable_actions / ts_ptable_walk / ts_ptable_score (tiler_slider_ptable.h) hold a network's greedy play on EVERY placement of
 * a level and stop at index spaces of 65,536 placements.  This library does the same on the states of a reachable distance table
 * (tiler_slider_rtable.h): the set R of a level is closed - every successor of a state of R is won or in R -, so a deterministic
 * policy is a successor function on R and its outcome from every state of R is exact.  It shares the data layout, ts_dims,
 * ts_state and ts_status of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*,
 * every call asynchronous, no allocation, no retained pointers), the slot format, the home function, the probe,
 * TS_RTABLE_ROOT_INIT, TS_RTABLE_ROOT_POS and TS_RTABLE_ABSENT of tiler_slider_rtable.h, the entry codes of tiler_slider_table.h,
 * the network ts_mlp and TS_POLICY_GREEDY of tiler_slider_policy.h, the score columns of tiler_slider_ptable.h, and has an ABI
 * version of its own.
 *
 * L = dims->n_boards is the number of levels; level n is board n's obstacles `blk` and targets `tgt`.  Row n of `table`
 * (uint64 [L][slots], slots a power of two in 2 .. 2^31) and count[n] (int32 [L]) are what ts_rtable_build wrote for it.  C = S * S.
 * The slot format, restated: a slot is 0 (empty) or
 *     bit 63 set | bits 56 .. 62 zero | bits 48 .. 55 the entry | bits 0 .. 47 the key,   key = sum_t cell_t * C^t,
 * and a state lies in the first free slot of its probe sequence: linear probing, slot + 1 modulo slots, from
 *     home(key) = (uint32)((key * 0x9e3779b97f4a7c15) >> 32) >> (32 - log2(slots)).
 * The PROBE for a key walks that sequence for at most `slots` steps, ends without it at a slot that is 0, and finds it in the
 * first slot with bit 63 set whose bits 0 .. 47 are the key.
 * A slot i of level n is LIVE when count[n] >= 0 and bit 63 of table[n][i] is set.  Its placement is
 *     cell_t = (key / C^t) % C  for t = 0 .. T - 1: always below C.
 * A level with count[n] < 0 (TS_REACH_FULL) has no live slot.  A move and a won board are what ts_step and ts_is_won compute;
 * cell ids >= C in tgt and in the root cells are clamped to C - 1 as the step kernels clamp them.
 *
 * SUPPORTED exactly where ts_rtable_supported(dims) and ts_policy_supported(dims, hidden) both hold (ts_rptable_supported): S <= 8,
 * n_tiles <= 8, n_targets <= 8, hidden 1 .. 64.  The walk and the score, which have no network, take hidden = 1.
 */
#ifndef TILER_SLIDER_RPTABLE_H
#define TILER_SLIDER_RPTABLE_H

#include "tiler_slider_policy.h"
#include "tiler_slider_ptable.h"
#include "tiler_slider_rtable.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_RPTABLE_ABI_VERSION 1
#define TS_RPTABLE_NO_ACTION 255  /* act of a slot that is not live */
#define TS_RPTABLE_FORM_NONE 0    /* no level: nothing is launched */
#define TS_RPTABLE_FORM_LDS 1     /* a level's working set lives in LDS */
#define TS_RPTABLE_FORM_GLOBAL 2  /* the walk of rows above lds_slots: the (succ, entry) pairs live in the output row */

int32_t ts_rptable_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_rptable_last_hip_error(void);
/* 1 where ts_rtable_supported(dims) == 1 and ts_policy_supported(dims, hidden) == 1, 0 otherwise, a negative ts_status for invalid
 * dims (TS_ERR_NULL, TS_ERR_DIMS).  Host only. */
int32_t ts_rptable_supported(const ts_dims *dims, int32_t hidden);

/* 1. THE ACTIONS.  act uint8 [L][slots]; logits float32 [L][slots][4], 16-byte aligned, or NULL.  On a live slot z is exactly what
 * ts_policy_logits gives on a board of level n standing on the slot's placement - the same sequence of float operations, so it
 * is bit-equal - and act[n][i] is TS_POLICY_GREEDY's choice on z, the lowest action among the largest logits (on the float32
 * values that are stored).  Every other slot gets act = TS_RPTABLE_NO_ACTION and four 0.0f.  Every byte of both outputs is
 * written exactly once.  Reads blk, tgt, table and count only.  Whatever bits the rows and the weights hold, no access leaves a
 * buffer and act of a live slot is <= 3.
 * One launch, asynchronous on `stream`: k_rptable_actions<S>, min(L, 1024) blocks; block b takes levels b, b + blocks, ...  A
 * block reads a row 1,024 slots at a time, writes the rows of the slots that are not live as it goes, compacts the live ones
 * into a list in LDS and evaluates the network on a full block of them at a time, one state per lane.
 * REFUSALS, in this order and before any HIP call:
 *   1. dims: TS_ERR_NULL, TS_ERR_DIMS or TS_ERR_LIMIT of the shared check
 *   2. mlp NULL: TS_ERR_NULL
 *   3. slots no power of two in 2 .. 2^31, a shape or width ts_rptable_supported refuses: TS_ERR_ARG
 *   4. n_boards = 0: TS_OK without a launch, no further pointer is looked at
 *   5. a missing pointer - st, table, count, act, a parameter of the network, blk, tgt where there are targets: TS_ERR_NULL
 *   6. a logits pointer that is not 16-byte aligned: TS_ERR_ARG */
int32_t ts_rptable_actions(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const uint64_t *table, int64_t slots,
                           const int32_t *count, uint8_t *act, float *logits, void *stream);

typedef struct ts_rptable_cfg {
  int32_t max_depth; /* 0 .. TS_TABLE_MAX_DEPTH */
  int32_t root;      /* TS_RTABLE_ROOT_INIT or TS_RTABLE_ROOT_POS: the cells root_moves is read at */
} ts_rptable_cfg;

typedef struct ts_rptable_out {
  uint64_t *table;     /* [L][slots], required; any contents: every slot of every row is written */
  int16_t *root_moves; /* [L], may be NULL: 0 for a won root, TS_REACH_FULL for a FULL level, TS_RTABLE_ABSENT where the row does
                          not hold the root (never the case for a built table), else the root's entry as ts_table_lookup maps
                          entries (1 .. 252, TS_SOLVE_NONE, TS_SOLVE_DEPTH) */
  int32_t *deepest;    /* [L], may be NULL: the largest entry 1 .. 252 of the row; 0 if there is none or the level is FULL */
} ts_rptable_out;

/* 2. THE WALK.  act uint8 [L][slots] may hold ANY bytes: a tabular policy need not come from a network.  For a live slot i of
 * level n, succ(i) is
 *     i itself where act[n][i] > 3;
 *     otherwise, with the placement after ts_step's move act[n][i]: WON if that board is won, else the slot of row n that the
 *     probe finds holding its key; a row that does not hold it (never the case for a built table) leaves i on itself.
 * The entry of a live slot is tiler_slider_rtable.h's Distance rule with this one successor in place of four: D by rounds
 * d = 1, 2, ...: round d resolves the unresolved live slots whose succ is WON (d = 1) or has the entry d - 1.  With R(d) the
 * live slots at distance exactly d, d >= 1: the level stops at the first d <= max_depth with R(d) empty, and everything
 * unresolved becomes TS_TABLE_NONE; otherwise it stops behind round max_depth, and everything unresolved becomes TS_TABLE_DEEP
 * (with max_depth = 0 no round runs: every live slot is TS_TABLE_DEEP).
 *     out->table[n][i] = bit 63 | entry << 48 | the key of table[n][i]  on a live slot, 0 on every other slot.
 * A FULL level's row is therefore all zero.  The same key lies in the same slot, so the output row is a valid reach-table row for
 * the same count: ts_rtable_lookup, ts_rstarts_index and every other reader of a row take it unchanged.  root_moves and deepest
 * are ts_rtable_out's, over the policy's entries; the root is read from st->init or st->pos only where root_moves is asked for.
 * No workspace: during the rounds a level's (succ, entry) pairs live in LDS where the row has at most lds_slots slots
 * (TS_RPTABLE_FORM_LDS, with the list of the live slots: succ is resolved once per live slot, one move and one probe, and the
 * rounds run over what of the list is still unresolved), and in the output row itself above that (TS_RPTABLE_FORM_GLOBAL: there
 * is nowhere to keep a list, so EVERY round reads the whole row - slots reads a round and level, up to max_depth rounds; a level
 * whose policy has long chains costs that much, which is the price of a capacity above lds_slots / 2).
 * The final pass re-reads the keys from `table`.  Integers only: the output bits are a function of the input bits.
 * One launch, asynchronous on `stream`: k_rptable_walk<S, GLOBAL>, min(L, 1024) blocks of four waves; block b takes levels
 * b, b + blocks, ...  Reads blk, tgt, table, count, act and the root cells.
 * REFUSALS, in this order and before any HIP call:
 *   1. dims: TS_ERR_NULL, TS_ERR_DIMS or TS_ERR_LIMIT of the shared check
 *   2. cfg or out NULL: TS_ERR_NULL
 *   3. slots no power of two in 2 .. 2^31, a shape ts_rptable_supported(dims, 1) refuses, max_depth outside
 *      0 .. TS_TABLE_MAX_DEPTH, root neither TS_RTABLE_ROOT_INIT nor TS_RTABLE_ROOT_POS: TS_ERR_ARG
 *   4. n_boards = 0: TS_OK without a launch, no further pointer is looked at
 *   5. a missing pointer - st, table, count, act, out->table, blk, tgt where there are targets, the root cells where root_moves is
 *      asked for and there are tiles: TS_ERR_NULL
 *   6. out->table sharing a byte with table or act: TS_ERR_ARG */
int32_t ts_rptable_walk(const ts_dims *dims, const ts_state *st, const uint64_t *table, int64_t slots, const int32_t *count,
                        const uint8_t *act, const ts_rptable_cfg *cfg, const ts_rptable_out *out, void *stream);

/* 3. THE SCORE.  score int32 [L][8], 4-byte aligned: ts_ptable_score's columns counted over the live slots of `table`.  With
 * o = the entry of table[n][i] (bits 48 .. 55) and p = bits 48 .. 55 of ptable[n][i], whatever its other bits hold:
 *     column 0  valid:     live slots
 *     column 1  solvable:  1 <= o <= 252
 *     column 2  solved:    1 <= p <= 252
 *     column 3  optimal:   solved and p = o
 *     column 4  agree:     solvable, act[n][i] <= 3, and the board after that move is won with o = 1, or the probe finds it in row n
 *                          of `table` with the entry o - 1
 *     column 5  excess:    the sum of p - o over the slots both solved and solvable, signed
 *     column 6  p = TS_TABLE_DEEP
 *     column 7  p = 0: always 0 for a table the walk wrote - won placements are not stored
 * A FULL level scores eight zeros.  Integers only and no atomics - a block per level, reduced by shuffles and through LDS:
 * the same bits on every run and for every slot order of the same set.  Over tables nobody built (any bytes) it reads nothing
 * outside its rows.  One launch: k_rptable_score<S>, min(L, 1024) blocks of four waves; block b takes levels b, b + blocks, ...
 * REFUSALS, in this order and before any HIP call:
 *   1. dims: TS_ERR_NULL, TS_ERR_DIMS or TS_ERR_LIMIT of the shared check
 *   2. slots no power of two in 2 .. 2^31, a shape ts_rptable_supported(dims, 1) refuses: TS_ERR_ARG
 *   3. n_boards = 0: TS_OK without a launch, no pointer is looked at
 *   4. a missing pointer - st, ptable, act, table, count, score, blk, tgt where there are targets: TS_ERR_NULL
 *   5. a score pointer that is not 4-byte aligned: TS_ERR_ARG */
int32_t ts_rptable_score(const ts_dims *dims, const ts_state *st, const uint64_t *ptable, const uint8_t *act, const uint64_t *table,
                         int64_t slots, const int32_t *count, int32_t *score, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_rptable_desc {
  int32_t form;              /* TS_RPTABLE_FORM_*: the walk LDS or GLOBAL by `slots`; the actions and the score LDS */
  int32_t threads_per_block; /* the actions 256, 128 or 64 (the policy library's forward plan), the walk and the score 256 */
  int32_t lds_bytes;         /* of a block, static and dynamic together, at most 64 KiB */
  int32_t lds_slots;         /* the walk: a row of at most so many slots is walked in LDS (the threshold); actions and score 0 */
  int32_t weights_in_lds;    /* the actions: 1 where the tile-plane weights are staged in LDS, 0 where gathered through L2 */
  int32_t reserved;
  int64_t blocks;            /* grid size; 0 where nothing is launched (name is empty) */
  char name[64];             /* as rocprofv3 prints it: "k_rptable_actions<5>", "k_rptable_walk<5, false>", "k_rptable_score<5>" */
} ts_rptable_desc;
/* dims or desc NULL: TS_ERR_NULL; then refusals 1 and 3 of ts_rptable_actions. */
int32_t ts_describe_rptable_actions(const ts_dims *dims, int32_t hidden, int64_t slots, ts_rptable_desc *desc);
/* dims or desc NULL: TS_ERR_NULL; then refusal 1 and the slots and the shape of refusal 3 of ts_rptable_walk. */
int32_t ts_describe_rptable_walk(const ts_dims *dims, int64_t slots, ts_rptable_desc *desc);
/* dims or desc NULL: TS_ERR_NULL; then refusals 1 and 2 of ts_rptable_score. */
int32_t ts_describe_rptable_score(const ts_dims *dims, int64_t slots, ts_rptable_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_RPTABLE_H */
