/*
 * tiler_slider_rexpert.h — C-ABI of the reach-table experts (lib/libtiler_slider_rexpert.so).
 *
 * The two consumers of a reachable distance table (tiler_slider_rtable.h) that an imitation loop needs, beyond the index spaces
 * of 65,536 placements at which ts_rollout's TS_ROLLOUT_TABLE and ts_traj_labels stop: K steps of the epsilon-greedy expert in
 * one launch (ts_rexpert_rollout), and the table's answer on every board a logged rollout visited (ts_rexpert_labels).  It
 * shares the data layout, ts_dims, ts_state, ts_status and the flag / mode bits of tiler_slider.h (every pointer a DEVICE pointer
 * owned by the caller, `stream` a hipStream_t as void*, every call asynchronous, no allocation, no retained pointers), the
 * outputs of tiler_slider_rollout.h and tiler_slider_targets.h, the table format and the lookup of tiler_slider_rtable.h - that
 * format is fixed there, and this library restates the probe from it -, and has an ABI version of its own.
 *
 * TS_REXPERT_ROLLOUT.  THE DEFINITION is the loop of tiler_slider_rollout.h for TS_ROLLOUT_TABLE with another lookup: for every
 * board n, ts_rexpert_rollout leaves exactly what this loop over the entry points of the other libraries leaves
 * (k = 0 .. steps - 1):
 *
 *     r[n]   = mix64(key_k + (board_offset + n) * kDrawMul),  key_k = mix64(seed ^ ((step_index + k) * kBoardMul))
 *     rnd[n] = r[n] >> 62                      -- exactly ts_fill_actions(n_boards, seed, board_offset, step_index + k)
 *     e      = the `action` output of ts_rtable_lookup(table, slots, count, n_rows, rows) on the board as it stands
 *     explore = (r[n] & 0xffffffff) < explore_threshold
 *     a[n]   = (explore or e == 255) ? rnd[n] : e
 *     ts_step(dims, st, a, mode, {flags_k, reward_k})
 *
 * The random draw plays wherever the lookup has no move: a won board, TS_SOLVE_NONE or TS_SOLVE_DEPTH, a FULL row,
 * TS_RTABLE_ABSENT, a row index outside the table.  The outputs are ts_rollout_out, with every meaning ts_rollout gives them.
 * The table is read only; it must not change while the launch runs.
 *
 * TS_REXPERT_LABELS.  For every sample (k, n) of tiler_slider_targets.h (c[0] = first, c[k] = pos_log[k - 1]; the last row of
 * pos_log is not read): exactly what ts_rtable_lookup writes for a board of level n that stands on c[k] - moves int16
 * (TS_REACH_FULL and TS_RTABLE_ABSENT included), best uint8, action uint8, each [K][N].  Won placements are not stored in a
 * reach table, so the win test is computed: unlike ts_traj_labels, this call reads st->tgt.
 *
 * THE PROBE, as ts_rtable_lookup promises it: every probe takes at most `slots` reads, each masked into the board's row, so
 * whatever bytes a row holds a call ends and reads nothing outside that row; for a row index outside 0 .. n_rows - 1 nothing of
 * table or count is read.  An entry that is no distance (0, TS_TABLE_INVALID, TS_TABLE_NONE) or TS_TABLE_DEEP gives no move.
 *
 * Supported shapes: those both parents take - S <= 8, n_tiles <= 8, n_targets <= 8.  Cell ids >= S*S are clamped as everywhere.
 */
#ifndef TILER_SLIDER_REXPERT_H
#define TILER_SLIDER_REXPERT_H

#include "tiler_slider_rollout.h"
#include "tiler_slider_rtable.h"
#include "tiler_slider_targets.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_REXPERT_ABI_VERSION 1

typedef struct ts_rexpert_cfg {
  int32_t steps;              /* K, 0 .. TS_ROLLOUT_MAX_STEPS */
  uint32_t mode;              /* TS_MODE_STRICT or TS_MODE_AUTORESET: ts_step's, unchanged */
  int32_t write_state;        /* 1: pos / step_count / done are stored back; 0: a playout, no state byte is touched */
  int32_t reserved;
  uint64_t seed;              /* the stream (seed, step_index + k, board_offset + n) */
  int64_t step_index;
  int64_t board_offset;
  uint64_t explore_threshold; /* 0 .. 2^32, epsilon * 2^32 */
  const uint64_t *table;      /* uint64 [n_rows][slots] of ts_rtable_build; may be NULL when n_rows is 0 */
  int64_t slots;              /* a power of two, 2 .. 2^31 */
  const int32_t *count;       /* int32 [n_rows] of ts_rtable_build; may be NULL when n_rows is 0 */
  int64_t n_rows;
  const int32_t *rows;        /* int32 [N] or NULL (board n reads row n) */
} ts_rexpert_cfg;

/* ts_labels_in with the reach table in place of the dense one */
typedef struct ts_rexpert_labels_in {
  const void *first;     /* cell_t [T][N]: c[0] */
  const void *pos_log;   /* cell_t [K][T][N]: c[k] = pos_log[k - 1]; may be NULL when steps == 1 */
  const uint64_t *table; /* uint64 [n_rows][slots]; may be NULL when n_rows == 0 */
  const int32_t *count;  /* int32 [n_rows]; may be NULL when n_rows == 0 */
  const int32_t *rows;   /* [N]: board n reads row rows[n]; NULL: row n */
  int64_t slots;         /* a power of two, 2 .. 2^31 */
  int64_t n_rows;
  int32_t steps;         /* K, 1 .. TS_ROLLOUT_MAX_STEPS */
  int32_t reserved;
} ts_rexpert_labels_in;

int32_t ts_rexpert_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_rexpert_last_hip_error(void);

/* 1 if both calls take these dims (ts_rollout_supported(dims, TS_ROLLOUT_RANDOM) and ts_rtable_supported(dims): S <= 8,
 * n_tiles <= 8, n_targets <= 8), 0 if the shape is beyond that, a negative ts_status for invalid dims (TS_ERR_NULL,
 * TS_ERR_DIMS).  Host only. */
int32_t ts_rexpert_supported(const ts_dims *dims);

/* One launch: k_rexpert_rollout<S>, one board per lane, no LDS.  Checked in this order, before any HIP call: dims (TS_ERR_NULL,
 * TS_ERR_DIMS, and TS_ERR_LIMIT for a size above 32 or more than 255 tiles or targets); cfg NULL (TS_ERR_NULL); an unsupported
 * shape (TS_ERR_LIMIT); a bad argument (TS_ERR_ARG: mode bits, steps outside 0 .. TS_ROLLOUT_MAX_STEPS, explore_threshold above
 * 2^32, n_rows < 0, slots no power of two in 2 .. 2^31); then n_boards = 0 and steps = 0 are TS_OK without a launch - nothing
 * is written and no pointer is looked at; then a missing pointer (TS_ERR_NULL: st, out, st->blk, st->step_count, st->done,
 * st->pos with tiles, st->init with tiles in TS_MODE_AUTORESET, st->tgt with targets, table or count with n_rows > 0, or
 * neither an output nor write_state).  Asynchronous on `stream`. */
int32_t ts_rexpert_rollout(const ts_dims *dims, const ts_state *st, const ts_rexpert_cfg *cfg, const ts_rollout_out *out, void *stream);

/* One launch: k_rexpert_labels<S>, ONE SAMPLE PER LANE: block (x, k) holds boards 256 x .. 256 x + 255 of step k.  (A board's K
 * samples are independent - each is five probes at addresses its own cells decide - so the launch offers K times the waves of
 * ts_traj_labels' deal of a board per lane to hide those probes behind; what that deal saves, one load of the level per board
 * instead of one per sample, is a few coalesced bytes beside five scattered 8-byte reads.)  Checked in this order, before any HIP
 * call: dims (as above); in or out NULL (TS_ERR_NULL); an unsupported shape (TS_ERR_LIMIT); a bad argument (TS_ERR_ARG: steps
 * outside 1 .. TS_ROLLOUT_MAX_STEPS, n_rows < 0, slots no power of two in 2 .. 2^31); then n_boards = 0 is TS_OK without a
 * launch; then a missing pointer (TS_ERR_NULL: st, st->blk, st->tgt with targets, first with tiles, pos_log with tiles and
 * steps > 1, table or count with n_rows > 0, no output at all).  Reads no state but blk and tgt and writes none. */
int32_t ts_rexpert_labels(const ts_dims *dims, const ts_state *st, const ts_rexpert_labels_in *in, const ts_labels_out *out, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_rexpert_desc {
  int32_t threads_per_block;
  int32_t lds_bytes; /* 0: neither kernel uses any */
  int64_t blocks;    /* grid size; 0 where nothing is launched (name is empty) */
  int64_t waves;     /* blocks * threads_per_block / 64 */
  int64_t samples;   /* steps * n_boards */
  int64_t bytes;     /* rollout: act_log + flags_log + pos_log that out_mask asks for; labels: the outputs of `what` */
  char name[64];     /* as rocprofv3 prints it, e.g. "k_rexpert_rollout<5>" */
} ts_rexpert_desc;
/* out_mask: TS_ROLLOUT_OUT_* bits.  dims, cfg or desc NULL is TS_ERR_NULL; then ts_rexpert_rollout's checks that need no
 * pointer of st / out, in its order. */
int32_t ts_describe_rexpert_rollout(const ts_dims *dims, const ts_rexpert_cfg *cfg, uint32_t out_mask, ts_rexpert_desc *desc);
/* what: TS_LABELS_OUT_* bits; bits beyond those, or none, give TS_ERR_ARG after steps.  dims or desc NULL is TS_ERR_NULL; then
 * dims, the shape (TS_ERR_LIMIT), steps, what. */
int32_t ts_describe_rexpert_labels(const ts_dims *dims, int32_t steps, uint32_t what, ts_rexpert_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_REXPERT_H */
