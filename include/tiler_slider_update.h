/*
 * tiler_slider_update.h — C-ABI of the in-place step (lib/libtiler_slider_update.so).
 *
 * A ninth library beside the step, search, table, rollout, policy, train, targets and actor-critic libraries: it shares the data
 * layout, ts_dims, ts_state, ts_step_out and ts_status of tiler_slider.h (every pointer a DEVICE pointer owned by the caller,
 * `stream` a hipStream_t as void*, every call asynchronous, no allocation, no retained pointers) and has an ABI version of its
 * own.
 *
 * ts_step rewrites the whole observation [N][S][S][3] on every call.  Of its three channels, 0 (obstacles) and 2 (targets) are
 * level data that no step changes, not even an autoreset, and channel 1 (tiles) changes in at most 2 T cells.  A caller that
 * steps into the SAME observation buffer every time - VecTilerSliderEnv with one observation buffer does - therefore rewrites
 * values that are already there: 192 of the 212 bytes per board of a 4x4 step.  ts_step_update writes only the cells whose
 * channel-1 value changes.
 *
 * THE CONTRACT.  `shown` is cell_t [T][N] (uint8: S <= 8): the tile cells the observation buffer currently displays.
 *   on entry   out->obs (or out->obs_u8) holds exactly what ts_encode (ts_encode_u8) writes for this level with pos = shown
 *   on exit    it holds exactly what ts_encode writes for the state after the step, and shown == pos, byte for byte
 * Everything else ts_step writes - pos, step_count, done, flags, reward - is byte-identical to ts_step's for the same inputs in
 * both modes, with the flag algebra of tiler_slider.h (environment.py:100-143).  `shown` exists because the state may be edited
 * from outside between two steps: the kernel does not trust pos to be what is drawn.  Channels 0 and 2 are NEVER written, and
 * no byte of channel 1 whose value stays.  The caller establishes the contract with a full write (ts_reset, ts_encode) followed
 * by a copy of pos into shown, and re-establishes it the same way after writing the buffer by any other means.
 *
 * THE DELTA.  Old cells are shown[t], new cells the cells after the step, both clamped to S*S - 1 as the encoder clamps.  The
 * channel-1 value of a cell under a set of cells is "the highest tile index on it wins": t + 1 in multi-colour mode, 1
 * otherwise, 0 for a cell without a tile.  For every cell among the old and the new ones the value is evaluated under both
 * sets, and the NEW value is stored where the two differ.  Every store carries the cell's final value, so the duplicate stores
 * of a board agree and no store order is relied on.
 */
#ifndef TILER_SLIDER_UPDATE_H
#define TILER_SLIDER_UPDATE_H

#include "tiler_slider.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_UPDATE_ABI_VERSION 1
#define TS_UPDATE_MAX_SIZE 8  /* the board in one register */
#define TS_UPDATE_MAX_TILES 8 /* tiles and targets a lane keeps */

#define TS_KERNEL_UPDATE 6 /* ts_launch_desc.kernel of this library: k_step_update<S, TMAX, U8>, one board per lane */

int32_t ts_update_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_update_last_hip_error(void);

/* TS_OK where ts_step_update takes the shape and the outputs (TS_OUT_* bits of tiler_slider.h): S <= 8, 1 <= T <= 8, Tt <= 8,
 * exactly one of TS_OUT_OBS / TS_OUT_OBS_U8, TS_OUT_REWARD if wanted (TS_OUT_FLAGS is implied and may be given); TS_ERR_LIMIT
 * for another shape, TS_ERR_ARG for other outputs (one-hot planes, valid, valid4, both observations or none), and the status of
 * ts_check_dims for invalid dims.  Host only. */
int32_t ts_update_supported(const ts_dims *dims, uint32_t outputs);

/* ts_step with the observation updated in place (see above).  Checks, in this order and before any HIP call: dims, out
 * (TS_ERR_NULL), shape and outputs as ts_update_supported, mode bits (TS_ERR_ARG); then n_boards = 0 is TS_OK without a launch;
 * then a missing pointer (TS_ERR_NULL: st, st->pos, st->blk, st->step_count, st->done, st->init in autoreset mode, st->tgt where
 * there are targets, actions, out->flags, shown), then a float observation or a reward that is not 4-byte aligned (TS_ERR_ARG).
 * The launch-policy fields of dims are ignored.  One launch, no LDS. */
int32_t ts_step_update(const ts_dims *dims, const ts_state *st, const uint8_t *actions, uint32_t mode, const ts_step_out *out,
                       void *shown, void *stream);

/* What ts_step_update would launch for these outputs, in the record of ts_describe_launch: kernel = TS_KERNEL_UPDATE,
 * tiles_per_lane = TMAX, output_bytes = resident_bytes = the bytes of the observation buffer it keeps current, out_of_cache
 * by those bytes against the 256 MiB Infinity Cache, xcd_piece = -1.  Touches no device. */
int32_t ts_describe_step_update(const ts_dims *dims, uint32_t outputs, ts_launch_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_UPDATE_H */
