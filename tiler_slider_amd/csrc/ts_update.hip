// ts_update.hip — the in-place step: ts_step with the observation updated where it changes (include/tiler_slider_update.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_update.so): the step library is pinned symbol by
// symbol and kernel by kernel, and nothing here touches it.
//
// k_step_update<S, TMAX, U8>: ONE BOARD PER LANE, no LDS, no scratch, no barrier.  The lane loads its board - the level
// (obstacle bitboard, target cells, in auto-reset mode the initial cells), the dynamic state (tile cells, step counter, done
// latch), the action byte and the cells the observation displays (`shown`) - with every load issued before the first is
// consumed (rows past the tile / target count read the last row, results unused: a predicate per row costs a memory round
// trip per row, ts_rollout.hip; only the initial cells wait, for the done latches of the wave), plays one step with the arithmetic of ts_core.h in the order of k_small, and stores the state
// as ts_step does.  Tiles live in a register array of TMAX (2 or 8) walked by fully unrolled loops predicated on t < T (T is
// uniform, so the predicates are scalar branches); a board with two tiles and two targets takes a second, straight-line body
// of the two-tile kernels, where those predicates are constants.  Every row of the state is addressed from a base pointer in
// scalar registers and the lane's 32-bit offset in its block (profiles/update_requests.md has what each of these is worth).
//
// The observation is never written as a whole: for every cell a tile leaves or enters, the channel-1 value under the old
// cells (`shown`) and under the new ones is evaluated, and the new value is stored where they differ - one scattered 4-byte
// (float32) or 1-byte (uint8) store per changed cell.  Most boards store nothing or two cells.
//
// Who stores them.  In the eight-tile kernels every lane stores the cells of its own board: the 64 active lanes of one store
// instruction then address 64 different boards, no two of them inside one 64-byte piece, and every changed cell is a write
// request of its own into the L2.  In the two-tile kernels (both bodies, both observation types) a lane packs what its board
// has to store - at most four cells: per tile the cell it enters and the cell it leaves - into one descriptor word (ts_quad.h)
// and stores nothing itself.  Where the wave has reconverged, four passes follow: in pass j the four lanes of every quad take
// the descriptor of the quad's lane j by a quad-broadcast DPP move (v_mov_b32_dpp quad_perm:[j,j,j,j]: registers only, no LDS)
// and lane k of the quad stores slot k of it, so that the up to four stores of one board leave in one instruction, inside that
// board's 3 C elements.  Four store instructions per wave, as with per-lane stores; the same addresses and the same values.
#include "../../include/tiler_slider_update.h"
#include "ts_launch.h"
#include "ts_quad.h"

namespace {

using ts::kWave;
constexpr int kThreads = 256;  // four waves per block; waves never interact
constexpr int64_t kInfinityCacheBytes = 256ll << 20;

struct UArgs {
  uint8_t *pos, *shown;  // cell_t = uint8 (S <= 8)
  const uint8_t *init, *tgt;
  const uint32_t *blk;
  int32_t *step_count;
  uint8_t *done;
  const uint8_t *actions;
  uint8_t *flags;
  int32_t *reward;  // may be NULL
  float *obs;       // one of obs / obs_u8, by the kernel's U8
  uint8_t *obs_u8;
  int64_t N;
  int32_t T, Tt, mc, max_steps, autoreset;
};

// The scattered observation stores.  A plain store leaves the touched line dirty in the XCD's L2 until capacity evicts it or
// the kernel ends; an agent-scope store (sc1) is written through the L2 as it arrives.  Which one a kernel uses: kThrough below.
// -DTS_UPDATE_NO_PUT compiles the stores out: the time of everything else (profiles/update_requests.md).
// Who issues them.  The two-tile kernels: the four lanes of a quad, one slot each of one board's descriptor, board after board
// (the file comment).  -DTS_UPDATE_LANE_PUT builds them as the eight-tile kernels are built: every lane stores its own board's
// cells (profiles/update_requests.md, section 5, has the two side by side).
template <int TMAX>
#if defined(TS_UPDATE_LANE_PUT)
constexpr bool kQuadStore = false;
#else
constexpr bool kQuadStore = TMAX == 2;
#endif
// Which flavour.  Written through where a quad stores AND a board's observation is 192 bytes, three whole 64-byte pieces
// (float32 on 4x4 boards, uint8 on 8x8): the L1 merges a quad's stores per piece, a board's changed cells mostly share one
// (1.02 pieces for 1.74 cells at cfg1) and no other board stores into it, so the written-through piece is the one fabric
// write it was going to be anyway - and it leaves while the launch still runs instead of after its last wave.  Plain
// everywhere else: where boards share pieces (float32 5x5, uint8 4x4 and 5x5: slower written through), on the 768-byte
// float32 8x8 board (no gain) and where every lane stores its own board (the eight-tile kernels, -DTS_UPDATE_LANE_PUT: a
// fabric write per changed float).  us per step, plain twice | written through twice, 1,048,576 boards where no number is
// given (profiles/update_requests.md, section 6, has all rows):
//   <4, 2, false>  17.92 17.82 | 16.49 16.74    524,288: 10.56 10.58 |  9.43  9.43    <8, 2, true>  524,288: 10.48 10.45 |  9.15  9.15
//   <4, 2, true>   12.51 12.46 | 12.79 12.75    <5, 2, false>  37.56 37.58 | 37.76 37.59    <5, 2, true>  14.11 14.13 | 14.44 14.45
//   <8, 2, false>  524,288: 19.73 19.70 | 19.89 19.72
// -DTS_UPDATE_STORE_PLAIN gives every kernel the plain store back and -DTS_UPDATE_STORE_SC1 the written-through one.
// Measured and not shipped, each replacing the rule above (section 6): -DTS_UPDATE_SC1_FIRST=K written through in the blocks
// below gridDim.x / K and plain elsewhere, -DTS_UPDATE_SC1_LAST=K the same in the last gridDim.x / K blocks (uniform per block:
// the two flavours of a store behind a scalar branch), -DTS_UPDATE_NT a nontemporal store.
template <int S, int TMAX, bool U8>
#if defined(TS_UPDATE_STORE_PLAIN)
constexpr bool kThrough = false;
#elif defined(TS_UPDATE_STORE_SC1)
constexpr bool kThrough = true;
#else
constexpr bool kThrough = kQuadStore<TMAX> && S * S * 3 * (U8 ? 1 : 4) == 192;
#endif
// A priority schedule per wave.  The SIMD picks the next instruction by priority, then by age, and every wave runs at priority
// 0: a wave that has just entered - one latency-bound round trip of loads away from having work - loses every pick to the
// arithmetic and the store instructions of older waves.  Where kLoadsFirst holds, a wave raises its priority (s_setprio)
// behind its wave-uniform early return, issues its loads - in a resetting wave the initial cells too - and drops to 0 again
// where the two paths of the reset branch have rejoined: at any moment the waves in their load phase stand above the waves in
// their store phase.  Raise and drop are asm statements with a memory clobber, so no load or store moves across them.
// Which kernels: those with a measured row on which both readings with the schedule lie below both without it - the two-tile
// kernels of 4x4, 5x5 and 8x8 boards, both observation types, and <8, 8, false>.  No other kernel has a row; they keep their
// code.  us per step, without twice | with twice, 1,048,576 boards where no number is given (profiles/update_requests.md,
// section 7, has all rows, the bench line and the timeline):
//   <4, 2, false>  16.58 16.51 | 16.07 18.80 (one whole process in the slow state section 6 met with both trees; six more
//                  pairs: 16.49 .. 16.71 | 16.02 .. 16.12)    524,288: 9.42 9.42 | 9.26 9.26    786,432: 13.47 13.48 | 12.64 12.63
//   <4, 2, true>   12.45 12.41 | 12.34 12.27    <5, 2, false>  37.99 37.96 | 36.46 37.01    <5, 2, true>  14.13 14.12 | 13.98 13.94
//   <8, 2, true>   524,288:  9.16  9.16 |  8.79  8.81    <8, 2, false>  524,288: 19.66 19.66 | 19.24 19.43
//   <8, 8, false>  524,288: 45.88 45.50 | 45.11 45.03
// -DTS_UPDATE_PRIO_OFF: false everywhere (the parent's code, instruction for instruction); -DTS_UPDATE_PRIO_ALL: true in all 32
// kernels.  -DTS_UPDATE_PRIO_LEVEL=1|2|3 the raised level (no difference between them: 16.12, 16.12, 16.11); -DTS_UPDATE_PRIO_UNTIL=
// issued|loaded|store where the drop stands: behind the last load instruction, behind the wait for all loads (16.12: in
// auto-reset mode a wave has waited for its done latches by then in either form), or in front of the first observation
// store, so that the step runs raised as well (16.74 to 16.81: slower than no schedule); -DTS_UPDATE_PRIO_STORES the control:
// loads at 0, the raise in front of the first observation store and no drop (16.59 to 16.68: the parent's time).
template <int S, int TMAX, bool U8>
#if defined(TS_UPDATE_PRIO_OFF)
constexpr bool kLoadsFirst = false;
#elif defined(TS_UPDATE_PRIO_ALL)
constexpr bool kLoadsFirst = true;
#else
constexpr bool kLoadsFirst = (TMAX == 2 && (S == 4 || S == 5 || S == 8)) || (S == 8 && TMAX == 8 && !U8);
#endif
#if defined(TS_UPDATE_PRIO_LEVEL)
constexpr int kPrioLevel = TS_UPDATE_PRIO_LEVEL;
#else
constexpr int kPrioLevel = 1;
#endif
static_assert(kPrioLevel >= 1 && kPrioLevel <= 3, "s_setprio takes 0 .. 3, and 0 is where a wave starts");
enum PrioUntil { kUntil_issued, kUntil_loaded, kUntil_store };
#if defined(TS_UPDATE_PRIO_UNTIL)
#define TS_PRIO_PASTE_(a, b) a##b
#define TS_PRIO_PASTE(a, b) TS_PRIO_PASTE_(a, b)
constexpr PrioUntil kPrioUntil = TS_PRIO_PASTE(kUntil_, TS_UPDATE_PRIO_UNTIL);  // another word does not compile
#else
constexpr PrioUntil kPrioUntil = kUntil_issued;
#endif
#if defined(TS_UPDATE_PRIO_STORES)
constexpr bool kPrioStores = true;
#else
constexpr bool kPrioStores = false;
#endif
// The memory clobber holds loads and stores on their side.  The drop behind the loads is pinned against the arithmetic as well
// (a scheduling barrier on either side emits nothing): left alone, the scheduler lifts the first consumers of the loaded values,
// and with them the wait for every load, above it - and the drop behind the issue becomes a drop behind the return.
template <int LEVEL, bool PINNED = false>
__device__ __forceinline__ void set_prio() {
  if constexpr (PINNED) __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_setprio %0" ::"n"(LEVEL) : "memory");
  if constexpr (PINNED) __builtin_amdgcn_sched_barrier(0);
}
// In front of a wave's first observation store: the late drop, or the control's raise.
template <bool PRIO>
__device__ __forceinline__ void prio_at_first_store() {
  if constexpr (PRIO && kPrioStores) set_prio<kPrioLevel>();
  else if constexpr (PRIO && kPrioUntil == kUntil_store) set_prio<0>();
}

#if defined(TS_UPDATE_SC1_FIRST) || defined(TS_UPDATE_SC1_LAST)
__device__ __forceinline__ bool written_through() {
#if defined(TS_UPDATE_SC1_FIRST)
  return blockIdx.x < gridDim.x / (TS_UPDATE_SC1_FIRST);
#else
  return blockIdx.x >= gridDim.x - gridDim.x / (TS_UPDATE_SC1_LAST);
#endif
}
#endif
template <bool THROUGH, class P>
__device__ __forceinline__ void put(P *dst, uint32_t v) {
#if defined(TS_UPDATE_NO_PUT)
  (void)dst, (void)v;
#elif defined(TS_UPDATE_SC1_FIRST) || defined(TS_UPDATE_SC1_LAST)
  if (written_through()) __hip_atomic_store(dst, (P)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *dst = (P)v;
#elif defined(TS_UPDATE_NT)
  __builtin_nontemporal_store((P)v, dst);  // global_store_* ... nt
#else
  if constexpr (THROUGH) __hip_atomic_store(dst, (P)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_store_* ... sc1
  else *dst = (P)v;
#endif
}

// -DTS_UPDATE_TRACE=1: the timeline of one launch (tools/update_timeline.py).  Every wave stamps the 100 MHz clock at entry,
// when its loads have returned (the trace waits for them there, all at once), before its first observation store and after
// its last store instruction (=2: after that store is acknowledged), and its lane 0 writes the four stamps, the XCC id in the
// top byte of the last, into an array of the code object that ts_update_trace_read copies out.  Never in the shipped build.
#if defined(TS_UPDATE_TRACE)
constexpr uint32_t kTraceWaves = 16384;  // cfg1: 4,096 blocks of four waves; waves past it are not recorded
__device__ uint64_t g_trace[kTraceWaves * 4];
__device__ __forceinline__ uint64_t stamp() {
  asm volatile("" ::: "memory");
  const uint64_t t = wall_clock64();
  asm volatile("" ::: "memory");
  return t;
}
#endif

// Row `row` of a row-major [rows][N] array from board b0 on.  Everything here is uniform: the sum is scalar arithmetic, and
// an access at(row_from(...), lane) takes the pointer from scalar registers and a 32-bit offset from the lane.  The empty
// asm pins the pointer to a scalar register pair where it is formed: without it the compiler adds the lane's offset to the
// array first and the row's offset to that, in 64-bit vector arithmetic (v_mad_u64_u32, v_lshl_add_u64).
template <class P>
using global_ptr = __attribute__((address_space(1))) P *;  // the asm hides where the pointer came from: say it is global memory
template <class P>
__device__ __forceinline__ global_ptr<P> row_from(P *base, int row, int64_t N, int64_t b0) {
  global_ptr<P> p = (global_ptr<P>)(base + ((int64_t)row * N + b0));
  asm volatile("" : "+s"(p));
  return p;
}
// Element i (< 256) of such a row: the byte offset is formed in 32 bits, next to the access, so that the access takes the
// `offset register, scalar base` form in whichever basic block it lands (the asm keeps the offset from being shared as a
// 64-bit value across blocks, where the instruction selector no longer sees that it is a 32-bit one).
template <class P>
__device__ __forceinline__ __attribute__((address_space(1))) P &at(global_ptr<P> row, uint32_t i) {
  uint32_t bytes = i * (uint32_t)sizeof(P);
  asm volatile("" : "+v"(bytes));
  return *(global_ptr<P>)((global_ptr<char>)row + bytes);
}

// One board of one lane.  FULL: the board has as many tiles and targets as the lane keeps (T == MT == Tt == TMAX), so every
// `t < T` / `j < Tt` predicate, every min(t, T - 1) row select and the `Tt > 0` branch is a constant and the unrolled loops
// are straight-line code.  The colour mode, auto-reset and the reward stay uniform run-time branches in both bodies: each
// is a scalar compare in front of a few instructions, and each would double the code once more.
template <int S, int TMAX, bool U8, bool FULL>
__device__ __forceinline__ void step_update_body(const UArgs &a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr int C = BB::C;
  constexpr int MT = C < TMAX ? C : TMAX;  // tiles a lane keeps (T <= C)
  constexpr M kFull = C == 64 ? ~M(0) : (M(1) << (C & 63)) - 1;
  static_assert(!FULL || MT == TMAX, "the straight-line body is for boards that can hold TMAX tiles");

  const int64_t N = a.N;
  const int64_t b0 = (int64_t)blockIdx.x * kThreads;  // the block's first board (b0 < N: blocks == ceil(N / 256))
  const uint32_t tid = threadIdx.x;
  const uint32_t here = (uint32_t)min(N - b0, (int64_t)kThreads);  // boards of this block, 1 .. 256
  if ((tid & ~(uint32_t)(kWave - 1)) >= here) return;              // wave-uniform
  constexpr bool kPrio = kLoadsFirst<S, TMAX, U8>;
  if constexpr (kPrio && !kPrioStores) set_prio<kPrioLevel>();  // this wave's loads before whatever older waves have to issue
  // lanes past the batch play a copy of the LAST board and write nothing
  const bool live = tid < here;
  const uint32_t ll = live ? tid : here - 1;
  const int T = FULL ? MT : a.T, Tt = FULL ? TMAX : a.Tt;  // 1 <= T <= MT, Tt <= TMAX
  const bool mc = a.mc != 0, autoreset = a.autoreset != 0;
#if defined(TS_UPDATE_TRACE)
  const uint64_t t_entry = stamp();
#endif

  // ---- loads: all but the initial cells unconditional and issued before the first one is consumed ----
  M blk = at(row_from(a.blk, 0, N, b0), ll);
  if constexpr (BB::wide) blk |= (M)at(row_from(a.blk, 1, N, b0), ll) << 32;
  blk &= kFull;
  uint32_t p[MT], sh[MT], in[MT], tg[TMAX];  // p: the cells as they lie in memory (an id >= C stays until the board moves)
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    p[t] = at(row_from(a.pos, min(t, T - 1), N, b0), ll);
    sh[t] = at(row_from(a.shown, min(t, T - 1), N, b0), ll);
    in[t] = 0;
  }
#pragma unroll
  for (int j = 0; j < TMAX; ++j) tg[j] = 0;
  if (Tt > 0) {
#pragma unroll
    for (int j = 0; j < TMAX; ++j) tg[j] = at(row_from(a.tgt, min(j, Tt - 1), N, b0), ll);
  }
  int32_t sc = at(row_from(a.step_count, 0, N, b0), ll);
  uint32_t done = at(row_from(a.done, 0, N, b0), ll);
  const uint32_t act = at(row_from(a.actions, 0, N, b0), ll);
  // The initial cells only in a wave where some board resets (0.2 % of the board-steps of a long-episode batch, one wave in
  // eight): a second round trip there, two loads fewer everywhere else.
  if (autoreset && __ballot(done != 0) != 0) {  // wave-uniform
#pragma unroll
    for (int t = 0; t < MT; ++t) in[t] = at(row_from(a.init, min(t, T - 1), N, b0), ll);
  }
  if constexpr (kPrio && !kPrioStores && kPrioUntil != kUntil_store) {
    if constexpr (kPrioUntil == kUntil_loaded) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    set_prio<0, kPrioUntil == kUntil_issued>();  // every load is issued, the initial cells of a resetting wave among them
  }
#if defined(TS_UPDATE_TRACE)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uint64_t t_loaded = stamp();
#endif

  // ---- the step (environment.py:100-143), the order of k_small: done on entry, bad action, slide ----
  M tgm = 0, occ = 0;
  uint32_t pc[MT];
#pragma unroll
  for (int j = 0; j < TMAX; ++j) {
    tg[j] = min(tg[j], (uint32_t)(C - 1));
    if (j < Tt) tgm |= M(1) << tg[j];
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    pc[t] = min(p[t], (uint32_t)(C - 1));  // clamp: malformed ids stay in-board
    if (t < T) occ |= M(1) << pc[t];
  }
  const int dir = (int)(act & 3u);
  uint32_t q[MT];
  bool same = true, ordered = T == Tt;
  M occ2 = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    q[t] = pc[t];
    if (t < T) {
      q[t] = (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir);
      same &= q[t] == pc[t];
      ordered &= q[t] == tg[t];  // MT <= TMAX
      occ2 |= M(1) << q[t];
    }
  }
  const bool won = mc ? ordered : (occ2 == tgm);  // state.py:172-186
  uint32_t flags;
  bool touched = true;  // a board the step leaves untouched keeps every state byte
  uint32_t r[MT];       // the cells after the step, as they will lie in memory
  if (done) {           // environment.py:113-114
    flags = autoreset ? TS_FLAG_AUTORESET : TS_FLAG_STEPPED_DONE;
    touched = autoreset;
#pragma unroll
    for (int t = 0; t < MT; ++t) r[t] = autoreset ? min(in[t], (uint32_t)(C - 1)) : p[t];
    if (autoreset) sc = 0, done = 0;
  } else if (act > 3u) {  // environment.py:116-117
    flags = TS_FLAG_BAD_ACTION;
    touched = false;
#pragma unroll
    for (int t = 0; t < MT; ++t) r[t] = p[t];
  } else {
    flags = (won ? (TS_FLAG_IS_WON | TS_FLAG_SUCCESS) : 0u) | (same ? TS_FLAG_INVALID_MOVE : 0u);
    sc += 1;
    done = won ? 1u : 0u;
    if (sc >= a.max_steps) {
      done = 1u;
      flags |= TS_FLAG_TIMEOUT;
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) r[t] = q[t];
  }
#if defined(TS_UPDATE_ARITH_TWICE)
  // Ablation (profiles/update_requests.md): the slides once more, on operands the compiler cannot tell from the first ones,
  // and both results alive up to the flag store.  The bit is never set: the two results are equal.
  {
    M occ_b = occ, blk_b = blk;
    asm volatile("" : "+v"(occ_b), "+v"(blk_b));
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      if (t < T) {
        uint32_t pb = pc[t];
        asm volatile("" : "+v"(pb));
        if ((uint32_t)ts::slide_cell<S>((int)pb, occ_b, blk_b, dir) != q[t]) flags |= 0x80u;
      }
    }
  }
#endif

  // ---- the observation delta: old cells = shown, new cells = r, both clamped as the encoder clamps ----
  uint32_t o[MT], c[MT];
  M occ_new = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    o[t] = min(sh[t], (uint32_t)(C - 1));
    c[t] = min(r[t], (uint32_t)(C - 1));
    if (t < T) occ_new |= M(1) << c[t];
  }
  using obs_t = typename std::conditional<U8, uint8_t, float>::type;
  obs_t *block_obs;  // the block's first board: a uniform pointer
  if constexpr (U8) block_obs = a.obs_u8 + b0 * (C * 3);
  else block_obs = a.obs + b0 * (C * 3);
  const uint32_t mine = tid * (uint32_t)(C * 3) + 1u;  // channel 1 of cell 0 of this board, from block_obs
#if defined(TS_UPDATE_TRACE)
  uint64_t t_store = 0;
  if constexpr (!kQuadStore<TMAX>) t_store = stamp();  // the per-lane stores begin in the loop below
#endif
  if constexpr (!kQuadStore<TMAX>) prio_at_first_store<kPrio>();
  uint32_t word = 0;                                   // kQuadStore: what this board has to store (ts_quad.h)
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t < T) {
      // the cell tile t stands on: the highest index on it wins, before and after (ascending u: the last match stays)
      uint32_t nv = 0, ov = 0;
#pragma unroll
      for (int u = 0; u < MT; ++u) {
        if (u < T) {
          nv = c[u] == c[t] ? (uint32_t)(u + 1) : nv;
          ov = o[u] == c[t] ? (uint32_t)(u + 1) : ov;
        }
      }
      if (!mc) nv = nv ? 1u : 0u, ov = ov ? 1u : 0u;
      const bool enters = live && nv != ov;
      // the cell it was drawn on, where no tile stands any more (else `enters` stores that cell's value)
      const bool leaves = live && !((occ_new >> o[t]) & M(1));
      if constexpr (kQuadStore<TMAX>) {
        word |= ts::quad_word(ts::quad_slot(enters, c[t], nv), 2 * t) | ts::quad_word(ts::quad_slot(leaves, o[t], 0u), 2 * t + 1);
      } else {
        if (enters) put<kThrough<S, TMAX, U8>>(block_obs + (mine + 3u * c[t]), nv);
        if (leaves) put<kThrough<S, TMAX, U8>>(block_obs + (mine + 3u * o[t]), 0u);
      }
    }
  }
  if constexpr (kQuadStore<TMAX>) {
    // Every lane is active here (lanes past the batch carry a word of zero and store for the live boards of their quad).
    // Pass j: the quad's four lanes take the word of its lane j (v_mov_b32_dpp quad_perm:[j,j,j,j]: no LDS) and one slot each.
    const uint32_t quad = (tid & ~3u) * (uint32_t)(C * 3) + 1u;  // channel 1 of cell 0 of the quad's first board
    const uint32_t my_slot = tid & 3u;
    auto pass = [&](auto j) {  // j: a constant, the DPP control is an immediate
      const uint32_t theirs = (uint32_t)__builtin_amdgcn_mov_dpp((int)word, j * 0x55, 0xf, 0xf, true);
      const uint32_t slot = ts::quad_slot_of(theirs, my_slot);
      if (ts::quad_present(slot)) put<kThrough<S, TMAX, U8>>(block_obs + (quad + (uint32_t)(j * C * 3) + 3u * ts::quad_cell(slot)), ts::quad_value(slot));
    };
    static_assert(ts::kQuadSlots == 4, "one pass per lane of a quad");
#if defined(TS_UPDATE_TRACE)
    t_store = stamp();
#endif
    prio_at_first_store<kPrio>();
    pass(std::integral_constant<int, 0>{}), pass(std::integral_constant<int, 1>{});
    pass(std::integral_constant<int, 2>{}), pass(std::integral_constant<int, 3>{});
  }

  // ---- build-defined Manhattan reward of the cells after the step (include/tiler_slider.h: ts_reward) ----
  if (a.reward) {  // uniform
    auto manhattan = [](uint32_t x, uint32_t y) -> int {
      return abs((int)(x / S) - (int)(y / S)) + abs((int)(x % S) - (int)(y % S));
    };
    int sum = 0;
    if (mc) {
      const int m = T < Tt ? T : Tt;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < m) sum += manhattan(c[t], tg[t]);
    } else if (Tt > 0) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (t < T) {
          int best = 1 << 30;
#pragma unroll
          for (int j = 0; j < TMAX; ++j)
            if (j < Tt) best = min(best, manhattan(c[t], tg[j]));
          sum += best;
        }
      }
    }
    if (live) at(row_from(a.reward, 0, N, b0), tid) = -sum;
  }

  if (!live) return;
  // -DTS_UPDATE_STATE_ALWAYS: the state rows under `live` alone - every store skipped here would write the byte that is there,
  // and a row stored by all lanes of a wave is one whole 64-byte write (section 6: measured, not shipped).  A macro, not a
  // constant or'ed into the conditions: that form reordered instructions of the default build.
#if defined(TS_UPDATE_STATE_ALWAYS)
#define TS_UPDATE_STATE_IF(cond) (true)
#else
#define TS_UPDATE_STATE_IF(cond) (cond)
#endif
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t < T) {
      if (TS_UPDATE_STATE_IF(touched)) at(row_from(a.pos, t, N, b0), tid) = (uint8_t)r[t];
      if (TS_UPDATE_STATE_IF(r[t] != sh[t])) at(row_from(a.shown, t, N, b0), tid) = (uint8_t)r[t];
    }
  }
  if (TS_UPDATE_STATE_IF(touched)) {
    at(row_from(a.step_count, 0, N, b0), tid) = sc;
    at(row_from(a.done, 0, N, b0), tid) = (uint8_t)done;
  }
  at(row_from(a.flags, 0, N, b0), tid) = (uint8_t)flags;
#if defined(TS_UPDATE_KICK)
  // -DTS_UPDATE_KICK=K: in every K-th group of eight blocks (eight: one block per XCD under the round-robin dealing, which
  // only the speed depends on) lane 0 of wave 0 asks its L2 to write its dirty lines back and does not wait: the lines of
  // earlier blocks leave while later ones still compute.  No store changes (section 6: measured, not shipped).
  if (tid == 0 && (blockIdx.x >> 3) % (TS_UPDATE_KICK) == (TS_UPDATE_KICK) - 1) asm volatile("buffer_wbl2 sc1" ::: "memory");
#endif
#if defined(TS_UPDATE_TRACE)
  if (TS_UPDATE_TRACE >= 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uint64_t t_end = stamp();
  uint32_t xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  const uint32_t wave = blockIdx.x * (uint32_t)(kThreads / kWave) + tid / kWave;
  if (tid % kWave == 0 && wave < kTraceWaves) {
    uint64_t *w = g_trace + 4 * (size_t)wave;
    w[0] = t_entry, w[1] = t_loaded, w[2] = t_store, w[3] = (t_end & 0x00ffffffffffffffull) | ((uint64_t)(xcc & 15u) << 56);
  }
#endif
}

// The kernel chooses its body once, on a uniform condition (full_body of _update_cabi.py says the same).  Only the two-tile
// kernels have the straight-line body: unrolled over eight tiles without a branch it takes 89 to 108 registers where the
// general body takes 62 to 74, and the registers of a kernel are those of its larger body - three waves per SIMD fewer for
// every board the eight-tile kernels step, full or not.
template <int S, int TMAX, bool U8>
__global__ __launch_bounds__(kThreads) void k_step_update(const UArgs a) {
  if constexpr (TMAX == 2 && S * S >= TMAX) {
    if (a.T == TMAX && a.Tt == TMAX) return step_update_body<S, TMAX, U8, true>(a);
  }
  step_update_body<S, TMAX, U8, false>(a);
}

using Kernel = void (*)(const UArgs);

template <int TMAX, bool U8>
Kernel sized_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_step_update<s, TMAX, U8>; });
}
Kernel kernel_of(int S, int tmax, bool u8) {
  if (tmax == 2) return u8 ? sized_kernel<2, true>(S) : sized_kernel<2, false>(S);
  return u8 ? sized_kernel<8, true>(S) : sized_kernel<8, false>(S);
}

constexpr uint32_t kKnownOutputs = TS_OUT_OBS | TS_OUT_REWARD | TS_OUT_ONEHOT | TS_OUT_VALID | TS_OUT_OBS_U8 | TS_OUT_VALID4 | TS_OUT_FLAGS;

// dims have passed check_dims: the shape, then the outputs
int32_t check_supported(const ts_dims *d, uint32_t outputs) {
  if (d->size > TS_UPDATE_MAX_SIZE || d->n_tiles < 1 || d->n_tiles > TS_UPDATE_MAX_TILES || d->n_targets > TS_UPDATE_MAX_TILES) return TS_ERR_LIMIT;
  const bool f32 = (outputs & TS_OUT_OBS) != 0, u8 = (outputs & TS_OUT_OBS_U8) != 0;
  if ((outputs & ~kKnownOutputs) || (outputs & (TS_OUT_ONEHOT | TS_OUT_VALID | TS_OUT_VALID4)) || f32 == u8) return TS_ERR_ARG;
  return TS_OK;
}

struct Plan {
  Kernel kernel = nullptr;
  uint32_t blocks = 0;
  ts_launch_desc desc{};
};

// Every check of ts_step_update that needs no pointer, and the launch it would make; touches no device.
int32_t plan_update(const ts_dims *d, uint32_t outputs, Plan &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (const int32_t rc = check_supported(d, outputs); rc != TS_OK) return rc;
  const bool u8 = (outputs & TS_OUT_OBS_U8) != 0;
  const int tmax = (d->n_tiles <= 2 && d->n_targets <= 2) ? 2 : 8;
  ts_launch_desc &k = p.desc;
  k.kernel = TS_KERNEL_NONE;
  k.lanes_per_board = k.boards_per_lane = 1;
  k.boards_per_wave = kWave;
  k.tiles_per_lane = tmax;
  k.extras = (outputs & TS_OUT_REWARD) ? 1 : 0;
  k.xcd_piece = -1;
  k.waves_per_block = kThreads / kWave;
  k.output_bytes = k.resident_bytes = (int64_t)(u8 ? 3 : 12) * d->size * d->size * d->n_boards;
  k.out_of_cache = k.resident_bytes > kInfinityCacheBytes ? 1 : 0;
  if (d->n_boards == 0) return TS_OK;  // nothing is launched
  const int64_t blocks = (d->n_boards + kThreads - 1) / kThreads;
  p.kernel = kernel_of(d->size, tmax, u8);
  if (!p.kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  k.kernel = TS_KERNEL_UPDATE;
  k.blocks = blocks;
  snprintf(k.name, sizeof k.name, "k_step_update<%d, %d, %s>", d->size, tmax, u8 ? "true" : "false");
  return TS_OK;
}

uint32_t outputs_of(const ts_step_out *out) {
  return (out->obs ? TS_OUT_OBS : 0u) | (out->reward ? TS_OUT_REWARD : 0u) | (out->onehot ? TS_OUT_ONEHOT : 0u) |
         (out->valid ? TS_OUT_VALID : 0u) | (out->obs_u8 ? TS_OUT_OBS_U8 : 0u) | (out->valid4 ? TS_OUT_VALID4 : 0u) |
         (out->flags ? TS_OUT_FLAGS : 0u);
}

}  // namespace

extern "C" {

int32_t ts_update_abi_version(void) { return TS_UPDATE_ABI_VERSION; }
int32_t ts_update_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_update_supported(const ts_dims *dims, uint32_t outputs) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  return check_supported(dims, outputs);
}

int32_t ts_describe_step_update(const ts_dims *dims, uint32_t outputs, ts_launch_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  Plan p;
  if (const int32_t rc = plan_update(dims, outputs, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_step_update(const ts_dims *dims, const ts_state *st, const uint8_t *actions, uint32_t mode, const ts_step_out *out,
                       void *shown, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!out) return TS_ERR_NULL;
  Plan p;
  if (const int32_t rc = plan_update(dims, outputs_of(out), p); rc != TS_OK) return rc;
  if (mode & ~TS_MODE_AUTORESET) return TS_ERR_ARG;
  if (!p.kernel) return TS_OK;  // an empty batch: nothing to launch, no pointer is looked at
  const bool autoreset = (mode & TS_MODE_AUTORESET) != 0;
  if (!st || !st->pos || !st->blk || !st->step_count || !st->done || (autoreset && !st->init) || (dims->n_targets > 0 && !st->tgt) ||
      !actions || !out->flags || !shown)
    return TS_ERR_NULL;
  if ((((uintptr_t)out->obs) | ((uintptr_t)out->reward)) & 3u) return TS_ERR_ARG;
  UArgs a{};
  a.pos = static_cast<uint8_t *>(st->pos), a.shown = static_cast<uint8_t *>(shown);
  a.init = static_cast<const uint8_t *>(st->init), a.tgt = static_cast<const uint8_t *>(st->tgt);
  a.blk = st->blk, a.step_count = st->step_count, a.done = st->done, a.actions = actions;
  a.flags = out->flags, a.reward = out->reward, a.obs = out->obs, a.obs_u8 = out->obs_u8;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.max_steps = dims->max_steps, a.autoreset = autoreset ? 1 : 0;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

#if defined(TS_UPDATE_TRACE)
// The last launch's stamps, four per wave, up to `words` 64-bit words of them; the number copied, or a negative TS_ERR_*.
int64_t ts_update_trace_read(uint64_t *dst, int64_t words) {
  if (!dst || words < 0) return TS_ERR_NULL;
  const int64_t n = words < (int64_t)kTraceWaves * 4 ? words : (int64_t)kTraceWaves * 4;
  if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_trace), (size_t)n * sizeof(uint64_t)) != hipSuccess) return TS_ERR_HIP;
  return n;
}
#endif

}  // extern "C"
