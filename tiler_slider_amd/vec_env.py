"""VecTilerSliderEnv — N independent Tiler-Slider boards stepped by one HIP kernel launch.

Same method names and return order as the reference's single-board environment
(ref: explainrl/environment/environment.py:14-194 TilerSliderEnv), batched:

    reset()              -> obs  float32 [N, S, S, 3]                      (environment.py:82-98)
    step(actions)        -> (obs, done bool [N], info)                     (environment.py:100-143)
    get_valid_moves()    -> bool [N, 4], column d = Move(d)                (environment.py:149-171)
    get_info()           -> dict                                           (environment.py:173-194)
    close()                                                                (environment.py:145-147)

PyTorch-ROCm tensors are the device buffers; all arithmetic happens in
csrc/ts_kernels.hip through the C-ABI of include/tiler_slider.h.  There is no CPU path.
"""
import ctypes as C
from collections.abc import Mapping

import numpy as np
import torch

from . import _cabi, _update_cabi
from .levels import blk_words, cell_dtype, pack_levels
from .moves import Move

_DONE_MSG = "Episode is done. Call reset() to start a new episode."  # environment.py:114


class StepInfo(Mapping):
    """The per-step info dict of the reference, as tensors, decoded lazily from the flag byte.

    Keys: is_won, invalid_move, success, timeout (bool [N]), step_count (int32 [N], the value
    BEFORE this step's increment, as in environment.py:128), plus the vector-env extras
    stepped_done, autoreset, bad_action and the raw `flags` byte.  Optional kernel outputs
    (reward, onehot, valid_moves) appear when the environment was built with them.

    Like the observation, the info of step k is a VIEW of the environment's own buffers: the
    next step() / reset() overwrites them, and an info object read afterwards reports the later
    step.  `info.snapshot()` returns a detached copy (a plain dict of cloned tensors) for
    callers that keep infos around, e.g. in a rollout buffer."""

    _BITS = {"is_won": _cabi.FLAG_IS_WON, "invalid_move": _cabi.FLAG_INVALID_MOVE, "success": _cabi.FLAG_SUCCESS,
             "timeout": _cabi.FLAG_TIMEOUT, "stepped_done": _cabi.FLAG_STEPPED_DONE,
             "autoreset": _cabi.FLAG_AUTORESET, "bad_action": _cabi.FLAG_BAD_ACTION}

    def __init__(self, flags, step_count, extras):
        self._flags, self._step_count, self._extras = flags, step_count, extras

    def __getitem__(self, key):
        if key == "flags":
            return self._flags
        if key in self._BITS:
            return (self._flags & self._BITS[key]) != 0
        if key == "step_count":
            frozen = _cabi.FLAG_STEPPED_DONE | _cabi.FLAG_AUTORESET | _cabi.FLAG_BAD_ACTION
            return self._step_count - ((self._flags & frozen) == 0).to(torch.int32)
        return self._extras[key]

    def __iter__(self):
        yield from ("is_won", "step_count", "invalid_move", "success", "timeout", "stepped_done", "autoreset",
                    "bad_action", "flags")
        yield from self._extras

    def __len__(self):
        return 9 + len(self._extras)

    def snapshot(self):
        """A dict of cloned tensors that the next step() cannot change."""
        frozen = StepInfo(self._flags.clone(), self._step_count.clone(), {k: v.clone() for k, v in self._extras.items()})
        return {k: frozen[k] for k in frozen}


class DistanceTable:
    """What VecTilerSliderEnv.build_table() returns: `dist` uint8 [L, (size * size) ** n_tiles] on the device, one row per level
    (include/tiler_slider_table.h: ts_table_build), and the shape it was built for - lookups refuse an environment of another."""

    def __init__(self, dist, size, n_tiles, n_targets, multi_color, max_depth):
        self.dist = dist
        self.size, self.n_tiles, self.n_targets, self.multi_color = int(size), int(n_tiles), int(n_targets), bool(multi_color)
        self.max_depth = int(max_depth)
        self._complete = None

    @property
    def shape_key(self):
        return (self.size, self.n_tiles, self.n_targets, self.multi_color)

    @property
    def complete(self):
        """bool [L]: the row holds no TABLE_DEEP entry, so lookups on it are exactly solve()'s answers.  Computed on first use."""
        if self._complete is None:
            from ._table_cabi import TABLE_DEEP
            self._complete = ~(self.dist == TABLE_DEEP).any(dim=1)
        return self._complete

    def __len__(self):
        return self.dist.shape[0]


class StartInfo:
    """What VecTilerSliderEnv.place_at_distance() returns (include/tiler_slider_starts.h), device tensors of [N]: `count` int32, the
    placements of the board's row whose distance lies in its band; `dist` uint8, the distance of the placement the board was put
    on, 255 where it was not placed; `deepest` uint8, the largest distance of the row, 255 where it holds none; `placed` bool,
    dist != 255, computed on first use."""
    __slots__ = ("count", "dist", "deepest", "_placed")

    def __init__(self, count, dist, deepest):
        self.count, self.dist, self.deepest, self._placed = count, dist, deepest, None

    @property
    def placed(self):
        if self._placed is None:
            self._placed = self.dist != 255
        return self._placed

    def __iter__(self):
        return iter((self.count, self.dist, self.deepest, self.placed))

    def __repr__(self):
        return f"StartInfo(count, dist, deepest, placed: [{self.count.shape[0]}])"


class ReachResult:
    """What VecTilerSliderEnv.solve_reachable() returns (include/tiler_slider_reach.h), tensors of [N]: `moves` int16 - 0 for a won
    board, the least number of moves, SOLVE_NONE, SOLVE_DEPTH or SOLVE_FULL; `bits` uint8, bit a set where Move a starts a
    shortest solution, and `best` bool [N, 4], its columns (both None when not asked for); `states` int32, the number of states
    expanded; `expert` uint8, the lowest best move, 255 where there is none - step() takes it as it is."""
    __slots__ = ("moves", "bits", "states", "_best", "_expert")

    def __init__(self, moves, bits, states):
        self.moves, self.bits, self.states, self._best, self._expert = moves, bits, states, None, None

    @property
    def best(self):
        if self._best is None and self.bits is not None:
            self._best = _bit_columns(self.bits)
        return self._best

    @property
    def expert(self):
        if self.bits is None:
            raise ValueError("expert needs the best-move bits: solve_reachable(with_best=True)")
        if self._expert is None:
            lut = torch.tensor(VecTilerSliderEnv._LOWEST_MOVE, dtype=torch.uint8, device=self.bits.device)
            self._expert = lut[self.bits.to(torch.int64)]
        return self._expert

    def __repr__(self):
        return f"ReachResult(moves, best, bits, states: [{self.moves.shape[0]}])"


class ReachTable:
    """What VecTilerSliderEnv.build_reach_table() returns (include/tiler_slider_rtable.h), on the device: `table` int64 [L, slots], a
    hash table per level - a slot is 0 or bit 63 | the entry << 48 | the key, so an occupied slot is negative; `count` int32 [L],
    the states the level holds, or SOLVE_FULL; `root_moves` int16 [L], the optimum from the root; `deepest` int32 [L], the largest
    distance of the row; `capacity`, `max_depth`, `root` ("init" or "pos") and the shape it was built for - lookups refuse an
    environment of another.  Which slot a state lies in differs from build to build: compare tables by entries()."""

    def __init__(self, table, count, root_moves, deepest, capacity, size, n_tiles, n_targets, multi_color, max_depth, root):
        self.table, self.count, self.root_moves, self.deepest = table, count, root_moves, deepest
        self.capacity, self.max_depth, self.root = int(capacity), int(max_depth), root
        self.size, self.n_tiles, self.n_targets, self.multi_color = int(size), int(n_tiles), int(n_targets), bool(multi_color)
        self._full = None

    @property
    def shape_key(self):
        return (self.size, self.n_tiles, self.n_targets, self.multi_color)

    @property
    def slots(self):
        return self.table.shape[1]

    @property
    def full(self):
        """bool [L]: the level reaches more than `capacity` states; every lookup into it answers SOLVE_FULL."""
        if self._full is None:
            from ._reach_cabi import SOLVE_FULL
            self._full = self.count == SOLVE_FULL
        return self._full

    def entries(self, level):
        """(keys int64 [count] ascending, entries uint8 [count]) of one level: key = sum_t cell_t * (size * size) ** t, entry
        1 .. 252, TABLE_DEEP or TABLE_NONE.  Both empty for a FULL level: its row holds nothing to use."""
        row = self.table[level]
        if int(self.count[level]) < 0:
            row = row[:0]
        row = row[row < 0]
        keys, order = torch.sort(row & ((1 << 48) - 1))
        return keys, ((row >> 48) & 0xFF).to(torch.uint8)[order]

    def __len__(self):
        return self.table.shape[0]

    def __repr__(self):
        return f"ReachTable({len(self)} levels x {self.slots} slots, capacity {self.capacity}, root {self.root!r})"


class Rollout:
    """What VecTilerSliderEnv.rollout() returns: the reductions and logs of include/tiler_slider_rollout.h (ts_rollout_out) as
    device tensors, None where not asked for.  wins, finished, first_win, win_moves, reward_sum int32 [N]; flags uint8 [N] (the
    last step's); act_log, flags_log uint8 [steps, N]; pos_log cell ids [steps, T, N] (the compact form ts_encode re-encodes).
    rollout_policy() can also log logits_log float32 [steps, N, 4] (include/tiler_slider_policy.h) and start_pos, cell ids [T, N]:
    a copy of the cells taken before the launch (log "start"; with pos_log it is what trajectory_logits() reads).
    rollout_policy(expert=...) can also log what the expert's table answers on the board each step was chosen on
    (include/tiler_slider_mixed.h): expert_log uint8 [steps, N] its move (255: none), moves_log int16 [steps, N], best_log uint8
    [steps, N] - trajectory_labels()' action, moves and best - and who_log uint8 [steps, N]: 0 the network played, 1 the expert,
    2 the random draw."""

    FIELDS = ("wins", "finished", "first_win", "win_moves", "reward_sum", "flags", "act_log", "flags_log", "pos_log")
    MIXED_LOGS = ("expert_log", "moves_log", "best_log", "who_log")
    __slots__ = FIELDS + ("steps", "logits_log", "start_pos") + MIXED_LOGS

    def __init__(self, steps, **tensors):
        self.steps = int(steps)
        self.logits_log = tensors.get("logits_log")
        self.start_pos = tensors.get("start_pos")
        for name in self.MIXED_LOGS:
            setattr(self, name, tensors.get(name))
        for name in self.FIELDS:
            setattr(self, name, tensors.get(name))

    def __repr__(self):
        return f"Rollout(steps={self.steps}, " + ", ".join(n for n in self.FIELDS if getattr(self, n) is not None) + ")"


class VecTilerSliderEnv:
    """N boards of one shape (size, tile count, target count, multi_color) on one GPU."""

    def __init__(self, size, blocked_locations=None, initial_locations=None, target_locations=None,
                 multi_color=False, max_steps=100, *, device=None, strict=False, auto_reset=False,
                 with_reward=False, with_onehot=False, with_valid_moves=False, obs_dtype="float32",
                 host_mapped=False, obs_buffers=1, placement_trials=0, output_memory="contiguous", obs_candidates=None,
                 obs_update="auto"):
        """blocked/initial/target_locations: one list of (row, col) per board.

        strict      : raise the reference's RuntimeError when any board is stepped after done
                      (costs a device sync per step).  Default: such boards are left untouched
                      and flagged `stepped_done`.
        auto_reset  : boards that are done when step() is called are reset in place instead
                      (flag `autoreset`); their returned observation is the reset observation.
        obs_dtype   : "float32" = the reference's observation format (default); "uint8" = the
                      same values as bytes, a quarter of the memory traffic (every value of the
                      reference observation is an integer 0..255, so nothing is lost); None = the
                      environment keeps NO observation (ts_step_out.obs = NULL): reset() and step()
                      return None in its place, encode() still renders one on request.  For actors whose
                      consumer re-encodes from the cell ids (distributed.gather_compact_and_encode): the
                      step then moves the state bytes only - 1M 4x4 boards 6.8 us instead of 30.
        obs_buffers : number of observation buffers step() cycles through (default 1: every step
                      overwrites the same tensor).  With 2, the tensor returned by step k stays
                      intact while step k+1 runs, so a consumer on another stream — the RCCL
                      all-gather of tiler_slider_amd.distributed — can overlap with the next step.
        output_memory : where the large output buffers (observations, one-hot planes) live when they do not fit the 256 MiB
                      Infinity Cache.  "contiguous" (default): physically contiguous device memory
                      (hipExtMallocWithFlags(hipDeviceMallocContiguous)), falling back to torch's allocator when the
                      runtime cannot provide it.  "torch": torch's caching allocator.  A store pattern of many concurrent
                      streams - what the step kernels' waves produce - runs at one of two speeds on ordinary allocations,
                      up to 17 % apart, decided by the physical pages behind the buffer (different windows of ONE
                      allocation differ); contiguous memory has the same physical layout in every
                      process, so the step time is a property of the code: the library's launch policy is tuned on it
                      (cfg2 118 us, cfg4 107 us on every run; ordinary allocations give cfg2 112-134, cfg4 103-118).
                      Smaller outputs always come from torch's allocator.
        obs_candidates : environments that write TWO large streams per step (observation + one-hot planes, beyond the Infinity
                      Cache) run at one of two speeds even in physically contiguous memory - cfg2: 109 us or 118-119 us -
                      decided by where the OBSERVATION buffer lies (crossing the buffers of a fast and a slow environment:
                      profiles/r04_cross_probe.log; fast and slow regions of VRAM come in runs of several GiB:
                      r04_period_probe.log; single-stream launches - no one-hot - show no classes: r04_class_probe.log).
                      k > 1: the constructor allocates up to k candidate observation buffers (all alive, so that each lands
                      elsewhere), rates each with eleven launches of the real step kernel at the library's static policy,
                      keeps the fastest and frees the rest; it stops as soon as both classes have been seen (about 2 ms and
                      one observation buffer of transient memory per candidate, at most a quarter of the free memory and 4 GiB in
                      all - cfg2: 13 candidates; the launch policy is not touched, results never differ; every candidate freed
                      is a device-synchronising hipFree).  The step time is therefore a property of the BOX: cfg2 runs at
                      0.98 of the roofline where a fast region turns up and at 0.91 where none does.  None (default): 16 for such two-stream
                      environments (the fast class turned up within six candidates in 40 of 40 constructions between other
                      allocations of 0-6 GiB on one box, in none of 16 on another: r04_obs_candidates_robustness.log), 0
                      otherwise.  `observation_placement_report` holds the timings.
        placement_trials : opt-in measuring at construction, for buffers that are NOT contiguous (or to squeeze the last
                      per cent out of a given box).  0 (default): none - the library's static launch policy.  1: the
                      constructor rates a handful of launch policies (the per-call fields of ts_dims: resident blocks per
                      CU, write-back edge stores, lanes per board, XCD pieces) with the real step kernel on the buffers it
                      allocated - about 100 launches, state restored afterwards - and keeps one only if it beats the static
                      policy by 2 %; k > 1: the same for up to k candidate sets of output buffers, keeping the best set
                      (k times the output memory during construction).  No effect on results.  `placement_report` holds
                      the timings, the static policy's among them.
        obs_update  : how step() keeps the observation buffer current.  "full": every step rewrites the whole buffer (ts_step).
                      "auto" (default): where the in-place step takes the shape and the outputs (boards up to 8x8 with 1 .. 8
                      tiles and at most 8 targets, a float32 or uint8 observation, no one-hot planes, no legality mask:
                      include/tiler_slider_update.h), with obs_buffers = 1 and device buffers, and inside the domain that measured
                      faster (in_place_pays: from 786,432 boards on while the observation buffer fits the Infinity Cache - the
                      library's cache threshold, 256 MiB; beyond it from 524,288 boards on with at least 170 bytes of
                      observation per tile),
                      a step stores only the cells of the tile channel that change
                      (ts_step_update: 1M 4x4 boards 20.7 us instead of 30.2) - the obstacle and target
                      channels are level data that reset() wrote and no step changes.  The observation step() returns is
                      then THE ENVIRONMENT'S BUFFER, UPDATED IN PLACE: writing into it corrupts every later observation
                      until the next reset().  Clone it to change it, or pass obs_update="full".  "inplace": in place wherever the shape and the outputs allow it, whatever the
                      size of the buffer (ValueError elsewhere); for measurements (tools/update_ab.py).  Results never differ.
        host_mapped : keep every buffer in pinned host memory that the GPU reads and writes in
                      place (zero-copy).  For a handful of boards driven move by move from Python
                      (the one-board adapters): a step is then one launch plus one stream
                      synchronisation, with no device-to-host copies.  step() synchronises and
                      returns CPU tensors.  Pointless for large batches (every byte crosses PCIe).
        """
        n = len(initial_locations or [])
        blocked_locations = blocked_locations if blocked_locations is not None else [[] for _ in range(n)]
        target_locations = target_locations if target_locations is not None else [[] for _ in range(n)]
        blk, init, tgt = pack_levels(size, blocked_locations, initial_locations or [], target_locations)
        self._setup(size, blk, init, tgt, multi_color, max_steps, device, strict, auto_reset, with_reward,
                    with_onehot, with_valid_moves, obs_dtype, host_mapped, obs_buffers, placement_trials, output_memory, obs_candidates,
                    obs_update)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_arrays(cls, size, blk, init, tgt, multi_color=False, max_steps=100, **kw):
        """Packed level arrays (numpy or torch) in the device layout: blk [W,N] 32-bit words,
        init [T,N] and tgt [Tt,N] cell ids (uint8 up to 16x16; uint16 / torch.int16 above)."""
        validate = kw.pop("validate", False)
        self = cls.__new__(cls)
        self._setup(size, blk, init, tgt, multi_color, max_steps, kw.pop("device", None), kw.pop("strict", False),
                    kw.pop("auto_reset", False), kw.pop("with_reward", False), kw.pop("with_onehot", False),
                    kw.pop("with_valid_moves", False), kw.pop("obs_dtype", "float32"), kw.pop("host_mapped", False),
                    kw.pop("obs_buffers", 1), kw.pop("placement_trials", 0), kw.pop("output_memory", "contiguous"),
                    kw.pop("obs_candidates", None), kw.pop("obs_update", "auto"))
        if kw:
            raise TypeError(f"unexpected arguments {sorted(kw)}")
        if validate:
            self.validate_levels()
        return self

    def validate_levels(self):
        """Checks the preconditions the kernels rely on and pack_levels enforces for list input
        (include/tiler_slider.h): cell ids below S*S, tiles pairwise distinct, no tile on an
        obstacle.  The raw arrays of from_arrays() / the C-ABI skip them by default (the kernels
        clamp ids silently, and two tiles on one cell collapse where the reference would step the
        second one back, state.py:155-165).  One device sync; raises ValueError."""
        C_ = self.size * self.size
        init, tgt = self._init.to(torch.int64), self._tgt.to(torch.int64)
        for name, t in (("init", init), ("tgt", tgt)):
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= C_):
                raise ValueError(f"{name}: cell id outside 0..{C_ - 1}")
        if init.shape[0] > 1:
            srt = init.sort(dim=0).values
            dup = (srt[1:] == srt[:-1]).any(dim=0)
            if bool(dup.any()):
                raise ValueError(f"board {int(dup.nonzero()[0])}: two tiles on one cell")
        if init.numel():
            words = torch.gather(self._blk.to(torch.int64) & 0xffffffff, 0, init >> 5)
            hit = ((words >> (init & 31)) & 1).any(dim=0)
            if bool(hit.any()):
                raise ValueError(f"board {int(hit.nonzero()[0])}: a tile on a blocked cell")

    @classmethod
    def from_levels(cls, levels, max_steps=100, **kw):
        """A list of level records (ref: environment.py:61-80 from_level, one per board)."""
        levels = list(levels)
        if not levels:
            raise ValueError("from_levels needs at least one level")
        size, mc = levels[0].size, bool(levels[0].multiple_colors)
        if any(l.size != size or bool(l.multiple_colors) != mc for l in levels):
            raise ValueError("all levels of a batch must share size and multiple_colors")
        return cls(size, [l.blocked_locations for l in levels], [l.initial_locations for l in levels],
                   [l.target_locations for l in levels], multi_color=mc, max_steps=max_steps, **kw)

    @classmethod
    def random(cls, n_boards, size=5, num_tiles=2, num_obstacles=3, seed=0, multi_color=False, max_steps=100,
               board_offset=0, **kw):
        """Random levels generated ON THE DEVICE with the distribution of the reference factory
        (ref: environment.py:202-234): obstacles, tiles and targets on distinct uniformly random
        cells.  Board n is a pure function of (seed, board_offset + n)."""
        device = _resolve_device(kw.get("device"))
        W = blk_words(size)
        blk = torch.zeros((W, n_boards), dtype=torch.int32, device=device)
        init = torch.zeros((num_tiles, n_boards), dtype=_cell_torch_dtype(size), device=device)
        tgt = torch.zeros((num_tiles, n_boards), dtype=_cell_torch_dtype(size), device=device)
        dims = _cabi.Dims(n_boards, size, num_tiles, num_tiles, int(bool(multi_color)), max_steps, 0)
        st = _cabi.State(None, init.data_ptr(), tgt.data_ptr(), blk.data_ptr(), None, None, None)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _cabi.check(_cabi.lib().ts_generate(C.byref(dims), C.byref(st), C.c_uint64(seed & (2**64 - 1)),
                                                board_offset, num_obstacles, stream), "ts_generate")
        return cls.from_arrays(size, blk, init, tgt, multi_color=multi_color, max_steps=max_steps, **kw)

    @classmethod
    def from_seeds(cls, seeds, size=5, num_tiles=2, num_obstacles=3, multi_color=False, max_steps=100, **kw):
        """One board per seed: the level TilerSliderEnvFactory.create_simple_env(size, num_tiles,
        num_obstacles, seed) of the reference builds (ref: environment.py:217-226), bit for bit,
        generated on the device (include/tiler_slider.h: ts_generate_mt19937)."""
        device = _resolve_device(kw.get("device"))
        if isinstance(seeds, torch.Tensor):
            sd = seeds.detach().to("cpu", torch.int64).numpy()
        else:
            sd = np.asarray(seeds, dtype=np.int64 if not isinstance(seeds, np.ndarray) or seeds.dtype.kind == "i" else seeds.dtype)
        sd = sd.astype(np.int64).reshape(-1)
        if sd.size and (sd.min() < 0 or sd.max() > 2**32 - 1):
            raise ValueError("Seed must be between 0 and 2**32 - 1")  # numpy's own message for np.random.seed
        n_boards = int(sd.size)
        seeds_dev = torch.from_numpy(sd.astype(np.uint32).view(np.int32)).to(device)
        W = blk_words(size)
        blk = torch.zeros((W, n_boards), dtype=torch.int32, device=device)
        init = torch.zeros((num_tiles, n_boards), dtype=_cell_torch_dtype(size), device=device)
        tgt = torch.zeros((num_tiles, n_boards), dtype=_cell_torch_dtype(size), device=device)
        dims = _cabi.Dims(n_boards, size, num_tiles, num_tiles, int(bool(multi_color)), max_steps, 0)
        st = _cabi.State(None, init.data_ptr() if init.numel() else None, tgt.data_ptr() if tgt.numel() else None,
                         blk.data_ptr() if blk.numel() else None, None, None, None)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _cabi.check(_cabi.lib().ts_generate_mt19937(C.byref(dims), C.byref(st), seeds_dev.data_ptr() if n_boards else None,
                                                        num_obstacles, stream), "ts_generate_mt19937")
        return cls.from_arrays(size, blk, init, tgt, multi_color=multi_color, max_steps=max_steps, **kw)

    # ------------------------------------------------------------------ setup
    def _setup(self, size, blk, init, tgt, multi_color, max_steps, device, strict, auto_reset, with_reward,
               with_onehot, with_valid_moves, obs_dtype="float32", host_mapped=False, obs_buffers=1, placement_trials=0,
               output_memory="contiguous", obs_candidates=None, obs_update="auto"):
        L = _cabi.lib()  # raises when the HIP library is missing: no fallback
        self._fns = {}
        self.device = _resolve_device(device)
        self.host_mapped = bool(host_mapped)
        self.size, self.multi_color, self.max_steps = int(size), bool(multi_color), int(max_steps)
        self.strict, self.auto_reset = bool(strict), bool(auto_reset)
        self._blk = self._place(_to_device(blk, torch.int32, "cpu" if self.host_mapped else self.device))
        self._init = self._place(_to_device(init, _cell_torch_dtype(self.size), "cpu" if self.host_mapped else self.device))
        self._tgt = self._place(_to_device(tgt, _cell_torch_dtype(self.size), "cpu" if self.host_mapped else self.device))
        W = blk_words(self.size)
        if self._blk.dim() != 2 or self._blk.shape[0] != W:
            raise ValueError(f"blk must have shape [{W}, N]")
        self.num_envs = N = self._blk.shape[1]
        if self._init.dim() != 2 or self._tgt.dim() != 2 or self._init.shape[1] != N or self._tgt.shape[1] != N:
            raise ValueError("init / tgt must have shape [T, N] / [Tt, N]")
        self.n_tiles, self.n_targets = self._init.shape[0], self._tgt.shape[0]
        self._dims = _cabi.Dims(N, self.size, self.n_tiles, self.n_targets, int(self.multi_color), self.max_steps, 0)
        _cabi.check(L.ts_check_dims(C.byref(self._dims)), "VecTilerSliderEnv")
        self._pos = self._place(self._init.clone())
        self._step_count = self._zeros(N, torch.int32)
        self._done = self._zeros(N, torch.uint8)
        self._flags = self._zeros(N, torch.uint8)
        self._actions = self._zeros(N, torch.uint8)
        obs_dtype = {"float32": torch.float32, "uint8": torch.uint8, "none": None}.get(obs_dtype, obs_dtype)
        if obs_dtype not in (torch.float32, torch.uint8, None):
            raise ValueError("obs_dtype must be 'float32', 'uint8' or None")
        self.obs_dtype = obs_dtype
        if int(obs_buffers) < 1:
            raise ValueError("obs_buffers must be >= 1")
        if obs_dtype is None and int(obs_buffers) != 1:
            raise ValueError("obs_buffers needs an observation (obs_dtype=None keeps none)")
        if output_memory not in ("torch", "contiguous"):
            raise ValueError("output_memory must be 'torch' or 'contiguous'")
        self.output_memory = output_memory
        # what one step writes into the large outputs: beyond the Infinity Cache the kernels take their out-of-cache forms,
        # and the buffers come from physically contiguous memory (output_memory)
        self.onehot_channels = L.ts_onehot_channels(C.byref(self._dims))
        obs_bytes = {torch.float32: 12, torch.uint8: 3, None: 0}[obs_dtype] * self.size * self.size
        per_board = obs_bytes + (4 * self.onehot_channels * self.size * self.size if with_onehot else 0)
        # Successive steps cycle through the observation ring, so what has to stay resident between two writes of one buffer is
        # the WHOLE ring (+ the planes): a ring of two 201-MB buffers is a 402-MB working set, and the cache-resident launch
        # forms (agent-scope stores) are the wrong ones for it - 39.4 us per step against 32.3 with the out-of-cache forms at
        # 1M 4x4 boards, 30.2 with a single buffer (profiles/r05_ring_probe.log).  ts_dims.ring_bytes tells the library.
        ring_bytes = (obs_bytes * int(obs_buffers) + (per_board - obs_bytes)) * N
        self._dims.ring_bytes = ring_bytes if int(obs_buffers) > 1 else 0
        self._outputs_beyond_cache = max(per_board * N, self._dims.ring_bytes) > self._PLACEMENT_MIN_BYTES
        self.output_memory_report = []  # one entry per large output buffer: where it was actually allocated (see _big_zeros)
        self._obs_ring = [self._big_zeros((N, self.size, self.size, 3), obs_dtype) if obs_dtype is not None else None
                          for _ in range(int(obs_buffers))]
        self._obs_slot = 0
        self._obs = self._obs_ring[0]  # always the buffer the latest reset() / step() wrote
        self._reward = self._zeros(N, torch.int32) if with_reward else None
        self._onehot = (self._big_zeros((N, self.onehot_channels, self.size, self.size), torch.float32)
                        if with_onehot else None)
        self._valid = self._zeros(N, torch.uint8) if with_valid_moves else None
        # the same mask in the reference's shape, written by the step kernel itself: uint8 [N, 4] of 0 / 1, viewed as bool
        self._valid4 = self._zeros((N, 4), torch.uint8) if with_valid_moves else None
        # per-level tables of the large-board kernel (include/tiler_slider.h: ts_prepare): the level
        # never changes during an episode, so they are built once, here
        lw = L.ts_lines_words(self.size)
        self._lines = self._zeros((N, lw), torch.int32) if lw and N else None
        self._state = _cabi.State(_ptr(self._pos), _ptr(self._init), _ptr(self._tgt), _ptr(self._blk),
                                  _ptr(self._step_count), _ptr(self._done), None)
        if self._lines is not None:
            self._call("ts_prepare", C.byref(self._dims), C.byref(self._state), _ptr(self._lines))
            self._state.lines = _ptr(self._lines)
        self._mode = _cabi.MODE_AUTORESET if self.auto_reset else _cabi.MODE_STRICT
        self._bind_outputs()
        self._setup_obs_update(obs_update)
        self.placement_report = self.observation_placement_report = None
        if obs_candidates is None:  # two large output streams: the observation buffer's place decides between two speeds
            obs_candidates = 16 if (self._onehot is not None and self.obs_dtype is not None and self._outputs_beyond_cache and not self.host_mapped) else 0
        # (both rate the full-write kernel: nothing to choose for an environment that steps in place)
        if int(obs_candidates) > 1 and not self._in_place:
            self._choose_observation_buffers(int(obs_candidates))
        if int(placement_trials) >= 1:
            if self._in_place:
                self.placement_report = {"skipped": "steps in place"}
            else:
                self._tune_placement(int(placement_trials))
        self.observation_shape = (self.size, self.size, 3)  # per board, environment.py:59
        self._started = False
        self._closed = False

    def _bind_outputs(self):
        f32 = self.obs_dtype == torch.float32
        self._outs = [_cabi.StepOut(_ptr(self._flags), _ptr(o) if f32 else None, _ptr(self._reward),
                                    _ptr(self._onehot), _ptr(self._valid), None if f32 else _ptr(o), _ptr(self._valid4))
                      for o in self._obs_ring]  # (obs_dtype None: both observation pointers NULL)
        self._obs_slot = 0
        self._obs = self._obs_ring[0]
        self._out = self._outs[0]

    def _setup_obs_update(self, obs_update):
        """obs_update of the constructor: does step() go through ts_step_update?  `_shown` [T, N] holds the cells the observation
        buffer displays (include/tiler_slider_update.h); `_obs_current` says that buffer and `_shown` agree - a full write
        (reset(), or the first step of an environment that was never reset) followed by _sync_shown() makes it so."""
        if obs_update not in ("auto", "full", "inplace"):
            raise ValueError("obs_update must be 'auto', 'full' or 'inplace'")
        self.obs_update = obs_update
        self._in_place, self._shown, self._obs_current = False, None, False
        if obs_update == "full":
            return
        f32 = self.obs_dtype == torch.float32
        outputs = ((_cabi.OUT_OBS if f32 else 0) | (_cabi.OUT_OBS_U8 if self.obs_dtype == torch.uint8 else 0)
                   | (_cabi.OUT_REWARD if self._reward is not None else 0) | (_cabi.OUT_ONEHOT if self._onehot is not None else 0)
                   | (_cabi.OUT_VALID | _cabi.OUT_VALID4 if self._valid is not None else 0))
        able = (self.num_envs > 0 and len(self._obs_ring) == 1 and not self.host_mapped
                and _update_cabi.update_supported(self._dims, outputs))
        if obs_update == "inplace" and not able:
            raise ValueError("obs_update='inplace' needs boards up to 8x8 with 1 .. 8 tiles and at most 8 targets, one float32 or uint8 "
                             "observation buffer in device memory, and neither one-hot planes nor the legality mask")
        obs_bytes = self._obs.numel() * self._obs.element_size() if self._obs is not None else 0
        self._in_place = able and (obs_update == "inplace" or self.in_place_pays(obs_bytes, self.num_envs, self.n_tiles))
        if self._in_place:
            self._shown = torch.empty_like(self._pos)
            self._dims.step_in_place = True  # _cabi.describe_launch(dims, OP_STEP, ...) then names the kernel that runs

    _IN_PLACE_MIN_BOARDS = 3 << 18         # 786,432: inside the cache
    _IN_PLACE_MIN_BOARDS_BEYOND = 1 << 19  # 524,288: beyond it
    _IN_PLACE_BYTES_PER_TILE = 170

    @classmethod
    def in_place_pays(cls, obs_bytes, n_boards, n_tiles):
        """The domain of obs_update="auto", as measured (profiles/update_ab.log; us per step in place / full).
        INSIDE the Infinity Cache - the threshold the full-write kernels switch their own launch forms by - 4x4 boards with 2
        tiles: up to 131,072 boards both paths sit at the launch floor (6.1 / 6.3); 262,144 boards 6.8 / 9.6, 524,288 boards
        12.0 / 16.6, 786,432 boards 15.9 / 23.0, 1,048,576 boards 20.6 / 30.2.  In place is taken from 786,432 boards on: up to
        524,288 boards default environments keep the full-write kernels, which tests/test_kernel_instantiations.py reaches
        through env.step and asserts by name.  BEYOND the cache every scattered store becomes a partial-line write to HBM and
        costs about a whole line at ~5 TB/s against a full write streaming at ~7 TB/s, 0.95 stores per tile and step: in
        place pays where a board has at least 128 x 0.95 x 7 / 5 = 170 bytes of observation per tile.  8x8 boards with 4 tiles
        (192 B per tile; 524,288 boards, 384 MiB) 47.7 / 56.8; 5x5 with 2 tiles (150 B per tile, 300 MiB) 47.4 / 44.4; 4x4 with
        2 tiles (96 B per tile) 201 / 116 at 768 MiB and 878 / 638 at 3 GiB.  That branch rests on one winning shape."""
        if obs_bytes <= _cabi.lib().ts_tuning(_cabi.TUNE_NT_THRESHOLD_BYTES, -1):
            return n_boards >= cls._IN_PLACE_MIN_BOARDS
        return n_boards >= cls._IN_PLACE_MIN_BOARDS_BEYOND and obs_bytes // n_boards >= cls._IN_PLACE_BYTES_PER_TILE * n_tiles

    def _sync_shown(self, stream=None):
        """After a full write of the observation buffer from the current cells: the buffer displays `pos`."""
        if self._in_place:
            if stream is None:
                self._shown.copy_(self._pos)
            else:
                with torch.cuda.stream(stream):
                    self._shown.copy_(self._pos)
            self._obs_current = True

    def _choose_observation_buffers(self, k):
        """`obs_candidates=k`: per slot of the observation ring, the fastest of up to k candidate buffers (see the constructor)."""
        if self.host_mapped or self.num_envs == 0 or not self._outputs_beyond_cache or self.obs_dtype is None:
            self.observation_placement_report = {"skipped": "outputs fit the Infinity Cache" if not self.host_mapped else "host-mapped"}
            return
        N, L = self.num_envs, _cabi.lib()
        with torch.cuda.device(self.device):
            free, _ = torch.cuda.mem_get_info()
        # (Keeping the candidates apart with unused allocations in between - 1.2 GiB, or 1 / 2 / 4 / 8 GiB in turn - finds the
        # fast class LESS often than candidates that follow each other directly: 16 and 19 of 20 constructions against 20 of
        # 20, profiles/r04_obs_candidates_robustness.log.)
        # transient memory: at most a quarter of what is free AND at most _CANDIDATE_MAX_BYTES (4 GiB) in all - on a 288-GB part
        # "a quarter of free memory" alone would let sixteen candidates of a large batch take tens of GB
        one = max(self._obs_ring[0].numel() * self._obs_ring[0].element_size(), 1)
        k = max(1, min(k, int(free * 0.25 // one), int(self._CANDIDATE_MAX_BYTES // one)))
        saved = (self._pos.clone(), self._step_count.clone(), self._done.clone(), self._flags.clone())
        acts = self._empty(N, torch.uint8)
        self._call("ts_fill_actions", N, C.c_uint64(0xAC710005), 0, 0, _ptr(acts))
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        report = []

        def rate(out):
            for i in range(11):
                if i == 3:
                    ev0.record()
                _cabi.check(L.ts_step(C.byref(self._dims), C.byref(self._state), _ptr(acts), _cabi.MODE_AUTORESET, C.byref(out), stream), "ts_step")
            ev1.record()
            ev1.synchronize()
            return ev0.elapsed_time(ev1) * 1e3 / 8

        original = list(self._obs_ring)
        try:
            with torch.cuda.device(self.device):
                # Clocks up before the first rating counts (a cold first rating reads 3-4 % slow and would pass for the slow
                # class) - but only as long as the clock is still rising: the first buffer is rated again and again until two
                # consecutive ratings no longer improve by 1 % (two ratings when the GPU is warm; at most ~35 ms of load).
                prev, settled, warmup_ratings = rate(self._outs[0]), 0, 1
                while settled < 2 and warmup_ratings < 30:
                    cur = rate(self._outs[0])
                    settled = settled + 1 if cur >= prev * 0.99 else 0
                    prev, warmup_ratings = cur, warmup_ratings + 1
                for slot in range(len(self._obs_ring)):
                    cands, times = [self._obs_ring[slot]], []
                    for c in range(k):
                        if c:
                            cands.append(self._big_zeros(tuple(cands[0].shape), cands[0].dtype))
                        self._obs_ring[slot] = cands[c]
                        self._bind_outputs()
                        times.append(rate(self._outs[slot]))
                        # both classes seen: the fastest so far is of the fast kind, stop looking
                        if len(times) >= 2 and max(times) >= min(times) * 1.035:
                            break
                    best = min(range(len(times)), key=times.__getitem__)
                    self._obs_ring[slot] = cands[best]
                    report.append({"us_per_step": [round(t, 2) for t in times], "chosen": best, "candidates_allowed": k,
                                   "clock_warmup_ratings": warmup_ratings})
                    del cands
        except BaseException:
            self._obs_ring = original
            raise
        finally:
            for o in self._obs_ring:
                o.zero_()
            if self._onehot is not None:
                self._onehot.zero_()
            self._pos.copy_(saved[0]), self._step_count.copy_(saved[1]), self._done.copy_(saved[2]), self._flags.copy_(saved[3])
            for t in (self._reward, self._valid, self._valid4):
                if t is not None:
                    t.zero_()
            self._bind_outputs()
        self.observation_placement_report = report

    # Beyond the Infinity Cache the step time depends on WHERE the large output buffers were allocated and, with that, on
    # the launch policy that suits them (resident blocks per CU, write-back edge stores, lanes per board): the same kernel
    # on the same data runs up to 20 % apart between allocations and boxes.  Nothing in the virtual
    # address tells them apart, so the constructor measures: a coordinate search over the per-call policy fields of
    # ts_dims on the real step kernel (~100 launches, state restored), and with placement_trials = k > 1 the same for up
    # to k candidate sets of output buffers, keeping the best.
    _PLACEMENT_MIN_BYTES = 256 << 20
    _CANDIDATE_MAX_BYTES = 4 << 30  # obs_candidates: transient memory of all candidate observation buffers together

    def _tune_placement(self, trials):
        N = self.num_envs
        out_bytes = sum(o.numel() * o.element_size() for o in self._obs_ring[:1] if o is not None)
        out_bytes += self._onehot.numel() * 4 if self._onehot is not None else 0
        if self.host_mapped or N == 0 or out_bytes <= self._PLACEMENT_MIN_BYTES:
            self.placement_report = {"skipped": "outputs fit the Infinity Cache" if not self.host_mapped else "host-mapped"}
            return
        set_bytes = sum(o.numel() * o.element_size() for o in self._obs_ring if o is not None) + (self._onehot.numel() * 4 if self._onehot is not None else 0)
        with torch.cuda.device(self.device):
            free, _ = torch.cuda.mem_get_info()
        trials = max(1, min(trials, 1 + int(free * 0.8 // max(set_bytes, 1))))
        L = _cabi.lib()
        saved = (self._pos.clone(), self._step_count.clone(), self._done.clone(), self._flags.clone())
        acts = self._empty(N, torch.uint8)
        self._call("ts_fill_actions", N, C.c_uint64(0xAC710005), 0, 0, _ptr(acts))
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        candidates, times, policies, policy_us = [(self._obs_ring, self._onehot)], [], [], []
        stream = torch.cuda.current_stream(self.device).cuda_stream
        d = self._dims

        def rate(policy):
            """us per step with ts_dims policy fields (launch_hint, emit_edges, lines_lanes); a set of buffers counts as its
            slowest member."""
            d.launch_hint, d.emit_edges, d.lines_lanes, d.xcd_piece = policy
            worst = 0.0
            for out in self._outs:
                for i in range(3):
                    _cabi.check(L.ts_step(C.byref(d), C.byref(self._state), _ptr(acts), _cabi.MODE_AUTORESET, C.byref(out), stream), "ts_step")
                ev0.record()
                for i in range(8):
                    _cabi.check(L.ts_step(C.byref(d), C.byref(self._state), _ptr(acts), _cabi.MODE_AUTORESET, C.byref(out), stream), "ts_step")
                ev1.record()
                ev1.synchronize()
                worst = max(worst, ev0.elapsed_time(ev1) * 1e3 / 8)
            return worst

        def search():
            """Coordinate search from the library's own policy (all fields 0): resident blocks per CU, then the edge stores, then
            (boards above 8x8) the lanes per board, then the block -> board-range mapping, then one refinement of the first."""
            seen = {}

            def best_of(cands):
                for c in cands:
                    if c not in seen:
                        seen[c] = rate(c)
                return min(cands, key=seen.__getitem__)

            cur = best_of([(h, 0, 0, 0) for h in (0, -2, 2, 4, 8)])
            cur = best_of([cur] + [(cur[0], e, 0, 0) for e in (1, 4)])
            if self.size > 8:
                cur = best_of([cur] + [(cur[0], cur[1], ln, 0) for ln in (4, 8, 16)])
            cur = best_of([cur] + [cur[:3] + (pc,) for pc in (1, 32, 64, 128)])  # 1 = one eighth of the batch per XCD
            cur = best_of([cur] + [(cur[0] + dh,) + cur[1:] for dh in (-1, 1, 2) if -8 <= cur[0] + dh <= 8])
            return cur, seen[cur], seen[(0, 0, 0, 0)]

        first = candidates[0]
        try:
            with torch.cuda.device(self.device):
                for k in range(trials):
                    if k:
                        candidates.append(([self._big_zeros(tuple(o.shape), o.dtype) if o is not None else None for o in self._obs_ring],
                                           self._big_zeros(tuple(self._onehot.shape), torch.float32) if self._onehot is not None else None))
                    self._obs_ring, self._onehot = candidates[k]
                    self._bind_outputs()
                    pol, us, base_us = search()
                    if us > base_us * 0.98:  # a non-zero policy must beat the static one by more than the noise of an 11-launch rating
                        pol, us = (0, 0, 0, 0), base_us
                    times.append(us), policies.append(pol), policy_us.append(base_us)
                    # two clearly separated speeds seen and the current one is of the fast kind: stop looking
                    if len(times) >= 2 and times[-1] <= min(times) * 1.02 and max(times) >= min(times) * 1.06:
                        break
            best = min(range(len(times)), key=times.__getitem__)
            chosen, policy = candidates[best], policies[best]
        except BaseException:
            chosen, policy = first, (0, 0, 0, 0)  # an exception in mid-search (OOM of a candidate, a failed launch): as constructed
            raise
        finally:
            # state, policy fields and output bindings are restored whatever happened
            self._obs_ring, self._onehot = chosen
            del candidates
            for o in self._obs_ring:
                if o is not None:
                    o.zero_()
            if self._onehot is not None:
                self._onehot.zero_()
            self._pos.copy_(saved[0]), self._step_count.copy_(saved[1]), self._done.copy_(saved[2]), self._flags.copy_(saved[3])
            for t in (self._reward, self._valid, self._valid4):
                if t is not None:
                    t.zero_()
            self._bind_outputs()
            d.launch_hint, d.emit_edges, d.lines_lanes, d.xcd_piece = policy
        self.placement_report = {"us_per_step": [round(t, 2) for t in times], "library_policy_us": [round(t, 2) for t in policy_us],
                                 "policy": [{"launch_hint": p[0], "emit_edges": p[1], "lines_lanes": p[2], "xcd_piece": p[3]} for p in policies],
                                 "launch_hint": [p[0] for p in policies], "chosen": best, "trials": len(times)}

    # buffers live on the GPU, or (host_mapped) in pinned host memory the GPU addresses directly
    def _pin(self, t):
        if not t.numel() or t.is_pinned():
            return t
        with torch.cuda.device(self.device):  # pin in the context of the GPU that will use it
            return t.pin_memory()

    def _zeros(self, shape, dtype):
        if self.host_mapped:
            return self._pin(torch.zeros(shape, dtype=dtype))
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def _big_zeros(self, shape, dtype):
        """Output buffers: beyond the Infinity Cache from physically contiguous memory (see `output_memory`)."""
        if not self.host_mapped and self.output_memory == "contiguous" and self._outputs_beyond_cache:
            t = _contiguous_zeros(tuple(shape), dtype, self.device)
            self.output_memory_report.append({"bytes": int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(),
                                              "memory": "contiguous" if t is not None else "torch (contiguous allocation refused)"})
            if t is not None:
                return t
        return self._zeros(shape, dtype)

    def _empty(self, shape, dtype):
        if self.host_mapped:
            return self._pin(torch.empty(shape, dtype=dtype))
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _place(self, t):
        return self._pin(t) if self.host_mapped else t

    def _sync_if_host(self):
        if self.host_mapped:
            torch.cuda.current_stream(self.device).synchronize()

    # ------------------------------------------------------------------ reference API
    def reset(self):
        """All boards back to their level's initial cells; returns the observation tensor."""
        self._require_open()
        if self.obs_dtype == torch.float32:
            self._call("ts_reset", C.byref(self._dims), C.byref(self._state), _ptr(self._obs))
        else:
            self._call("ts_reset", C.byref(self._dims), C.byref(self._state), None)
            if self.obs_dtype is not None:
                self._call("ts_encode_u8", C.byref(self._dims), C.byref(self._state), _ptr(self._obs))
        self._sync_shown()
        self._sync_if_host()
        self._started = True
        return self._obs

    def step(self, actions):
        """actions: uint8/int tensor [N] of Move values, a numpy array, or a list of Move.
        Returns (obs, done, info).  `obs` is the environment's own buffer, overwritten by the
        next step()/reset() — clone it to keep it.  Where the environment steps in place (obs_update:
        the default for large batches of small boards) the next step UPDATES that buffer instead of
        rewriting it: writing into it corrupts later observations - clone it, or construct with
        obs_update="full"."""
        self._require_open()
        if not self._started:
            raise RuntimeError("Call reset() before step().")
        act = self._stage_actions(actions)
        if self.strict and not self.auto_reset and bool(self._done.any()):
            raise RuntimeError(_DONE_MSG)
        self.step_async(act)
        self._sync_if_host()
        if self.strict and bool((self._flags & _cabi.FLAG_BAD_ACTION).any()):
            raise ValueError("actions must be Move values 0..3")  # state.py:43-45
        return self._obs, self._done.view(torch.bool), self._info()

    def step_async(self, act=None, stream=None):
        """The bare launch: one ts_step - or, where the environment steps in place (obs_update), one ts_step_update, which
        stores only the observation cells that change: the buffer is the environment's, do not write into it - on the current
        stream (or on `stream`, a torch.cuda.Stream), no validation, no sync.  `act` is a uint8 device tensor [N] (default: the
        env's own action buffer)."""
        a = self._actions if act is None else act
        if self._obs_current:  # in place (_mode stays what the rollout libraries read)
            if stream is None:
                self._call("ts_step_update", C.byref(self._dims), C.byref(self._state), a.data_ptr(), self._mode, C.byref(self._out),
                           self._shown.data_ptr(), binding=_update_cabi)
            else:
                _update_cabi.check(_update_cabi.lib().ts_step_update(C.byref(self._dims), C.byref(self._state), a.data_ptr(), self._mode,
                                                                     C.byref(self._out), self._shown.data_ptr(), stream.cuda_stream),
                                   "ts_step_update")
            return
        if len(self._obs_ring) > 1:  # next observation buffer: the previous one stays intact
            self._obs_slot = (self._obs_slot + 1) % len(self._obs_ring)
            self._obs, self._out = self._obs_ring[self._obs_slot], self._outs[self._obs_slot]
        if stream is None:
            self._call("ts_step", C.byref(self._dims), C.byref(self._state), a.data_ptr(), self._mode,
                       C.byref(self._out))
        else:  # no stream context switch from Python: the handle goes straight into the C-ABI
            _cabi.check(_cabi.lib().ts_step(C.byref(self._dims), C.byref(self._state), a.data_ptr(), self._mode,
                                            C.byref(self._out), stream.cuda_stream), "ts_step")
        self._sync_shown(stream)  # in place, never reset: this full write is what the following steps update

    def capture_steps(self, action_buffers):
        """Capture one ts_step per action buffer (uint8 device tensors [N], read at replay time)
        into a hipGraph and return it; `graph.replay()` then runs the whole sequence with one
        host call.  For small batches, where a step is shorter than a kernel launch from Python
        (4096 4x4 boards: ~5 us of kernel per ~8 us of launch), this removes the host from the
        loop; large batches are not launch-bound and gain nothing.  With obs_buffers = k the captured steps
        cycle through the k observation buffers like eager steps (pass a multiple of k action buffers)."""
        self._require_open()
        if self.host_mapped:
            raise ValueError("capture_steps needs device buffers (host_mapped=False)")
        bufs = [b for b in action_buffers]
        if len(bufs) % len(self._obs_ring):
            # the captured sequence rotates through the observation ring exactly as eager steps do; it must end on
            # the slot it started from, so that `_obs` names the last written buffer after every replay
            raise ValueError(f"capture_steps needs a multiple of obs_buffers={len(self._obs_ring)} action buffers")
        for b in bufs:
            if not (isinstance(b, torch.Tensor) and b.dtype == torch.uint8 and b.device == self.device
                    and b.shape == (self.num_envs,) and b.is_contiguous()):
                raise TypeError("action buffers must be contiguous uint8 device tensors of shape [N]")
        if self._in_place and not self._obs_current:
            # never reset: the full write that the in-place steps update happens now, not inside the graph - the buffer and
            # `_shown` then agree whether the next launch is a replay or an eager step
            self.encode(out=self._obs)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(self.device)
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                for b in bufs:
                    self.step_async(b)
        graph._ts_action_buffers = bufs  # keep the captured pointers alive
        self._started = True
        return graph

    def get_valid_moves(self):
        """bool [N, 4]: column d is True where Move(d) would change the board (one launch: the kernel writes the
        0 / 1 rows itself, ts_valid_moves4; the bool tensor is a view of them)."""
        self._require_open()
        mask4 = self._empty((self.num_envs, 4), torch.uint8)
        if not self._started:  # environment.py:156-157: [] before reset
            return torch.zeros((self.num_envs, 4), dtype=torch.bool, device=mask4.device)
        if self.num_envs:
            self._call("ts_valid_moves4", C.byref(self._dims), C.byref(self._state), mask4.data_ptr())
        self._sync_if_host()
        return mask4.view(torch.bool)

    def valid_move_bits(self, out=None):
        """uint8 [N]: bit d set where Move(d) would change the board — the kernel's raw output,
        without the [N, 4] bool expansion of get_valid_moves() (one launch, nothing else)."""
        self._require_open()
        out = self._empty(self.num_envs, torch.uint8) if out is None else out
        self._call("ts_valid_moves", C.byref(self._dims), C.byref(self._state), out.data_ptr())
        self._sync_if_host()
        return out

    def get_info(self):
        """ref: environment.py:173-194, batched."""
        if not self._started or self._closed:
            return {"initialized": False}
        return {"initialized": True, "size": self.size, "step_count": self._step_count.clone(),
                "max_steps": self.max_steps, "done": self._done.view(torch.bool).clone(), "is_won": self.is_won(),
                "num_tiles": self.n_tiles, "num_targets": self.n_targets, "multi_color": self.multi_color,
                "valid_moves": self.get_valid_moves()}

    def close(self):
        self._started = False
        self._closed = True

    # ------------------------------------------------------------------ extras
    @property
    def step_count(self):
        return self._step_count

    @property
    def done(self):
        return self._done.view(torch.bool)

    @property
    def positions(self):
        """[T, N] current cell ids (r * size + c): uint8 up to 16x16, int16 above."""
        return self._pos

    def encode(self, out=None):
        """The reference observation of the current boards (state.py:188-211)."""
        if out is None:
            out = self._empty((self.num_envs, self.size, self.size, 3), self.obs_dtype or torch.float32)
        name = "ts_encode" if out.dtype == torch.float32 else "ts_encode_u8"
        self._call(name, C.byref(self._dims), C.byref(self._state), out.data_ptr())
        if self._obs is not None and out.data_ptr() == self._obs.data_ptr():  # the buffer itself or a view of it
            self._sync_shown()
        self._sync_if_host()
        return out

    def encode_onehot(self, out=None):
        """Build-defined one-hot planes float32 [N, Ch, S, S] (see include/tiler_slider.h)."""
        if out is None:
            out = self._empty((self.num_envs, self.onehot_channels, self.size, self.size), torch.float32)
        self._call("ts_encode_onehot", C.byref(self._dims), C.byref(self._state), out.data_ptr())
        self._sync_if_host()
        return out

    def reward(self, out=None):
        """Build-defined Manhattan reward int32 [N] (see include/tiler_slider.h)."""
        out = self._empty(self.num_envs, torch.int32) if out is None else out
        self._call("ts_reward", C.byref(self._dims), C.byref(self._state), out.data_ptr())
        self._sync_if_host()
        return out

    def is_won(self):
        """bool [N]: GameState.is_won() of the current boards (state.py:172-186)."""
        won = self._empty(self.num_envs, torch.uint8)
        self._call("ts_is_won", C.byref(self._dims), C.byref(self._state), won.data_ptr())
        self._sync_if_host()
        return won.view(torch.bool)

    # ------------------------------------------------------------------ solver (lib/libtiler_slider_search.so)
    def solve(self, max_depth=64, with_best=True):
        """Breadth-first search of every board from its CURRENT cells, on the device: one launch (include/tiler_slider_search.h:
        ts_solve) and two small torch kernels that spread the best-move bits into bool columns.  Returns (moves, best): moves int16 [N] - 0 for a won board, else the least number of moves that wins it within
        `max_depth`, else SOLVE_NONE (no sequence of moves wins) or SOLVE_DEPTH (not within max_depth, unexpanded states remain);
        best bool [N, 4] - column a True where Move a starts a shortest solution (all False where moves < 1; the kernel writes one
        byte of four bits per board, solve_bits() returns it as it is).  `done`, the step counters and max_steps play no part, and
        no state is written.  with_best=False: (moves, None).
        Boards up to 8x8 whose index space (S * S) ** n_tiles is at most 65,536: ValueError otherwise."""
        moves, bits = self.solve_bits(max_depth, with_best)
        if bits is None:
            return moves, None
        return moves, _bit_columns(bits)

    def solve_bits(self, max_depth=64, with_best=True):
        """solve() with the kernel's raw second output: (moves int16 [N], best uint8 [N] with bit a set where Move a starts a
        shortest solution).  One launch, nothing else."""
        from . import _search_cabi as sc
        self._require_open()
        if sc.solve_states(self._dims) == 0:
            raise ValueError(f"solve() searches boards up to {sc.SOLVE_MAX_SIZE}x{sc.SOLVE_MAX_SIZE} whose index space (size * size) ** n_tiles is at "
                             f"most {sc.SOLVE_MAX_STATES}; {self.size}x{self.size} with {self.n_tiles} tiles is beyond that (the hash set in "
                             "global memory is a different kernel: solve_reachable())")
        if not 0 <= int(max_depth) <= sc.SOLVE_MAX_DEPTH:
            raise ValueError(f"max_depth must be 0..{sc.SOLVE_MAX_DEPTH}")
        moves = self._empty(self.num_envs, torch.int16)
        best = self._empty(self.num_envs, torch.uint8) if with_best else None
        self._call("ts_solve", C.byref(self._dims), C.byref(self._state), int(max_depth), _ptr(moves), _ptr(best), binding=sc)
        self._sync_if_host()
        return moves, best

    _LOWEST_MOVE = (255, 0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0)  # lowest set bit of a four-bit mask, 255 for none

    def expert_actions(self, max_depth=64):
        """uint8 [N]: for every board the lowest Move that starts a shortest solution (solve()), 255 where there is none - a won
        board, an unsolvable one, one not solved within max_depth.  step() leaves a board untouched on 255 and flags it
        `bad_action`, so the tensor can be fed to step() as it is."""
        _, bits = self.solve_bits(max_depth)
        lut = torch.tensor(self._LOWEST_MOVE, dtype=torch.uint8, device=bits.device)
        return lut[bits.to(torch.int64)]

    # ------------------------------------------------------------------ hashed solver (lib/libtiler_slider_reach.so)
    def solve_reachable(self, max_depth=64, capacity=4096, with_best=True, workspace_bytes=1 << 30):
        """solve() for boards whose index space is beyond it: breadth-first search of every board from its CURRENT cells with a
        hash set in device memory (include/tiler_slider_reach.h: ts_reach_solve, one launch), which costs memory by what a board
        reaches.  Returns a ReachResult: moves int16 [N] as solve()'s, or SOLVE_FULL where a board reached more than `capacity`
        states before the search ended; best bool [N, 4] and bits uint8 [N] as solve() and solve_bits() (None with
        with_best=False); states int32 [N], the number of states expanded; `.expert`, ready for step().  Single-colour boards are
        not canonicalised: two orders of the same cells are two states.
        The workspace is allocated here - one slice per board in flight, at most 1,024 boards and at most `workspace_bytes` - and
        freed on return; boards beyond it are played through the same slices in the same launch.
        Boards up to 8x8 with up to 8 tiles: ValueError otherwise."""
        from . import _reach_cabi as rc
        self._require_open()
        if self.size > rc.REACH_MAX_SIZE or self.n_tiles > rc.REACH_MAX_TILES:
            raise ValueError(f"solve_reachable() searches boards up to {rc.REACH_MAX_SIZE}x{rc.REACH_MAX_SIZE} with up to {rc.REACH_MAX_TILES} tiles; "
                             f"{self.size}x{self.size} with {self.n_tiles} tiles is beyond that")
        if not 0 <= int(max_depth) <= rc.REACH_MAX_DEPTH:
            raise ValueError(f"max_depth must be 0..{rc.REACH_MAX_DEPTH}")
        if not 1 <= int(capacity) <= rc.REACH_MAX_CAPACITY:
            raise ValueError(f"capacity must be 1..{rc.REACH_MAX_CAPACITY}")
        n = self.num_envs
        moves = self._empty(n, torch.int16)
        bits = self._empty(n, torch.uint8) if with_best else None
        states = self._empty(n, torch.int32)
        if n:
            per_board = rc.workspace_bytes(self._dims, capacity, 1)
            if int(workspace_bytes) < per_board:
                raise ValueError(f"one board at capacity {int(capacity)} takes {per_board} bytes of workspace, above workspace_bytes = {int(workspace_bytes)}")
            in_flight = rc.describe_reach(self._dims, max_depth, capacity, workspace_bytes)["boards_in_flight"]
            ws = torch.empty(in_flight * per_board // 8, dtype=torch.int64, device=self.device)
            cfg = rc.ReachCfg(int(max_depth), int(capacity), ws.data_ptr(), in_flight * per_board)
            out = rc.ReachOut(_ptr(moves), _ptr(bits), _ptr(states))
            self._call("ts_reach_solve", C.byref(self._dims), C.byref(self._state), C.byref(cfg), C.byref(out), binding=rc)
        self._sync_if_host()
        return ReachResult(moves, bits, states)

    # ------------------------------------------------------------------ distance-to-win tables (lib/libtiler_slider_table.so)
    def build_table(self, max_depth=252, max_bytes=4 << 30):
        """Solve every board's LEVEL once (include/tiler_slider_table.h: ts_table_build, one launch): a DistanceTable whose `.dist`
        is uint8 [N, (size * size) ** n_tiles] - for every placement of the tiles its least number of moves to a won board
        (0 .. 252), TABLE_INVALID (253: not a placement), TABLE_DEEP (254: not resolved within `max_depth` rounds) or TABLE_NONE
        (255: no sequence of moves wins).  The level - obstacles and targets - never changes, so the table stays right through
        reset() and auto-reset; lookup(), lookup_bits() and expert_actions_from() then answer from wherever the boards stand with
        five byte reads per board instead of a search.  Reads no tile and writes no state.
        The table takes N * states bytes: above `max_bytes` this raises - build the table on an environment of the DISTINCT levels
        and pass `rows=` to the lookups.  Shapes as solve(): ValueError otherwise."""
        from . import _table_cabi as tc
        self._require_open()
        states = self._table_states(tc)
        if not 0 <= int(max_depth) <= tc.TABLE_MAX_DEPTH:
            raise ValueError(f"max_depth must be 0..{tc.TABLE_MAX_DEPTH}")
        nbytes = self.num_envs * states
        if nbytes > int(max_bytes):
            raise ValueError(f"a table of {self.num_envs} boards x {states} placements takes {nbytes} bytes, above max_bytes = {int(max_bytes)}: "
                             "build it on an environment of the distinct levels and pass rows= to lookup() / expert_actions_from()")
        dist = torch.empty((self.num_envs, states), dtype=torch.uint8, device=self.device)
        self._call("ts_table_build", C.byref(self._dims), C.byref(self._state), int(max_depth), _ptr(dist), binding=tc)
        self._sync_if_host()
        return DistanceTable(dist, self.size, self.n_tiles, self.n_targets, self.multi_color, int(max_depth))

    def lookup(self, table, rows=None):
        """(moves int16 [N], best bool [N, 4]) of the boards as they stand, read from `table` (build_table): what solve() returns
        wherever the table is complete.  `rows` int32 [N]: board n reads table row rows[n] (default: row n) - the caller's promise
        that the row was built for that board's level.  `table` may be a ReachTable (build_reach_table): moves can then be
        SOLVE_FULL or SOLVE_ABSENT as well."""
        moves, bits = self.lookup_bits(table, rows)
        return moves, _bit_columns(bits)

    def lookup_bits(self, table, rows=None):
        """lookup() with the kernel's raw second output: (moves int16 [N], best uint8 [N]), as solve_bits().  One launch, nothing else."""
        moves, best, _ = self._lookup(table, rows, True, True, False)
        return moves, best

    def expert_actions_from(self, table, rows=None):
        """uint8 [N]: the lowest Move that starts a shortest solution, 255 where there is none - expert_actions() read from `table`,
        one launch, ready for step()."""
        return self._lookup(table, rows, False, False, True)[2]

    def _table_states(self, tc):
        states = tc.table_states(self._dims)
        if states == 0:
            raise ValueError(f"distance tables cover boards up to 8x8 whose index space (size * size) ** n_tiles is at most 65536; "
                             f"{self.size}x{self.size} with {self.n_tiles} tiles is beyond that")
        return states

    def _lookup(self, table, rows, want_moves, want_best, want_action):
        from . import _table_cabi as tc
        self._require_open()
        if isinstance(table, ReachTable):
            return self._lookup_reach(table, rows, want_moves, want_best, want_action)
        dist, n_rows, rows = self._check_table(table, rows)
        moves = self._empty(self.num_envs, torch.int16) if want_moves else None
        best = self._empty(self.num_envs, torch.uint8) if want_best else None
        action = self._empty(self.num_envs, torch.uint8) if want_action else None
        self._call("ts_table_lookup", C.byref(self._dims), C.byref(self._state), _ptr(dist), n_rows, _ptr(rows), _ptr(moves), _ptr(best),
                   _ptr(action), binding=tc)
        self._sync_if_host()
        return moves, best, action

    # ------------------------------------------------------------------ reachable distance tables (lib/libtiler_slider_rtable.so)
    def build_reach_table(self, capacity=4096, max_depth=252, root="init", max_bytes=4 << 30, workspace_bytes=1 << 30):
        """build_table() for boards whose index space is beyond it: solve every board's LEVEL once over the placements play can
        REACH from its root (include/tiler_slider_rtable.h: ts_rtable_build, one launch) - a ReachTable, one hash table of
        pow2ceil(2 * capacity) 64-bit slots per level.  root="init": the level's initial cells, so the table stays right through
        reset() and auto-reset; root="pos": the cells as they stand.  A level that reaches more than `capacity` states is FULL
        (`.full`).  lookup(), lookup_bits() and expert_actions_from() take the table as they take build_table()'s: moves is 0 on
        a won board, the least number of moves, SOLVE_NONE, SOLVE_DEPTH (not resolved within `max_depth` rounds), SOLVE_FULL for
        a FULL level, or SOLVE_ABSENT where the level's table does not hold the board's placement - play from the root never
        gets there.  Reads the level and the root only and writes no state.
        The table takes N * slots * 8 bytes: above `max_bytes` this raises - build the table on an environment of the DISTINCT
        levels and pass `rows=` to the lookups.  The workspace is allocated here - one slice per level in flight, at most 1,024
        levels and at most `workspace_bytes` - and freed on return.  Boards up to 8x8 with up to 8 tiles: ValueError otherwise."""
        from . import _reach_cabi as rc, _rtable_cabi as xc, _table_cabi as tc
        self._require_open()
        self._require_reach_table_shape(rc)
        if not 0 <= int(max_depth) <= tc.TABLE_MAX_DEPTH:
            raise ValueError(f"max_depth must be 0..{tc.TABLE_MAX_DEPTH}")
        if not 1 <= int(capacity) <= rc.REACH_MAX_CAPACITY:
            raise ValueError(f"capacity must be 1..{rc.REACH_MAX_CAPACITY}")
        if root not in xc.ROOTS:
            raise ValueError(f"root must be one of {sorted(xc.ROOTS)}, got {root!r}")
        n, slots = self.num_envs, xc.slots(capacity)
        nbytes = n * slots * 8
        if nbytes > int(max_bytes):
            raise ValueError(f"a table of {n} boards x {slots} slots takes {nbytes} bytes, above max_bytes = {int(max_bytes)}: "
                             "build it on an environment of the distinct levels and pass rows= to lookup() / expert_actions_from()")
        table = torch.empty((n, slots), dtype=torch.int64, device=self.device)
        count = self._empty(n, torch.int32)
        root_moves = self._empty(n, torch.int16)
        deepest = self._empty(n, torch.int32)
        if n:
            per_level = xc.workspace_bytes(self._dims, capacity, 1)
            if int(workspace_bytes) < per_level:
                raise ValueError(f"one level at capacity {int(capacity)} takes {per_level} bytes of workspace, above workspace_bytes = {int(workspace_bytes)}")
            in_flight = xc.describe_rtable_build(self._dims, max_depth, capacity, workspace_bytes)["levels_in_flight"]
            ws = torch.empty(in_flight * per_level // 8, dtype=torch.int64, device=self.device)
            cfg = xc.RtableCfg(int(max_depth), int(capacity), xc.ROOTS[root], ws.data_ptr(), in_flight * per_level)
            out = xc.RtableOut(_ptr(table), _ptr(count), _ptr(root_moves), _ptr(deepest))
            self._call("ts_rtable_build", C.byref(self._dims), C.byref(self._state), C.byref(cfg), C.byref(out), binding=xc)
        self._sync_if_host()
        return ReachTable(table, count, root_moves, deepest, capacity, self.size, self.n_tiles, self.n_targets, self.multi_color, max_depth, root)

    def _require_reach_table_shape(self, rc):
        if self.size > rc.REACH_MAX_SIZE or self.n_tiles > rc.REACH_MAX_TILES:
            raise ValueError(f"reachable distance tables cover boards up to {rc.REACH_MAX_SIZE}x{rc.REACH_MAX_SIZE} with up to {rc.REACH_MAX_TILES} tiles; "
                             f"{self.size}x{self.size} with {self.n_tiles} tiles is beyond that")

    def _check_reach_table(self, table, rows):
        """The ReachTable and rows of a lookup, validated: (n_rows, rows as contiguous int32 on the device or None)."""
        n_rows = self._check_reach_table_itself(table)
        return n_rows, self._check_rows(rows, n_rows)

    def _check_reach_table_itself(self, table):
        """A ReachTable of this environment's shape and device: its number of levels."""
        from . import _reach_cabi as rc
        if not isinstance(table, ReachTable):
            raise TypeError(f"table must be a ReachTable (build_reach_table()), got {type(table)}")
        self._require_reach_table_shape(rc)
        mine = (self.size, self.n_tiles, self.n_targets, self.multi_color)
        if table.shape_key != mine:
            raise ValueError(f"the table was built for (size, tiles, targets, multi colour) = {table.shape_key}, the environment is {mine}")
        if table.table.device != self.device:
            raise ValueError(f"the table lives on {table.table.device}, the environment on {self.device}")
        return len(table)

    def _lookup_reach(self, table, rows, want_moves, want_best, want_action):
        from . import _rtable_cabi as xc
        n_rows, rows = self._check_reach_table(table, rows)
        moves = self._empty(self.num_envs, torch.int16) if want_moves else None
        best = self._empty(self.num_envs, torch.uint8) if want_best else None
        action = self._empty(self.num_envs, torch.uint8) if want_action else None
        self._call("ts_rtable_lookup", C.byref(self._dims), C.byref(self._state), _ptr(table.table), table.slots, _ptr(table.count), n_rows,
                   _ptr(rows), _ptr(moves), _ptr(best), _ptr(action), binding=xc)
        self._sync_if_host()
        return moves, best, action

    # ------------------------------------------------------------------ reach-table curricula (lib/libtiler_slider_rstarts.so)
    def build_reach_index(self, table, max_bytes=4 << 30):
        """What place_at_distance() reads of a ReachTable: every level's states sorted by (distance, key), and for every
        distance where its states begin (include/tiler_slider_rstarts.h: ts_rstarts_index, one launch) - a ReachIndex of
        `sorted` int64 [L, capacity] and `first` int32 [L, 256].  A FULL level has an empty index: no board is placed from it.
        The index is a function of what the table holds, not of where it holds it: two builds of one table give the same bits.
        It takes L * (capacity * 8 + 1024) bytes: above `max_bytes` this raises - build the table on an environment of the
        DISTINCT levels and pass `rows=` to place_at_distance().  Reads the table only and writes no state."""
        from .rstarts import build_reach_index
        return build_reach_index(self, table, max_bytes)

    # ------------------------------------------------------------------ curriculum starts (lib/libtiler_slider_starts.so)
    def place_at_distance(self, table, min_moves=1, max_moves=None, rows=None, band=None, seed=0, step_index=0, board_offset=0,
                          only_done=False, set_initial=True):
        """Put every board on a placement of its tiles, drawn uniformly among those whose distance to the win - read from `table`
        (build_table) - lies in min_moves .. max_moves (max_moves=None: 252, the largest distance a table holds), in ONE launch
        (include/tiler_slider_starts.h: ts_starts_place) and without a synchronisation: a StartInfo of count, dist, deepest and
        placed.  A board whose row holds no such placement is not placed: it stands where it stood and reports dist 255.
        `band` uint8 [2, N] on the device gives every board its own (min, max) and overrides the two numbers; `rows` int32 [N]
        as lookup(); the draw is the action stream's at (seed, board_offset + n, step_index), so another step_index draws
        again.  only_done=True places only the boards that are done - fresh starts between strict-mode rollouts.  A placed
        board gets step_count 0 and done False, and with set_initial=True the placement becomes its level's initial cells:
        reset() and the auto-reset return there.  The observation buffer shows the new cells afterwards (the full write of
        reset()); the last step's `info` is left as it is.
        `table` may be a ReachIndex (build_reach_index) instead: the same call on the shapes beyond build_table()
        (include/tiler_slider_rstarts.h: ts_rstarts_place), with one difference - a reach table stores no won placement, so
        distance 0 never matches."""
        from . import _starts_cabi as sc
        from ._table_cabi import TABLE_MAX_DEPTH
        from .rstarts import ReachIndex, place_reach
        self._require_open()
        reach = isinstance(table, ReachIndex)
        if not reach:
            dist_table, n_rows, rows = self._check_table(table, rows, 'place_at_distance() takes what build_reach_index() makes of it')
        N = self.num_envs
        lo, hi = int(min_moves), TABLE_MAX_DEPTH if max_moves is None else int(max_moves)
        if not (0 <= lo <= TABLE_MAX_DEPTH and 0 <= hi <= TABLE_MAX_DEPTH):
            raise ValueError(f"min_moves and max_moves must be 0..{TABLE_MAX_DEPTH}")
        if band is not None:
            if not (isinstance(band, torch.Tensor) and band.dtype == torch.uint8 and tuple(band.shape) == (2, N) and band.device == self.device):
                raise ValueError(f"band must be a uint8 tensor of shape (2, {N}) on {self.device}")
            band = band.contiguous()
        count, dist, deepest = self._empty(N, torch.int32), self._empty(N, torch.uint8), self._empty(N, torch.uint8)
        cfg = sc.StartsCfg(lo, hi, _ptr(band), sc.DONE if only_done else sc.ALL, 1, 1 if set_initial else 0, 0,
                           int(seed) & (2 ** 64 - 1), int(step_index), int(board_offset))
        out = sc.StartsOut(_ptr(count), _ptr(dist), _ptr(deepest))
        if reach:
            place_reach(self, table, rows, cfg, out)
        else:
            self._call("ts_starts_place", C.byref(self._dims), C.byref(self._state), _ptr(dist_table), n_rows, _ptr(rows), C.byref(cfg),
                       C.byref(out), binding=sc)
        if self._obs is not None:
            self.encode(out=self._obs)  # the full write reset() makes, and _sync_shown(): an environment that steps in place stays right
        self._sync_if_host()
        self._started = True
        return StartInfo(count, dist, deepest)

    # ------------------------------------------------------------------ fused rollouts (lib/libtiler_slider_rollout.so)
    _ROLLOUT_STATS = ("wins", "finished", "first_win", "win_moves", "reward_sum", "flags")
    _ROLLOUT_LOGS = ("act", "flags", "pos")
    _ROLLOUT_START = ("start",)  # rollout() only: rollout_policy() adds its own names to _ROLLOUT_LOGS

    def rollout(self, steps, policy="random", actions=None, table=None, rows=None, epsilon=0.0, seed=0, step_index=0, board_offset=0,
                stats=True, log=(), advance=True):
        """`steps` steps of every board in ONE launch (include/tiler_slider_rollout.h: ts_rollout): a board is loaded once, played in
        its lane's registers and stored once, and each action is drawn or looked up by the kernel itself.  The result is exactly
        what `steps` rounds of ts_fill_actions / expert_actions_from / step() leave.
          policy "given":  actions uint8 [steps, N] on the device
                 "random": the stream of ts_fill_actions(seed, board_offset, step_index + k)
                 "table":  the expert move of `table` (build_table(); `rows` as in lookup()), replaced by the random draw with
                           probability `epsilon` and wherever the expert has no move
                 "reach":  the same on a ReachTable (build_reach_table()), for shapes beyond the tables' index space: still one
                           launch (include/tiler_slider_rexpert.h: ts_rexpert_rollout); no move also where the row is FULL or
                           does not hold the board's placement
          stats=True: wins, finished, first_win, win_moves, reward_sum, flags (False: none; or an iterable of those names)
          log: any of "act", "flags", "pos" - the per-step logs act_log, flags_log uint8 [steps, N], pos_log [steps, T, N] - and
                 "start": Rollout.start_pos, a copy of the cells before the launch (what trajectory_labels() and a reward on
                 progress need beside "pos")
          advance=True: the environment moves on as `steps` calls of step() would move it (state, last flags; an observation-
                 keeping environment re-encodes its current observation once at the end).  advance=False: a playout from where the
                 boards stand; the environment is left untouched.
        Returns a Rollout.  Boards up to 8x8 with at most 8 tiles and 8 targets; "table" also needs the tables' index space
        (size * size) ** n_tiles <= 65536: ValueError otherwise."""
        if policy == "reach":  # lib/libtiler_slider_rexpert.so: the rollout library is not consulted
            from .rexpert import rollout_reach
            return rollout_reach(self, steps, table, rows, epsilon, seed, step_index, board_offset, stats, log, advance)
        from . import _rollout_cabi as rc
        self._require_open()
        if not self._started:
            raise RuntimeError("Call reset() before rollout().")
        if self.host_mapped:
            raise ValueError("rollout needs device buffers (host_mapped=False)")
        if policy not in rc.POLICIES:
            raise ValueError(f"policy must be one of {sorted(rc.POLICIES)}, got {policy!r}")
        pol = rc.POLICIES[policy]
        if not rc.rollout_supported(self._dims, pol):
            raise ValueError(f"rollout() plays boards up to {rc.ROLLOUT_MAX_SIZE}x{rc.ROLLOUT_MAX_SIZE} with at most {rc.ROLLOUT_MAX_TILES} tiles and "
                             f"{rc.ROLLOUT_MAX_TILES} targets, and the table policy an index space (size * size) ** n_tiles of at most 65536; "
                             f"{self.size}x{self.size} with {self.n_tiles} tiles and {self.n_targets} targets is beyond that")
        steps = int(steps)
        if not 0 <= steps <= rc.ROLLOUT_MAX_STEPS:
            raise ValueError(f"steps must be 0..{rc.ROLLOUT_MAX_STEPS}")
        if not 0.0 <= float(epsilon) <= 1.0:
            raise ValueError("epsilon must be 0..1")
        N = self.num_envs
        cfg = rc.RolloutCfg(steps, self._mode, pol, 1 if advance else 0, None, int(seed) & (2**64 - 1), int(step_index), int(board_offset),
                            int(round(float(epsilon) * 2**32)), None, 0, None)
        if pol == rc.GIVEN:
            if not (isinstance(actions, torch.Tensor) and actions.dtype == torch.uint8 and actions.device == self.device
                    and tuple(actions.shape) == (steps, N) and actions.is_contiguous()):
                raise TypeError(f"actions must be a contiguous uint8 device tensor of shape [{steps}, {N}]")
            cfg.actions = _ptr(actions)
        elif pol == rc.TABLE:
            dist, n_rows, rows = self._check_table(table, rows)
            cfg.table, cfg.n_rows, cfg.rows = _ptr(dist), n_rows, _ptr(rows)
        names = self._ROLLOUT_STATS if stats is True else () if not stats else tuple(stats)
        logs = (log,) if isinstance(log, str) else tuple(log)
        if set(names) - set(self._ROLLOUT_STATS) or set(logs) - set(self._ROLLOUT_LOGS + self._ROLLOUT_START):
            raise ValueError(f"stats are {self._ROLLOUT_STATS}, logs {self._ROLLOUT_LOGS + self._ROLLOUT_START}")
        got = {name: torch.zeros(N, dtype=torch.uint8 if name == "flags" else torch.int32, device=self.device) for name in names}
        start_pos = self._pos.clone() if "start" in logs else None  # before the launch: with advance=True it overwrites the only other copy
        for name in logs:
            if name == "start":
                continue
            shape = (steps, self.n_tiles, N) if name == "pos" else (steps, N)
            got[name + "_log"] = torch.zeros(shape, dtype=self._pos.dtype if name == "pos" else torch.uint8, device=self.device)
        bound = dict(got)
        if advance:  # the environment's own flag byte becomes the last step's, as after step(); a Rollout's `flags` is then that tensor
            bound["flags"] = self._flags
            if "flags" in got:
                got["flags"] = self._flags
        out = rc.RolloutOut(*(_ptr(bound.get(f)) for f in rc.OUT_FIELDS))
        if steps and N and bound:
            self._call("ts_rollout", C.byref(self._dims), C.byref(self._state), C.byref(cfg), C.byref(out), binding=rc)
            if advance and self.obs_dtype is not None:  # one encode into the current buffer: env._obs stays truthful
                self._call("ts_encode" if self.obs_dtype == torch.float32 else "ts_encode_u8", C.byref(self._dims), C.byref(self._state),
                           _ptr(self._obs))
                self._sync_shown()
        return Rollout(steps, **got) if start_pos is None else Rollout(steps, start_pos=start_pos, **got)

    # ------------------------------------------------------------------ neural-policy rollouts (lib/libtiler_slider_policy.so)
    def policy_logits(self, policy):
        """float32 [N, 4]: the logits of `policy` (tiler_slider_amd.MlpPolicy) on the boards as they stand - what the network gives on
        encode_onehot().flatten(1), computed from the cell ids in one launch (include/tiler_slider_policy.h: ts_policy_logits); the
        planes are never written.  No state is touched."""
        from .policy import policy_logits
        return policy_logits(self, policy)

    def rollout_policy(self, steps, policy, select="sample", epsilon=0.0, seed=0, step_index=0, board_offset=0, stats=True, log=(),
                       advance=True, expert=None, beta=0.0, rows=None):
        """rollout() with a network choosing every action, still ONE launch (include/tiler_slider_policy.h: ts_policy_rollout):
        at every step the kernel evaluates `policy` (an MlpPolicy) on the board as it stands and plays
          select "greedy": the lowest action among the largest logits
                 "sample": a draw from softmax(logits), from bits 32 .. 55 of the step's draw of ts_fill_actions' stream
        replaced by that stream's random action with probability `epsilon`.  seed, step_index, board_offset, stats, log and
        advance are rollout()'s; `log` also accepts "logits": Rollout.logits_log float32 [steps, N, 4], the values each action was
        chosen from, and "start": Rollout.start_pos, a copy of the cells before the launch (what trajectory_logits() needs beside
        "pos").  Shapes as rollout("random"), hidden widths 1 .. 64: ValueError otherwise.
        expert=table (anything lookup() takes: a DistanceTable or PolicyTable, a ReachTable or ReachPolicyTable; `rows` as in
        lookup()): the table's expert SHARES the play, still one launch (include/tiler_slider_mixed.h: ts_mixed_rollout).  Per
        board and step the expert's move is played with probability `beta` - DAgger's behaviour policy - wherever it has one
        (elsewhere the network plays), and the random action still replaces either with probability `epsilon`.  The kernel looks
        the table up on every board it visits, so `log` also accepts "expert", "moves", "best" - Rollout.expert_log, moves_log,
        best_log: byte for byte trajectory_labels()' action, moves and best of this rollout, without the second launch - and
        "who": Rollout.who_log, 0 where the network played, 1 the expert, 2 the random draw.  With beta = 0 and none of the three
        asked for, the table is not read and the play is rollout_policy()'s without an expert.  Without `expert`, beta != 0, rows
        and the four logs are a ValueError."""
        if expert is not None:
            from .mixed import rollout_mixed
            return rollout_mixed(self, steps, policy, expert, beta, rows, select, epsilon, seed, step_index, board_offset, stats, log, advance)
        if beta != 0 or rows is not None:
            raise ValueError("beta and rows belong to expert=: without an expert the network plays alone")
        from .policy import rollout_policy
        return rollout_policy(self, steps, policy, select, epsilon, seed, step_index, board_offset, stats, log, advance)

    # ------------------------------------------------------------------ policy tables (lib/libtiler_slider_ptable.so)
    def build_policy_table(self, policy, max_depth=252, max_bytes=4 << 30, logits=False, table=None):
        """A PolicyTable: the greedy play of `policy` (an MlpPolicy, or a PolicyNet / ActorCriticNet through its .policy()) from
        EVERY placement of every board's level, exactly, in two launches (include/tiler_slider_ptable.h: ts_ptable_actions, the
        network once per placement; ts_ptable_walk, the outcome of following its moves).  `.dist` uint8 [N, states] has
        build_table()'s format and codes - the moves the policy needs to the win, TABLE_NONE where greedy play never wins
        (deterministic play ends in a cycle or stands still), TABLE_DEEP where it has not won within `max_depth` moves - so
        lookup(), place_at_distance() and every other call that takes a DistanceTable take it as it is.  `.act` uint8 [N, states]
        is the move on each placement (255 on an invalid one) and, with logits=True, `.logits` float32 [N, states, 4] the values
        it was chosen from, bit-equal to policy_logits() on a board standing there.  Reads no tile and writes no state; no
        sampling, no horizon, no start distribution.  max_bytes as build_table() (2 bytes per placement, 18 with the logits).
        table=rt, a ReachTable (build_reach_table()) of this environment's levels, one row per board: the same on the shapes
        beyond the dense index space, over the states rt holds (include/tiler_slider_rptable.h: ts_rptable_actions,
        ts_rptable_walk) - a ReachPolicyTable, a ReachTable itself: `.table` holds the policy's entries in rt's slots, `.act`
        uint8 [N, slots] the move on each state's slot (255 on every other), `.logits` float32 [N, slots, 4]; lookup(),
        build_reach_index() and through it place_at_distance() take it as they take rt.  9 bytes per slot, 25 with the logits."""
        if table is not None:
            from .rptable import build_policy_table
            return build_policy_table(self, policy, table, max_depth, max_bytes, logits)
        from .ptable import build_policy_table
        return build_policy_table(self, policy, max_depth, max_bytes, logits)

    def walk_actions(self, act, max_depth=252, table=None, max_bytes=4 << 30):
        """build_policy_table()'s second launch alone, over a given action table: `act` uint8 [N, states] on the device, any bytes -
        a move 0 .. 3 is played, anything else stands still - gives the PolicyTable of that tabular policy.  Walking the
        expert's moves reproduces build_table().  table=rt, a ReachTable of this environment's levels: `act` is uint8 [N, rt.slots],
        read on the slots of rt's states, and the result the ReachPolicyTable of that tabular policy; walking the expert's moves
        reproduces rt's entries.  The result takes 8 bytes a slot beside the byte of `act`: above `max_bytes` (9 bytes a slot,
        as build_policy_table(table=rt) counts them) this raises; `max_bytes` is read on this path only.  A table of more than
        8,192 slots (capacity above 4,096) is walked in its output row, every round reading the whole row
        (include/tiler_slider_rptable.h: TS_RPTABLE_FORM_GLOBAL): long chains cost rounds x slots there."""
        if table is not None:
            from .rptable import walk_actions
            return walk_actions(self, act, table, max_depth, max_bytes)
        from .ptable import walk_actions
        return walk_actions(self, act, max_depth)

    def score_policy(self, ptable, table):
        """PolicyScore of a PolicyTable against the optimal DistanceTable of the same levels (build_table()), one launch
        (ts_ptable_score), integers only and the same bits on every run: per level the valid, solvable, solved and optimally
        solved placements, those on which the policy's move is one of the expert's, the excess moves, and `solved_share`,
        `optimal_share`, `agreement` over all levels as 0-dim device tensors.  A ReachPolicyTable is scored against the ReachTable
        of the same levels and slots (ts_rptable_score): the same columns, counted over the states the table holds."""
        from .rptable import ReachPolicyTable
        if isinstance(ptable, ReachPolicyTable):
            from .rptable import score_policy
            return score_policy(self, ptable, table)
        from .ptable import score_policy
        return score_policy(self, ptable, table)

    # ------------------------------------------------------------------ trainable policies (lib/libtiler_slider_train.so)
    def trajectory_logits(self, net, rollout=None):
        """float32 [K, N, 4]: the logits of `net` (a tiler_slider_amd.PolicyNet or an MlpPolicy) on every board-step of `rollout`
        - a Rollout of rollout_policy(K, ..., log=("start", "pos")): step k's logits on the board that step was chosen on - or,
        with rollout=None, on the boards as they stand (K = 1).  One launch (include/tiler_slider_train.h: ts_train_forward); the
        one-hot planes are never built and no state is touched.  Given a PolicyNet whose parameters require grad (and outside
        torch.no_grad()) the result carries a grad_fn: loss.backward() is one more launch (ts_train_backward) that fills the four
        parameters' .grad, in float32 with float atomic adds - not bit-reproducible from run to run.  TypeError / ValueError for a
        rollout without start_pos / pos_log, of another N or T, on another device, or a host-mapped environment."""
        from .train import trajectory_logits
        return trajectory_logits(self, net, rollout)

    # ------------------------------------------------------------------ the actor-critic network (lib/libtiler_slider_ac.so)
    def trajectory_outputs(self, net, rollout=None):
        """(logits float32 [K, N, 4], values float32 [K, N]) of `net` (a tiler_slider_amd.ActorCriticNet) on every board-step of
        `rollout`, or with rollout=None on the boards as they stand (K = 1: values[0] is trajectory_returns()' last_value).
        trajectory_logits() with a value head on the same hidden layer: ONE launch for both (include/tiler_slider_ac.h:
        ts_ac_forward), and where parameters require grad both results carry the grad_fn of one function whose backward is ONE
        launch (ts_ac_backward) taking both cotangents - a loss that uses only one of the two gives the other a zero one.
        `values` feeds trajectory_returns(values=...) as it is.  Checks and errors as trajectory_logits()."""
        from .actor_critic import trajectory_outputs
        return trajectory_outputs(self, net, rollout)

    # ------------------------------------------------------------------ lookahead (lib/libtiler_slider_lookahead.so)
    def lookahead(self, net, depth=2, rollout=None, leaf=None, gamma=1.0, reward=None):
        """Lookahead(q, value, best, win_in): the values of `net` backed up through a full-width search of `depth` plies (1 .. 4) of
        the exact environment, ONE launch (include/tiler_slider_lookahead.h: ts_lookahead) - on the boards as they stand
        (q float32 [N, 4], value float32 [N], best uint8 [N], win_in uint8 [N]) or, with a Rollout that logged ("start", "pos"), on
        every board it visited ([K, N, ...], row k the board step k was chosen on).
          q[..., a] = r + gamma * (0 if the move wins, else the best backed-up value of the board after it), r = reward.step
                      + reward.win on a winning move + reward.invalid on a move that changes nothing; at the last ply the value
                      of a board is the leaf's
          leaf: "value" - the value head of an ActorCriticNet (its default); "qmax" - the largest logit, the network read as a
                Q-network (the default of a PolicyNet / MlpPolicy; an ActorCriticNet may ask for it); "zero" - no network is read
                (the default of net=None): plain reward search
          value = q.max(-1); best = the lowest action that attains it - step(best) plays the search's move, and as
                trajectory_loss(labels=best) it is an expert-iteration target; win_in = the plies to the nearest win inside the
                horizon, 0 if there is none
        A board that is already won gets q = 0, value = 0, best = 255 (left alone by step(), no sample for a loss), win_in = 0.
        An invalid move costs a ply like any other; there is no transposition table, no pruning and no timeout: reward.timeout,
        reward.dist and reward.progress must be 0 (ValueError).  The results are targets and carry no grad_fn.  Shapes and widths
        as rollout_policy(); checks and errors as trajectory_logits().  No state is touched."""
        from .lookahead import lookahead
        return lookahead(self, net, depth, rollout, leaf, gamma, reward)

    def td_targets(self, net, rollout=None, gamma=0.99, reward=None):
        """float32 [N, 4] or [K, N, 4]: the one-step targets of ALL FOUR actions of every board - lookahead(depth=1).q:
        r(s, a) + gamma V(s') with an ActorCriticNet, r(s, a) + gamma max_a' Q(s', a') with a PolicyNet / MlpPolicy read as a
        Q-network, 0 beyond a winning move and on a board that is already won.  One launch; no twin environment is stepped and
        no successor board is encoded.  gather() the logged action's column for TD(0) or Q-learning."""
        from .lookahead import lookahead
        return lookahead(self, net, 1, rollout, None, gamma, reward).q

    # ------------------------------------------------------------------ trajectory targets (lib/libtiler_slider_targets.so)
    def trajectory_returns(self, rollout, gamma=0.99, lam=1.0, values=None, last_value=None, reward=None):
        """TrajectoryReturns(reward, adv, ret float32 [K, N], mask bool [K, N]) of a Rollout that logged its flags: per-step rewards,
        GAE(gamma, lam) advantages and returns ret = adv + values, in ONE launch that walks each board's log backwards
        (include/tiler_slider_targets.h: ts_traj_returns).  mask is False where a step played no transition - the board was done
        on entry (strict mode: it stays; auto-reset: the step restarts it) or the action byte was no move; reward, adv and ret
        are 0 there and the recursion passes over the step.  Both SUCCESS and TIMEOUT end an episode: nothing is bootstrapped
        across them.
          reward: a RewardWeights(step=0, win=1, timeout=0, invalid=0, dist=0, progress=0); `dist` and `progress` weigh the
                  Manhattan reward of reward() on the cells after the step and its plain difference across the step - they need
                  log "pos" (and "start" for progress); with both 0 the cells are never read
          values: float32 [K, N] on the device, V(s_k) of the board step k was chosen on - contiguous, or a column view
                  t[..., c] of a contiguous [K, N, 4] tensor, read in place (the logits of a critic PolicyNet); detached.
                  None: 0, and with lam = 1 `ret` is the discounted return-to-go
          last_value: float32 [N], V of the boards after the last step (None: 0)
        Shapes as rollout("random"): ValueError otherwise.  Nothing is read from or written to the environment's state."""
        from .targets import trajectory_returns
        return trajectory_returns(self, rollout, gamma, lam, values, last_value, reward)

    def trajectory_vtrace(self, rollout, logits=None, values=None, last_value=None, gamma=0.99, lam=1.0, rho_bar=1.0, c_bar=1.0,
                          select="sample", epsilon=0.0, beta=0.0, reward=None):
        """VtraceTargets(reward, adv, ret, mask, weight, log_mu) of a Rollout whose actions were NOT drawn from the network being
        trained - rollout_policy(expert=, beta=), epsilon > 0, select "greedy", or a log replayed after the weights have moved -
        in ONE launch (include/tiler_slider_vtrace.h: ts_traj_vtrace).  V-trace (Espeholt et al. 2018): trajectory_returns()'
        backward recursion with the truncated importance weights rho = min(rho_bar, pi / mu) and c = lam min(c_bar, pi / mu)
        inside; `ret` is the V-trace target v_s, `adv` the policy-gradient advantage rho (r + gamma v_(s+1) - V) with its weight
        included, `weight` pi / mu unclipped and `log_mu` the log of the behaviour probability of the action played.  mu follows
        exactly from what the rollout logged - it needs log ("flags", "act", "logits"), and ("expert",) where beta > 0 - and from
        the `select`, `epsilon` and `beta` it was made with, which the caller passes again.
          logits: float32 [K, N, 4], the network's logits NOW (trajectory_logits() / trajectory_outputs(); detached).  None: the
                  logged logits - with select "sample" and epsilon = beta = 0 every weight is then exactly 1 and, for bars >= 1,
                  `ret` is trajectory_returns()' and `adv` its adv at lam = 1
          values, last_value, gamma, reward: trajectory_returns()'; masks, void steps and episode ends as there
        vt.returns is a TrajectoryReturns: trajectory_loss(logits, rollout, vt.returns, values=v) at clip=0 is the V-trace
        actor-critic loss.  Shapes as rollout("random"): ValueError otherwise.  No state is touched."""
        from .vtrace import trajectory_vtrace
        return trajectory_vtrace(self, rollout, logits, values, last_value, gamma, lam, rho_bar, c_bar, select, epsilon, beta, reward)

    def trajectory_labels(self, rollout, table, rows=None):
        """(moves int16 [K, N], best uint8 [K, N], action uint8 [K, N]): lookup_bits() and expert_actions_from() of `table` on every
        board a Rollout visited - row k is the answer on the board step k was chosen on (start_pos, then pos_log[k - 1]) - in ONE
        launch (include/tiler_slider_targets.h: ts_traj_labels).  `action` is a cross_entropy target wherever it is not 255 (the
        expert has no move: the board is won, cannot be won, or its row lies outside the table).  The rollout needs log
        ("start", "pos"); table and rows as lookup().  No state is touched.  `table` may be a ReachTable (build_reach_table()):
        still one launch (include/tiler_slider_rexpert.h: ts_rexpert_labels), and moves can be SOLVE_FULL or SOLVE_ABSENT as well."""
        if isinstance(table, ReachTable):
            from .rexpert import trajectory_labels_reach
            return trajectory_labels_reach(self, rollout, table, rows)
        from .targets import trajectory_labels
        return trajectory_labels(self, rollout, table, rows)

    def trajectory_loss(self, logits, rollout, targets=None, values=None, labels=None, clip=0.0, value_coef=0.5, entropy_coef=0.0,
                        normalize_adv=False):
        """LossInfo of the fused actor-critic loss (include/tiler_slider_loss.h: ts_actor_critic_loss, four launches, no float
        atomics) between trajectory_outputs()' or trajectory_logits()' `logits` [K, N, 4] - and `values` [K, N] - and the targets
        of `rollout`; its `.loss` carries one grad_fn, so `.loss.backward()` goes on into the network's own backward launch.
        The actions are `labels` where given (uint8 [K, N], trajectory_labels()' action: a cross-entropy, 255 is no sample),
        otherwise rollout.act_log.  `targets`, a TrajectoryReturns, gives the mask, the advantages and, with `values`, the returns
        of value_coef (values - ret)^2; without it every sample with a move counts with advantage 1.  clip > 0 is PPO's clipped
        ratio against the policy that played: the rollout must have logged its logits.  entropy_coef weighs the entropy bonus,
        normalize_adv standardises the advantages over the live samples.  The plain-torch loss remains what it was; this
        call is tiler_slider_amd.actor_critic_loss() with the arguments looked up, and raises ValueError where one is missing
        or of another shape, dtype or device."""
        from .loss import trajectory_loss
        return trajectory_loss(self, logits, rollout, targets, values, labels, clip, value_coef, entropy_coef, normalize_adv)

    def _check_table(self, table, rows, reach_advice='a ReachTable is played by rollout(policy="reach") and read by lookup() and trajectory_labels()'):
        """The table and rows of a lookup, validated: (dist, n_rows, rows as contiguous int32 on the device or None)."""
        from . import _table_cabi as tc
        if not isinstance(table, DistanceTable):
            raise TypeError(f"table must be a DistanceTable (build_table()), got {type(table)}"
                            + (f"; {reach_advice}" if isinstance(table, ReachTable) else ""))
        states = self._table_states(tc)
        mine = (self.size, self.n_tiles, self.n_targets, self.multi_color)
        if table.shape_key != mine or table.dist.shape[1] != states:
            raise ValueError(f"the table was built for (size, tiles, targets, multi colour) = {table.shape_key}, the environment is {mine}")
        if table.dist.device != self.device:
            raise ValueError(f"the table lives on {table.dist.device}, the environment on {self.device}")
        n_rows = table.dist.shape[0]
        return table.dist, n_rows, self._check_rows(rows, n_rows)

    def _check_rows(self, rows, n_rows):
        """The rows of a lookup in a table of n_rows rows, validated: contiguous int32 on the device, or None."""
        if rows is None:
            if n_rows != self.num_envs:
                raise ValueError(f"the table has {n_rows} rows for {self.num_envs} boards: pass rows= (int32 [{self.num_envs}])")
        else:
            rows = torch.as_tensor(rows)
            if rows.shape != (self.num_envs,) or rows.dtype == torch.bool or rows.is_floating_point():
                raise ValueError(f"rows must be an integer tensor of shape ({self.num_envs},)")
            if rows.dtype != torch.int32:  # a wider index must not wrap into the table: whatever lies outside becomes -1
                rows = rows.to(self.device)
                rows = torch.where((rows < 0) | (rows >= n_rows), torch.full_like(rows, -1), rows)
            rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
            if self.strict and self.num_envs and bool(((rows < 0) | (rows >= n_rows)).any()):  # a sync, as step()'s strict check
                raise ValueError(f"rows outside the table's 0..{n_rows - 1}")
        return rows

    # ------------------------------------------------------------------ internals
    def _info(self):
        extras = {}
        if self._reward is not None:
            extras["reward"] = self._reward
        if self._onehot is not None:
            extras["onehot"] = self._onehot
        if self._valid is not None:
            extras["valid_moves"] = self._valid4.view(torch.bool)
        return StepInfo(self._flags, self._step_count, extras)

    def _stage_actions(self, actions):
        if isinstance(actions, torch.Tensor):
            if actions.dtype == torch.bool or actions.is_floating_point() or actions.is_complex():
                raise TypeError(f"actions tensor must hold integers, got {actions.dtype}")
            if actions.shape != (self.num_envs,):
                raise ValueError(f"actions must have shape ({self.num_envs},)")
            if (not self.host_mapped and actions.dtype == torch.uint8 and actions.device == self.device
                    and actions.is_contiguous()):
                return actions
            a = actions.to(self._actions.device, non_blocking=True)
            if a.dtype != torch.uint8:  # anything outside a byte becomes 255 = "bad action" for the kernel
                a = torch.where((a < 0) | (a > 255), torch.full_like(a, 255), a)
            self._actions.copy_(a)
            return self._actions
        if isinstance(actions, np.ndarray):
            if actions.dtype.kind not in "iu":
                raise TypeError(f"actions array must hold integers, got {actions.dtype}")
            a = np.where((actions < 0) | (actions > 255), 255, actions).astype(np.uint8)
            return self._stage_actions(torch.from_numpy(np.ascontiguousarray(a)))
        vals = []
        for a in actions:
            if not isinstance(a, Move):  # environment.py:116-117
                raise TypeError(f"Action must be a GameState.Move enum, got {type(a)}")
            vals.append(a.value)
        return self._stage_actions(torch.tensor(vals, dtype=torch.uint8))

    def _call(self, name, *args, binding=_cabi):
        """One C-ABI call on the current stream of the environment's device; `binding`: the library's binding module.
        (The device context manager is entered only when another device is current: with it a small launch - ts_valid_moves4
        takes 5 us on the GPU - cost three times its kernel.)"""
        fn = self._fns.get(name)
        if fn is None:
            fn = self._fns[name] = getattr(binding.lib(), name)
        if torch.cuda.current_device() == self.device.index:
            rc = fn(*args, torch.cuda.current_stream(self.device).cuda_stream)
        else:
            with torch.cuda.device(self.device):
                rc = fn(*args, torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            binding.check(rc, name)

    def _require_open(self):
        if self._closed:
            raise RuntimeError("environment is closed")


class _ContiguousBuffer:
    """Device memory from hipExtMallocWithFlags(hipDeviceMallocContiguous): physically contiguous VRAM, exposed to torch
    through __cuda_array_interface__ (torch.as_tensor keeps this object alive for as long as the tensor lives)."""

    _hip = None

    def __init__(self, nbytes, device):
        cls = type(self)
        if cls._hip is None:
            lib = C.CDLL("libamdhip64.so")
            lib.hipExtMallocWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
            lib.hipFree.argtypes = [C.c_void_p]
            lib.hipGetLastError.restype = C.c_int
            cls._hip = lib
        p = C.c_void_p()
        with torch.cuda.device(device):
            rc = cls._hip.hipExtMallocWithFlags(C.byref(p), nbytes, 0x4)  # hipDeviceMallocContiguous
        if rc != 0 or not p.value:
            # A failed HIP call leaves the thread's "last error" set until somebody reads it, and the library's launches check
            # exactly that (ts_kernels.hip: finish_launch -> hipGetLastError) - unread, the error of this allocation would surface
            # as TS_ERR_HIP on the next ts_prepare / ts_reset although the caller has fallen back to torch's allocator.
            cls._hip.hipGetLastError()
            raise MemoryError(f"hipExtMallocWithFlags(contiguous, {nbytes} B) failed with {rc}")
        self.ptr, self.nbytes, self.device = p.value, nbytes, device
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (p.value, False), "version": 2, "strides": None}

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                type(self)._hip.hipFree(C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:  # interpreter shutdown
            pass


def _contiguous_zeros(shape, dtype, device):
    """A zeroed tensor in physically contiguous device memory, or None when the runtime cannot provide it."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    try:
        buf = _ContiguousBuffer(n, device)
        t = torch.as_tensor(buf, device=device).view(dtype).view(shape)
    except Exception:  # no such flag in this runtime, fragmented VRAM, ...: the caching allocator will do
        return None
    t.zero_()
    return t


def _resolve_device(device):
    if not torch.cuda.is_available():
        raise RuntimeError("tiler_slider_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device must be a cuda (ROCm) device, got {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _cell_torch_dtype(size):
    # torch has no general uint16 arithmetic; int16 holds the same bits (cell ids < 1024)
    return torch.uint8 if cell_dtype(size) == np.uint8 else torch.int16


def _to_device(a, dtype, device):
    if isinstance(a, np.ndarray):
        if dtype == torch.int32 and a.dtype == np.uint32:
            a = a.view(np.int32)
        if dtype == torch.int16 and a.dtype == np.uint16:
            a = a.view(np.int16)
        a = torch.from_numpy(np.ascontiguousarray(a))
    if a.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {a.dtype}")
    return a.to(device).contiguous()


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _bit_columns(bits):
    """bool [N, 4] of a uint8 [N] of best-move bits: column a is bit a."""
    return (bits.unsqueeze(1) >> torch.arange(4, dtype=torch.uint8, device=bits.device) & 1).to(torch.bool)

