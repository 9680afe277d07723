"""Reach-table curricula (lib/libtiler_slider_rstarts.so, include/tiler_slider_rstarts.h): place_at_distance() on the shapes beyond
the dense tables' index space.

build_reach_index() is one k_rstarts_index launch: every level's states sorted by (distance, key) and the 256 lower bounds of the
distances - a ReachIndex.  place_reach() is one k_rstarts_place launch that reads it: what place_at_distance() does with a
DistanceTable, a handful of reads per board.  There is no CPU path and no torch fallback.
"""
import ctypes as C

import torch

from . import _rstarts_cabi as xs


class ReachIndex:
    """What VecTilerSliderEnv.build_reach_index() returns (include/tiler_slider_rstarts.h), on the device: `sorted` int64
    [L, capacity], the slot words of every level's states in ascending (entry, key) order - as unsigned words; an occupied word
    has bit 63 set, so it is negative here - then zeros; `first` int32 [L, 256], first[l, d] the number of states of level l whose
    entry is below d; `capacity` and the shape of the table it was built from - place_at_distance() refuses an environment of
    another.  A FULL level has an empty index.  Two builds of one ReachTable give the same bits."""

    def __init__(self, sorted_, first, capacity, size, n_tiles, n_targets, multi_color):
        self.sorted, self.first, self.capacity = sorted_, first, int(capacity)
        self.size, self.n_tiles, self.n_targets, self.multi_color = int(size), int(n_tiles), int(n_targets), bool(multi_color)

    @property
    def shape_key(self):
        return (self.size, self.n_tiles, self.n_targets, self.multi_color)

    def band_count(self, lo=1, hi=252):
        """int32 [L]: the states of every level whose distance lies in lo .. hi (hi is cut at 252; an empty band gives 0) - what
        place_at_distance() reports as `count` for a board of that level."""
        lo, hi = int(lo), min(int(hi), 252)
        if not (0 <= lo <= 255 and hi >= 0):
            raise ValueError("lo must be 0..255 and hi at least 0")
        return (self.first[:, hi + 1] - self.first[:, lo]).clamp_(min=0)

    def __len__(self):
        return self.sorted.shape[0]

    def __repr__(self):
        return f"ReachIndex({len(self)} levels x {self.capacity} states)"


def build_reach_index(env, table, max_bytes=4 << 30):
    """VecTilerSliderEnv.build_reach_index(): see there."""
    from .vec_env import _ptr
    env._require_open()
    n_rows = env._check_reach_table_itself(table)  # any number of levels: the boards come with rows= at the placement
    width = table.capacity
    nbytes = n_rows * (width * 8 + xs.FIRST * 4)
    if nbytes > int(max_bytes):
        raise ValueError(f"an index of {n_rows} levels x {width} states takes {nbytes} bytes, above max_bytes = {int(max_bytes)}: "
                         "build the table on an environment of the distinct levels and pass rows= to place_at_distance()")
    sorted_ = torch.empty((n_rows, width), dtype=torch.int64, device=env.device)
    first = torch.empty((n_rows, xs.FIRST), dtype=torch.int32, device=env.device)
    if n_rows:
        env._call("ts_rstarts_index", _ptr(table.table), table.slots, _ptr(table.count), n_rows, width, _ptr(sorted_), _ptr(first), binding=xs)
    env._sync_if_host()
    return ReachIndex(sorted_, first, width, *table.shape_key)


def check_reach_index(env, index, rows):
    """The ReachIndex and rows of a placement, validated: (n_rows, rows as contiguous int32 on the device or None)."""
    from . import _reach_cabi as rc
    env._require_reach_table_shape(rc)
    mine = (env.size, env.n_tiles, env.n_targets, env.multi_color)
    if index.shape_key != mine:
        raise ValueError(f"the index was built for (size, tiles, targets, multi colour) = {index.shape_key}, the environment is {mine}")
    if index.sorted.device != env.device:
        raise ValueError(f"the index lives on {index.sorted.device}, the environment on {env.device}")
    n_rows = len(index)
    return n_rows, env._check_rows(rows, n_rows)


def place_reach(env, index, rows, cfg, out):
    """The launch of VecTilerSliderEnv.place_at_distance() on a ReachIndex; cfg and out are the dense call's structs."""
    from .vec_env import _ptr
    n_rows, rows = check_reach_index(env, index, rows)
    env._call("ts_rstarts_place", C.byref(env._dims), C.byref(env._state), _ptr(index.sorted), _ptr(index.first), index.capacity, n_rows,
              _ptr(rows), C.byref(cfg), C.byref(out), binding=xs)
