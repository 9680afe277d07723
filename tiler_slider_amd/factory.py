"""Level factories.

ref: explainrl/environment/environment.py:197-288 (TilerSliderEnvFactory).
"""
import numpy as np

from .env import TilerSliderEnv
from .levels import parse_board_string
from .vec_env import VecTilerSliderEnv


def simple_level(size=5, num_tiles=2, num_obstacles=3, seed=None):
    """(blocked, initial, targets) of the reference's random level for `seed`.

    ref: environment.py:217-226.  The reference draws from numpy's legacy global stream
    (np.random.seed + np.random.shuffle of the row-major cell list) and slices
    obstacles / tiles / targets off the front; the same two numpy calls are made here so
    that seed -> level is identical (pinned by the vectors in SURVEY.md §8c)."""
    if seed is not None:
        np.random.seed(seed)
    cells = [(r, c) for r in range(size) for c in range(size)]
    np.random.shuffle(cells)
    k, t = num_obstacles, num_tiles
    return cells[:k], cells[k:k + t], cells[k + t:k + 2 * t]


class TilerSliderEnvFactory:
    @staticmethod
    def create_simple_env(size=5, num_tiles=2, num_obstacles=3, seed=None, **kw):
        blocked, initial, targets = simple_level(size, num_tiles, num_obstacles, seed)
        return TilerSliderEnv(size=size, blocked_locations=blocked, initial_locations=initial,
                              target_locations=targets, multi_color=False, **kw)

    @staticmethod
    def create_from_string(board_str, multi_color=False, **kw):
        size, blocked, initial, targets = parse_board_string(board_str)
        return TilerSliderEnv(size=size, blocked_locations=blocked, initial_locations=initial,
                              target_locations=targets, multi_color=multi_color, **kw)

    @staticmethod
    def create_vec_env(n_envs, size=5, num_tiles=2, num_obstacles=3, seed=0, multi_color=False, max_steps=100, **kw):
        """N random boards generated on the GPU (same level distribution, counter-based stream)."""
        return VecTilerSliderEnv.random(n_envs, size=size, num_tiles=num_tiles, num_obstacles=num_obstacles,
                                        seed=seed, multi_color=multi_color, max_steps=max_steps, **kw)

    @staticmethod
    def create_vec_env_from_seeds(seeds, size=5, num_tiles=2, num_obstacles=3, max_steps=100, **kw):
        """One board per seed, each exactly the reference's create_simple_env(seed) level
        (environment.py:202-234: multi_color=False, max_steps=100), generated ON THE DEVICE by
        ts_generate_mt19937 — numpy's legacy MT19937 stream and list shuffle restated in HIP, one
        thread per seed.  `seeds`: integers in 0..2**32-1 (any sequence, numpy array or tensor)."""
        return VecTilerSliderEnv.from_seeds(seeds, size=size, num_tiles=num_tiles, num_obstacles=num_obstacles,
                                            multi_color=kw.pop("multi_color", False), max_steps=max_steps, **kw)

    @staticmethod
    def solvable_seeds(n, size=5, num_tiles=2, num_obstacles=3, multi_color=False, start_seed=0, min_moves=1, max_moves=None,
                       device=None, batch_size=1 << 16, capacity=4096):
        """The first `n` seeds >= start_seed, ascending (uint32 NumPy array), whose create_simple_env(size, num_tiles,
        num_obstacles, seed) level can be solved, in no fewer than `min_moves` and (if given) no more than `max_moves` moves.
        Most random levels cannot be solved at all (one in five at 4x4 with two tiles, one in ten at the reference's default
        shape: DESIGN.md section 11), and slides cannot be undone, so solvable levels have to be found: the seeds are turned into
        levels (ts_generate_mt19937) and solved (ts_solve) on the device, `batch_size` seeds at a time.  The result does not
        depend on batch_size.  Feed it to create_vec_env_from_seeds / VecTilerSliderEnv.from_seeds.  Raises ValueError when the
        seeds run out at 2**32 first.
        Shapes ts_solve refuses - an index space above 65,536 placements - are solved by the hashed search instead
        (ts_reach_solve, boards up to 8x8 with up to 8 tiles), each board within `capacity` reached states.  A board that reaches
        more (SOLVE_FULL) is NOT a found seed, whether or not it can be solved: the result then depends on `capacity`, but never
        on batch_size.  `capacity` plays no part for the shapes ts_solve takes."""
        import torch
        from . import _search_cabi as sc
        n, seed, batch_size = int(n), int(start_seed), max(1, int(batch_size))
        if n < 0 or not 0 <= seed <= 2**32 - 1:
            raise ValueError("n must be >= 0 and start_seed between 0 and 2**32 - 1")
        depth = sc.SOLVE_MAX_DEPTH if max_moves is None else max(0, min(int(max_moves), sc.SOLVE_MAX_DEPTH))
        found, have = [], 0
        while have < n:
            if seed > 2**32 - 1:
                raise ValueError(f"only {have} of {n} seeds found below 2**32")
            seeds = np.arange(seed, min(seed + batch_size, 2**32), dtype=np.int64)
            env = VecTilerSliderEnv.from_seeds(seeds, size=size, num_tiles=num_tiles, num_obstacles=num_obstacles, multi_color=multi_color,
                                               device=device, obs_dtype=None)
            hashed = sc.solve_states(env._dims) == 0
            moves = env.solve_reachable(depth, capacity, with_best=False).moves if hashed else env.solve_bits(depth, with_best=False)[0]
            # (searched no deeper than max_moves: a longer optimum reads SOLVE_DEPTH, which is negative like SOLVE_NONE)
            hit = seeds[torch.nonzero(moves >= int(min_moves)).flatten().cpu().numpy()]
            found.append(hit)
            have += hit.size
            seed += batch_size
        return (np.concatenate(found) if found else np.zeros(0, np.int64))[:n].astype(np.uint32)
