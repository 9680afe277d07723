"""The quad store of the in-place step's two-tile kernels on the GPU (csrc/ts_update.hip, csrc/ts_quad.h): the four lanes of a quad
store the changed cells of one board after another, so a lane stores for its neighbours - lanes past the batch included - and
nothing may depend on which lane issued a store.  Everything here is byte for byte against ts_step, the CPU oracle and
ts_encode of the final state; the helpers are those of tests/test_gpu_update.py, the levels those of tests/update_cases.py."""
import itertools

import numpy as np
import pytest

import table_harness as th
import update_cases as cases
from test_gpu_update import _Raw, _between_guards, _compare_run, _launches, _oracle_run, _upload, torch_cuda  # noqa: F401 (fixture)
from update_cases import ACTION_SEED, AUTORESET, INVALID_MOVE, LEVEL_SEED, TIMEOUT, VOID

pytestmark = pytest.mark.gpu

STEPS = 24
# The bodies of the two-tile kernels, by the case table's shapes: <4, 2> two tiles and two targets, the straight-line body;
# <5, 2> two tiles and one target, the general body with both tiles' slots in use; <3, 2> one tile and no target, the general
# body with the second tile's slots never present.
STEMS = ("k_step_update<4, 2, ", "k_step_update<5, 2, ", "k_step_update<3, 2, ")
# a quad and its neighbours (1 .. 5: lanes past the batch store for live boards), either side of a wave, either side of a block
BATCHES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257)


def _check_guards(a, held, what):
    """Every guarded buffer of the in-place copy: guard bytes intact, inputs unwritten, outputs equal to the ts_step twin's."""
    for f, (g, before) in held.items():
        try:
            now = th.payload(g, before.dtype, before.shape)  # asserts the guard bytes
        except AssertionError as e:
            raise AssertionError((what, f, str(e))) from None
        if f in ("init", "tgt", "blk"):
            assert np.array_equal(now, before), (what, f, "an input was written")
        else:
            assert np.array_equal(now, getattr(a, "pos" if f == "shown" else f).cpu().numpy()), (what, f)


def _final_encoding(torch, b, what):
    full = torch.empty_like(b.obs)
    b.encode(into=full)
    assert torch.equal(b.obs, full), (what, "the observation against ts_encode of the final state")


@pytest.mark.parametrize("mc", (True, False), ids=("multi", "single"))
@pytest.mark.parametrize("stem", STEMS)
def test_quad_store_over_small_and_boundary_batches(torch_cuda, oracle, stem, mc):
    """Both bodies, both observation types, both colour modes, both step modes, batches of 1 .. 5, 63 .. 65 and 255 .. 257
    boards, 24 steps with max_steps 6, every buffer of the in-place copy between guard bytes.  After every step pos, step_count,
    done, flags, reward and the observation equal ts_step's and the oracle's and shown == pos; after the last one the
    observation is ts_encode of the final state, no guard byte has changed and no input was written."""
    torch = torch_cuda
    S, T, Tt, K = cases.CASES[stem + "false>"]
    for N in BATCHES:
        lv = cases.levels(oracle, stem + "false>", N, mc)
        for mode in (oracle.MODE_AUTORESET, oracle.MODE_STRICT):
            run = _oracle_run(oracle, S, mc, 6, lv, mode, STEPS)
            for u8 in (False, True):
                what = (stem, N, mc, mode, u8)
                a = _Raw(torch, S, T, Tt, mc, 6, *lv, u8)
                b = _Raw(torch, S, T, Tt, mc, 6, *lv, u8)
                assert _launches(b, stem + ("true>" if u8 else "false>"))
                b.show()
                held = _between_guards(torch, b)
                bad = _compare_run(torch, a, b, _upload(torch, run), mode)
                assert not bad, (what, bad[:8])
                _final_encoding(torch, b, what)
                _check_guards(a, held, what)


def _roles_pool(oracle, mc):
    """Of 512 levels of the 4x4 / 2 tiles / 2 targets / 2 obstacles shape: (levels, boards with an action that moves both tiles
    and the cells they reach, boards with an action that moves nothing), by the oracle's own single steps."""
    blk, init, tgt = oracle.generate(4, 2, 2, 2, 512, seed=LEVEL_SEED)
    both, none = {}, {}
    for act in range(4):
        ref = oracle.OracleBatch(4, mc, 1 << 20, blk, init, tgt)
        ref.reset()
        flags = ref.step(np.full(512, act, np.uint8), mode=oracle.MODE_STRICT, obs=False)["flags"]
        for i in np.flatnonzero(((flags & (VOID | INVALID_MOVE)) == 0) & (ref.pos[0] != init[0]) & (ref.pos[1] != init[1])).tolist():
            both.setdefault(i, (act, ref.pos[:, i].copy()))
        for i in np.flatnonzero((flags & INVALID_MOVE) != 0).tolist():
            none.setdefault(i, act)
    assert len(both) >= 24 and len(none) >= 24, (len(both), len(none))
    return (blk, init, tgt), sorted(both.items()), sorted(none.items())


def test_the_four_boards_of_a_quad_differ_in_the_same_step(torch_cuda, oracle):
    """99 boards of the straight-line body: 24 quads hold, in each of the 24 orders, a board that is done on entry (reset in
    autoreset mode, left alone in strict mode), one with an action above 3, one where both tiles move and one where nothing
    moves; the last quad is cut after three boards.  The oracle's flags of the first step say that each board plays its part;
    the run then goes on for 8 steps of the usual action stream.  Both colour modes, both step modes, float32 and uint8."""
    torch = torch_cuda
    for mc in (True, False):
        (blk, init, tgt), both, none = _roles_pool(oracle, mc)
        pick, act0, role, away = [], [], [], []
        for q, order in enumerate(itertools.chain(itertools.permutations(range(4)), [(2, 0, 3)])):
            for r in order:
                far, (_, cells) = both[(q + 7) % len(both)]  # the done board stands where a move took it: a reset redraws both tiles
                board, act = {0: (far, 1), 1: (5 * q + 2, 4 + q), 2: (both[q % len(both)][0], both[q % len(both)][1][0]),
                              3: none[q % len(none)]}[r]
                pick.append(board), act0.append(act), role.append(r), away.append(cells)
        pick, act0, role, away = np.array(pick), np.array(act0, np.uint8), np.array(role), np.array(away, np.uint8).T
        N = len(pick)
        assert N == 99
        lv = tuple(np.ascontiguousarray(x[:, pick]) for x in (blk, init, tgt))
        start = np.where(role == 0, away, lv[1])  # the cells on entry
        assert (start[:, role == 0] != lv[1][:, role == 0]).all()
        for mode in (oracle.MODE_AUTORESET, oracle.MODE_STRICT):
            ref = oracle.OracleBatch(4, mc, 6, *lv)
            ref.reset()
            ref.pos[:] = start
            ref.done[role == 0] = 1
            ref.step_count[role == 0] = 3
            run = []
            for k in range(9):
                act = act0 if k == 0 else oracle.fill_actions(N, seed=ACTION_SEED, step_index=k)
                before = ref.pos.copy()
                want = ref.step(act, mode=mode, reward=True)
                run.append(dict(act=act, obs=want["obs"], flags=want["flags"], reward=want["reward"], pos=ref.pos.copy(),
                                step_count=ref.step_count.copy(), done=ref.done.copy()))
                if k == 0:
                    f = want["flags"]
                    assert (f[role == 0] == (0x20 if mode == oracle.MODE_AUTORESET else 0x10)).all()
                    assert (f[role == 1] == 0x40).all() and ((f[role == 3] & INVALID_MOVE) != 0).all()
                    moved = (ref.pos != before).all(axis=0)
                    assert ((f[role == 2] & (VOID | INVALID_MOVE)) == 0).all() and moved[role == 2].all()
                    assert moved[role == 0].all() if mode == oracle.MODE_AUTORESET else not moved[role == 0].any()
                    assert not moved[(role == 1) | (role == 3)].any()
            for u8 in (False, True):
                what = (mc, mode, u8)
                a = _Raw(torch, 4, 2, 2, mc, 6, *lv, u8)
                b = _Raw(torch, 4, 2, 2, mc, 6, *lv, u8)
                assert _launches(b, f"k_step_update<4, 2, {'true' if u8 else 'false'}>")
                for raw in (a, b):
                    raw.pos.copy_(torch.from_numpy(start))
                    raw.done[torch.from_numpy(role == 0).cuda()] = 1
                    raw.step_count[torch.from_numpy(role == 0).cuda()] = 3
                b.show()
                held = _between_guards(torch, b)
                bad = _compare_run(torch, a, b, _upload(torch, run), mode)
                assert not bad, (what, bad[:8])
                _final_encoding(torch, b, what)
                _check_guards(a, held, what)


def test_cell_ids_past_the_board_and_two_tiles_on_one_cell(torch_cuda, oracle):
    """pos is overwritten between steps - ids >= S*S (the descriptor's cell is the clamped one), two tiles on one cell (two slots
    of one word address one float) - and shown is left alone; 5 boards and 66, both two-tile shapes with two tiles, float32 and
    uint8: the next step's observation is ts_encode of the new state and every field equals ts_step's from the same cells."""
    torch = torch_cuda
    for stem in STEMS[:2]:
        S, T, Tt, K = cases.CASES[stem + "false>"]
        for N in (5, 66):
            for mc in (True, False):
                lv = cases.levels(oracle, stem + "false>", N, mc)
                for u8 in (False, True):
                    a = _Raw(torch, S, T, Tt, mc, 6, *lv, u8)
                    b = _Raw(torch, S, T, Tt, mc, 6, *lv, u8)
                    assert _launches(b, stem + ("true>" if u8 else "false>"))
                    b.show()
                    held = _between_guards(torch, b)
                    for k in range(9):
                        act = torch.from_numpy(oracle.fill_actions(N, seed=ACTION_SEED, step_index=k)).cuda()
                        edit = a.pos.clone()
                        if k % 3 == 0:
                            edit[0, ::3] = 200           # ids >= S*S: clamped like everywhere else
                            edit[1, 1::4] = S * S
                            edit[:, 2::5] = 255          # both tiles past the board: both clamp to the last cell
                        elif k % 3 == 1:
                            edit[1, ::2] = edit[0, ::2]  # two tiles on one cell: the higher index is drawn
                        a.pos.copy_(edit)
                        b.pos.copy_(edit)                # shown still holds the cells of the step before
                        for mode in (oracle.MODE_AUTORESET, oracle.MODE_STRICT):
                            what = (stem, N, mc, u8, k, mode)
                            a.step(act, mode)
                            b.step_update(act, mode)
                            _final_encoding(torch, b, what)
                            for f, t in a.fields().items():
                                assert torch.equal(t, b.fields()[f]), (what, f)
                            assert torch.equal(b.shown, b.pos), (what, "shown")
                    _check_guards(a, held, (stem, N, mc, u8))


def test_max_steps_1(torch_cuda, oracle):
    """max_steps = 1 on the two-tile kernels' two bodies, 5 and 257 boards: every played step times out and in autoreset mode
    every other step is a reset, so every other step every board of every quad redraws both tiles."""
    torch = torch_cuda
    for stem in STEMS[:2]:
        S, T, Tt, K = cases.CASES[stem + "false>"]
        for N in (5, 257):
            for mc in (True, False):
                lv = cases.levels(oracle, stem + "false>", N, mc)
                for mode in (oracle.MODE_AUTORESET, oracle.MODE_STRICT):
                    run = _oracle_run(oracle, S, mc, 1, lv, mode, 8)
                    flags = np.stack([row["flags"] for row in run])
                    played = (flags & VOID) == 0
                    assert ((flags[played] & TIMEOUT) != 0).all() and played[0].sum() >= N - 2
                    if mode == oracle.MODE_AUTORESET:
                        assert int(((flags & AUTORESET) != 0).sum()) >= 4 * (N - 8)
                    for u8 in (False, True):
                        what = (stem, N, mc, mode, u8)
                        a = _Raw(torch, S, T, Tt, mc, 1, *lv, u8)
                        b = _Raw(torch, S, T, Tt, mc, 1, *lv, u8)
                        assert _launches(b, stem + ("true>" if u8 else "false>"))
                        b.show()
                        held = _between_guards(torch, b)
                        bad = _compare_run(torch, a, b, _upload(torch, run), mode)
                        assert not bad, (what, bad[:8])
                        _final_encoding(torch, b, what)
                        _check_guards(a, held, what)


def test_uint8_observation_at_an_odd_address(torch_cuda, oracle):
    """The header asks no alignment of a uint8 observation: the in-place copy's starts 1 and 3 bytes into its allocation, on both
    bodies of the two-tile kernels, 5 and 331 boards.  Contents equal the ts_step twin's and the oracle's after every step; no
    byte of the allocation outside the view changes."""
    torch = torch_cuda
    for stem in STEMS[:2]:
        name = stem + "true>"
        S, T, Tt, K = cases.CASES[name]
        for N in (5, 331):
            mc = S % 2 == 0
            lv = cases.levels(oracle, name, N, mc)
            want = _upload(torch, _oracle_run(oracle, S, mc, 6, lv, oracle.MODE_AUTORESET, 12))
            for off in (1, 3):
                a = _Raw(torch, S, T, Tt, mc, 6, *lv, True)
                b = _Raw(torch, S, T, Tt, mc, 6, *lv, True)
                n = b.obs.numel()
                b.whole = torch.full((n + 2 * th.GUARD,), 99, dtype=torch.uint8, device="cuda")
                b.obs = b.whole[th.GUARD + off:th.GUARD + off + n].view(N, S, S, 3)
                b.bind()
                assert b.obs.data_ptr() % 4 == off and a.obs.data_ptr() % 4 == 0 and _launches(b, name)
                b.obs.copy_(a.encode())  # the contract on entry: the full encoding, written by other means
                b.shown.copy_(b.pos)
                bad = _compare_run(torch, a, b, want, oracle.MODE_AUTORESET)
                assert not bad, (name, N, off, bad[:8])
                full = torch.empty_like(a.obs)
                b.encode(into=full)
                assert torch.equal(b.obs, full), (name, N, off, "ts_encode_u8 of the final state")
                assert bool((b.whole[:th.GUARD + off] == 99).all()) and bool((b.whole[th.GUARD + off + n:] == 99).all()), (name, N, off)
