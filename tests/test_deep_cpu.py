"""The deep fixture and its chain policies, held to the CPU yardsticks alone (no GPU, no kernel): tests/golden/deep_levels.npz is
what tools/find_deep_levels.py says it is, and tests/deep_cases.py gives tests/test_gpu_deep.py the inputs it is written for.

Measured with table_reference.exact and ptable_reference.walk_exact over the oracle:

    level                                                  states   valid  deepest D  placements at distance >= 36
    8x8 two tiles multi colour                               4096    2550      106        722
    8x8 two tiles single colour                              4096    2550       58        312
    8x8 two tiles three targets one repeated single colour   4096    2550       58        312
    5x5 two tiles multi colour                                625     306       37          3
    5x5 three tiles multi colour                            15625    4080       61       2515

    chain policy (deep_cases.CHAIN_SEED)     longest chain L   placements at chain length >= 128    > 252
    8x8 two tiles multi colour                     137                  141                            0
    5x5 two tiles multi colour                      79                    0                            0
    5x5 three tiles multi colour                   341                 3308                         1603
"""
import os

import numpy as np
import pytest

import deep_cases as dc
import ptable_reference as xref
import table_reference as tref


def _finite(d):
    return (d >= 0) & (d < tref.UNREACHABLE)


def test_the_fixture_is_small_and_holds_the_five_levels():
    assert os.path.getsize(dc.FIXTURE) < 8192
    lv = dc.levels()
    assert set(lv) == {dc.MULTI, dc.SINGLE, dc.REPEATED, dc.SMALL, dc.LARGE}
    shape = lambda n: (lv[n].S, lv[n].T, lv[n].Tt, lv[n].mc)
    assert shape(dc.MULTI) == (8, 2, 2, True) and shape(dc.SINGLE) == (8, 2, 2, False) and shape(dc.SMALL)[:2] == (5, 2)
    assert np.array_equal(lv[dc.MULTI].blk, lv[dc.SINGLE].blk) and np.array_equal(lv[dc.MULTI].tgt, lv[dc.SINGLE].tgt)     # the same layout
    assert (lv[dc.LARGE].S ** 2) ** lv[dc.LARGE].T >= 15625
    r = lv[dc.REPEATED]
    assert not r.mc and r.T != r.Tt and len(set(r.tgt[:, 0].tolist())) < r.Tt


@pytest.mark.parametrize("name", (dc.MULTI, dc.SINGLE, dc.REPEATED, dc.SMALL, dc.LARGE))
def test_the_recorded_depth_is_the_yardsticks_and_beyond_the_shallow_suite(oracle, name):
    lv = dc.levels()[name]
    dist = dc.exact(oracle, lv)
    D = dc.deepest(dist)
    n_deep = int((_finite(dist) & (dist >= dc.DEEP_FROM)).sum())
    print(f"{name}: D = {D}, {n_deep} placements at distance >= {dc.DEEP_FROM}, {(dist >= 0).sum()} valid of {dist.size}")
    assert D == lv.deepest and D > 35
    assert dist[tref.index_of(lv.S, lv.init)[0]] == D                   # init stands at the deepest distance
    present = np.bincount(dist[_finite(dist)], minlength=D + 1)
    assert (present > 0).all()                                          # every distance 0 .. D is held: every round stores
    if name == dc.MULTI:
        assert D >= 64 and n_deep >= 200
        assert all(present[lo:lo + 10].sum() >= 50 for lo in range(40, 100, 10))
    # the cuts the GPU tests run fall INSIDE the level (DEEP) and the default one beyond it (NONE)
    unreachable = int((dist == tref.UNREACHABLE).sum())
    for depth in (252, D + 1):                                          # R(D + 1) is empty: the level ends first
        cut = tref.cut(dist[None, :], depth)[0]
        assert not (cut == tref.DEEP).any() and (cut == tref.NONE).sum() == unreachable and (cut == D).any()
    for depth in (D, D - 1, 36):                                        # at D every distance is stored and R(D) is not empty: DEEP
        if depth == D and not unreachable:
            continue
        cut = tref.cut(dist[None, :], depth)[0]
        beyond = int((_finite(dist) & (dist > depth)).sum())
        assert not (cut == tref.NONE).any() and (cut == tref.DEEP).sum() == unreachable + beyond > 0 and (beyond > 0) == (depth < D)


def test_the_boards_that_share_a_wave_with_the_deep_level_stop_early(oracle):
    lv = dc.levels()[dc.MULTI]
    c = dc.companions(lv)
    d = {k: dc.exact(oracle, v) for k, v in c.items()}
    assert 1 <= dc.deepest(d["shallow"]) <= 3 and (d["shallow"] == tref.UNREACHABLE).any()
    assert not _finite(d["never won"]).any() and (d["never won"] == tref.UNREACHABLE).sum() == (dc.exact(oracle, lv) >= 0).sum()
    assert sorted(d["won or stuck"][d["won or stuck"] >= 0].tolist()) == [0, tref.UNREACHABLE]


def _links_go_down_by_one(oracle, lv, act, chain):
    succ = xref.successors(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, act[None, :])[0]
    on = _finite(chain) & (chain >= 1)
    assert (act[on] <= 3).all() and (act[~on] == xref.NO_ACTION).all()
    assert np.array_equal(chain[succ[on]], chain[on] - 1)


def test_the_chain_policy_of_the_8x8_level(oracle):
    lv = dc.levels()[dc.MULTI]
    act, chain = dc.chain_policy(oracle, lv)
    L, n128 = dc.longest(chain), int((_finite(chain) & (chain >= 128)).sum())
    print(f"{lv.name}: longest chain L = {L}, {n128} placements at chain length >= 128")
    assert L >= 128 and n128 >= 50
    _links_go_down_by_one(oracle, lv, act, chain)
    # the tree spans everything that can win: the policy solves what the level allows, by detours
    dist = dc.exact(oracle, lv)
    assert np.array_equal(_finite(chain), _finite(dist)) and (chain >= dist).all()
    # deterministic
    dc._chains.clear()
    again, _ = dc.chain_policy(oracle, lv)
    assert np.array_equal(again, act)
    # bytes >= 128 right and left of the int8 boundary, and the cuts of the GPU walk tests
    walked = xref.walk(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, act[None, :])[0]
    assert {127, 128, 129, L} <= set(walked.tolist()) and not (walked == tref.DEEP).any()
    for depth in (128, 127, L - 1):
        assert (xref.walk(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, act[None, :], depth)[0] == tref.DEEP).any()


def test_a_chain_beyond_252_puts_deep_into_a_table_at_the_default_cut(oracle):
    """On the 5x5 level of three tiles the depth-first tree is deeper than TS_TABLE_MAX_DEPTH, so the
    walk at the DEFAULT cut holds 252 next to DEEP."""
    lv = dc.levels()[dc.LARGE]
    act, chain = dc.chain_policy(oracle, lv)
    L = dc.longest(chain)
    print(f"{lv.name}: longest chain L = {L}, {(_finite(chain) & (chain > 252)).sum()} placements beyond 252")
    assert L > 253 and (chain == 252).any() and (chain == 253).any()
    _links_go_down_by_one(oracle, lv, act, chain)
    walked = xref.walk(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, act[None, :])[0]
    assert np.array_equal(walked == tref.DEEP, _finite(chain) & (chain > 252) | (chain == tref.UNREACHABLE))
    assert (walked == 252).any() and (walked == tref.DEEP).sum() >= 100


def test_the_small_level_has_chains_beyond_its_depth(oracle):
    lv = dc.levels()[dc.SMALL]
    act, chain = dc.chain_policy(oracle, lv)
    print(f"{lv.name}: longest chain L = {dc.longest(chain)}")
    assert dc.longest(chain) >= 64
    _links_go_down_by_one(oracle, lv, act, chain)


@pytest.mark.parametrize("name", (dc.MULTI, dc.LARGE))
def test_the_score_of_a_chain_policy_has_long_detours(oracle, name):
    lv = dc.levels()[name]
    act, _ = dc.chain_policy(oracle, lv)
    table = tref.cut(dc.exact(oracle, lv)[None, :])
    walked = xref.walk(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, act[None, :])
    score = xref.score(oracle, lv.S, lv.mc, lv.blk, lv.tgt, lv.T, walked, act[None, :], table)[0]
    both = (walked >= 1) & (walked <= 252) & (table >= 1) & (table <= 252)
    excess = np.where(both, walked.astype(np.int64) - table, 0)[0]
    print(f"{name}: valid / solvable / solved / optimal / agree / excess / deep / won {score.tolist()}, excess > 0 on {(excess > 0).sum()}, largest {excess.max()}")
    assert score[5] == excess.sum() and (excess > 0).sum() >= 100 and excess.max() >= 100
    assert 0 < score[3] < score[2] and score[4] < score[1]              # some optimal, most not
