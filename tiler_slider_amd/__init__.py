"""tiler_slider_amd — MI355X-native vectorised Tiler-Slider environment.

Export names follow the reference package (ref: explainrl/environment/__init__.py:13-25):
GameState, TilerSliderEnv, TilerSliderEnvFactory, TextRender — plus the batched
VecTilerSliderEnv that is the point of this build.  Importing the package loads nothing
native; constructing an environment loads lib/libtiler_slider_hip.so and lib/libtiler_slider_update.so, the first solve()
lib/libtiler_slider_search.so, the first build_table() or lookup() lib/libtiler_slider_table.so, the first rollout()
lib/libtiler_slider_rollout.so, the first policy_logits() or rollout_policy() lib/libtiler_slider_policy.so, the first
trajectory_logits() lib/libtiler_slider_train.so, the first trajectory_outputs() lib/libtiler_slider_ac.so, the first
trajectory_returns() or trajectory_labels() lib/libtiler_slider_targets.so, the first actor_critic_loss() or trajectory_loss()
lib/libtiler_slider_loss.so, the first FusedAdam.step() lib/libtiler_slider_optim.so,
the first place_at_distance() lib/libtiler_slider_starts.so, the first build_policy_table(), walk_actions() or score_policy()
lib/libtiler_slider_ptable.so, the first solve_reachable() lib/libtiler_slider_reach.so, the first build_reach_table() or
lookup() of a ReachTable lib/libtiler_slider_rtable.so, the first rollout(policy="reach") or trajectory_labels() of a ReachTable
lib/libtiler_slider_rexpert.so, the first build_reach_index() or place_at_distance() of a ReachIndex
lib/libtiler_slider_rstarts.so, the first build_policy_table(), walk_actions() or score_policy() of a ReachTable
lib/libtiler_slider_rptable.so, the first lookahead() or td_targets() lib/libtiler_slider_lookahead.so, the first
rollout_policy(expert=...) lib/libtiler_slider_mixed.so, the first trajectory_vtrace() lib/libtiler_slider_vtrace.so, and each fails loudly if its library is missing (no CPU fallback).
"""
from ._ac_cabi import build_library as build_ac_library
from ._cabi import TilerSliderLibraryError, build_library
from ._lookahead_cabi import build_library as build_lookahead_library
from ._loss_cabi import build_library as build_loss_library
from ._mixed_cabi import build_library as build_mixed_library
from ._optim_cabi import build_library as build_optim_library
from ._policy_cabi import build_library as build_policy_library
from ._ptable_cabi import build_library as build_ptable_library
from ._reach_cabi import SOLVE_FULL
from ._reach_cabi import build_library as build_reach_library
from ._rexpert_cabi import build_library as build_rexpert_library
from ._rollout_cabi import build_library as build_rollout_library
from ._rptable_cabi import build_library as build_rptable_library
from ._rstarts_cabi import build_library as build_rstarts_library
from ._rtable_cabi import SOLVE_ABSENT
from ._rtable_cabi import build_library as build_rtable_library
from ._search_cabi import SOLVE_DEPTH, SOLVE_NONE
from ._search_cabi import build_library as build_search_library
from ._starts_cabi import build_library as build_starts_library
from ._table_cabi import TABLE_DEEP, TABLE_INVALID, TABLE_MAX_DEPTH, TABLE_NONE
from ._table_cabi import build_library as build_table_library
from ._targets_cabi import build_library as build_targets_library
from ._train_cabi import build_library as build_train_library
from ._update_cabi import build_library as build_update_library
from ._vtrace_cabi import build_library as build_vtrace_library
from .actor_critic import ActorCriticNet
from .env import GameState, TilerSliderEnv
from .factory import TilerSliderEnvFactory, simple_level
from .gym_wrapper import GymVecTilerSlider
from .lookahead import Lookahead
from .loss import LossInfo, actor_critic_loss, actor_critic_loss_grads
from .levels import ImageLoader, Level, pack_levels, parse_board_string
from .moves import Move
from .optim import FusedAdam
from .pipelined import PipelinedTilerSliderEnv
from .policy import MlpPolicy
from .ptable import PolicyScore, PolicyTable
from .render import TextRender
from .rptable import ReachPolicyTable
from .rstarts import ReachIndex
from .targets import RewardWeights, TrajectoryReturns
from .train import PolicyNet
from .vtrace import VtraceTargets
from .vec_env import DistanceTable, ReachResult, ReachTable, Rollout, StartInfo, StepInfo, VecTilerSliderEnv

__version__ = "0.1.0"
__all__ = ["GameState", "Move", "TilerSliderEnv", "TilerSliderEnvFactory", "ImageLoader", "TextRender",
           "VecTilerSliderEnv", "PipelinedTilerSliderEnv",
           "StepInfo", "GymVecTilerSlider", "Level", "pack_levels", "parse_board_string", "simple_level", "build_library",
           "build_search_library", "SOLVE_NONE", "SOLVE_DEPTH", "TilerSliderLibraryError",
           "DistanceTable", "build_table_library", "TABLE_MAX_DEPTH", "TABLE_INVALID", "TABLE_DEEP", "TABLE_NONE",
           "Rollout", "build_rollout_library", "MlpPolicy", "build_policy_library",
           "PolicyNet", "build_train_library", "RewardWeights", "TrajectoryReturns", "build_targets_library",
           "ActorCriticNet", "build_ac_library", "build_update_library",
           "LossInfo", "actor_critic_loss", "actor_critic_loss_grads", "build_loss_library",
           "FusedAdam", "build_optim_library", "StartInfo", "build_starts_library",
           "PolicyTable", "PolicyScore", "build_ptable_library",
           "ReachResult", "SOLVE_FULL", "build_reach_library",
           "ReachTable", "SOLVE_ABSENT", "build_rtable_library", "build_rexpert_library",
           "ReachIndex", "build_rstarts_library",
           "ReachPolicyTable", "build_rptable_library",
           "Lookahead", "build_lookahead_library", "build_mixed_library",
           "VtraceTargets", "build_vtrace_library"]
