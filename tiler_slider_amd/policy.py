"""Neural policies for the fused rollouts (lib/libtiler_slider_policy.so, include/tiler_slider_policy.h).

MlpPolicy holds a one-hidden-layer ReLU network in the kernels' layout; VecTilerSliderEnv.policy_logits() and
VecTilerSliderEnv.rollout_policy() are thin wrappers around the two functions at the bottom.  There is no CPU path and no torch
fallback: the logits and the actions come from k_policy_logits / k_policy_rollout or from nowhere.
"""
import ctypes as C

import torch

from . import _policy_cabi as pc


class MlpPolicy:
    """logits = w2 @ relu(w1 @ x + b1) + b2 on x = env.encode_onehot().flatten(1), the input a network trained on those planes
    expects.  Tensors come in torch.nn.Linear's layout - w1 [H, D], b1 [H], w2 [4, H], b2 [4], float32, all on one CUDA device -
    and are transposed once into the kernels' (w1 [D][H], w2 [H][4]); later changes to the originals are not seen.
    1 <= H <= 64; D is checked against the environment at every call."""

    def __init__(self, w1, b1, w2, b2):
        for name, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
            if t.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, got {t.dtype}")
            if t.device != w1.device:
                raise ValueError(f"{name} lives on {t.device}, w1 on {w1.device}")
        if w1.dim() != 2 or w1.shape[0] < 1 or w1.shape[0] > pc.POLICY_MAX_HIDDEN:
            raise ValueError(f"w1 must be [H, D] with 1 <= H <= {pc.POLICY_MAX_HIDDEN}, got {tuple(w1.shape)}")
        H, D = w1.shape
        if tuple(b1.shape) != (H,) or tuple(w2.shape) != (4, H) or tuple(b2.shape) != (4,):
            raise ValueError(f"with w1 [{H}, {D}]: b1 must be [{H}], w2 [4, {H}], b2 [4]; got {tuple(b1.shape)}, {tuple(w2.shape)}, {tuple(b2.shape)}")
        if w1.device.type != "cuda":
            raise ValueError(f"the network must live on the environment's GPU, got {w1.device}")
        self.hidden, self.features, self.device = int(H), int(D), w1.device
        self.w1 = w1.detach().t().contiguous()
        self.b1 = b1.detach().clone().contiguous()
        self.w2 = w2.detach().t().contiguous()
        self.b2 = b2.detach().clone().contiguous()

    @classmethod
    def from_linear(cls, l1, l2):
        """From two torch.nn.Linear layers (both with bias): l2(relu(l1(x)))."""
        if l1.bias is None or l2.bias is None:
            raise ValueError("both layers need a bias")
        return cls(l1.weight, l1.bias, l2.weight, l2.bias)

    @classmethod
    def from_kernel_layout(cls, w1, b1, w2, b2):
        """From tensors already in the kernels' layout - w1 [D, H], b1 [H], w2 [H, 4], b2 [4], float32, contiguous, on one CUDA
        device - whose storage the policy SHARES: nothing is cloned, and a later in-place change (an optimiser's step) is what the
        next call plays.  tiler_slider_amd.PolicyNet.policy() is this on its parameters."""
        for name, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
            if t.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, got {t.dtype}")
            if t.device != w1.device:
                raise ValueError(f"{name} lives on {t.device}, w1 on {w1.device}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous: its storage is shared, not copied")
        if w1.dim() != 2 or w1.shape[1] < 1 or w1.shape[1] > pc.POLICY_MAX_HIDDEN:
            raise ValueError(f"w1 must be [D, H] with 1 <= H <= {pc.POLICY_MAX_HIDDEN}, got {tuple(w1.shape)}")
        D, H = w1.shape
        if tuple(b1.shape) != (H,) or tuple(w2.shape) != (H, 4) or tuple(b2.shape) != (4,):
            raise ValueError(f"with w1 [{D}, {H}]: b1 must be [{H}], w2 [{H}, 4], b2 [4]; got {tuple(b1.shape)}, {tuple(w2.shape)}, {tuple(b2.shape)}")
        if w1.device.type != "cuda":
            raise ValueError(f"the network must live on the environment's GPU, got {w1.device}")
        self = cls.__new__(cls)
        self.hidden, self.features, self.device = int(H), int(D), w1.device
        self.w1, self.b1, self.w2, self.b2 = w1.detach(), b1.detach(), w2.detach(), b2.detach()
        return self

    def _mlp(self, env):
        """The ts_mlp of this network for `env`, validated against its shape and device."""
        D = env.onehot_channels * env.size * env.size
        if self.features != D:
            raise ValueError(f"the network reads {self.features} features, the environment's one-hot planes have "
                             f"{env.onehot_channels} x {env.size} x {env.size} = {D}")
        if self.device != env.device:
            raise ValueError(f"the network lives on {self.device}, the environment on {env.device}")
        return pc.Mlp(self.w1.data_ptr(), self.b1.data_ptr(), self.w2.data_ptr(), self.b2.data_ptr(), self.hidden, 0)

    def __repr__(self):
        return f"MlpPolicy(features={self.features}, hidden={self.hidden}, device={self.device})"


def _prepare(env, policy):
    env._require_open()
    if not env._started:
        raise RuntimeError("Call reset() before a policy call.")
    if env.host_mapped:
        raise ValueError("policy calls need device buffers (host_mapped=False)")
    if not isinstance(policy, MlpPolicy):
        raise TypeError(f"policy must be an MlpPolicy, got {type(policy)}")
    if not pc.policy_supported(env._dims, policy.hidden):
        from ._rollout_cabi import ROLLOUT_MAX_SIZE, ROLLOUT_MAX_TILES
        raise ValueError(f"policy rollouts play boards up to {ROLLOUT_MAX_SIZE}x{ROLLOUT_MAX_SIZE} with at most {ROLLOUT_MAX_TILES} tiles and "
                         f"{ROLLOUT_MAX_TILES} targets; {env.size}x{env.size} with {env.n_tiles} tiles and {env.n_targets} targets is beyond that")
    return policy._mlp(env)


def policy_logits(env, policy):
    """float32 [N, 4]: the network's logits on the boards as they stand.  One launch (ts_policy_logits); no state is touched."""
    mlp = _prepare(env, policy)
    out = torch.empty((env.num_envs, 4), dtype=torch.float32, device=env.device)
    if env.num_envs:
        env._call("ts_policy_logits", C.byref(env._dims), C.byref(env._state), C.byref(mlp), out.data_ptr(), binding=pc)
    return out


def rollout_policy(env, steps, policy, select="sample", epsilon=0.0, seed=0, step_index=0, board_offset=0, stats=True, log=(), advance=True):
    """VecTilerSliderEnv.rollout_policy: see there."""
    from ._rollout_cabi import ROLLOUT_MAX_STEPS
    from .vec_env import Rollout, _ptr
    mlp = _prepare(env, policy)
    if select not in pc.SELECTS:
        raise ValueError(f"select must be one of {sorted(pc.SELECTS)}, got {select!r}")
    steps = int(steps)
    if not 0 <= steps <= ROLLOUT_MAX_STEPS:
        raise ValueError(f"steps must be 0..{ROLLOUT_MAX_STEPS}")
    if not 0.0 <= float(epsilon) <= 1.0:
        raise ValueError("epsilon must be 0..1")
    N = env.num_envs
    cfg = pc.PolicyCfg(steps, env._mode, pc.SELECTS[select], 1 if advance else 0, int(seed) & (2**64 - 1), int(step_index), int(board_offset),
                       int(round(float(epsilon) * 2**32)))
    names = env._ROLLOUT_STATS if stats is True else () if not stats else tuple(stats)
    logs = (log,) if isinstance(log, str) else tuple(log)
    all_logs = env._ROLLOUT_LOGS + ("logits", "start")
    if set(names) - set(env._ROLLOUT_STATS) or set(logs) - set(all_logs):
        raise ValueError(f"stats are {env._ROLLOUT_STATS}, logs {all_logs}")
    got = {name: torch.zeros(N, dtype=torch.uint8 if name == "flags" else torch.int32, device=env.device) for name in names}
    for name in logs:
        if name == "start":
            continue
        shape = {"pos": (steps, env.n_tiles, N), "logits": (steps, N, 4)}.get(name, (steps, N))
        dtype = env._pos.dtype if name == "pos" else torch.float32 if name == "logits" else torch.uint8
        got[name + "_log"] = torch.zeros(shape, dtype=dtype, device=env.device)
    bound = dict(got)
    if advance:  # the environment's own flag byte becomes the last step's, as after step(); a Rollout's `flags` is then that tensor
        bound["flags"] = env._flags
        if "flags" in got:
            got["flags"] = env._flags
    out = pc.PolicyOut(*(_ptr(bound.get(f)) for f in pc.OUT_FIELDS))
    if "start" in logs:  # the cells before the launch: with advance=True the launch overwrites the only other copy
        got["start_pos"] = env._pos.clone()
    if steps and N and bound:
        env._call("ts_policy_rollout", C.byref(env._dims), C.byref(env._state), C.byref(mlp), C.byref(cfg), C.byref(out), binding=pc)
        if advance and env.obs_dtype is not None:  # one encode into the current buffer: env._obs stays truthful
            env._call("ts_encode" if env.obs_dtype == torch.float32 else "ts_encode_u8", C.byref(env._dims), C.byref(env._state), _ptr(env._obs))
            env._sync_shown()
    return Rollout(steps, **got)
