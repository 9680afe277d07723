"""The fused optimiser (lib/libtiler_slider_optim.so, include/tiler_slider_optim.h): clip_grad_norm_, AdamW and zero_grad over
the handful of small tensors of a PolicyNet or an ActorCriticNet in ONE launch.

FusedAdam is a torch.optim.Optimizer: `opt.step()` is one ts_adam_step on the current stream, with no host synchronisation -
the global norm, the count of applied and of skipped updates live on the device (opt.grad_norm, opt.steps_applied,
opt.steps_skipped).  torch's optimisers stay what they were: this is an opt-in.  There is no CPU path and no torch fallback.
"""
import ctypes as C

import torch

from . import _optim_cabi as oc


class FusedAdam(torch.optim.Optimizer):
    """AdamW (decoupled weight decay; weight_decay = 0 is Adam) with clip_grad_norm_'s global-norm clip in front, one launch per
    step on networks up to the library's one-block constant, three deterministic launches beyond.

        opt = FusedAdam(net.parameters(), lr=1e-2, max_grad_norm=1.0)
        loss.backward(); opt.step(zero_grad=True)

    max_grad_norm=None (or 0) does not clip.  skip_nonfinite: a step whose global gradient norm is Inf or NaN changes no
    parameter and no moment and counts in opt.steps_skipped instead of opt.steps_applied - decided on the device.
    `lr` may be a 0-dim float32 tensor on the parameters' device: the launch reads it, so a schedule that writes it in place works
    inside a captured graph.

    ONE parameter group (the norm is global); float32, contiguous parameters on one CUDA device with dense gradients; at most 32
    parameters with a gradient in a step.  Parameters whose .grad is None are left out of the step, as torch leaves them out.
    THE ONE DIFFERENCE FROM torch.optim.AdamW: the bias correction uses this optimiser's single device counter (steps_applied),
    not a step count per parameter - a parameter that sat out some steps is corrected as if it had taken them.

    Not built: amsgrad, coupled (L2) decay, several groups, bf16 state."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=True):
        if not isinstance(lr, torch.Tensor) and not lr >= 0.0:
            raise ValueError(f"invalid learning rate: {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas: {betas}")
        if not eps >= 0.0 or not weight_decay >= 0.0:
            raise ValueError(f"invalid eps or weight_decay: {eps}, {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError(f"invalid max_grad_norm: {max_grad_norm}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, skip_nonfinite=bool(skip_nonfinite))
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f"FusedAdam takes one parameter group (the gradient norm is global), got {len(self.param_groups)}")
        ps = self.param_groups[0]["params"]
        for p in ps:
            self._check_param(p)
        if len({p.device for p in ps}) != 1:
            raise ValueError("the parameters must live on one CUDA device")
        self._device = ps[0].device
        self._counters = torch.zeros(2, dtype=torch.int64, device=self._device)
        self._grad_norm = torch.zeros(1, dtype=torch.float32, device=self._device)
        self._workspace = torch.empty(oc.workspace_bytes(1), dtype=torch.uint8, device=self._device)  # the grid is bounded: so is this
        self._out = oc.OptimOut(self._counters.data_ptr(), self._grad_norm.data_ptr(), self._workspace.data_ptr())
        self._key, self._tensors = None, None

    @staticmethod
    def _check_param(p):
        if p.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
            raise ValueError(f"FusedAdam needs contiguous float32 CUDA parameters, got {p.dtype} {tuple(p.shape)} on {p.device}"
                             f"{'' if p.is_contiguous() else ', not contiguous'}")

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("FusedAdam takes one parameter group (the gradient norm is global)")
        super().add_param_group(param_group)

    # ---- the device's scalars: 0-dim views, reading one synchronises, nothing else does
    @property
    def grad_norm(self):
        """float32: the global gradient norm of the last step, before clipping."""
        return self._grad_norm[0]

    @property
    def steps_applied(self):
        return self._counters[0]

    @property
    def steps_skipped(self):
        return self._counters[1]

    def _gather(self, group):
        """The ts_optim_tensors of the parameters that have a gradient; built again only when a pointer changed."""
        live = [p for p in group["params"] if p.grad is not None]
        if len(live) > oc.MAX_TENSORS:
            raise ValueError(f"{len(live)} parameters with a gradient: one call takes at most {oc.MAX_TENSORS}")
        rows = []
        for p in live:
            g = p.grad
            if g.is_sparse or g.layout != torch.strided:
                raise ValueError("FusedAdam needs dense gradients")
            if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or not p.is_contiguous():
                raise ValueError("FusedAdam needs contiguous float32 gradients on the parameter's device")
            st = self.state[p]
            if "exp_avg" not in st:  # lazily, as torch does
                st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format), torch.zeros_like(p, memory_format=torch.contiguous_format)
            rows.append((p.numel(), p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()))
        key = tuple(rows)
        if key != self._key:
            t = oc.OptimTensors(n_tensors=len(rows))
            for i, (n, pp, gp, mp, vp) in enumerate(rows):
                t.numel[i], t.param[i], t.grad[i], t.m[i], t.v[i] = n, pp, gp, mp, vp
            self._key, self._tensors = key, t
        return self._tensors

    def init_state(self):
        """Create the moments of every parameter that has a gradient now; the first step() does otherwise.  Call it before a
        step() is captured into a graph, so that nothing is allocated inside the capture."""
        self._gather(self.param_groups[0])

    @torch.no_grad()
    def step(self, closure=None, zero_grad=False):
        """One ts_adam_step on the current stream.  zero_grad: the launch leaves every gradient it read at 0 (what
        zero_grad(set_to_none=False) does, without its launches)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        tensors = self._gather(group)
        lr = group["lr"]
        lr_dev = None
        if isinstance(lr, torch.Tensor):
            if lr.device.type == "cuda":
                if lr.device != self._device or lr.dtype != torch.float32 or lr.numel() != 1:
                    raise ValueError("a tensor lr must be one float32 on the parameters' device")
                lr_dev, lr = lr.data_ptr(), 0.0
            else:
                lr = float(lr)
        beta1, beta2 = group["betas"]
        cfg = oc.AdamCfg(beta1, beta2, lr_dev, lr, group["eps"], group["weight_decay"], group["max_grad_norm"] or 0.0,
                         int(bool(group["skip_nonfinite"])), int(bool(zero_grad)))
        with torch.cuda.device(self._device):
            rc = oc.lib().ts_adam_step(C.byref(tensors), C.byref(cfg), C.byref(self._out), torch.cuda.current_stream(self._device).cuda_stream)
        if rc:
            oc.check(rc, "ts_adam_step")
        return loss

    def state_dict(self):
        """torch's, plus the device counters under "fused_adam"."""
        d = super().state_dict()
        d["fused_adam"] = {"counters": self._counters.clone(), "grad_norm": self._grad_norm.clone()}
        return d

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        own = state_dict.pop("fused_adam", None)
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError("FusedAdam takes one parameter group")
        for st in self.state.values():
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    st[k] = st[k].to(dtype=torch.float32).contiguous().clone()      # torch hands over the dict's own tensors: never share moments
        if own is not None:
            self._counters.copy_(own["counters"])
            self._grad_norm.copy_(own["grad_norm"])
        self._key = None
