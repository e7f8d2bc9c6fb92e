"""Fused Adam for the joint HRNet + ShiftNet update.

Drop-in for the reference's `optim.Adam(list(fusion_model.parameters()) + list(regis_model.parameters()), lr=...)`
(src/train.py:252) including `lr_scheduler.ReduceLROnPlateau` on top of it (train.py:253): same constructor arguments,
`param_groups`, `zero_grad()`, `step()`, `state_dict()` surface, torch.optim.Adam's arithmetic (no amsgrad).

What is different underneath: every parameter of a group is re-homed into ONE flat fp32 device buffer (the parameters
become views of it), their gradients live in one flat buffer as well (`p.grad` are views), and `step()` is a single
`hrn_adam_step` launch per group instead of ~10 framework kernels per tensor.  The flat gradient buffer is also what
the data-parallel exchange reduces (`allreduce()`, between `loss.backward()` and `step()`): with `overlap_early=regis_model.parameters()`
ShiftNet's 137 MB slice goes on the wire from a backward hook as soon as `hrn_shiftnet_backward` has written it, under the whole
HRNet backward pass; `allreduce()` then reduces HRNet's 2.4 MB and waits (hrnet_hip.dist.GradBuckets).

Beyond torch.optim.Adam, all on the device and without a host sync (csrc/optim_guard.hip; any of the four keyword arguments switches
`step()` from the one `adam_step` launch to `grad_sumsq` per group, then `optim_prepare` + `adam_step_ex` per group):
  max_grad_norm           clip by the global norm over every group, `clip_grad_norm_`'s coefficient min(1, max / (norm + 1e-6)).  Unlike
                          `clip_grad_norm_` the gradient buffers are NOT rewritten (the scaled gradient exists in registers only: `.grad`
                          still holds the unclipped values after `step()`), and the squares are summed in fp64, so gradients beyond
                          2e19 clip to the right coefficient instead of to 0.
  guard                   a step with a NaN or an infinity anywhere in any group's gradient changes nothing - parameters, moments, EMA
                          and the step count of the bias corrections - and is counted in `step_counts()[1]`.  The other three imply it.
  decoupled_weight_decay  torch.optim.AdamW: p *= 1 - lr weight_decay instead of g += weight_decay p.
  ema_decay               an exponential moving average of the weights, ema = decay ema + (1 - decay) p after every applied step
                          (`ema_parameters()`, `with optimizer.ema_weights():` to validate or save on the averaged weights).
After `allreduce()` every rank holds the same gradient, so every rank clips and skips alike with no further communication.
"""
import contextlib

import torch

from . import binding


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, overlap_early=None, *, max_grad_norm=None,
                 decoupled_weight_decay=False, ema_decay=None, guard=False):
        """overlap_early: parameters (consecutive in `params`, e.g. `regis_model.parameters()`) whose gradients autograd completes
        first: their slice of the flat gradient buffer is all-reduced from a backward hook while the rest of the backward pass
        still runs (hrnet_hip.dist.GradBuckets); `allreduce()` then only has the remainder left."""
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameters")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be positive (got {max_grad_norm}); None for no clipping")
        if ema_decay is not None and not 0 <= ema_decay < 1:
            raise ValueError(f"ema_decay must be in [0, 1) (got {ema_decay})")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm, self.decoupled_weight_decay, self.ema_decay = max_grad_norm, bool(decoupled_weight_decay), ema_decay
        self._extended = max_grad_norm is not None or self.decoupled_weight_decay or ema_decay is not None or bool(guard)
        live = [[p for p in group["params"] if p.requires_grad] for group in self.param_groups]
        if self._extended:
            if sum(1 for ps in live if ps) > binding.OPTIM_MAX_GROUPS:
                raise ValueError(f"clipping, the guard, decoupled decay and the EMA take at most {binding.OPTIM_MAX_GROUPS} parameter groups")
            if len({p.device for ps in live for p in ps}) > 1:
                raise ValueError("the global gradient norm needs every parameter group on one device")
        early_ids = {id(p) for p in (overlap_early or [])}
        self._flat = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            if not ps:
                self._flat.append(None)
                continue
            dev = ps[0].device
            for p in ps:
                if not p.is_cuda or p.device != dev or p.dtype != torch.float32:
                    raise RuntimeError("FusedAdam needs float32 parameters on one ROCm device (no CPU fallback)")
            n = sum(p.numel() for p in ps)
            n_pad = (n + 3) // 4 * 4
            flat_p = torch.zeros(n_pad, dtype=torch.float32, device=dev)
            flat_g = torch.zeros(n_pad, dtype=torch.float32, device=dev)
            off = 0
            with torch.no_grad():
                for p in ps:
                    k = p.numel()
                    flat_p[off:off + k].copy_(p.reshape(-1))
                    p.data = flat_p[off:off + k].view(p.shape)          # the parameter now lives in the flat buffer
                    p.grad = flat_g[off:off + k].view(p.shape)
                    off += k
            from .dist import GradBuckets
            buckets = GradBuckets(flat_g, ps, [p for p in ps if id(p) in early_ids])
            self._flat.append(dict(params=ps, p=flat_p, g=flat_g, m=torch.zeros_like(flat_p), v=torch.zeros_like(flat_p), step=0, buckets=buckets))
            if ema_decay is not None:
                self._flat[-1]["ema"] = flat_p.clone()
        self._live = [k for k, f in enumerate(self._flat) if f is not None]          # row i of the control blocks belongs to group _live[i]
        self._ctl = None
        if self._extended and self._live:
            self._ctl = torch.zeros((len(self._live), binding.OPTIM_CTL_WORDS), dtype=torch.int64, device=self._flat[self._live[0]]["p"].device)
        binding.bump_param_epoch()

    # -- the extended step's state: all of it on the device
    def _need_extended(self, what):
        if self._ctl is None:
            raise RuntimeError(f"{what} needs max_grad_norm, guard, decoupled_weight_decay or ema_decay (and a parameter that requires grad)")

    @property
    def grad_norm(self):
        """The last step's global gradient norm before clipping (over the finite elements, if the step was skipped): a 0-d float64 device
        tensor.  No sync."""
        self._need_extended("grad_norm")
        return binding.optim_ctl_field(self._ctl, 0, "norm").clone()

    def step_counts(self):
        """(applied, skipped) steps as ints, of the first parameter group (the groups differ only after loading a checkpoint whose groups
        do).  Syncs: for logging and checkpoints."""
        self._need_extended("step_counts()")
        row = self._ctl[0, :2].cpu()
        return int(row[0]), int(row[1])

    def ema_parameters(self):
        """The averaged weights, one view of the flat EMA buffers per parameter, in the order of the parameters."""
        if self.ema_decay is None:
            raise RuntimeError("ema_parameters() needs ema_decay")
        for f in self._flat:
            if f is None:
                continue
            off = 0
            for p in f["params"]:
                k = p.numel()
                yield f["ema"][off:off + k].view(p.shape)
                off += k

    def _swap_ema(self):
        for f in self._flat:
            if f is not None:
                tmp = f["p"].clone()
                f["p"].copy_(f["ema"])
                f["ema"].copy_(tmp)
        binding.bump_param_epoch()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the parameters hold the averaged weights (and the EMA buffers the trained ones): validate or save there.  Device
        copies of the flat buffers on entry and on exit; do not step inside."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weights() needs ema_decay")
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    def zero_grad(self, set_to_none=False):
        """Zero the flat gradient buffers; `.grad` stays a view of them (set_to_none is ignored on purpose)."""
        for f in self._flat:
            if f is None:
                continue
            f["g"].zero_()
            self._rebind(f)
            f["buckets"].begin()

    @staticmethod
    def _rebind(f):
        off = 0
        for p in f["params"]:
            k = p.numel()
            view = f["g"][off:off + k].view(p.shape)
            if p.grad is None or p.grad.data_ptr() != view.data_ptr():
                if p.grad is not None:
                    view.add_(p.grad)                                   # someone replaced .grad: fold it back in
                p.grad = view
            off += k

    def allreduce(self):
        """Average the flat gradient buffers over the process group (identity without one): waits for the slice a backward hook has
        already put on the wire (`overlap_early`) and reduces the rest.  Call between backward() and step() - step() does it itself
        if the caller did not (the stock train.py loop with only the constructor swapped).  Returns bytes reduced."""
        total = 0
        for f in self._flat:
            if f is None:
                continue
            b = f["buckets"]
            if b.early_launched_in_backward:
                b.wait_early()                # nothing may be folded into a slice that is still on the wire
            self._rebind(f)
            total += b.finish()
        return total

    def close(self):
        """Detach from the parameters' backward hooks (call before building another optimiser over the same parameters)."""
        for f in self._flat:
            if f is not None:
                f["buckets"].close()

    def __del__(self):
        try:
            self.close()
        except Exception:                     # noqa: BLE001 - interpreter shutdown
            pass

    # -- torch.optim.Adam's checkpoint surface: per-parameter `step`, `exp_avg`, `exp_avg_sq` (the moments live in flat buffers here)
    def state_dict(self):
        self.state.clear()
        if self._ctl is not None:                            # the applied counts live on the device (a sync)
            for i, applied in enumerate(self._ctl[:, 0].cpu().tolist()):
                self._flat[self._live[i]]["step"] = int(applied)
        for f in self._flat:
            if f is None:
                continue
            off = 0
            for p in f["params"]:
                k = p.numel()
                self.state[p] = {"step": torch.tensor(float(f["step"])), "exp_avg": f["m"][off:off + k].view(p.shape).clone(),
                                 "exp_avg_sq": f["v"][off:off + k].view(p.shape).clone()}
                if "ema" in f:
                    self.state[p]["ema"] = f["ema"][off:off + k].view(p.shape).clone()
                off += k
        sd = super().state_dict()
        self.state.clear()
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)                  # param_groups (lr, betas, ...) + per-parameter state, cast to the parameters
        for f in self._flat:
            if f is None:
                continue
            off, steps = 0, set()
            for p in f["params"]:
                k = p.numel()
                st = self.state.get(p)
                if st:
                    f["m"][off:off + k].copy_(st["exp_avg"].reshape(-1))
                    f["v"][off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                    steps.add(int(st["step"]))
                if "ema" in f:                               # a checkpoint without it (torch.optim.Adam's, or one written without ema_decay):
                    src = st["ema"] if st and "ema" in st else f["p"][off:off + k]        # the average starts from the current parameters
                    f["ema"][off:off + k].copy_(src.reshape(-1))
                off += k
            if len(steps) > 1:
                raise ValueError("FusedAdam keeps one step count per parameter group; the checkpoint holds several")
            if steps:
                f["step"] = steps.pop()
        if self._ctl is not None:                            # applied counts as loaded, skipped counts from zero, the rest rewritten by the next step
            rows = torch.zeros(tuple(self._ctl.shape), dtype=torch.int64)
            rows[:, 0] = torch.tensor([self._flat[k]["step"] for k in self._live], dtype=torch.int64)
            self._ctl.copy_(rows)
        self.state.clear()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group, f in zip(self.param_groups, self._flat):
            if f is None:
                continue
            b = f["buckets"]
            if b._active() and not b._reduced:      # the caller did not run the exchange: do it here rather than step on local gradients
                if b.early_launched_in_backward:
                    b.wait_early()
                self._rebind(f)
                b.finish()
            self._rebind(f)
            if self._extended:
                continue
            f["step"] += 1
            b1, b2 = group["betas"]
            torch.ops.hrnet_hip.adam_step(f["p"], f["g"], f["m"], f["v"], float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                          float(group["weight_decay"]), int(f["step"]))
        if self._ctl is not None:
            self._step_extended()
        return loss

    def _step_extended(self):
        """Every group's sum of squares first (the norm and the skip are global), then the control block and the update of each group."""
        ops = torch.ops.hrnet_hip
        sums = [ops.grad_sumsq(self._flat[k]["g"]) for k in self._live]
        sums = torch.stack(sums) if len(sums) > 1 else sums[0].view(1, 2)
        for i, k in enumerate(self._live):
            group, f = self.param_groups[k], self._flat[k]
            b1, b2 = group["betas"]
            ops.optim_prepare(sums, self._ctl, i, float(self.max_grad_norm or 0.0), float(group["lr"]), float(b1), float(b2))
            ops.adam_step_ex(f["p"], f["g"], f["m"], f["v"], f.get("ema"), self._ctl, i, float(b1), float(b2), float(group["eps"]),
                             float(group["weight_decay"]), self.decoupled_weight_decay, float(self.ema_decay or 0.0))
