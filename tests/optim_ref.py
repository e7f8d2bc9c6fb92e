"""The guarded optimiser step (csrc/optim_guard.hip) restated in fp64: the sum of squares, the prepare step, the extended Adam / AdamW
update with the EMA, and a whole step over several parameter groups.  tests/test_optim_host.py checks these against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / AdamW + torch.optim.swa_utils on the CPU; tests/test_gpu_optim.py holds the kernels to
them.  The `wrong` switches are the negative controls: each is a plausible misreading of the definition."""
import math

import numpy as np
import torch

import kernel_refs as K

CLIP_EPS = 1e-6          # clip_grad_norm_'s: coef = max_norm / (norm + 1e-6), clamped to 1


def ref_sumsq(g):
    """(sum of the fp64 squares of the finite elements - exact for an fp32 tensor - correctly rounded; number of non-finite elements)"""
    x = g.detach().cpu().reshape(-1).double().numpy()
    fin = np.isfinite(x)
    return math.fsum((x[fin] * x[fin]).tolist()), int((~fin).sum())


def new_ctl(applied=0, skipped=0):
    """a step-control block as the optimiser allocates it (include/hrnet_hip.h, hrn_optim_ctl)"""
    return dict(applied=applied, skipped=skipped, norm=0.0, coef=0.0, step_size=0.0, inv_bc2_sqrt=0.0, lr=0.0, skip=0)


def ref_prepare(sums, ctl, max_norm, lr, b1, b2, count_skips=False):
    """sums: [(sum of squares, non-finite count)] of every group -> the new control block (a dict, every value in fp64) of the group
    with this lr / betas.  count_skips (wrong): a skipped step advances the applied count."""
    total = 0.0
    for s, _ in sums:
        total += s
    out = dict(ctl, norm=math.sqrt(total))
    if any(bad for _, bad in sums):
        out.update(skipped=ctl["skipped"] + 1, skip=1)
        if count_skips:
            out.update(applied=ctl["applied"] + 1)
        return out
    applied = ctl["applied"] + 1
    coef = min(1.0, max_norm / (out["norm"] + CLIP_EPS)) if max_norm > 0 else 1.0
    out.update(applied=applied, coef=coef, step_size=lr / (1.0 - b1 ** applied), inv_bc2_sqrt=1.0 / math.sqrt(1.0 - b2 ** applied), lr=lr, skip=0)
    return out


def ref_step_ex(p, g, m, v, ema, ctl, b1, b2, eps, wd, decoupled, ema_decay, m_new=None, v_new=None, p_new=None, decay_after=False,
                ema_old_p=False):
    """The update under a control block, fp64 tensors in -> dict(m, Tm, v, Tv, p, upd, ema): T_m, T_v the sums of the absolute terms,
    upd = |update| (+ |lr wd p| when decoupled).  p from (m_new, v_new) when given, ema from p_new when given (what the kernel stored).
    decay_after (wrong): the decoupled decay applied to the updated p.  ema_old_p (wrong): the EMA takes the p from before the update."""
    if ctl["skip"]:
        return dict(m=m, Tm=m.abs(), v=v, Tv=v.abs(), p=p, upd=torch.zeros_like(p), ema=ema)
    lr, step, gs = ctl["lr"], ctl["applied"], ctl["coef"] * g
    m1, Tm, v1, Tv, p1, upd = K.ref_adam(p, gs, m, v, lr, b1, b2, eps, 0.0 if decoupled else wd, step, m_new=m_new, v_new=v_new)
    if decoupled:
        p1 = (p1 * (1.0 - lr * wd)) if decay_after else p * (1.0 - lr * wd) - (p - p1)
        upd = upd + lr * wd * p.abs()
    e1 = None
    if ema is not None:
        src = p if ema_old_p else (p1 if p_new is None else p_new)
        e1 = ema_decay * ema + (1.0 - ema_decay) * src
    return dict(m=m1, Tm=Tm, v=v1, Tv=Tv, p=p1, upd=upd, ema=e1)


def ref_fused_step(groups, grads, max_norm, decoupled, ema_decay, clip_per_group=False, **wrong):
    """One FusedAdam step of the extended path.  groups: [dict(p, m, v, ema or None, ctl, lr, betas, eps, wd)], fp64 tensors, updated in
    place (rebound); grads: one tensor per group.  The norm and the skip are global.  clip_per_group (wrong): each group is
    clipped by its own norm.  Other switches go to ref_prepare / ref_step_ex."""
    sums = [ref_sumsq(g) for g in grads]
    prep = {k: wrong[k] for k in ("count_skips",) if k in wrong}
    upd = {k: wrong[k] for k in ("decay_after", "ema_old_p") if k in wrong}
    for i, (G, g) in enumerate(zip(groups, grads)):
        b1, b2 = G["betas"]
        mine = [(s if j == i else 0.0, bad) for j, (s, bad) in enumerate(sums)] if clip_per_group else sums
        G["ctl"] = ref_prepare(mine, G["ctl"], max_norm or 0.0, G["lr"], b1, b2, **prep)
        r = ref_step_ex(G["p"], g.double(), G["m"], G["v"], G["ema"], G["ctl"], b1, b2, G["eps"], G["wd"], decoupled, ema_decay or 0.0, **upd)
        G.update(p=r["p"], m=r["m"], v=r["v"], ema=r["ema"])
    return groups

