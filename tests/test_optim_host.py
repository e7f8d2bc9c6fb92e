"""CPU: the fp64 restatements of tests/optim_ref.py against torch - torch.nn.utils.clip_grad_norm_ over every parameter, then
torch.optim.Adam / AdamW, then torch.optim.swa_utils' EMA - on two parameter groups with different learning rates, over five applied
steps with an lr change, a step below and steps above max_norm, and a step with a NaN gradient that torch's side does not take (as a
loop that skips optimizer.step() does).  And the negative controls: four plausible misreadings each leave the trajectory."""
import math

import pytest
import torch

import optim_ref as R

SIZES = (1027, 301)
LRS = (3e-3, 1e-3)
BETAS, EPS, WD, MAX_NORM, DECAY = (0.9, 0.99), 1e-8, 1e-2, 1.5, 0.9
TOL = 1e-12
# gradient scale per step: the norms are about 36 x scale, so 0.01 stays below MAX_NORM (coef = 1 exactly) and the others are clipped
SCALES = (0.1, 0.01, 0.3, None, 0.1, 0.2)          # None: the step with a NaN
LR_CHANGE_AFTER = 2


def _inputs():
    gen = torch.Generator().manual_seed(11)
    ps = [torch.randn(n, generator=gen, dtype=torch.float64) for n in SIZES]
    grads = []
    for s in SCALES:
        gs = [torch.randn(n, generator=gen, dtype=torch.float64) * (s or 0.1) for n in SIZES]
        if s is None:
            gs[1][17] = float("nan")
        grads.append(gs)
    return ps, grads


def _torch_run(decoupled):
    ps, grads = _inputs()
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([dict(params=[params[0]], lr=LRS[0]), dict(params=[params[1]], lr=LRS[1])], betas=BETAS, eps=EPS, weight_decay=WD)
    ema = [p.detach().clone() for p in params]
    ema_update = torch.optim.swa_utils.get_ema_multi_avg_fn(DECAY)
    norms, applied = [], 0
    for it, gs in enumerate(grads):
        for p, g in zip(params, gs):
            p.grad = g.clone()
        if all(bool(torch.isfinite(g).all()) for g in gs):
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, MAX_NORM)))
            opt.step()
            applied += 1
            with torch.no_grad():
                ema_update(ema, [p.detach() for p in params], applied)
        else:
            norms.append(None)
        if it == LR_CHANGE_AFTER:
            for g in opt.param_groups:
                g["lr"] *= 0.5
    state = [opt.state[p] for p in params]
    return dict(p=[p.detach() for p in params], m=[s["exp_avg"] for s in state], v=[s["exp_avg_sq"] for s in state], ema=ema, norms=norms,
                applied=applied)


def _ref_run(decoupled, **wrong):
    ps, grads = _inputs()
    groups = [dict(p=p.clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), ema=p.clone(), ctl=R.new_ctl(), lr=lr, betas=BETAS, eps=EPS, wd=WD)
              for p, lr in zip(ps, LRS)]
    norms, history = [], []
    for it, gs in enumerate(grads):
        before = [{k: (v.clone() if torch.is_tensor(v) else dict(v) if isinstance(v, dict) else v) for k, v in G.items()} for G in groups]
        R.ref_fused_step(groups, gs, MAX_NORM, decoupled, DECAY, **wrong)
        norms.append(groups[0]["ctl"]["norm"])
        history.append((before, [dict(G) for G in groups]))
        if it == LR_CHANGE_AFTER:
            for G in groups:
                G["lr"] *= 0.5
    return dict(p=[G["p"] for G in groups], m=[G["m"] for G in groups], v=[G["v"] for G in groups], ema=[G["ema"] for G in groups],
                norms=norms, applied=groups[0]["ctl"]["applied"], skipped=groups[0]["ctl"]["skipped"], groups=groups, history=history)


def _worst(a, b):
    return max(float(((x - y).abs() / (y.abs() + 1.0)).max()) for k in ("p", "m", "v", "ema") for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_reference_is_clip_then_torch_adam_then_swa_ema(decoupled):
    want, got = _torch_run(decoupled), _ref_run(decoupled)
    assert want["applied"] == 5 and (got["applied"], got["skipped"]) == (5, 1)
    worst = _worst(got, want)
    print(f"decoupled={decoupled}: worst |ref - torch| / (|torch| + 1) over p, m, v, ema of both groups: {worst:.3e}")
    assert worst <= TOL
    for it, (a, b) in enumerate(zip(got["norms"], want["norms"])):
        if b is not None:
            assert abs(a - b) <= 1e-12 * b, (it, a, b)
    # the cases this trajectory is meant to hold: a step with coef = 1 exactly, steps with coef < 1, two learning rates, a changed lr
    coefs = [after[0]["ctl"]["coef"] for _, after in got["history"] if not after[0]["ctl"]["skip"]]
    assert coefs.count(1.0) == 1 and sum(c < 1.0 for c in coefs) == 4
    assert got["groups"][0]["ctl"]["lr"] == LRS[0] * 0.5 and got["groups"][1]["ctl"]["lr"] == LRS[1] * 0.5


def test_skipped_step_leaves_every_state_value_and_the_applied_count():
    got = _ref_run(True)
    (it, (before, after)), = [(i, h) for i, h in enumerate(got["history"]) if h[1][0]["ctl"]["skip"]]
    for B, A in zip(before, after):
        for k in ("p", "m", "v", "ema"):
            assert torch.equal(B[k], A[k]), k
        assert A["ctl"]["applied"] == B["ctl"]["applied"] and A["ctl"]["skipped"] == B["ctl"]["skipped"] + 1
        for k in ("coef", "step_size", "inv_bc2_sqrt", "lr"):
            assert A["ctl"][k] == B["ctl"][k], k
    # and the step after it is applied with the bias correction of the next count, not the one after
    nxt = got["history"][it + 1][1]
    assert nxt[0]["ctl"]["applied"] == before[0]["ctl"]["applied"] + 1 and nxt[0]["ctl"]["skip"] == 0


def test_prepare_formulas():
    c = R.ref_prepare([(9.0, 0), (16.0, 0)], R.new_ctl(applied=999), 2.0, 1e-4, 0.9, 0.999)
    assert c["norm"] == 5.0 and c["coef"] == 2.0 / (5.0 + 1e-6) and c["applied"] == 1000 and c["skip"] == 0
    assert c["step_size"] == 1e-4 / (1.0 - 0.9 ** 1000) and c["inv_bc2_sqrt"] == 1.0 / math.sqrt(1.0 - 0.999 ** 1000)
    assert R.ref_prepare([(9.0, 0)], R.new_ctl(), 0.0, 1e-3, 0.9, 0.999)["coef"] == 1.0          # max_norm <= 0: no clipping
    assert R.ref_prepare([(9.0, 0)], R.new_ctl(), 4.0, 1e-3, 0.9, 0.999)["coef"] == 1.0          # below max_norm: exactly 1
    s = R.ref_prepare([(9.0, 0), (16.0, 2)], c, 2.0, 1e-4, 0.9, 0.999)
    assert s["skip"] == 1 and s["skipped"] == 1 and s["applied"] == 1000 and s["norm"] == 5.0 and s["coef"] == c["coef"]


def test_sumsq_is_exact_where_fp32_overflows():
    g = torch.tensor([3e20, -3e20, 1e-30, float("inf"), float("-inf"), float("nan"), 0.0])
    total, bad = R.ref_sumsq(g)
    big = float(torch.tensor(3e20)) ** 2
    assert bad == 3 and math.isfinite(total) and abs(total - 2 * big) <= 2.0 ** -52 * total
    assert not math.isfinite(float((g[:2] * g[:2]).sum()))                                       # what an fp32 sum makes of it


WRONG = {"clip_per_group": dict(clip_per_group=True), "skip_advances_the_step_count": dict(count_skips=True),
         "decoupled_decay_after_the_update": dict(decay_after=True), "ema_of_the_old_p": dict(ema_old_p=True)}


@pytest.mark.parametrize("control", sorted(WRONG))
def test_negative_control(control):
    """the comparison that passes for the right reference fails for each wrong one"""
    want = _torch_run(True)
    ok, worst = _worst(_ref_run(True), want), _worst(_ref_run(True, **WRONG[control]), want)
    print(f"{control}: worst error against torch {worst:.3e} (the right reference {ok:.3e}, tolerance {TOL:.0e})")
    assert ok <= TOL < worst
