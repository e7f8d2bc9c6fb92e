"""GPU: the guarded optimiser step (csrc/optim_guard.hip) - the fp64 sum of squares, the prepare step and the extended Adam / AdamW
update with the EMA, per element against the fp64 restatements of tests/optim_ref.py (checked against torch by
tests/test_optim_host.py) - and FusedAdam's extended path end to end against clip_grad_norm_ + torch.optim.Adam(W) + swa_utils' EMA.

Bounds.  Sum of squares: |got - want| <= n 2^-53 want - every term is non-negative, every square is exact in fp64, and any order of at
most n fp64 additions meets it.  Prepare: norm to 2^-52 relative (one sqrt of a sum of at most 8 terms), coef to one float rounding,
step_size and inv_bc2_sqrt to 2^-23 relative.  Step: test_adam's bounds (tests/test_gpu_kernels_shiftnet.py) - m' within C T_m, v' within
C T_v + 2^-126, p' within 2^-24 max(|got|, |want|) + C |update| of the fp64 formula on the stored m', v', with |update| including
|lr wd p| when the decay is decoupled; ema' within 2^-23 max(|ema|, |p'|) of the fp64 lerp of the stored p'.

Shapes: n in {1, 3, 4, 5, 1027} - below one vector, the scalar tail alone, one vector, vector + tail, several blocks with a tail - and
one pass of each kernel's grid + 7 (1024 blocks for the sum, 4096 for the step): the grid-stride loops and the tail together."""
import math
import struct

import numpy as np
import pytest
import torch

import optim_ref as R
import util
from kernel_bounds import C
from kernel_refs import ADAM_EPS, ADAM_SETTINGS, adam_inputs
from kt import _p, _stream

pytestmark = pytest.mark.gpu

SUMSQ_PASS = 1024 * 256 * 4                  # elements one pass of grad_sumsq_kernel's largest grid covers
STEP_PASS = 4096 * 256 * 4                   # the same for adam_ex_kernel
SUMSQ_N = [1, 3, 4, 5, 1027, SUMSQ_PASS + 7]
STEP_N = [1, 3, 4, 5, 1027, STEP_PASS + 7]
GUARD = 64                                   # NaN elements behind every buffer
F32 = lambda h: float(np.float32(h))         # a hyper-parameter as the ABI receives it
CTL_FMT = "<qqdffffii"
CTL_KEYS = ("applied", "skipped", "norm", "coef", "step_size", "inv_bc2_sqrt", "lr", "skip", "reserved")


def _lib():
    from hrnet_hip import binding
    return binding.load_library()


def _guarded(t):
    return torch.cat([t, torch.full((GUARD,), float("nan"), dtype=t.dtype)]).cuda()


def _guard_ok(dev, n):
    return bool(torch.isnan(dev[n:]).all())


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _ctl_dev(rows):
    """control blocks (dicts of CTL_KEYS, missing fields zero) -> a (G, 6) int64 device tensor"""
    raw = b"".join(struct.pack(CTL_FMT, *[r.get(k, 0) for k in CTL_KEYS]) for r in rows)
    return torch.frombuffer(bytearray(raw), dtype=torch.int64).reshape(len(rows), 6).cuda()


def _ctl_host(ctl):
    raw = ctl.cpu().numpy().tobytes()
    return [dict(zip(CTL_KEYS, struct.unpack_from(CTL_FMT, raw, 48 * i))) for i in range(ctl.shape[0])]


def _sumsq(dev, n, offset=0):
    """hrn_grad_sumsq over dev[offset : offset + n] -> (sum, count) as Python floats, bit-exact"""
    lib = _lib()
    out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    nbytes = lib.hrn_grad_sumsq_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    import ctypes
    ptr = ctypes.c_void_p(dev.data_ptr() + 4 * offset)
    assert lib.hrn_grad_sumsq(ptr, n, _p(out), _p(ws), nbytes, _stream()) == 0, lib.hrn_last_error()
    got = out.cpu()
    return float(got[0]), float(got[1])


def _assert_sumsq(tag, got, g_cpu):
    want, bad = R.ref_sumsq(g_cpu)
    n = g_cpu.numel()
    err, bound = abs(got[0] - want), n * 2.0 ** -53 * want
    print(f"{tag}: sum {got[0]:.17g}, want {want:.17g}: error {err:.3e}, bound {bound:.3e}; non-finite {got[1]:.0f} (want {bad})")
    assert math.isfinite(got[0]) and err <= bound and got[1] == bad, tag
    return want


# ----------------------------------------------------------------------------------------------------------- sum of squares
SUMSQ_INPUTS = {}


def _sumsq_input(n):
    if n not in SUMSQ_INPUTS:
        SUMSQ_INPUTS[n] = adam_inputs(n, 130 + n % 1000)[1]
    return SUMSQ_INPUTS[n]


@pytest.mark.parametrize("n", SUMSQ_N, ids=lambda v: f"n{v}")
def test_sumsq(n):
    g = _sumsq_input(n)
    dev = _guarded(g)                              # a read past n would count the guard's NaN
    got = _sumsq(dev, n)
    _assert_sumsq(f"sumsq n={n} gradients", got, g)
    assert _sumsq(dev, n) == got, "two runs differ"
    # the same values at another offset of a larger allocation (16-byte aligned, as the flat buffers are)
    big = torch.cat([torch.full((12,), float("nan")), g, torch.full((GUARD,), float("nan"))]).cuda()
    assert _sumsq(big, n, offset=12) == got, "the result depends on where the buffer lies"
    assert _guard_ok(dev, n)
    for value, tag in ((3e20, "3e20 (fp32 squares overflow)"), (1e-30, "1e-30 (fp32 squares underflow)"), (0.0, "zeros")):
        x = torch.full((n,), value)
        x[1::2] *= -1
        want = _assert_sumsq(f"sumsq n={n} {tag}", _sumsq(_guarded(x), n), x)
        assert (want == 0.0) == (value == 0.0)


@pytest.mark.parametrize("n", SUMSQ_N, ids=lambda v: f"n{v}")
def test_sumsq_counts_non_finite_elements_and_keeps_them_out_of_the_sum(n):
    g = _sumsq_input(n)
    clean = _sumsq(_guarded(g), n)
    spots = {"index 0": 0, "last full vector": n // 4 * 4 - 2, "scalar tail": n - 1, "beyond the first grid pass": SUMSQ_PASS + 2}
    spots = {k: i for k, i in spots.items() if 0 <= i < n and (k != "scalar tail" or n % 4) and (k != "last full vector" or n >= 4)}
    for bad in (float("inf"), float("-inf"), float("nan")):
        for where, i in spots.items():
            x = g.clone()
            x[i] = bad
            got = _sumsq(_guarded(x), n)
            _assert_sumsq(f"sumsq n={n} {bad} at {where}", got, x)
            assert got[1] == 1.0
        x = g.clone()
        for i in spots.values():
            x[i] = bad
        got = _sumsq(_guarded(x), n)
        _assert_sumsq(f"sumsq n={n} {bad} at every spot", got, x)
        assert got[1] == len(set(spots.values())) and got[0] <= clean[0]


def test_sumsq_of_nothing_is_zero():
    assert _sumsq(torch.full((GUARD,), float("nan")).cuda(), 0) == (0.0, 0.0)


# ----------------------------------------------------------------------------------------------------------- prepare
def _prepare(sums, ctl, group, max_norm, lr, b1, b2):
    lib = _lib()
    s = torch.tensor(sums, dtype=torch.float64).cuda()
    assert lib.hrn_optim_prepare(_p(s), len(sums), group, max_norm, lr, b1, b2, _p(ctl), _stream()) == 0, lib.hrn_last_error()


def _assert_prepared(tag, got, want):
    assert (got["applied"], got["skipped"], got["skip"]) == (want["applied"], want["skipped"], want["skip"]), (tag, got, want)
    assert abs(got["norm"] - want["norm"]) <= 2.0 ** -52 * want["norm"], (tag, got["norm"], want["norm"])
    assert abs(got["coef"] - want["coef"]) <= 2.0 ** -24 * want["coef"], (tag, got["coef"], want["coef"])
    for k in ("step_size", "inv_bc2_sqrt"):
        assert abs(got[k] - want[k]) <= 2.0 ** -23 * abs(want[k]), (tag, k, got[k], want[k])
    assert got["lr"] == want["lr"], tag


@pytest.mark.parametrize("si", range(len(ADAM_SETTINGS)), ids=lambda v: f"s{v}")
def test_prepare(si):
    lr, b1, b2, _, step = ADAM_SETTINGS[si]
    lr, b1, b2 = F32(lr), F32(b1), F32(b2)
    sums = [(1.25e-3, 0), (7.0e41, 0), (3.3e-7, 0)]             # the middle one is beyond fp32
    norm = math.sqrt(sum(s for s, _ in sums))
    for max_norm, tag in ((0.0, "no clipping"), (F32(2.0 * norm), "below max_norm"), (F32(0.37 * norm), "clipped"), (1.0, "clipped hard")):
        for group in range(3):
            rows = [R.new_ctl(applied=step - 1, skipped=5) for _ in range(3)]
            ctl = _ctl_dev(rows)
            _prepare(sums, ctl, group, max_norm, lr, b1, b2)
            got = _ctl_host(ctl)
            want = R.ref_prepare(sums, rows[group], max_norm, lr, b1, b2)
            _assert_prepared(f"prepare setting {si} {tag} group {group}", got[group], want)
            assert got[group]["applied"] == step and (got[group]["coef"] == 1.0) == (tag in ("no clipping", "below max_norm"))
            assert all(got[k] == dict(rows[k], reserved=0) for k in range(3) if k != group), "another group's block was written"


def test_prepare_counters_across_apply_skip_apply():
    lr, b1, b2 = F32(1e-3), F32(0.9), F32(0.999)
    ctl, want = _ctl_dev([R.new_ctl()]), R.new_ctl()
    seen = []
    for sums in ([(4.0, 0), (5.0, 0)], [(4.0, 0), (5.0, 2)], [(1.0, 0), (0.0, 0)], [(1.0, 1), (2.0, 1)], [(16.0, 0), (9.0, 0)]):
        _prepare(sums, ctl, 0, 2.0, lr, b1, b2)
        want = R.ref_prepare(sums, want, 2.0, lr, b1, b2)
        got = _ctl_host(ctl)[0]
        _assert_prepared(f"prepare after {sums}", got, want)
        seen.append((got["applied"], got["skipped"], got["skip"]))
    assert seen == [(1, 0, 0), (1, 1, 1), (2, 1, 0), (2, 2, 1), (3, 2, 0)]


# ----------------------------------------------------------------------------------------------------------- the step
CONFIGS = {"coupled": dict(decoupled=False, ema=False, clip=False), "decoupled-clip": dict(decoupled=True, ema=False, clip=True),
           "coupled-ema-clip": dict(decoupled=False, ema=True, clip=True), "decoupled-ema": dict(decoupled=True, ema=True, clip=False)}
EMA_DECAY = 0.99
STEP_INPUTS = {}


def _step_inputs(n):
    if n not in STEP_INPUTS:
        p, g, m, v = adam_inputs(n, 130 + n % 1000)
        e = p + 0.01 * torch.randn(n, generator=torch.Generator().manual_seed(7 + n % 1000))
        STEP_INPUTS[n] = (p, g, m, v, e, R.ref_sumsq(g))
    return STEP_INPUTS[n]


def _step_case(n, setting, decoupled, ema, clip, wd=None, skip=False):
    """sum of squares -> prepare -> hrn_adam_step_ex on guarded buffers, as FusedAdam runs them"""
    import ctypes
    lib = _lib()
    lr, b1, b2, wd0, step = setting
    wd = wd0 if wd is None else wd
    p, g, m, v, e, (total, _) = _step_inputs(n)
    dev = [_guarded(t) for t in (p, g, m, v, e)]
    sums = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    nbytes = lib.hrn_grad_sumsq_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert lib.hrn_grad_sumsq(_p(dev[1]), n, _p(sums), _p(ws), nbytes, _stream()) == 0
    max_norm = F32(0.5 * math.sqrt(total)) if clip else 0.0
    ctl = _ctl_dev([R.new_ctl(applied=step - 1)])
    assert lib.hrn_optim_prepare(_p(sums), 1, 0, max_norm, lr, b1, b2, _p(ctl), _stream()) == 0
    block = _ctl_host(ctl)[0]
    assert block["skip"] == 0 and block["applied"] == step and (block["coef"] < 1.0) == clip and (not clip or block["coef"] > 0.4)
    if skip:
        ctl = _ctl_dev([dict(block, skip=1)])
    assert lib.hrn_adam_step_ex(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]) if ema else ctypes.c_void_p(0), n, b1, b2, ADAM_EPS,
                                wd, int(decoupled), EMA_DECAY, _p(ctl), _stream()) == 0, lib.hrn_last_error()
    torch.cuda.synchronize()
    got = [t.cpu() for t in dev]
    assert all(_guard_ok(t, n) for t in got), "a write past a buffer"
    assert torch.equal(_bits(got[1][:n]), _bits(g)), "the gradient was written"
    assert _ctl_host(ctl)[0] == (dict(block, skip=1) if skip else block), "the step wrote its control block"
    if not ema:
        assert torch.equal(_bits(got[4][:n]), _bits(e)), "the EMA buffer was written without being passed"
    ctl64 = dict(block, lr=F32(lr))                             # as the kernel reads it: float coef, the lr the ABI received
    return dict(p=got[0][:n].double(), m=got[2][:n].double(), v=got[3][:n].double(), ema=got[4][:n].double(), raw=[t[:n] for t in got],
                ins=[t.double() for t in (p, g, m, v, e)], ctl=ctl64, hyper=(F32(b1), F32(b2), F32(ADAM_EPS), F32(wd)), decoupled=decoupled,
                with_ema=ema)


def _step_ratios(r, **change):
    """error / bound of m', v', p' (on the stored m', v') and ema' (on the stored p') against ref_step_ex; `change` overrides what the
    reference is told (the negative controls)"""
    p, g, m, v, e = r["ins"]
    a = dict(ctl=r["ctl"], decoupled=r["decoupled"], ema_old_p=False)
    a.update(change)
    first = R.ref_step_ex(p, g, m, v, e, a["ctl"], *r["hyper"], a["decoupled"], F32(EMA_DECAY))
    stored = R.ref_step_ex(p, g, m, v, e, a["ctl"], *r["hyper"], a["decoupled"], F32(EMA_DECAY), m_new=r["m"], v_new=r["v"], p_new=r["p"],
                           ema_old_p=a["ema_old_p"])
    out = dict(m=(r["m"] - first["m"]).abs() / (C * first["Tm"] + 1e-300),
               v=(r["v"] - first["v"]).abs() / (C * first["Tv"] + 2.0 ** -126),
               p=(r["p"] - stored["p"]).abs() / (2.0 ** -24 * torch.maximum(r["p"].abs(), stored["p"].abs()) + C * stored["upd"] + 1e-300))
    if r["with_ema"]:
        out["ema"] = (r["ema"] - stored["ema"]).abs() / (2.0 ** -23 * torch.maximum(e.abs(), r["p"].abs()) + 1e-300)
    return {k: float(x.max()) for k, x in out.items()}


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("si", range(len(ADAM_SETTINGS)), ids=lambda v: f"s{v}")
@pytest.mark.parametrize("n", STEP_N, ids=lambda v: f"n{v}")
def test_step(n, si, config):
    r = _step_case(n, ADAM_SETTINGS[si], **CONFIGS[config])
    ratios = _step_ratios(r)
    print(f"adam_ex n={n} setting {ADAM_SETTINGS[si]} {config}: error / bound " + ", ".join(f"{k}' {x:.3e}" for k, x in ratios.items()))
    assert max(ratios.values()) <= 1.0
    assert not torch.equal(r["p"], r["ins"][0]), "nothing was updated"


@pytest.mark.parametrize("n", [5, 1027, STEP_PASS + 7], ids=lambda v: f"n{v}")
def test_step_with_skip_set_keeps_every_bit(n):
    r = _step_case(n, ADAM_SETTINGS[1], decoupled=True, ema=True, clip=True, skip=True)
    for got, want, name in zip(r["raw"], r["ins"], ("p", "g", "m", "v", "ema")):
        assert torch.equal(_bits(got), _bits(want.float())), name


WRONG = {"coupled_decay_for_decoupled": dict(decoupled=False), "coef_ignored": "coef", "ema_of_the_old_p": dict(ema_old_p=True)}


@pytest.mark.parametrize("control", sorted(WRONG))
def test_step_negative_control(control):
    """the bounds that hold for the right reference reject, on the same GPU output, a reference that is wrong in one way"""
    r = _step_case(1027, ADAM_SETTINGS[1], decoupled=True, ema=True, clip=True)
    ok = _step_ratios(r)
    change = dict(ctl=dict(r["ctl"], coef=1.0)) if control == "coef_ignored" else WRONG[control]
    bad = _step_ratios(r, **change)
    print(f"{control}: error / bound against the wrong reference {bad} (the right one {ok})")
    assert max(ok.values()) <= 1.0 < max(bad.values())


# ----------------------------------------------------------------------------------------------------------- the dispatcher ops
def test_ops_are_registered_and_opcheck():
    from hrnet_hip import binding
    ops = torch.ops.hrnet_hip
    basic = ("test_schema", "test_faketensor")
    n = 4099 // 4 * 4 + 4
    g = torch.rand(n, device="cuda") - 0.5
    torch.library.opcheck(ops.grad_sumsq.default, (g,), test_utils=basic)
    sums = ops.grad_sumsq(g).view(1, 2)
    want, _ = R.ref_sumsq(g)
    assert abs(float(sums[0, 0]) - want) <= n * 2.0 ** -53 * want and float(sums[0, 1]) == 0.0
    ctl = torch.zeros((1, binding.OPTIM_CTL_WORDS), dtype=torch.int64, device="cuda")
    torch.library.opcheck(ops.optim_prepare.default, (sums, ctl, 0, 1.0, 1e-3, 0.9, 0.999), test_utils=basic)
    ops.optim_prepare(sums, ctl, 0, 1.0, 1e-3, 0.9, 0.999)
    p, m, v = torch.rand(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    e = p.clone()
    torch.library.opcheck(ops.adam_step_ex.default, (p, g, m, v, e, ctl, 0, 0.9, 0.999, 1e-8, 1e-2, True, 0.99), test_utils=basic)
    torch.library.opcheck(ops.adam_step_ex.default, (p, g, m, v, None, ctl, 0, 0.9, 0.999, 1e-8, 1e-2, False, 0.0), test_utils=basic)
    norm = math.sqrt(float(sums[0, 0]))
    assert abs(float(binding.optim_ctl_field(ctl, 0, "norm")) - norm) <= 2.0 ** -52 * norm
    with pytest.raises(ValueError, match="ctl"):
        ops.optim_prepare(sums, ctl.int(), 0, 1.0, 1e-3, 0.9, 0.999)
    with pytest.raises(ValueError, match="ema"):
        ops.adam_step_ex(p, g, m, v, e[:-4], ctl, 0, 0.9, 0.999, 1e-8, 0.0, False, 0.5)


# ----------------------------------------------------------------------------------------------------------- FusedAdam end to end
def _tiny(seed=3):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(53, 30), torch.nn.PReLU(), torch.nn.Linear(30, 7)).cuda()


def _two_groups(net, lrs=(3e-3, 1e-3)):
    """1621 and 217 parameters: neither a multiple of 4"""
    return [dict(params=[*net[0].parameters(), *net[1].parameters()], lr=lrs[0]), dict(params=list(net[2].parameters()), lr=lrs[1])]


def _backward(net, x, scale=1.0):
    (scale * (net(x) ** 2).mean()).backward()


HYPER = dict(betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
SCALES = (1.0, 0.05, 1.0, "nan", 1.0, 0.5)
DECAY = 0.9


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_fused_adam_extended_matches_the_torch_composition(decoupled):
    """six steps on two groups: clipped and unclipped steps, an lr change, one step with a NaN gradient that changes nothing; then a
    state_dict round trip that continues bit-identically, and a checkpoint without `ema`"""
    from hrnet_hip.optim import FusedAdam
    net = _tiny()
    x = torch.randn(11, 53, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    _backward(net, x)
    max_norm = 0.5 * float(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).double().norm())      # the first step clips by ~ 0.5
    ref = [torch.nn.Parameter(p.detach().double().cpu()) for p in net.parameters()]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    o_ref = cls([dict(params=ref[:3], lr=3e-3), dict(params=ref[3:], lr=1e-3)], **HYPER)
    ema_ref, ema_update = [p.detach().clone() for p in ref], torch.optim.swa_utils.get_ema_multi_avg_fn(DECAY)
    opt = FusedAdam(_two_groups(net), **HYPER, max_grad_norm=max_norm, decoupled_weight_decay=decoupled, ema_decay=DECAY)
    assert all(torch.equal(e, p) for e, p in zip(opt.ema_parameters(), net.parameters()))
    coefs, applied = [], 0
    for it, scale in enumerate(SCALES):
        opt.zero_grad()
        _backward(net, x, 1.0 if scale == "nan" else scale)
        if scale == "nan":
            net[2].weight.grad[3, 4] = float("nan")
        grads = [p.grad.detach().clone() for p in net.parameters()]
        before = [t.clone() for f in opt._flat for t in (f["p"], f["m"], f["v"], f["ema"])]
        opt.step()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, (p.grad for p in net.parameters()))), "step() rewrote .grad"
        if scale == "nan":
            after = [t for f in opt._flat for t in (f["p"], f["m"], f["v"], f["ema"])]
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, after)), "the skipped step changed something"
            assert opt.step_counts() == (applied, 1)
        else:
            for p, g in zip(ref, grads):
                p.grad = g.double().cpu()
            norm = float(torch.nn.utils.clip_grad_norm_(ref, max_norm))
            o_ref.step()
            applied += 1
            with torch.no_grad():
                ema_update(ema_ref, [p.detach() for p in ref], applied)
            got = opt.grad_norm
            assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda and abs(float(got) - norm) <= 1e-6 * norm, (float(got), norm)
            coefs.append(min(1.0, max_norm / (norm + 1e-6)))
        if it == 2:
            for g in (*opt.param_groups, *o_ref.param_groups):
                g["lr"] *= 0.5
    assert opt.step_counts() == (5, 1) and coefs.count(1.0) >= 1 and sum(c < 1.0 for c in coefs) >= 1, coefs
    for k, (a, b, e, f) in enumerate(zip(net.parameters(), ref, opt.ema_parameters(), ema_ref)):
        assert torch.allclose(a.detach().cpu(), b.detach().float(), rtol=2e-5, atol=1e-7), (k, (a.detach().cpu() - b.detach()).abs().max())
        assert torch.allclose(e.cpu(), f.float(), rtol=2e-5, atol=1e-7), (k, (e.cpu() - f).abs().max())

    # a checkpoint, loaded into a fresh optimiser over a copy of the module, continues bit for bit
    sd = opt.state_dict()
    assert all(float(s["step"]) == 5.0 and "ema" in s for s in sd["state"].values()) and len(sd["state"]) == 5
    twin = _tiny()
    twin.load_state_dict(net.state_dict())
    opt2 = FusedAdam(_two_groups(twin), **HYPER, max_grad_norm=max_norm, decoupled_weight_decay=decoupled, ema_decay=DECAY)
    opt2.load_state_dict(sd)
    assert opt2.step_counts() == (5, 0) and opt2.param_groups[0]["lr"] == 1.5e-3
    for _ in range(2):
        for n_, o in ((net, opt), (twin, opt2)):
            o.zero_grad()
            _backward(n_, x)
            o.step()
    for fa, fb in zip(opt._flat, opt2._flat):
        for k in ("p", "m", "v", "ema"):
            assert torch.equal(_bits(fa[k]), _bits(fb[k])), k
    assert opt2.step_counts() == (7, 0)
    # a checkpoint without `ema` (torch.optim.Adam's, or the default FusedAdam's): the average starts from the current parameters
    for s in sd["state"].values():
        del s["ema"]
    third = _tiny(seed=9)
    opt3 = FusedAdam(_two_groups(third), **HYPER, ema_decay=DECAY)
    opt3.load_state_dict(sd)
    assert opt3.step_counts() == (5, 0)
    assert all(torch.equal(e, p) for e, p in zip(opt3.ema_parameters(), third.parameters()))
    assert torch.equal(opt3._flat[1]["m"][:7 * 30].view(7, 30), sd["state"][3]["exp_avg"].cuda())


def test_fused_adam_guard_alone_and_constructor_refusals():
    from hrnet_hip.optim import FusedAdam
    net = _tiny()
    for bad in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(ema_decay=1.0), dict(ema_decay=-0.1)):
        with pytest.raises(ValueError):
            FusedAdam(net.parameters(), **bad)
    nine = [dict(params=[torch.nn.Parameter(torch.zeros(3, device="cuda"))]) for _ in range(9)]
    with pytest.raises(ValueError, match="8 parameter groups"):
        FusedAdam(nine, guard=True)
    FusedAdam(nine).step()                                      # the default path has no such limit
    # guard=True alone: plain Adam arithmetic (coef = 1 exactly), but a NaN step is not applied
    x = torch.randn(11, 53, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    plain_net, guard_net = _tiny(), _tiny()
    plain, guarded = FusedAdam(plain_net.parameters(), lr=3e-3, **HYPER), FusedAdam(guard_net.parameters(), lr=3e-3, **HYPER, guard=True)
    with pytest.raises(RuntimeError):
        plain.step_counts()
    for it in range(3):
        for n_, o in ((plain_net, plain), (guard_net, guarded)):
            o.zero_grad()
            _backward(n_, x)
        if it == 1:                                             # the guarded optimiser meets an infinity; the plain one sits this step out
            guard_net[0].bias.grad[0] = float("inf")
            keep = [p.detach().clone() for p in guard_net.parameters()]
            guarded.step()
            assert all(torch.equal(_bits(a), _bits(p.detach())) for a, p in zip(keep, guard_net.parameters()))
        else:
            plain.step()
            guarded.step()
    assert guarded.step_counts() == (2, 1)
    for a, b in zip(plain_net.parameters(), guard_net.parameters()):
        assert torch.allclose(a, b, rtol=2e-5, atol=1e-7)


def test_default_fused_adam_still_runs_the_plain_op_bit_for_bit(monkeypatch):
    from hrnet_hip import binding
    from hrnet_hip.optim import FusedAdam
    net = _tiny()
    x = torch.randn(11, 53, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    opt = FusedAdam(net.parameters(), lr=3e-3, **HYPER)
    assert opt._ctl is None and "ema" not in opt._flat[0]
    calls, plain_step = [], binding.adam_step
    monkeypatch.setattr(binding, "adam_step", lambda *a: (calls.append(a[-1]), plain_step(*a))[1])
    for name in ("grad_sumsq", "optim_prepare", "adam_step_ex"):
        monkeypatch.setattr(binding, name, lambda *a, _n=name: pytest.fail(f"the default FusedAdam called {_n}"))
    for it in range(2):
        opt.zero_grad()
        _backward(net, x)
        f = opt._flat[0]
        p, m, v = f["p"].clone(), f["m"].clone(), f["v"].clone()
        plain_step(p, f["g"], m, v, 3e-3, 0.9, 0.99, 1e-8, 1e-2, it + 1)          # the plain op's output on the same inputs
        opt.step()
        for a, b in ((p, f["p"]), (m, f["m"]), (v, f["v"])):
            assert torch.equal(_bits(a), _bits(b))
    assert calls == [1, 2]


# ----------------------------------------------------------------------------------------------------------- EMA swap, training plumbing
def test_ema_weights_swaps_the_averaged_weights_in_and_back():
    from hrnet_hip.optim import FusedAdam
    rng = np.random.Generator(np.random.PCG64(17))
    lrs, alphas = util.dev(rng.random((2, 4, 32, 32), dtype=np.float32)), util.dev(np.ones((2, 4), np.float32))
    m = util._fresh_model()
    opt = FusedAdam(m.parameters(), lr=1e-3, ema_decay=0.9)
    for _ in range(2):
        opt.zero_grad()
        ((m(lrs, alphas) - 0.1) ** 2).mean().backward()
        opt.step()
    trained = [p.detach().clone() for p in m.parameters()]
    averaged = [e.clone() for e in opt.ema_parameters()]
    assert any(not torch.equal(a, b) for a, b in zip(trained, averaged))
    other = util._fresh_model(seed=99)
    state = dict(m.state_dict())
    state.update({k: e for (k, _), e in zip(m.named_parameters(), averaged)})
    other.load_state_dict(state)
    m.eval(), other.eval()
    with torch.no_grad():
        out_trained, want = m(lrs, alphas).clone(), other(lrs, alphas)
        with opt.ema_weights():
            assert all(torch.equal(p.detach(), e) for p, e in zip(m.parameters(), averaged))
            assert all(torch.equal(e, t) for e, t in zip(opt.ema_parameters(), trained))
            inside = m(lrs, alphas).clone()
        assert torch.equal(_bits(inside), _bits(want)) and not torch.equal(inside, out_trained)
        assert all(torch.equal(_bits(p.detach()), _bits(t)) for p, t in zip(m.parameters(), trained))
        assert all(torch.equal(_bits(e), _bits(a)) for e, a in zip(opt.ema_parameters(), averaged))
        assert torch.equal(_bits(m(lrs, alphas)), _bits(out_trained))


def test_shift_loss_steps_with_clipping_and_ema_skip_a_nan_batch():
    """Plumbing, in the pattern of tests/test_gpu_shift_loss.py's five bf16 steps: HRNet in bf16 training precision, the searched loss and
    FusedAdam with max_grad_norm and ema_decay; one batch carries a NaN in lrs - that step is skipped, the next clean one is finite."""
    from DeepNetworks.HRNet import HRNet
    from hrnet_hip import losses
    from hrnet_hip.optim import FusedAdam
    from oracle import weights
    fusion = HRNet(weights.HRNET_CONFIG)
    fusion.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
    fusion.train_precision = "bf16"
    fusion = fusion.cuda().train()
    optimizer = FusedAdam(list(fusion.parameters()), lr=1e-4, max_grad_norm=1.0, ema_decay=0.99)
    rng = np.random.Generator(np.random.PCG64(121))
    lrs = util.dev(rng.random((2, 4, 16, 16), dtype=np.float32))
    alphas = util.dev(np.ones((2, 4), np.float32))
    hrs = util.dev(rng.random((2, 48, 48), dtype=np.float32))
    maps = util.dev((rng.random((2, 48, 48)) > 0.1).astype(np.float32))
    poisoned = lrs.clone()
    poisoned[1, 2, 5, 7] = float("nan")
    seen = []
    for it in range(5):
        optimizer.zero_grad()
        loss = (-losses.shift_loss(fusion(poisoned if it == 2 else lrs, alphas), hrs, maps)).mean()
        loss.backward()
        if it == 2:
            before = [p.detach().clone() for p in fusion.parameters()]
        optimizer.step()
        if it == 2:
            assert all(torch.equal(_bits(a), _bits(p.detach())) for a, p in zip(before, fusion.parameters()))
        else:
            seen.append(float(loss.detach()))
    assert np.isfinite(seen).all() and len(seen) == 4 and optimizer.step_counts() == (4, 1)
    assert all(bool(torch.isfinite(t).all()) for t in (*fusion.parameters(), *optimizer.ema_parameters()))
    assert math.isfinite(float(optimizer.grad_norm))
