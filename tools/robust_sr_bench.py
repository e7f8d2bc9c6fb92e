#!/usr/bin/env python3
"""Time the robust, regularised reconstruction: the kernels of csrc/robust_sr.hip and an iteration of
`binding.reconstruct`, beside one `back_project` iteration measured in the same run.

In ONE process, after a warm-up, at (B, V, H, W) = (32, 32, 128, 128) and at one (1, 32, 2048, 1536) scene, both x3, masks 30 % hidden,
shifts within 1.5 px, brightness on, delta 0.1, lam 4e-4, P 2, alpha 0.7, eps 0.02.  With lr = B V H W and sr = S^2 B H W elements of
four bytes:

    robust_sums     hrn_robust_sums + hrn_robust_finish:  4 (2 lr)        residual and masks read
    robust_apply    hrn_robust_apply:                     4 (3 lr)        residual and masks read, the re-weighted plane written
    btv_step        hrn_btv_step:                         4 (2 sr)        x read, out written
    btv_value       hrn_btv_value (both launches):        4 sr            x read
    plain           one back_project iteration:           4 (sr + 3 lr) + 4 (2 lr + 2 sr)      (tools/observe_bench.py's "iteration")
    welsch          plain + robust_sums + robust_apply:   plain + 4 (5 lr)
    btv             plain + btv_step:                     plain + 4 (2 sr)
    welsch_btv      all of it, the defaults of `reconstruct`
    thirty          thirty iterations of the defaults (binding.reconstruct, no trace)

Every time is a pair of device events around `reps` calls enqueued back to back on one stream; the calls walk over enough input sets to
exceed the 256 MB last-level cache.  The figure is the median over the rounds with min and max as the run-to-run spread; the byte floors
are the algorithmic bytes at the 6.3 TB/s a streaming kernel reaches on an MI355X; every iteration is also given as a ratio to `plain`.
There is no pass / fail threshold on time and no target ratio.

usage: python tools/robust_sr_bench.py [--rounds R] [--reps N]
"""
import _common
import torch

from _common import HBM_ACHIEVABLE, LLC_BYTES
from hrnet_hip import binding

PARSER = _common.parser(__doc__, rounds=7, reps=10)
CASES = [(32, 32, 128, 128, 3), (1, 32, 2048, 1536, 3)]          # (B, V, H, W, scale)
DELTA, LAM, P, ALPHA, EPS = 0.1, 4e-4, 2, 0.7, 0.02


def floor_us(B, V, H, W, scale, what):
    """the byte floor in microseconds (the formulas of the module's text)"""
    lr, sr = B * V * H * W, B * H * W * scale * scale
    plain = (sr + 3 * lr) + (2 * lr + 2 * sr)
    n = {"robust_sums": 2 * lr, "robust_apply": 3 * lr, "btv_step": 2 * sr, "btv_value": sr, "plain": plain, "welsch": plain + 5 * lr,
         "btv": plain + 2 * sr, "welsch_btv": plain + 5 * lr + 2 * sr, "thirty": 30 * (plain + 5 * lr + 2 * sr)}[what]
    return 4.0 * n / HBM_ACHIEVABLE * 1e6


def _times(call, nsets, rounds, reps):
    for i in range(max(nsets, 2)):
        call(i)
    torch.cuda.synchronize()
    out = []
    for r in range(rounds):
        k = [r * reps]

        def one():
            call(k[0])
            k[0] += 1
        out.append(_common.timed_us(one, reps))
    return out


def bench_case(B, V, H, W, S, rounds, reps):
    dev = torch.device("cuda:0")
    lr, sr = B * V * H * W, B * H * W * S * S
    per_set = 4 * (3 * lr + 2 * sr)
    nsets = min(16, max(2, -(-2 * LLC_BYTES // per_set)))
    gen = torch.Generator(device=dev).manual_seed(S)
    xs = [torch.rand((B, S * H, S * W), device=dev, generator=gen) for _ in range(nsets)]
    lrs = [torch.rand((B, V, H, W), device=dev, generator=gen) for _ in range(nsets)]
    masks = [(torch.rand((B, V, H, W), device=dev, generator=gen) >= 0.3).float() for _ in range(nsets)]
    shifts = (torch.rand((B, V, 2), device=dev, generator=gen) * 3.0 - 1.5).contiguous()
    state, rstate = binding.ConsistencyState(B, V, H, W, dev), binding.RobustState(B, V, H, W, dev)
    loss, wloss, value = (torch.empty((B,), device=dev) for _ in range(3))
    c = torch.full((B,), LAM, device=dev)
    outs = [torch.empty((B, S * H, S * W), device=dev) for _ in range(2)]
    ws = binding.btv_workspace(B, S * H, S * W, dev)
    lib = binding.load_library()
    ptr, opt, stream = binding._ptr, binding._opt_ptr, binding._stream
    residual = lambda i: binding.consistency_residual(xs[i % nsets], lrs[i % nsets], masks[i % nsets], None, shifts, S, 1.0, True, state, loss)
    residual(0)
    rstate.beta_prev.copy_(state.beta)
    planes = []
    for i in range(nsets):                                               # residual planes of their own, one per input set
        residual(i)
        planes.append(state.residual.clone())

    def sums(i):
        binding._check(lib.hrn_robust_sums(ptr(planes[i % nsets]), opt(masks[i % nsets]), opt(None), ptr(shifts), ptr(rstate.beta_prev),
                                           ptr(rstate.workspace), rstate.ws_bytes, B, V, H, W, S, DELTA, stream()), "hrn_robust_sums")
        binding._check(lib.hrn_robust_finish(ptr(rstate.workspace), rstate.ws_bytes, ptr(state.count), ptr(rstate.beta), ptr(rstate.inlier),
                                             ptr(wloss), B, V, H, W, 1, stream()), "hrn_robust_finish")

    def apply(i):
        binding._check(lib.hrn_robust_apply(ptr(planes[i % nsets]), opt(masks[i % nsets]), opt(None), ptr(shifts), ptr(rstate.beta_prev),
                                            ptr(rstate.beta), ptr(rstate.weighted), B, V, H, W, S, DELTA, stream()), "hrn_robust_apply")

    sums(0)
    btv_step = lambda i: binding.btv_step(xs[i % nsets], c, P, ALPHA, EPS, out=outs[i % 2])
    btv_value = lambda i: binding.btv_value(xs[i % nsets], P, ALPHA, EPS, gain=LAM, out=value, workspace=ws)

    def iteration(robust, lam):
        def run(i):
            x, m = xs[i % nsets], masks[i % nsets]
            binding.consistency_residual(x, lrs[i % nsets], m, None, shifts, S, 1.0, True, state, loss)
            if robust:
                binding.robust_step(state, rstate, m, None, shifts, S, DELTA, True, wloss)
                binding.observe_adjoint(rstate.weighted, m, None, shifts, None, state.coef_step, None, x, S, out=outs[0])
            else:
                binding.observe_adjoint(state.residual, m, None, shifts, state.beta, state.coef_step, None, x, S, out=outs[0])
            if lam:
                binding.btv_step(outs[0], c, P, ALPHA, EPS, out=outs[1])
        return run

    thirty = lambda i: binding.reconstruct(xs[i % nsets], lrs[i % nsets], masks[i % nsets], None, shifts, S, 30, 1.0, True, True, DELTA, LAM, P,
                                           ALPHA, EPS, want_trace=False)
    res = {"B": B, "V": V, "H": H, "W": W, "scale": S, "input_sets": nsets, "rounds": rounds, "reps": reps}
    runs = {"robust_sums": sums, "robust_apply": apply, "btv_step": btv_step, "btv_value": btv_value, "plain": iteration(False, False),
            "welsch": iteration(True, False), "btv": iteration(False, True), "welsch_btv": iteration(True, True), "thirty": thirty}
    print(f"({B}, {V}, {H}, {W}) -> x{S}: median of {rounds} rounds x {reps} calls over {nsets} input sets")
    for name, call in runs.items():
        med, lo, hi = _common.spread(_times(call, nsets, rounds, reps if name != "thirty" else 1))
        floor = floor_us(B, V, H, W, S, name)
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi, "floor_us": floor}
        line = f"    {name:13s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   byte floor {floor:.1f} us = {100 * floor / med:.0f} % of it"
        if name in ("welsch", "btv", "welsch_btv"):
            line += f";   {med / res['plain']['median_us']:.2f} x one back_project iteration"
        if name == "thirty":
            line += f";   {med / 30 / res['plain']['median_us']:.2f} x one back_project iteration, per iteration"
        print(line)
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("robust_sr_bench")
    _common.emit("robust_sr_bench", [bench_case(B, V, H, W, S, o.rounds, o.reps) for B, V, H, W, S in CASES])


if __name__ == "__main__":
    main()
