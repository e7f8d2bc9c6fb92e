#!/usr/bin/env python3
"""Time the observation model's derivative in the shifts: the two passes of csrc/observe_shift.hip beside the
existing passes they share a staged window with, and a joint iteration beside a `back_project` and a `reconstruct` iteration.

In ONE process, after a warm-up, the candidates of a shape alternating round by round, at (B, V, H, W) = (32, 32, 128, 128) and at one
(1, 32, 2048, 1536) scene, both x3, masks 30 % hidden, shifts within 1.5 px, brightness on, delta 0.1, lam 4e-4, P 2, alpha 0.7, eps 0.02,
damping 1e-3, max_step 0.5, view 0 fixed.  With lr = B V H W and sr = S^2 B H W elements of four bytes:

    residual        hrn_consistency_residual + hrn_consistency_finish:   4 (sr + 3 lr)   the yardstick of the normal pass
    normal          hrn_shift_normal (residual written) + _finish:       4 (sr + 3 lr)   the same bytes; ten sums a tile instead of three
    normal_only     the same without the residual plane:                 4 (sr + 2 lr)
    backward        hrn_observe_adjoint, the loss' existing backward:    4 (2 lr + sr)   the yardstick of the grad pass
    grad            hrn_observe_shift_grad + _finish (the loss' form):   4 (sr + 2 lr)
    plain           one back_project iteration:                          4 (sr + 3 lr) + 4 (2 lr + 2 sr)
    plain_joint     the same with the normal pass IN PLACE of the residual pass (binding.reconstruct_joint's updating iteration:
                    normal, hrn_consistency_finish on its plain sums, the normal finish with the update, the adjoint):    plain's bytes
    welsch_btv      one iteration of `reconstruct`'s defaults:           plain + 4 (5 lr) + 4 (2 sr)
    welsch_joint    the same with the normal pass in place of the residual pass:                                         welsch_btv's bytes

Every time is a pair of device events around `reps` calls enqueued back to back on one stream; the calls walk over enough input sets to
exceed the 256 MB last-level cache (the residual planes that `backward` and `grad` read rotate with them).  The figure is the median
over the rounds with min and max as the run-to-run spread; the byte floors are the algorithmic bytes at the 6.3 TB/s a streaming kernel
reaches on an MI355X.  Ratios are stated, none is a threshold.

usage: python tools/observe_shift_bench.py [--rounds R] [--reps N]
"""
import _common
import torch

from _common import HBM_ACHIEVABLE, LLC_BYTES
from hrnet_hip import binding

PARSER = _common.parser(__doc__, rounds=7, reps=10)
CASES = [(32, 32, 128, 128, 3), (1, 32, 2048, 1536, 3)]          # (B, V, H, W, scale)
DELTA, LAM, P, ALPHA, EPS, DAMPING, MAX_STEP = 0.1, 4e-4, 2, 0.7, 0.02, 1e-3, 0.5
RATIOS = {"normal": "residual", "normal_only": "residual", "grad": "backward", "plain_joint": "plain", "welsch_joint": "welsch_btv"}


def floor_us(B, V, H, W, scale, what):
    """the byte floor in microseconds (the formulas of the module's text)"""
    lr, sr = B * V * H * W, B * H * W * scale * scale
    plain = (sr + 3 * lr) + (2 * lr + 2 * sr)
    n = {"residual": sr + 3 * lr, "normal": sr + 3 * lr, "normal_only": sr + 2 * lr, "backward": 2 * lr + sr, "grad": sr + 2 * lr, "plain": plain,
         "plain_joint": plain, "welsch_btv": plain + 5 * lr + 2 * sr, "welsch_joint": plain + 5 * lr + 2 * sr}[what]
    return 4.0 * n / HBM_ACHIEVABLE * 1e6


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
    fixed = torch.zeros((B, V), dtype=torch.uint8, device=dev)
    fixed[:, 0] = 1
    state, rstate = binding.ConsistencyState(B, V, H, W, dev), binding.RobustState(B, V, H, W, dev)
    loss, wloss, gain = torch.empty((B,), device=dev), torch.empty((B,), device=dev), torch.ones((B,), device=dev)
    c = torch.full((B,), LAM, device=dev)
    outs = [torch.empty((B, S * H, S * W), device=dev) for _ in range(2)]
    ws = binding.shift_workspace(B, V, H, W, dev)
    normal, nxt, plane = torch.empty((B, V, 8), dtype=torch.float64, device=dev), torch.empty_like(shifts), torch.empty((B, V, H, W), device=dev)
    k = [0]
    left = []                                                            # what the residual pair leaves of every input set

    def pick(with_left=False):
        i = k[0] % nsets
        k[0] += 1
        return (xs[i], lrs[i], masks[i]) + ((left[i],) if with_left else ())

    def residual():
        x, y, m = pick()
        binding.consistency_residual(x, y, m, None, shifts, S, 1.0, True, state, loss)

    for i in range(nsets):
        binding.consistency_residual(xs[i], lrs[i], masks[i], None, shifts, S, 1.0, True, state, loss)
        left.append((state.residual.clone(), state.beta.clone(), state.coef_loss.clone()))
    rstate.beta_prev.copy_(state.beta)

    def shift_normal(with_plane, bp=None):
        def run():
            x, y, m = pick()
            binding.shift_normal(x, y, m, None, shifts, S, True, bp, DELTA, fixed, DAMPING, MAX_STEP, shifts_out=nxt,
                                 residual=plane if with_plane else None, workspace=ws, normal=normal)
        return run

    def backward():
        x, y, m, (r, bt, cf) = pick(True)
        binding.observe_adjoint(r, m, None, shifts, bt, cf, gain, None, S, out=outs[0])

    def grad():
        x, y, m, (r, bt, cf) = pick(True)
        binding.observe_shift_grad(x, r, m, None, shifts, bt, cf, gain, S, workspace=ws)

    def iteration(robust, joint):
        def run():
            x, y, m = pick()
            if joint:
                binding.shift_normal(x, y, m, None, shifts, S, True, rstate.beta_prev if robust else None, DELTA, fixed, DAMPING, MAX_STEP,
                                     shifts_out=nxt, workspace=ws, normal=normal, state=state, step=1.0, loss=loss)
            else:
                binding.consistency_residual(x, y, m, None, shifts, S, 1.0, True, state, loss)
            if robust:
                binding.robust_step(state, rstate, m, None, shifts, S, DELTA, True, wloss)
                binding.observe_adjoint(rstate.weighted, m, None, shifts, None, state.coef_step, None, x, S, out=outs[0])
                binding.btv_step(outs[0], c, P, ALPHA, EPS, out=outs[1])
            else:
                binding.observe_adjoint(state.residual, m, None, shifts, state.beta, state.coef_step, None, x, S, out=outs[0])
        return run

    runs = {"residual": residual, "normal": shift_normal(True), "normal_only": shift_normal(False), "backward": backward, "grad": grad,
            "plain": iteration(False, False), "plain_joint": iteration(False, True), "welsch_btv": iteration(True, False),
            "welsch_joint": iteration(True, True)}
    times = _common.alternate(runs, rounds, reps, max(nsets, 2))
    res = {"B": B, "V": V, "H": H, "W": W, "scale": S, "input_sets": nsets, "rounds": rounds, "reps": reps}
    print(f"({B}, {V}, {H}, {W}) -> x{S}: median of {rounds} rounds x {reps} calls over {nsets} input sets, candidates alternating")
    for name in runs:
        med, lo, hi = _common.spread(times[name])
        floor = floor_us(B, V, H, W, S, name)
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi, "floor_us": floor}
        line = f"    {name:13s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   byte floor {floor:.1f} us = {100 * floor / med:.0f} % of it"
        if name in RATIOS:
            line += f";   {med / res[RATIOS[name]]['median_us']:.2f} x {RATIOS[name]}"
        print(line)
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("observe_shift_bench")
    _common.emit("observe_shift_bench", [bench_case(B, V, H, W, S, o.rounds, o.reps) for B, V, H, W, S in CASES])


if __name__ == "__main__":
    main()
