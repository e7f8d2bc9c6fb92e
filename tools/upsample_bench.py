#!/usr/bin/env python3
"""Time the bicubic upsampler and the forward with the global residual.

In ONE process, after a warm-up, at 32 planes of 128 x 128 -> x2 / x3 / x4 and at one 2048 x 1536 plane at x3:

    forward        hrn_upsample without base:   4 n (HW + S^2 HW) bytes
    forward_base   hrn_upsample with base:      4 n (HW + 2 S^2 HW) bytes (base read, out written)
    backward       hrn_upsample_backward:       4 n (HW + S^2 HW) bytes
    torch_*        torch.nn.functional.interpolate(mode="bicubic") (+ torch.add) and aten's upsample_bicubic2d_backward on the device

A kernel's time is the pair of device events the library's profiler (hrn_profile_enable) puts around its launch; the calls walk over
enough input sets to exceed the 256 MB last-level cache, so the bytes come from HBM.  The torch calls are timed with a pair of device
events around `reps` calls.  A round is `reps` calls of each; the figure is the median over the rounds, with min and max as the
run-to-run spread.  The byte floors are the algorithmic bytes at the 6.3 TB/s a streaming kernel reaches on an MI355X.  Before anything
is timed the kernels' results are compared with torch's.  Then HRNet.forward in bf16 at B = 32, 32 views of 128 x 128 with
`global_residual` on against off, alternating (--skip-forward leaves it out).  There is no pass / fail threshold on time.

usage: python tools/upsample_bench.py [--rounds R] [--reps N] [--skip-forward]
"""
import _common
import torch
import torch.nn.functional as F

from _common import HBM_ACHIEVABLE, LLC_BYTES
from hrnet_hip import binding

PARSER = _common.parser(__doc__, rounds=7, reps=10, skip_forward=False)
CASES = [(32, 128, 128, 2), (32, 128, 128, 3), (32, 128, 128, 4), (1, 2048, 1536, 3)]        # (planes, H, W, scale)
A = -0.75


def floor_us(n, H, W, scale, with_base):
    """the byte floor in microseconds: the frames in, the output out, and with `base` the output-sized operand in as well"""
    return 4.0 * n * H * W * (1 + (2 if with_base else 1) * scale * scale) / HBM_ACHIEVABLE * 1e6


def _kernel_us(family, call, nsets, rounds, reps):
    for i in range(nsets):
        call(i)
    torch.cuda.synchronize()
    out = []
    for r in range(rounds):
        binding.profile_enable(True)
        for i in range(reps):
            call(r * reps + i)
        torch.cuda.synchronize()
        rec = binding.profile_read()[family]
        binding.profile_enable(False)
        out.append(rec["ms"] * 1e3 / rec["launches"])
    return out


def bench_case(n, H, W, S, rounds, reps):
    dev = torch.device("cuda:0")
    per_set = 4 * n * H * W * (1 + 2 * S * S)
    nsets = min(64, max(2, -(-2 * LLC_BYTES // per_set)))
    gen = torch.Generator(device=dev).manual_seed(S)
    frames = [torch.rand((n, H, W), device=dev, generator=gen) for _ in range(nsets)]
    bases = [torch.rand((n, S * H, S * W), device=dev, generator=gen) for _ in range(nsets)]
    outs = [torch.empty((n, S * H, S * W), device=dev) for _ in range(2)]
    interp = lambda f: F.interpolate(f[None], scale_factor=S, mode="bicubic", align_corners=False)[0]
    t_bwd = lambda g: torch.ops.aten.upsample_bicubic2d_backward(g[None], [S * H, S * W], [1, n, H, W], False)[0]
    # what is timed computes what torch computes in fp64 (torch's fp32 kernel forms every pixel's source coordinate from a rounded
    # 1 / S, so its weights drift with the index; the library's S phases are exact): 1e-5 of the sum of the absolute terms, <= 2 and 2 S^2
    f64, b64 = frames[0].double(), bases[0].double()
    assert torch.allclose(binding.upsample(frames[0], None, S, A).double(), interp(f64), rtol=0, atol=2e-5)
    assert torch.allclose(binding.upsample(frames[0], bases[0], S, A).double(), interp(f64) + b64, rtol=0, atol=3e-5)
    assert torch.allclose(binding.upsample_backward(bases[0], H, W, S, A).double(), t_bwd(b64), rtol=0, atol=2e-5 * S * S)
    del f64, b64
    res = {"planes": n, "H": H, "W": W, "scale": S, "input_sets": nsets, "rounds": rounds, "reps": reps}
    runs = {
        "forward": ("upsample", lambda i: binding.upsample(frames[i % nsets], None, S, A, out=outs[i % 2]), False,
                    lambda i: interp(frames[i % nsets])),
        "forward_base": ("upsample", lambda i: binding.upsample(frames[i % nsets], bases[i % nsets], S, A, out=outs[i % 2]), True,
                         lambda i: torch.add(interp(frames[i % nsets]), bases[i % nsets])),
        "backward": ("upsample_backward", lambda i: binding.upsample_backward(bases[i % nsets], H, W, S, A), False,
                     lambda i: t_bwd(bases[i % nsets])),
    }
    print(f"{n} x {H} x {W} -> x{S}: median of {rounds} rounds x {reps} calls over {nsets} input sets")
    for name, (family, call, with_base, tcall) in runs.items():
        kern = _kernel_us(family, call, nsets, rounds, reps)
        for i in range(2):
            tcall(i)
        comp = [_common.timed_us(lambda: tcall(r), 1) for r in range(rounds * 2)]
        floor = floor_us(n, H, W, S, with_base)
        (med, lo, hi), (tmed, tlo, thi) = _common.spread(kern), _common.spread(comp)
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi, "floor_us": floor}
        res["torch_" + name] = {"median_us": tmed, "min_us": tlo, "max_us": thi}
        print(f"    {name:13s} {med:9.1f} us   (min {lo:.1f}, max {hi:.1f})   byte floor {floor:.1f} us = {100 * floor / med:.0f} % of it;"
              f"   torch {tmed:9.1f} us (min {tlo:.1f}, max {thi:.1f}) = {tmed / med:.1f} x")
    return res


def bench_forward(rounds, reps):
    """HRNet.forward, bf16, B = 32, 32 views of 128 x 128: global_residual on against off, alternating"""
    _common.tests_on_path()
    import util
    from oracle import synth
    lrs, alphas = synth.fast_batch(5, 32, 32, 128)
    x, a = util.dev(lrs), util.dev(alphas)
    m = util.hip_hrnet("bf16")

    def run(flag):
        m.global_residual = flag
        try:
            return m(x, a)
        finally:
            m.global_residual = None

    with torch.no_grad():
        times = _common.alternate({"forward_off": lambda: run(None), "forward_on": lambda: run(True)}, rounds, reps, 2)
    res = {}
    for name, t in times.items():
        med, lo, hi = _common.spread(t)
        res[name] = {"median_us": med, "min_us": lo, "max_us": hi}
        print(f"    {name + ' bf16':24s} {med / 1e3:9.3f} ms   (min {lo / 1e3:.3f}, max {hi / 1e3:.3f})")
    return res


def main():
    o = PARSER.parse_args()
    _common.require_gpu("upsample_bench")
    results = [bench_case(n, H, W, S, o.rounds, o.reps) for n, H, W, S in CASES]
    if not o.skip_forward:
        results.append(bench_forward(o.rounds, o.reps))
    _common.emit("upsample_bench", results)


if __name__ == "__main__":
    main()
