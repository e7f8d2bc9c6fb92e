#!/usr/bin/env python3
"""Per-kernel-family timing of one HRNet forward (library hipEvent profiler).  Usage: python tools/kbench.py [prec] [B] [V] [S]"""
import _common
import torch
import bench
from hrnet_hip import binding
from DeepNetworks.HRNet import HRNet

PARSER = _common.parser(__doc__, positional=dict(prec="bf16", B=32, V=32, S=128))

if __name__ == "__main__":
    o = PARSER.parse_args()
    prec, B, V, S = o.prec, o.B, o.V, o.S
    _common.require_gpu("kbench")
    torch.manual_seed(1234)
    net = HRNet(dict(bench.NETWORK, precision=prec)).cuda().eval()
    lrs, alphas = bench.synth_inputs(B, V, S, "cuda", 100)
    packed, dt = net.packed_parameters()
    sr = torch.empty((B, 1, 3 * S, 3 * S), device="cuda")
    forward = lambda: binding.hrnet_forward(packed, dt, 2, True, lrs, alphas, out=sr)
    for _ in range(2):
        forward()
    torch.cuda.synchronize()
    n = 3
    prof = bench.profile_families(binding, "cuda", forward, n)
    tot = sum(v["ms"] for v in prof.values()) / n
    print(f"{prec} B={B} V={V} S={S}: {tot:.3f} ms/fwd  {B / tot * 1e3:.1f} frames/s")
    for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
        print(f"   {k:24s} {v['launches'] // n:3d} x {v['ms'] / v['launches']:8.4f} ms  {v['flops'] / v['ms'] / 1e9:8.1f} TF/s  {v['bytes'] / v['ms'] / 1e6:8.1f} GB/s")

