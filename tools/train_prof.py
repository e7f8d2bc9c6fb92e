"""Per-kernel-family time of one train step (bench.py's step) under the library's hipEvent profiler: python tools/train_prof.py [precision]"""
import _common
import torch
import bench
from hrnet_hip import binding

PARSER = _common.parser(__doc__, positional=dict(precision="fp32"))

if __name__ == "__main__":
    o = PARSER.parse_args()
    prec = o.precision
    _common.require_gpu("train_prof")
    dev = torch.device("cuda", 0)
    step = bench.make_train_step(dev, 32, 32, 64, precision=prec)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    pf = bench.profile_families(binding, dev, step, 1)
    tot = sum(v["ms"] for v in pf.values())
    print(f"{prec}: profiled families {tot:.1f} ms (the step also runs unprofiled elementwise kernels)")
    for k, v in sorted(pf.items(), key=lambda kv: -kv[1]["ms"]):
        print(f"  {k:34s} {v['launches']:4d} x {v['ms'] / v['launches'] * 1e3:9.1f} us = {v['ms']:7.2f} ms   {v['flops'] / max(v['ms'], 1e-9) / 1e9:8.1f} TFLOP/s {v['bytes'] / max(v['ms'], 1e-9) / 1e6:8.1f} GB/s")

