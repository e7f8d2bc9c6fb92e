"""Time ShiftNet's fc1 (the library named by HRNET_HIP_LIB) at B = 32: prints us per launch and the bandwidth."""
import _common
import torch
import bench
from DeepNetworks.ShiftNet import ShiftNet
from hrnet_hip import binding

PARSER = _common.parser(__doc__)

if __name__ == "__main__":
    PARSER.parse_args()
    _common.require_gpu("fc1_time")
    sn = ShiftNet().cuda().eval()
    x = torch.rand(32, 2, 128, 128, device="cuda")
    with torch.no_grad():
        for _ in range(3):
            sn(x)
        v = bench.profile_families(binding, "cuda", lambda: sn(x), 20)["fc1"]
    print(f"{v['ms'] / v['launches'] * 1e3:.1f} us  {v['bytes'] / v['ms'] / 1e6:.0f} GB/s")

