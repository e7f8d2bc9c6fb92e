"""hrnet_hip: the MI355X (gfx950) HighRes-net hot path behind a C ABI (include/hrnet_hip.h).

`binding` wraps libhrnet_hip.so for PyTorch-ROCm tensors; `registration` is the sub-pixel registration of LR views, `composite` the cloud-free
reference frame from the views and their masks, `upsample` the bicubic x2 / x3 / x4 interpolation behind HRNet's global residual,
`shiftadd` the shift-and-add fusion of registered views onto the HR grid, `observation` the observation model (what a view should
have recorded of an HR frame), its consistency loss and iterative back-projection;
`build.build_library()` compiles it in-tree.
The sibling modules `DeepNetworks.HRNet`, `DeepNetworks.ShiftNet` and `lanczos` re-expose the reference's
module names on top of it so that the reference's train.py / predict.py import them unchanged.
"""
from . import binding  # noqa: F401
from . import composite  # noqa: F401
from . import observation  # noqa: F401
from . import registration  # noqa: F401
from . import shiftadd  # noqa: F401
from . import upsample  # noqa: F401
from .binding import BF16, F32, HrnetHipError, load_library  # noqa: F401
