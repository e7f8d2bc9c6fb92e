"""Per-parameter gradient error of the bf16x3 training mode against the fp64 autograd oracle (and the fp32 HIP path), for one shape:
python tools/x3_grad_debug.py [B V S]"""
import os

import _common
import numpy as np
from oracle import synth, weights

PARSER = _common.parser(__doc__, group=("B V S", (2, 4, 16)))

if __name__ == "__main__":
    o = PARSER.parse_args()
    B, V, S = o.B, o.V, o.S
    _common.require_gpu("x3_grad_debug")
    _common.tests_on_path()
    import conftest  # noqa
    import util, test_gpu_backward as T
    lrs, alphas, _ = synth.make_batch(5, B, V, S, V)
    rng = np.random.Generator(np.random.PCG64(77))
    cot = rng.standard_normal((B, 1, 3 * S, 3 * S)).astype(np.float32)
    SL = None
    if os.environ.get("SLOPE"):
        SL = {k: float(os.environ["SLOPE"]) for k in weights.hrnet_state(1234) if k.endswith((".1.weight", ".3.weight", "fuse.2.weight")) and "block" in k or k in ("encode.init_layer.1.weight", "fuse.fuse.2.weight", "decode.deconv.1.weight")}
    want_sr, want = T._oracle_grads(lrs, alphas, cot, True, slopes=SL)
    res = {}
    for prec in ("fp32", "bf16x3"):
        m = T._fresh_model(True, precision=prec, slopes=SL)
        sr = m(util.dev(lrs), util.dev(alphas))
        (sr * util.dev(cot)).sum().backward()
        res[prec] = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
        print(prec, "sr err", util.rel_err(sr.detach().cpu().numpy(), want_sr))
    for k in res["fp32"]:
        if res["fp32"][k].size > 1:
            print(f"{k:45s} fp32 {util.rel_err(res['fp32'][k], want[k]):.2e}  x3 {util.rel_err(res['bf16x3'][k], want[k]):.2e}")

