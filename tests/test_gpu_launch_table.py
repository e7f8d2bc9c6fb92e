"""GPU (-m gpu): the launch table of HRNet's host walks - pack, inference forward, training forward and backward - against
tests/golden/hrnet_launch_table.json.

For every case the step runs under kt._launches and the whole {name: launches} dict, the zero entries included, has to equal the
recorded one.  Together with tools/device_code_diff.py ("device code identical") and bit-identical outputs this is what a host-only
change of csrc/api.hip, csrc/train.hip or csrc/hrnet_layout.h has to show: the same kernels, as many times.

The fixture was recorded on the commit BEFORE the conv-site table, not on the code under test: this file uses only what that commit has
(HRNet, kt._launches), was copied into a checkout of it, and its __main__ was run there on an MI355X; the JSON is committed unchanged.
To record again (after a change that means to launch differently), from the repository root:

    PYTHONPATH=.:highres-net_amd python tests/test_gpu_launch_table.py [out.json]

All cases are B = 2, H = W = 16 - smaller than any convolution tile, so every kernel runs its edge path:
    V = 1 (no fusion level: the memcpy branch), 2 (one level, which is also the last and writes `fused`), 5 (odd parity, two levels)
    x num_layers 0, 2  x  fp32, bf16, bf16x3  x  pack, inference forward, training forward, full backward;
    at V = 5, num_layers = 2: the backward with part of the model frozen and with lrs / alphas requiring grad; one case at scale 2.
"""
import copy
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from kt import _launches
from oracle import weights
from util import _state

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hrnet_launch_table.json")
PRECS = ("fp32", "bf16", "bf16x3")
FROZEN = {                                                    # the patterns of tests/test_gpu_frozen.py
    "encoder": lambda k: k.startswith("encode."),
    "encoder+fuse": lambda k: k.startswith(("encode.", "fuse.")),
    "decoder": lambda k: k.startswith("decode."),
    "one_slope": lambda k: k == "fuse.fuse.2.weight",
}
ALL_STEPS = ("pack", "forward", "forward_train", "backward")

# case id -> dict(V, num_layers, prec, scale, frozen, inputs_grad, steps)
CASES = {}
for _V in (1, 2, 5):
    for _nl in (0, 2):
        for _prec in PRECS:
            CASES[f"V{_V}-nl{_nl}-{_prec}"] = dict(V=_V, nl=_nl, prec=_prec, scale=3, frozen=None, inputs_grad=False, steps=ALL_STEPS)
for _prec in PRECS:
    for _pat in FROZEN:
        CASES[f"V5-nl2-{_prec}-frozen:{_pat}"] = dict(V=5, nl=2, prec=_prec, scale=3, frozen=_pat, inputs_grad=False, steps=("backward",))
    CASES[f"V5-nl2-{_prec}-inputs_grad"] = dict(V=5, nl=2, prec=_prec, scale=3, frozen=None, inputs_grad=True, steps=("backward",))
CASES["V5-nl2-bf16-scale2"] = dict(V=5, nl=2, prec="bf16", scale=2, frozen=None, inputs_grad=False, steps=ALL_STEPS)


def _tables(V, nl, prec, scale, frozen, inputs_grad, steps, B=2, H=16):
    """-> {step: {name: launches}} of one case."""
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["encoder"]["num_layers"] = nl
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    m = HRNet(cfg)
    st = _state(scale)
    m.load_state_dict({k: st[k] for k in m.state_dict()})
    m.precision = m.train_precision = prec
    m = m.cuda()
    for k, p in m.named_parameters():
        p.requires_grad_(frozen is None or not FROZEN[frozen](k))
    rng = np.random.Generator(np.random.PCG64(3))
    lrs = torch.from_numpy(rng.random((B, V, H, H), dtype=np.float32)).cuda()
    alphas = torch.from_numpy((rng.random((B, V)) > 0.3).astype(np.float32)).cuda()
    cot = torch.from_numpy(rng.standard_normal((B, 1, scale * H, scale * H)).astype(np.float32)).cuda()
    out = {}
    # the blob of this precision is packed once, here; the forwards below find it in the module's cache
    out["pack"], _ = _launches(lambda: m.packed_parameters())
    m.eval()
    with torch.no_grad():
        out["forward"], _ = _launches(lambda: m(lrs, alphas))
    m.train()
    lrs.requires_grad_(inputs_grad)
    alphas.requires_grad_(inputs_grad)
    out["forward_train"], sr = _launches(lambda: m(lrs, alphas))
    out["backward"], _ = _launches((sr * cot).sum().backward)
    return {s: out[s] for s in steps}


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_case_and_tells_a_frozen_encoder_apart():
    rec = _recorded()
    assert sorted(rec) == sorted(CASES)
    for prec in PRECS:
        assert rec[f"V5-nl2-{prec}"]["backward"] != rec[f"V5-nl2-{prec}-frozen:encoder"]["backward"]
        assert rec[f"V5-nl2-{prec}"]["backward"]["conv_dgrad"] > 0 and rec[f"V5-nl2-{prec}"]["pack"] != rec[f"V5-nl2-{prec}"]["forward"]


@pytest.mark.parametrize("case", list(CASES))
def test_launch_table_is_the_recorded_one(case):
    got = _tables(**CASES[case])
    want = _recorded()[case]
    for step in CASES[case]["steps"]:
        assert got[step] == want[step], (case, step)
    assert sorted(got) == sorted(want)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    tables = {case: _tables(**kw) for case, kw in CASES.items()}
    with open(path, "w") as f:
        json.dump(tables, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(tables)} cases -> {path}")
