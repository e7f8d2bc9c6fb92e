"""CPU: HRNet at upscale factors x2 / x4 (decoder.deconv kernel_size == stride == S, src/DeepNetworks/HRNet.py:147-156) - the
module builds with the reference's parameter shapes, unsupported decoders are refused, and the scale-taking C entry points size the
packed blob by S and reject a bad scale before any launch.  No kernel is launched here."""
import ctypes
import copy
import os

import pytest

from oracle import weights


def _cfg(kernel_size, stride=None):
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["decoder"]["deconv"]["kernel_size"] = kernel_size
    cfg["decoder"]["deconv"]["stride"] = kernel_size if stride is None else stride
    return cfg


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


@pytest.mark.parametrize("s", [2, 3, 4])
def test_hrnet_builds_at_each_scale(s):
    from DeepNetworks.HRNet import HRNet
    m = HRNet(_cfg(s))
    assert m._scale == s
    st = m.state_dict()
    assert tuple(st["decode.deconv.0.weight"].shape) == (64, 64, s, s)
    assert [k for k, _ in weights.HRNET_SHAPES] == list(st.keys())       # same keys / order as at x3: reference checkpoints load


@pytest.mark.parametrize("kernel_size,stride", [(3, 2), (4, 2), (2, 4), (5, 5), (1, 1)])
def test_unsupported_decoders_are_refused(kernel_size, stride):
    from DeepNetworks.HRNet import HRNet
    with pytest.raises(NotImplementedError, match=r"\(2, 3, 4\)"):
        HRNet(_cfg(kernel_size, stride))


def test_other_knobs_stay_refused():
    from DeepNetworks.HRNet import HRNet
    for path, value in ((("decoder", "final", "kernel_size"), 3), (("encoder", "channel_size"), 32),
                        (("decoder", "deconv", "out_channels"), 32)):
        cfg = _cfg(2)
        d = cfg
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] = value
        with pytest.raises(NotImplementedError):
            HRNet(cfg)


def test_packed_bytes_scale_with_the_decoder_weights(lib):
    # bf16 packs the decoder weights as bf16; fp32 and bf16x3 keep them fp32 (bf16x3 runs the fp32 decoder)
    for dt, es in ((0, 4), (1, 2), (2, 4)):
        for nl in (0, 2, 8):
            n3 = lib.hrn_hrnet_packed_bytes(dt, nl)
            assert lib.hrn_hrnet_packed_bytes_s(dt, nl, 3) == n3
            for s in (2, 4):
                delta = 64 * 64 * (s * s - 9) * es
                assert abs(lib.hrn_hrnet_packed_bytes_s(dt, nl, s) - (n3 + delta)) < 256, (dt, nl, s)
    for bad in (0, 1, 5, -3):
        assert lib.hrn_hrnet_packed_bytes_s(0, 2, bad) == 0
    assert lib.hrn_hrnet_packed_bytes_s(3, 2, 2) == 0 and lib.hrn_hrnet_packed_bytes_s(0, 99, 2) == 0


@pytest.mark.parametrize("bad", [0, 1, 5])
def test_bad_scale_fails_before_any_launch(lib, bad):
    from hrnet_hip import binding
    null = ctypes.c_void_p(0)
    # every pointer is null: a launch would fault, so -2 here means the scale was checked first
    calls = {
        "hrn_hrnet_forward_s": lambda: lib.hrn_hrnet_forward_s(null, 0, 2, bad, 1, null, null, 1, 2, 8, 8, null, null, 0, null),
        "hrn_decoder_forward_s": lambda: lib.hrn_decoder_forward_s(null, 0, 2, bad, null, 1, 8, 8, null, null),
        "hrn_hrnet_pack_s": lambda: lib.hrn_hrnet_pack_s(ctypes.byref(binding.HrnetParams()), 0, bad, null, 0, null),
        "hrn_hrnet_forward_train_s": lambda: lib.hrn_hrnet_forward_train_s(null, 0, 2, bad, 1, null, null, 1, 2, 8, 8, null, null, 0, null),
        "hrn_hrnet_backward_s": lambda: lib.hrn_hrnet_backward_s(null, 0, bad, ctypes.byref(binding.HrnetParams()), 1, null, null, 1, 2, 8, 8,
                                                                  null, ctypes.byref(binding.HrnetParams()), null, 0, null),
    }
    for name, call in calls.items():
        assert call() == -2, name
        assert b"scale" in lib.hrn_last_error(), (name, lib.hrn_last_error())
    # a good scale gets past the check to the next one (null pointers here)
    assert lib.hrn_hrnet_forward_s(null, 0, 2, 2, 1, null, null, 1, 2, 8, 8, null, null, 0, null) == -2
    assert b"null" in lib.hrn_last_error()
