"""CPU: the conditions under which the fp32 cases of tests/test_gpu_kernels_fwd.py mean what they say, with that file's own builders, seeds
and constants (tests/kernel_refs.py): the `full` operand set carries more than 16 significant bits in most elements (and the `exact` set at
most 8, so that operand rounding is a no-op there); a plain float32 evaluation on the CPU stays inside C_F32 T of the fp64 reference; and
every asserted negative control's wrong reference lies, at its worst element, at least twice the bound from the right one - the GPU's own
error is at most once the bound, so it cannot hide the control.  Controls listed as unasserted are printed with their separation."""
import pytest
import torch

import kernel_bounds
import kernel_refs as K

D = torch.float64
DEC_CASE = (2, 17, 50, 3)            # the decoder control's case: DEC_SHAPES["17x50"] at S = 3
STEM_CASE = (2, 15, 33)              # the stem control's: STEM_SHAPES["15x33"] as (M, H, W)


def _conv_args(name, opset="full", dtype=D):
    """the arguments of ref_conv_epi for instance `name` at the controls' case, as tests/test_gpu_kernels_fwd.py::_conv_case builds them"""
    inst = K.F32_INSTANCES[name]
    geo = K.conv_geometry(inst, K.F32_CONTROL_SHAPE)
    ops = K.f32_conv_operands(inst, geo, K.F32_CONTROL_SEED, opset)
    cast = lambda t: None if t is None else t.to(dtype)
    x = ops["inp"] if ops["inp"] is not None else K._pair_gather(ops["stack"][:, :geo["n"]], geo["half"], geo["pair_last"])
    alph = K.conv_alphas(geo["B"], geo["V"], opset) if inst[4] == 3 else None
    return dict(x=cast(x), w=cast(ops["w"]), b=cast(ops["bias"]), slope=K.f32_slope(K.F32_CONTROL_SLOPE, opset), res_mode=inst[4],
                res=cast(ops["res"]), stack=cast(ops["stack"]), geo=geo, alph=alph), ops


def _case(target, dtype=D):
    """-> the case dict of kernel_refs.f32_control_reference for a control's target, evaluated in `dtype`"""
    if target == "stem":
        M, H, W = STEM_CASE
        ops = K.f32_stem_operands("f32", M, H, W, 17 + M + H)
        slope = K.f32_slope([None, 0.25, K.BF(-0.3), 1.5][3 % 4], "full")        # 15x33 is STEM_SHAPES' entry 3
        return dict(kind="stem", args=dict(x0=ops["x0"].to(dtype), x1=ops["x1"].to(dtype), rep1=ops["rep1"], sub=None, w=ops["w"].to(dtype),
                                           b=ops["bias"].to(dtype), slope=slope, m0=0, m1=M))
    if target == "decoder":
        N, H, W, S = DEC_CASE
        ops = K.f32_decoder_operands(N, H, W, S, 1000 + 10 * S + N)
        slope = K.f32_slope([0.25, K.BF(-0.3), 1.5, 0.0][(S + 3) % 4], "full")    # 17x50 is DEC_SHAPES' entry 3
        return dict(kind="decoder", args=dict(fused=ops["fused"].to(dtype), wd=ops["wd"].to(dtype), bd=ops["bd"].to(dtype), slope=slope,
                                              wf=ops["wf"].to(dtype), bf=ops["bf"].to(dtype), S=S))
    return dict(kind="conv", args=_conv_args(target, "full", dtype)[0])


TARGETS = list(K.F32_INSTANCES) + ["stem", "decoder"]
_RIGHT = {}


def _right(target):
    """the right fp64 reference of a target, computed once"""
    if target not in _RIGHT:
        _RIGHT[target] = K.f32_control_reference(None, _case(target))
    return _RIGHT[target]


def test_case_constants_match_the_gpu_tests():
    """the shapes this file restates (it cannot import a test module) are the ones the control table names"""
    assert K.SHAPES[K.F32_CONTROL_SHAPE] == STEM_CASE[1:] == (15, 33)
    assert K.F32_CONTROL_DECODER == (f"{DEC_CASE[1]}x{DEC_CASE[2]}", DEC_CASE[3])
    assert {n for _, n in K.F32_CONTROLS + K.F32_CONTROLS_UNASSERTED} <= set(TARGETS)
    assert not set(K.F32_CONTROLS) & set(K.F32_CONTROLS_UNASSERTED)
    assert 0 < 4 * kernel_bounds.F32_MEASURED[0] <= K.C_F32 <= K.C        # four times the measured maximum, under the ceiling


def test_rotation_gives_every_instance_the_full_set():
    """kernel_refs.f32_opset: every fp32 instance meets `full` at 15x33, at multi and at two more shapes, and keeps `exact` somewhere"""
    shapes = list(K.SHAPES)
    for ii in range(40):
        sets = [K.f32_opset(ii, si) for si in range(len(shapes))]
        assert sets[shapes.index("15x33")] == sets[shapes.index("multi")] == "full"
        assert sets.count("full") >= 4 and sets.count("exact") >= 2, (ii, sets)


@pytest.mark.parametrize("name", list(K.F32_INSTANCES))
def test_conv_operand_sets(name):
    """`full`: more than 16 significant bits in most elements of every operand, slope and alphas included; `exact`: at most 8 everywhere.
    No zero of either sign in any operand (the alpha = 0 slot is compared bit for bit with its residual)."""
    for si, shape in enumerate(K.SHAPES):
        if shape == "multi":
            continue                    # (its image count depends on the GPU's CU count; the same builder at 3 x 33)
        geo = K.conv_geometry(K.F32_INSTANCES[name], shape)
        for opset in ("full", "exact"):
            ops = K.f32_conv_operands(K.F32_INSTANCES[name], geo, 100 + 7 * si, opset)
            for key, t in ops.items():
                if t is None:
                    continue
                bits = K.sig_bits(t)
                assert not bool((t == 0).any())
                if opset == "exact":
                    assert int(bits.max()) <= 8, (name, shape, key)
                else:
                    assert float((bits > 16).double().mean()) > 0.95, (name, shape, key, float((bits > 16).double().mean()))
    for a in K.SLOPES_FULL:
        if a not in (None, 0.0, 1.0):
            assert int(K.sig_bits(torch.tensor([a], dtype=torch.float32))) > 16 and float(torch.tensor(a, dtype=torch.float32)) == a
    al = K.conv_alphas(3, 7, "full")
    assert set(al.unique().tolist()) == {0.0, 1.0, K.ALPHA_FULL} and int(K.sig_bits(torch.tensor([K.ALPHA_FULL]))) > 16
    assert [None if a is None else (a < 0, a == 0, a == 1, a > 1) for a in K.SLOPES] == \
           [None if a is None else (a < 0, a == 0, a == 1, a > 1) for a in K.SLOPES_FULL]


def test_stem_and_decoder_operands_are_general_fp32():
    for mode in ("f32", "f32sub"):
        ops = K.f32_stem_operands(mode, 9, 15, 33, 41)
        for key in ("x0", "x1", "w", "bias") + (("sub",) if mode == "f32sub" else ()):
            frac = float((K.sig_bits(ops[key].contiguous()) > 16).double().mean())
            assert frac > 0.9, (mode, key, frac)
    ops = K.f32_stem_operands("f32sub", 9, 15, 33, 41)
    assert torch.equal(ops["x"][:, 0], ops["x0"]) and torch.equal(ops["x"][:, 1], ops["x1"]) and ops["rep1"] == 1
    assert float((ops["sub"].double() - ops["x"].double().mean((2, 3))).abs().max()) < 1e-6
    ops = K.f32_decoder_operands(2, 9, 27, 3, 5)
    for key, t in ops.items():
        if t.numel() > 1:
            assert float((K.sig_bits(t) > 16).double().mean()) > 0.95, key


@pytest.mark.parametrize("target", TARGETS)
def test_float32_evaluation_is_inside_the_bound(target):
    """the same formula evaluated in float32 on the CPU (F.conv2d / conv_transpose2d in fp32) against the fp64 reference: <= C_F32 T"""
    want, T = _right(target)
    c32 = _case(target, torch.float32)
    got, _ = {"conv": K.ref_conv_epi, "stem": K.ref_stem_fwd, "decoder": K.ref_decoder_fwd}[c32["kind"]](with_T=False, **c32["args"])
    assert got.dtype == torch.float32
    r = float(((got.double() - want).abs() / (K.C_F32 * T + 1e-300)).max())
    print(f"{target}: float32 on the CPU, max error / (C_F32 T) = {r:.3e}   (C needed {r * K.C_F32:.2e})")
    assert r <= 1.0


def _separation(control, target, c):
    want, T = _right(target)
    bad, Tb = K.f32_control_reference(control, _case(target))
    return float(((bad - want).abs() / (c * torch.maximum(T, Tb) + 1e-300)).max())


@pytest.mark.parametrize("control,target", K.F32_CONTROLS)
def test_control_is_separated_by_twice_the_bound(control, target):
    """|wrong - right| >= 2 C_F32 max(T, T_wrong) at the worst element: with the kernel within C_F32 T of the right reference, it is then
    further than C_F32 T_wrong from the wrong one.  The bf16 and 10-bit roundings clear twice the suite's ceiling C as well."""
    sep = _separation(control, target, K.C_F32)
    print(f"{control} {target}: |wrong - right| / (C_F32 T) = {sep:.3g} at the worst element")
    assert sep >= 2.0
    if control.startswith(("round8_", "round11_")):
        assert _separation(control, target, K.C) >= 2.0


def test_exact_set_cannot_see_operand_rounding():
    """on the `exact` operands every rounding control is a no-op (the wrong reference IS the right one): what the `full` set is for"""
    args, _ = _conv_args("f32enc", "exact")
    case = dict(kind="conv", args=args)
    want, _ = K.f32_control_reference(None, case)
    for control in ("round8_x", "round8_w", "round11_x", "round16_w"):
        assert torch.equal(K.f32_control_reference(control, case)[0], want)


def test_unasserted_controls_are_reported():
    """controls below twice the bound under C_F32 are asserted nowhere; their separation is printed (and must really be below 2)"""
    for control, target in K.F32_CONTROLS_UNASSERTED:
        sep = _separation(control, target, K.C_F32)
        print(f"NOT ASSERTED {control} {target}: |wrong - right| / (C_F32 T) = {sep:.3g}")
        assert sep < 2.0, "this control is separated: move it to F32_CONTROLS"
