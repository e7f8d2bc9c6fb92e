"""CPU: the C-ABI library loads, exports every symbol include/hrnet_hip.h declares, and its host-only entry points
(sizes, argument validation) behave; no kernel is launched here.  And the three ctypes tables - binding.SIGNATURES, io_binding.SIGNATURES
and the test hooks' kt.SIGNATURES - agree with the C declarations they bind, argument by argument (text against table: no library)."""
import ctypes
import os
import re

import pytest

import kt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hrn_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from hrnet_hip import binding
    syms = declared_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/hrnet_hip.h but not exported"
    assert sorted(binding.SIGNATURES) == syms, "binding.SIGNATURES and the header disagree"


def test_version_and_sizes(lib):
    assert lib.hrn_version() == 1
    # packed HRNet parameters: every conv weight once, in the storage dtype (+ small f32 tensors, 256-B aligned)
    w_elems = 4 * 64 * 64 * 9 + 64 * 64 * 9 + 2 * 128 * 128 * 9 + 128 * 64 * 9 + 64 * 64 * 9
    for dt, es in ((0, 4), (1, 2), (2, 4)):       # f32, bf16, bf16x3 (two bf16 planes; fp32 decoder weights)
        n = lib.hrn_hrnet_packed_bytes(dt, 2)
        assert w_elems * es < n < w_elems * es + 64 * 1024
    assert lib.hrn_hrnet_packed_bytes(3, 2) == 0 and lib.hrn_hrnet_packed_bytes(0, 99) == 0
    # workspace: reference frame + 3 view stacks + fused state
    B, V, H = 32, 32, 128
    stack = B * V * H * H * 64 * 2
    ws = lib.hrn_hrnet_workspace_bytes(1, B, V, H, H)
    assert 3 * stack < ws < 3 * stack + B * H * H * (4 + 128) + 4096
    assert lib.hrn_hrnet_workspace_bytes(1, 0, V, H, H) == 0
    conv_bytes = 4 * 9 * (2 * 64 + 3 * 64 * 64 + 64 * 128 + 3 * 128 * 128)
    assert conv_bytes < lib.hrn_shiftnet_packed_bytes() < conv_bytes + 64 * 1024       # fc1.weight (134 MB) is read in place, not packed
    assert lib.hrn_shiftnet_workspace_bytes(4) > 2 * 4 * 128 * 128 * 64 * 4


def test_bad_arguments_fail_before_any_launch(lib):
    null = ctypes.c_void_p(0)
    rc = lib.hrn_hrnet_forward(null, 0, 2, 1, null, null, 1, 2, 8, 8, null, null, 0, null)
    assert rc == -2 and b"null" in lib.hrn_last_error()
    rc = lib.hrn_hrnet_forward(null, 7, 2, 1, null, null, 1, 2, 8, 8, null, null, 0, null)
    assert rc == -2 and b"dtype" in lib.hrn_last_error()
    rc = lib.hrn_lanczos_shift(null, null, 1, 1, 2, 2, null, null)
    assert rc == -2
    assert lib.hrn_profile_enable(0) == 0 and lib.hrn_profile_count() == 0


# ----------------------------------------------------------------------------- declarations against ctypes tables
SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "long": ctypes.c_long,
           "void": None}
STRUCTS = {"hrn_hrnet_params": "HrnetParams", "hrn_shiftnet_params": "ShiftnetParams"}


def _c_kind(decl, what):
    """a C parameter or return type (its name already taken off) -> a scalar's ctype (None for void), "ptr", or a struct's Python name"""
    if "*" in decl:
        base = decl.replace("*", " ").replace("const", " ").split()
        return STRUCTS.get(base[0], "ptr") if len(base) == 1 else "ptr"
    base = " ".join(t for t in decl.split() if t != "const")
    assert base in SCALARS, f"{what}: C type `{decl}` is not one this reader knows"
    return SCALARS[base]


def declarations(path):
    """every `ret name(args);` of a C header -> {name: (return kind, [argument kinds])}; anything else left in the text is an error"""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\b[^{;]*\{[^}]*\}\s*\w+\s*;", " ", text)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.replace("}", " ").split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(\w+) ?\((.*)\)", stmt)
        assert m, f"{path}: cannot read `{stmt}`"
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, name
        kinds = []
        if args != "void":
            for k, a in enumerate(args.split(",")):
                m2 = re.fullmatch(r"(.*?)(\w+)", a.strip())          # the parameter's name is its last word
                assert m2 and m2.group(1).strip(), f"{name}: argument {k} `{a}` has no name or no type"
                kinds.append(_c_kind(m2.group(1), f"{name}: argument {k}"))
        out[name] = (_c_kind(ret, f"{name}: return type"), kinds)
    return out


def _agrees(kind, ct, structs):
    if kind == "ptr":
        return ct in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(ct, type) and issubclass(ct, ctypes._Pointer))
    if isinstance(kind, str):
        return ct is ctypes.POINTER(structs[kind])
    return ct is kind


def mismatches(decls, table, structs=None):
    """-> one line per disagreement between a header's declarations and a name -> (return ctype, argument ctypes) table"""
    bad = [f"{n}: declared but not in the table" for n in sorted(set(decls) - set(table))]
    bad += [f"{n}: in the table but not declared" for n in sorted(set(table) - set(decls))]
    for n in sorted(set(decls) & set(table)):
        (ret, args), (res, cts) = decls[n], table[n]
        if not _agrees(ret, res, structs):
            bad.append(f"{n}: return type: C {ret}, table {res}")
        if len(args) != len(cts):
            bad.append(f"{n}: {len(args)} arguments in C, {len(cts)} in the table")
            continue
        bad += [f"{n}: argument {k}: C {a}, table {t}" for k, (a, t) in enumerate(zip(args, cts)) if not _agrees(a, t, structs)]
    return bad


def _abis():
    from hrnet_hip import binding, io_binding
    structs = {"HrnetParams": binding.HrnetParams, "ShiftnetParams": binding.ShiftnetParams}
    return {"hrnet_hip": (os.path.join(ROOT, "include", "hrnet_hip.h"), binding.SIGNATURES, structs),
            "hrnet_io": (os.path.join(ROOT, "include", "hrnet_io.h"), io_binding.SIGNATURES, structs),
            "kernel_test": (os.path.join(ROOT, "highres-net_amd", "hrnet_hip", "csrc", "kernel_test.h"), kt.SIGNATURES, structs)}


@pytest.mark.parametrize("abi", ["hrnet_hip", "hrnet_io", "kernel_test"])
def test_table_agrees_with_the_declarations(abi):
    path, table, structs = _abis()[abi]
    decls = declarations(path)
    assert len(decls) >= 8
    bad = mismatches(decls, table, structs)
    assert not bad, "\n".join(bad)


def test_comparison_reports_a_wrong_type_a_dropped_argument_and_a_missing_function():
    """the negative control, on a copy of the hooks' own table"""
    path, table, structs = _abis()["kernel_test"]
    decls = declarations(path)
    name = "hrn_kt_conv3x3_epi"
    res, args = table[name]
    k = args.index(ctypes.c_int)
    wrong = dict(table, **{name: (res, args[:k] + [ctypes.c_size_t] + args[k + 1:])})
    assert mismatches(decls, wrong, structs) == [f"{name}: argument {k}: C {ctypes.c_int}, table {ctypes.c_size_t}"]
    short = dict(table, **{name: (res, args[:-1])})
    assert mismatches(decls, short, structs) == [f"{name}: {len(args)} arguments in C, {len(args) - 1} in the table"]
    gone = {n: v for n, v in table.items() if n != name}
    assert mismatches(decls, gone, structs) == [f"{name}: declared but not in the table"]


def test_reader_refuses_what_it_does_not_know(tmp_path):
    h = tmp_path / "x.h"
    h.write_text("int f(unsigned n);")
    with pytest.raises(AssertionError, match="not one this reader knows"):
        declarations(str(h))
    h.write_text("int f(int n) { return n; }")
    with pytest.raises(AssertionError, match="cannot read"):
        declarations(str(h))


def test_every_hook_is_exported(lib):
    for name in kt.SIGNATURES:
        assert hasattr(lib, name), f"{name} is in kt.SIGNATURES but not exported"


# ----------------------------------------------------------------------------- the parameter table against the module and the struct
@pytest.mark.parametrize("num_layers", range(9))
def test_param_table_keys_are_the_modules_parameters(num_layers):
    import copy
    from hrnet_hip import binding
    from oracle import weights
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["encoder"]["num_layers"] = num_layers
    keys = [k for k, _ in HRNet(cfg).named_parameters()]
    assert [k for k, _, _ in binding.hrnet_param_table(num_layers)] == keys
    assert binding.hrnet_param_names(num_layers) == keys


def test_param_table_covers_every_pointer_of_the_struct_once():
    from hrnet_hip import binding
    assert binding.MAX_RES_LAYERS == 8
    slots = []
    for name, ctype in binding.HrnetParams._fields_:
        if ctype is ctypes.c_void_p:
            slots.append((name, None))
        elif issubclass(ctype, ctypes.Array):
            slots += [(name, i) for i in range(ctype._length_)]
    assert len(slots) == 3 + 3 * 16 + 2 + 3 * 2 + 3 + 5
    pairs = [(f, i) for _, f, i in binding.hrnet_param_table(8)]
    assert len(set(pairs)) == len(pairs) and sorted(pairs, key=str) == sorted(slots, key=str)
