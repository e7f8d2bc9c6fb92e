"""CPU: the plumbing every tool under tools/ shares (tools/_common.py, tools/steps.sh): the timing helpers on fake callables, every
tool's command line against a hand-written table, the usage errors, --help, the refusal to run without a device, and the shell
scripts' `step`.  Nothing here compiles or needs a GPU."""
import glob
import importlib
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import _common  # noqa: E402

# tools with a module-level PARSER, imported here; the three script-style ones parse before their heavy imports and run as children
IMPORTED = ("ensemble_bench", "tiled_bench", "shift_loss_bench", "train_step_bench", "loader_rate", "kbench", "train_prof", "fc1_time",
            "soak", "x3_grad_debug", "gpu_diag", "pmc_summary", "pmc_busy_summary", "variant")
SCRIPTS = ("prof_collect.py", "stamps/read_r64.py", "stamps/read_v6.py")
ON_DEVICE = ("ensemble_bench", "tiled_bench", "shift_loss_bench", "train_step_bench", "loader_rate", "kbench", "train_prof", "fc1_time",
             "soak", "x3_grad_debug", "gpu_diag", "stamps/read_r64", "stamps/read_v6")
PARTIAL_GROUPS = (("ensemble_bench", "4 32"), ("ensemble_bench", "4 32 128 7"), ("train_step_bench", "32 32 64"), ("train_step_bench", "32"),
                  ("x3_grad_debug", "2 4"))


def tool(name):
    return importlib.import_module(name)


def parse(name, argv):
    """What the tool makes of a command line: its PARSER, and for train_step_bench the checks of the values that follow it."""
    mod = tool(name)
    return vars(mod.options(argv.split()) if hasattr(mod, "options") else mod.PARSER.parse_args(argv.split()))


def child(script, *argv):
    return subprocess.run([sys.executable, os.path.join(TOOLS, script), *argv], capture_output=True, text=True, cwd=ROOT)


# ---------------------------------------------------------------- device_code_diff.py --opcodes

def test_opcode_differences_counts_per_opcode_and_skips_labels():
    diff = tool("device_code_diff").opcode_differences
    a = ("s_load_dword s0, s[0:1], 0x0", ".LBB_1:", "v_add_f64 v[0:1], v[0:1], v[2:3]", "s_nop 0", "s_endpgm")
    b = ("s_load_dword s0, s[0:1], 0x0", "v_add_f64 v[0:1], v[0:1], v[2:3]", ".LBB_2:", "v_add_f64 v[4:5], v[0:1], v[2:3]", "s_endpgm")
    assert diff(a, b) == [("s_nop", 1, 0), ("v_add_f64", 1, 2)]
    assert diff(a, a) == [] and diff((), b[:1]) == [("s_load_dword", 0, 1)]


# ---------------------------------------------------------------- timing helpers

def test_spread_is_median_min_max():
    assert _common.spread([3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert _common.spread([4, 1, 3, 2]) == (2.5, 1.0, 4.0)            # an even count: the mean of the middle two, like numpy.median
    assert _common.spread(iter([7.5])) == (7.5, 7.5, 7.5)
    assert all(type(v) is float for v in _common.spread([1, 2, 3]))  # json.dumps must not meet a numpy scalar


def test_alternate_warms_every_candidate_then_times_round_by_round(monkeypatch):
    log = []
    runs = {name: (lambda name=name: log.append(("call", name))) for name in ("b", "a", "c")}      # dictionary order, not sorted order
    ticks = iter(range(100))

    def fake_timed(fn, reps):
        fn()                                                          # which candidate this is shows up in the log
        kind, name = log.pop()
        log.append(("timed", name, reps))
        return float(next(ticks))

    monkeypatch.setattr(_common, "timed_us", fake_timed)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: log.append(("sync",)))
    times = _common.alternate(runs, rounds=2, reps=5, warmup=3)
    warm = [("call", n) for n in ("b", "a", "c") for _ in range(3)]
    assert log == warm + [("sync",)] + [("timed", n, 5) for _ in range(2) for n in ("b", "a", "c")]
    assert times == {"b": [0.0, 3.0], "a": [1.0, 4.0], "c": [2.0, 5.0]} and list(times) == ["b", "a", "c"]


def test_timed_us_puts_the_events_round_reps_calls(monkeypatch):
    log = []

    class Event:
        def __init__(self, enable_timing):
            assert enable_timing
            self.id = len([e for e in log if e[0] == "new"])
            log.append(("new", self.id))

        def record(self):
            log.append(("record", self.id))

        def synchronize(self):
            log.append(("wait", self.id))

        def elapsed_time(self, other):
            assert (self.id, other.id) == (0, 1)
            return 6.0                                                # milliseconds

    monkeypatch.setattr(torch.cuda, "Event", Event)
    assert _common.timed_us(lambda: log.append(("call",)), 4) == 1500.0
    assert log == [("new", 0), ("new", 1), ("record", 0)] + [("call",)] * 4 + [("record", 1), ("wait", 1)]


def test_constants_and_emit(capsys):
    assert (_common.HBM_ACHIEVABLE, _common.LLC_BYTES, _common.LAUNCH_US) == (6.3e12, 256 << 20, 1.5)
    _common.emit("x_bench", [{"a": 1}])
    assert capsys.readouterr().out == '{"x_bench": [{"a": 1}]}\n'


def test_each_helper_is_defined_once():
    """The copies this module replaced stay gone: no tool parses argv by hand, times with events of its own or restates a constant."""
    for path in glob.glob(os.path.join(TOOLS, "**", "*.py"), recursive=True):
        text = open(path).read()
        if os.path.basename(path) not in ("_common.py", "device_code_diff.py", "instr_r64.py"):      # the last two: stdlib only, not ported
            assert "import _common" in text, path
            assert not re.search(r"def _options|def _timed|HBM_ACHIEVABLE *=|LLC_BYTES *=|LAUNCH_US *=|sys\.argv\[|sys\.path\.insert\(0, ROOT", text), path
    for path in glob.glob(os.path.join(TOOLS, "*.sh")):
        assert not re.search(r"\|\| true|rm -rf", open(path).read()), path


# ---------------------------------------------------------------- command lines

NONE = [None]
TABLE = [          # (tool, argv as the docstrings, README.md, DESIGN.md and profiles/README.md write it, what the parent's parser made of it)
    ("ensemble_bench", "", dict(B=4, V=32, S=128, precision=["bf16", "bf16x3"], mode="dihedral", rounds=7, reps=10)),
    ("ensemble_bench", "2 8 64 --precision bf16 --mode flip --rounds 3 --reps 5",
     dict(B=2, V=8, S=64, precision=["bf16"], mode="flip", rounds=3, reps=5)),
    ("tiled_bench", "", dict(only=["tax", "kernels", "big"], precision=["bf16", "bf16x3"], tiles=[128, 256], scene=[1, 32, 512, 512],
                             big=[1, 32, 2048, 1536], big_tile=128, rounds=5, reps=3)),
    ("tiled_bench", "--only tax,kernels --precision bf16 --tiles 64 --scene 1,8,300,200 --big 1,8,1024,768 --big-tile 256 --rounds 3 --reps 2",
     dict(only=["tax", "kernels"], precision=["bf16"], tiles=[64], scene=[1, 8, 300, 200], big=[1, 8, 1024, 768], big_tile=256, rounds=3, reps=2)),
    ("shift_loss_bench", "", dict(B=32, sizes=[192, 384], border=3, rounds=7, reps=20)),
    ("shift_loss_bench", "32 --rounds 5 --reps 20", dict(B=32, sizes=[192, 384], border=3, rounds=5, reps=20)),
    ("shift_loss_bench", "8 --sizes 96 --border 2", dict(B=8, sizes=[96], border=2, rounds=7, reps=20)),
    ("train_step_bench", "", dict(B=32, V=32, S=64, steps=5, torch_adam=False, precision=NONE, shiftnet_precision=NONE, repeats=1,
                                  freeze=["none"], scale=3, loss=["shiftnet"])),
    ("train_step_bench", "32 32 64 10 --precision fp32,bf16x3,bf16 --repeats 3",
     dict(B=32, V=32, S=64, steps=10, precision=["fp32", "bf16x3", "bf16"], shiftnet_precision=NONE, repeats=3)),
    ("train_step_bench", "32 32 64 10 --precision bf16 --shiftnet-precision fp32,bf16 --repeats 3",
     dict(steps=10, precision=["bf16"], shiftnet_precision=["fp32", "bf16"], repeats=3)),
    ("train_step_bench", "32 32 64 10 --precision bf16 --freeze none,encoder,encoder+fuse,shiftnet --repeats 3",
     dict(steps=10, precision=["bf16"], freeze=["none", "encoder", "encoder+fuse", "shiftnet"], repeats=3)),
    ("train_step_bench", "32 32 64 5 --precision bf16 --scale 2", dict(steps=5, precision=["bf16"], scale=2, repeats=1)),
    ("train_step_bench", "32 32 64 10 --precision bf16 --loss shiftnet,shift --repeats 3", dict(loss=["shiftnet", "shift"], repeats=3)),
    ("train_step_bench", "32 32 64 4 --precision bf16 --shiftnet-precision bf16", dict(steps=4, shiftnet_precision=["bf16"])),
    ("train_step_bench", "8 4 32 2 --loss shift --scale 2 --torch-adam", dict(B=8, V=4, S=32, steps=2, loss=["shift"], scale=2, torch_adam=True)),
    ("loader_rate", "--threads 16", dict(sets=64, threads=16, json=None, no_prof=False, child=None, shape=None, batches=200, repeats=5, augment=None)),
    ("loader_rate", "--threads 16 --repeats 2 --no-prof --augment dihedral", dict(threads=16, repeats=2, no_prof=True, augment="dihedral")),
    ("kbench", "", dict(prec="bf16", B=32, V=32, S=128)),
    ("kbench", "bf16x3", dict(prec="bf16x3", B=32, V=32, S=128)),
    ("kbench", "bf16 32 32 512", dict(prec="bf16", B=32, V=32, S=512)),
    ("kbench", "fp32 16", dict(prec="fp32", B=16, V=32, S=128)),                          # [prec] [B] [V] [S]: each optional on its own
    ("train_prof", "", dict(precision="fp32")),
    ("train_prof", "bf16x3", dict(precision="bf16x3")),
    ("soak", "", dict(prec="bf16")),
    ("soak", "bf16x3", dict(prec="bf16x3")),
    ("x3_grad_debug", "", dict(B=2, V=4, S=16)),
    ("x3_grad_debug", "2 4 64", dict(B=2, V=4, S=64)),
    ("variant", "v6_abl1 conv3x3_v6.hip -DV6_ABL=1", dict(name="v6_abl1", source="conv3x3_v6.hip", defines=["V6_ABL=1"])),
    ("variant", "wgx_3 wgrad_x3.hip -DWGX_ABL=3 -DNDEBUG", dict(name="wgx_3", source="wgrad_x3.hip", defines=["WGX_ABL=3", "NDEBUG"])),
    ("variant", "copy stem.hip", dict(defines=[])),
    ("pmc_busy_summary", "kt.csv cc.csv", dict(kernel_trace_csv="kt.csv", counters_csv="cc.csv")),
    ("pmc_summary", "a b", dict(dirs=["a", "b"])),
]


@pytest.mark.parametrize("name,argv,want", TABLE, ids=[f"{t[0]} {t[1]}".strip() for t in TABLE])
def test_documented_command_lines_keep_their_meaning(name, argv, want):
    got = parse(name, argv)
    assert {k: got[k] for k in want} == want


@pytest.mark.parametrize("name,argv", [(n, "--bogus 1") for n in IMPORTED] + [("train_step_bench", "--precison bf16")] + list(PARTIAL_GROUPS)
                         + [("train_step_bench", "--precision fp16"), ("train_step_bench", "--freeze decoder"), ("train_step_bench", "--loss l2"),
                            ("train_step_bench", "32 32 32 5 --scale 3"), ("tiled_bench", "--rounds"), ("variant", "x nosuch.hip")])
def test_usage_errors_exit_2_with_the_usage(name, argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse(name, argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and err.startswith("usage: ") and "error: " in err


@pytest.mark.parametrize("name", IMPORTED)
def test_help_is_the_docstring(name, capsys):
    mod = tool(name)
    with pytest.raises(SystemExit) as e:
        mod.PARSER.parse_args(["--help"])
    out = capsys.readouterr().out
    assert e.value.code == 0
    for line in mod.__doc__.strip().splitlines():
        assert line.rstrip() in out


@pytest.mark.parametrize("script", SCRIPTS)
def test_script_style_tools_usage_and_help(script):
    """These parse their command line before the heavy imports, so a child costs little."""
    r = child(script, "--bogus")
    assert r.returncode == 2 and r.stderr.startswith("usage: ") and "Traceback" not in r.stderr
    r = child(script, "--help")
    doc = re.search(r'"""(.*?)"""', open(os.path.join(TOOLS, script)).read(), re.S).group(1)
    assert r.returncode == 0 and all(line.rstrip() in r.stdout for line in doc.strip().splitlines())


@pytest.mark.skipif(torch.cuda.is_available(), reason="there is a device: the tools would start measuring")
@pytest.mark.parametrize("name", ON_DEVICE)
def test_no_device_is_one_line_and_status_2(name):
    r = child(name + ".py")
    assert r.returncode == 2 and "Traceback" not in r.stderr
    assert r.stderr.strip().splitlines()[-1] == f"{os.path.basename(name)} needs a ROCm device: a time cannot be measured without one"
    assert r.stdout == ""


def test_gpu_diag_goes_on_past_a_comparison_only():
    diag = tool("gpu_diag")

    def fails(exc):
        def fn():
            raise exc
        return fn

    diag.guarded(fails(AssertionError("mismatch")))
    diag.guarded(fails(ValueError("shapes")))
    from hrnet_hip import HrnetHipError
    for exc in (RuntimeError("HIP error: an illegal memory access was encountered"), HrnetHipError("hrn_hrnet_forward failed"), KeyError("k")):
        with pytest.raises(type(exc)):
            diag.guarded(fails(exc))


# ---------------------------------------------------------------- shell scripts

def bash(script, tmp_path):
    return subprocess.run(["bash", "-c", script.replace("LOG", str(tmp_path / "log"))], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ, HRN_OUT=str(tmp_path / "out")))


def test_step_ends_the_script_at_a_time_limit_or_a_failure(tmp_path):
    r = bash("source tools/steps.sh; step 1 LOG sleep 5; echo after", tmp_path)
    assert r.returncode == 124 and "after" not in r.stdout
    r = bash("source tools/steps.sh; step 1 LOG false; echo after", tmp_path)
    assert r.returncode == 1 and "after" not in r.stdout
    r = bash("source tools/steps.sh; step 5 LOG sh -c 'echo oops >&2; exit 7'; echo after", tmp_path)
    assert r.returncode == 7 and "after" not in r.stdout and "oops" in r.stderr            # the end of the log is shown
    r = bash("source tools/steps.sh; step 1 LOG true; echo after", tmp_path)
    assert r.returncode == 0 and r.stdout == "after\n"
    r = bash("source tools/steps.sh; step 5 LOG echo out", tmp_path)
    assert r.returncode == 0 and r.stdout == "out\n"                                         # stdout stays the caller's


def test_gpu_scripts_run_every_gpu_program_through_step():
    for name in ("prof_all.sh", "ab.sh", "wgx_abl.sh"):
        text = open(os.path.join(TOOLS, name)).read()
        assert "steps.sh" in text
        for line in text.splitlines():
            line = re.sub(r"(^|\s)#.*", "", line)                                            # comments may name a program
            if re.search(r"\b(python3?|rocprofv3)\b", line):
                assert re.search(r"\bstep \d+ ", line) or re.search(r"tools/(variant|pmc_busy_summary)\.py", line), line


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(TOOLS, "**", "*.sh"), recursive=True)), ids=os.path.basename)
def test_shell_scripts_parse(path):
    r = subprocess.run(["bash", "-n", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
