"""What every tool under tools/ shares: the import path, the command line, the refusal to run without a device, the timing
helpers and the JSON last line.  Tools run as `python tools/x.py`, so `import _common` resolves."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "highres-net_amd")]

HBM_ACHIEVABLE = 6.3e12                      # bytes / s: a float4 copy on the MI355X (79 % of the 8 TB/s peak)
LLC_BYTES = 256 << 20                        # the last-level cache: a working set of twice this comes from HBM
LAUNCH_US = 1.5                              # a dependent kernel boundary on one stream, microseconds


def tests_on_path():
    """For the two tools that compare against the suite's own helpers (tests/util.py, tests/test_gpu_backward.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))


class _Parser(argparse.ArgumentParser):
    group = None

    def parse_args(self, args=None, namespace=None):
        o = super().parse_args(args, namespace)
        if self.group:
            names, defaults = self.group[0].split(), self.group[1]
            if len(o.group) not in (0, len(names)):
                self.error(f"[{self.group[0]}] takes {len(names)} values or none (got {len(o.group)})")
            vars(o).update(zip(names, o.group or defaults))
        return o


def parser(doc, group=None, positional={}, **flags):
    """An argparse parser whose help is the tool's docstring; an unknown flag or a partly given group is a usage error (status 2).
    group=("B V S", (4, 32, 128)) is the positional group [B V S] of integers: all of it or none of it.  positional={name: default}
    are positionals that may each be left out.  Every other keyword is a flag with that default (big_tile=128 is --big-tile).  The
    default gives the type: False a switch, a list a comma-separated list of what it holds (strings for [None]), None a string."""
    ap = _Parser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter, allow_abbrev=False)
    if group:
        ap.group = group
        ap.add_argument("group", nargs="*", type=int, metavar=group[0])
    for name, default in positional.items():
        ap.add_argument(name, nargs="?", default=default, type=type(default))
    for name, default in flags.items():
        flag = "--" + name.replace("_", "-")
        if default is False:
            ap.add_argument(flag, action="store_true")
        elif isinstance(default, list):
            kind = str if default[0] is None else type(default[0])
            ap.add_argument(flag, default=default, type=lambda text, kind=kind: [kind(v) for v in text.split(",")])
        else:
            ap.add_argument(flag, default=default, type=str if default is None else type(default))
    return ap


def require_gpu(tool):
    """Called before any model or tensor is built: one line and status 2 where there is no device, instead of a traceback."""
    import torch
    if not torch.cuda.is_available():
        print(f"{tool} needs a ROCm device: a time cannot be measured without one", file=sys.stderr)
        raise SystemExit(2)


def timed_us(fn, reps):
    """Microseconds per call: device events around `reps` calls enqueued back to back."""
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def alternate(runs, rounds, reps, warmup):
    """{name: fn} -> {name: [microseconds per call, one per round]}: `warmup` calls of every candidate (every shape of the timed
    window, workspace growth included), then the candidates timed round by round in dictionary order."""
    import torch
    for fn in runs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(timed_us(fn, reps))
    return times


def spread(values):
    """(median, min, max) of the per-round values: the figure and its run-to-run spread."""
    values = [float(v) for v in values]
    return statistics.median(values), min(values), max(values)


def emit(key, results):
    """The JSON last line of a tool: {key: results}."""
    print(json.dumps({key: results}))
