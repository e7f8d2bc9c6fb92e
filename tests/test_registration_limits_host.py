"""CPU: a size query of the tiled registration paths and its entry point state the same limits (csrc/api.hip: the query is the entry
point's own checks run silently).  For every problem of a sweep the query answers 0 exactly where the entry point refuses the problem
for a reason other than a null pointer, and a query that answers 0 leaves hrn_last_error as it was.

Nothing is launched and no GPU is needed: every call of an entry point passes a NULL output (`shifts` / `field`), so a problem inside
every limit stops at "null argument", which the entry points check before the workspace and before any launch.  The other pointers
are a dummy that is never dereferenced.  The levels and radii are valid ones; the pyramid's radius is 1, which the size query - it has
no radius - assumes, so the reach rule (radius * 2**octaves <= 128) cannot separate the two.

The sweep: 3072 (B, V, H, W, P) problems for the scene search, times the five blocks for the local search (15360), times the six octave
counts for the pyramid (18432, of which the entry point refuses 17704)."""
import ctypes
import itertools
import os

import pytest

BS, VS = (0, 1, 2, 1 << 15), (0, 1, 3)
SIDES = (15, 16, 31, 63, 64, 130, 16384, 16385)
POINTS = (2, 3, 9, 10)
BLOCKS = (0, 64, 96, 4096, 4160)
OCTAVES = (-1, 0, 1, 2, 6, 7)
PROBLEMS = list(itertools.product(BS, VS, SIDES, SIDES, POINTS))
HUGE = 1 << 62                                  # workspace_bytes: never the reason for a refusal
NULL, P_ = ctypes.c_void_p(0), ctypes.c_void_p(64)    # P_ is never dereferenced: every call fails a check first


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def _sweep(lib, who, query, entry, problems):
    """-> (accepted, refused) over `problems`; query(*problem) is the size, entry(*problem) the return code of the call without an output"""
    accepted = refused = 0
    for problem in problems:
        rc = entry(*problem)
        err = lib.hrn_last_error()
        assert rc == -2 and err.startswith(who + b": "), (who, problem, rc, err)
        inside = err == who + b": null argument"
        size = query(*problem)
        assert (size != 0) == inside, (who, problem, size, err)
        assert lib.hrn_last_error() == err, (who, problem, "the size query touched hrn_last_error")
        accepted, refused = accepted + inside, refused + (not inside)
    assert accepted and refused, (who, accepted, refused)
    return accepted, refused


def test_scene_size_query_and_entry_point_agree(lib):
    def entry(B, V, H, W, P):
        return lib.hrn_mncc_search_scene_from(P_, P_, P_, P_, P_, B, V, H, W, P, 4, 1.0, NULL, P_, P_, HUGE, NULL)

    n = _sweep(lib, b"hrn_mncc_search_scene_from", lib.hrn_mncc_scene_workspace_bytes, entry, PROBLEMS)
    print(f"scene: {n[0]} accepted, {n[1]} refused of {len(PROBLEMS)}")
    assert sum(n) == 3072


def test_local_size_query_and_entry_point_agree(lib):
    def entry(B, V, H, W, P, block):
        return lib.hrn_mncc_search_local(P_, P_, P_, P_, P_, B, V, H, W, P, 4, 0.5, block, 0.25, NULL, P_, P_, P_, HUGE, NULL)

    problems = [p + (block,) for p in PROBLEMS for block in BLOCKS]
    n = _sweep(lib, b"hrn_mncc_search_local", lib.hrn_mncc_local_workspace_bytes, entry, problems)
    print(f"local: {n[0]} accepted, {n[1]} refused of {len(problems)}")
    assert sum(n) == 15360


def test_pyramid_size_query_and_entry_point_agree(lib):
    def entry(B, V, H, W, P, octaves):
        return lib.hrn_mncc_search_pyramid(P_, P_, P_, P_, B, V, H, W, P, octaves, 6, 1.0, 3, 1.0, NULL, P_, P_, HUGE, NULL)

    problems = [p + (octaves,) for p in PROBLEMS for octaves in OCTAVES]
    n = _sweep(lib, b"hrn_mncc_search_pyramid", lib.hrn_mncc_pyramid_workspace_bytes, entry, problems)
    print(f"pyramid: {n[0]} accepted, {n[1]} refused of {len(problems)}")
    assert sum(n) == 18432
