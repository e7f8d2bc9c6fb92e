"""CPU: the flip / rotate self-ensemble and the ESA-normalised validation score, as far as they live on the host - the rule in
hrnet_hip/augment.py (ensemble_codes, expand, mean_inverse), the refusals of hrn_dihedral_expand / hrn_dihedral_mean (nothing is
launched), the fake kernels of the two dispatcher ops, and hrnet_hip.validate.evaluate / sharded_val_score on CPU stand-ins."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from hrnet_hip import augment
from util import Toy, _esa_table, _free_port, _score, _sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- the rule
def test_ensemble_codes():
    assert augment.ensemble_codes("flip") == [0, 1, 2, 3]
    assert augment.ensemble_codes("dihedral") == list(range(8))
    assert augment.ensemble_codes(True) == list(range(8))
    for bad in (None, False, "none", "rot90", 4):
        with pytest.raises(ValueError):
            augment.ensemble_codes(bad)
    for bad in ([], list(range(8)) + [0], [0, 0], [8], [1, 2.5]):
        with pytest.raises(ValueError):
            augment.check_codes(bad)


def _network():
    """A deliberately NON-equivariant x3 "network" in float64 on (..., n, n): a fixed random 3x3 convolution (zero padding), then a
    Kronecker product with a fixed, asymmetric 3x3 pattern."""
    rng = np.random.Generator(np.random.PCG64(11))
    taps = rng.standard_normal((3, 3))
    pattern = rng.standard_normal((3, 3))

    def f(x):
        n = x.shape[-1]
        p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(1, 1), (1, 1)])
        y = sum(taps[a, b] * p[..., a:a + n, b:b + n] for a in range(3) for b in range(3))
        return (y[..., :, None, :, None] * pattern[:, None, :]).reshape(x.shape[:-2] + (3 * n, 3 * n))
    return f


@pytest.mark.parametrize("mode", ["flip", "dihedral"])
def test_ensemble_is_equivariant(mode):
    """E(x) = mean_inverse(f(expand(x))) commutes with every transform of the mode, E(apply(x, t)) == apply(E(x), t), although f does
    not: averaging over the group is what buys that.  Bound 1e-12 (float64; the sums differ only in their order).  Putting `code`
    where `inverse(code)` belongs breaks it by O(1) for every t but the identity and the half turn, so the bound discriminates."""
    f = _network()
    codes = augment.ensemble_codes(mode)
    x = np.random.Generator(np.random.PCG64(5)).standard_normal((2, 12, 12))

    def E(z):
        return augment.mean_inverse(f(augment.expand(z, codes)), codes)

    def E_wrong(z):
        y = f(augment.expand(z, codes))
        return sum(augment.apply(y[k], c) for k, c in enumerate(codes)) / len(codes)

    assert E(x).shape == (2, 36, 36) and E(x).dtype == np.float64
    for t in codes:
        err = float(np.abs(E(augment.apply(x, t)) - augment.apply(E(x), t)).max())
        alone = float(np.abs(f(augment.apply(x, t)) - augment.apply(f(x), t)).max())
        wrong = float(np.abs(E_wrong(augment.apply(x, t)) - augment.apply(E_wrong(x), t)).max())
        print(f"{mode} t={t}: ensemble {err:.2e}, f alone {alone:.2e}, wrong inverse {wrong:.2e}")
        assert err <= 1e-12, (t, err)
        if t:
            assert alone > 1, (t, alone)                       # f itself is not equivariant: the test cannot pass vacuously
        if mode == "dihedral" and t in (1, 2, 4, 5, 6, 7):
            assert wrong > 1, (t, wrong)


def test_expand_and_mean_inverse_numpy_and_torch_agree():
    """Same bits from numpy and torch in fp32, the stated summation order, K = 1 included; a wrong member count is refused."""
    rng = np.random.Generator(np.random.PCG64(2))
    for codes in ([0], [6], [3, 5, 0], list(range(8))):
        x = rng.standard_normal((3, 10, 10)).astype(np.float32)
        en, et = augment.expand(x, codes), augment.expand(torch.from_numpy(x), codes)
        assert en.shape == (len(codes), 3, 10, 10) and np.array_equal(en, et.numpy())
        for k, c in enumerate(codes):
            assert np.array_equal(en[k], augment.apply(x, c))
        y = rng.standard_normal((len(codes), 3, 10, 10)).astype(np.float32)
        mn, mt = augment.mean_inverse(y, codes), augment.mean_inverse(torch.from_numpy(y), codes)
        assert mn.dtype == np.float32 and mt.dtype == torch.float32 and np.array_equal(mn, mt.numpy())
        total = augment.apply(y[0], augment.inverse(codes[0])).copy()
        for k in range(1, len(codes)):
            total = total + augment.apply(y[k], augment.inverse(codes[k]))
        assert np.array_equal(mn, total * np.float32(1.0 / len(codes)))
        assert np.allclose(augment.mean_inverse(en, codes), x, rtol=1e-6, atol=0)      # the members of x itself average back to x
    with pytest.raises(ValueError):
        augment.mean_inverse(np.zeros((2, 4, 4), np.float32), [0, 1, 2])


# --------------------------------------------------------------------------- the C ABI's refusals
@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


@pytest.mark.parametrize("fn", ["hrn_dihedral_expand", "hrn_dihedral_mean"])
def test_refusals_before_any_launch(lib, fn):
    """Every refusal returns -2 with a message that names the fault.  Nothing is launched: the pointers below are host memory."""
    call = getattr(lib, fn)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def run(codes, H=4, W=4, x=p, out=p, K=None, null_codes=False):
        arr = (ctypes.c_int32 * max(1, len(codes)))(*codes)
        return call(x, 1, H, W, None if null_codes else arr, len(codes) if K is None else K, out, None), lib.hrn_last_error()

    for codes, kw, word in (([], {}, b"K must be in 1..8 (got 0)"),
                            (list(range(8)) + [0], {}, b"K must be in 1..8 (got 9)"),
                            ([0, 8], {}, b"bad code 8 at position 1"),
                            ([0, -1], {}, b"bad code -1"),
                            ([0, 3, 3], {}, b"duplicate code 3 at position 2"),
                            ([0, 1, 4], {"H": 4, "W": 8}, b"code 4 transposes"),
                            ([0], {"x": None}, b"null"),
                            ([0], {"out": None}, b"null"),
                            ([0], {"null_codes": True}, b"null"),
                            ([0], {"H": 0}, b"bad shape")):
        rc, msg = run(codes, **kw)
        assert rc == -2 and fn.encode() in msg and word in msg, (codes, kw, rc, msg)


def test_python_binding_refuses_bad_member_lists():
    from hrnet_hip import binding
    x = torch.zeros(2, 4, 4)
    for bad in ([], [0, 0], [9]):
        with pytest.raises(ValueError):
            binding.dihedral_expand(x, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        binding.dihedral_expand(x, [0, 1])                          # a host tensor: no quiet fall-back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        binding.dihedral_mean(torch.zeros(2, 2, 4, 4), [0, 1])


def test_fake_kernels_infer_shapes():
    from hrnet_hip import binding  # noqa: F401  (registers the ops)
    ops = torch.ops.hrnet_hip
    x = torch.empty((5, 16, 16), device="meta")
    e = ops.dihedral_expand(x, [0, 3, 6])
    assert tuple(e.shape) == (3, 5, 16, 16) and e.dtype == torch.float32 and e.device.type == "meta"
    m = ops.dihedral_mean(e, [0, 3, 6])
    assert tuple(m.shape) == (5, 16, 16) and m.dtype == torch.float32 and m.device.type == "meta"
    lrs = torch.empty((2, 4, 8, 8), device="meta")
    assert tuple(ops.dihedral_expand(lrs, list(range(8))).shape) == (8, 2, 4, 8, 8)
    assert tuple(ops.dihedral_mean(torch.empty((4, 2, 1, 24, 24), device="meta"), [0, 1, 2, 3]).shape) == (2, 1, 24, 24)


def test_hrnet_ensemble_attribute():
    from oracle import weights
    from DeepNetworks.HRNet import HRNet
    m = HRNet(weights.HRNET_CONFIG)
    assert m.ensemble is None
    assert HRNet(dict(weights.HRNET_CONFIG, ensemble="flip")).ensemble == "flip"
    x, a = torch.zeros(1, 2, 8, 8), torch.ones(1, 2)
    with pytest.raises(ValueError):
        m.forward_ensemble(x, a, "rot90")
    for bad in (0, 9, 2.0):
        with pytest.raises(ValueError):
            m.forward_ensemble(x, a, "dihedral", members_per_pass=bad)
    with pytest.raises(ValueError):
        m.forward_ensemble(x, a, "flip", members_per_pass=5)


# --------------------------------------------------------------------------- evaluate / sharded_val_score on CPU stand-ins
def test_evaluate_esa_score_is_the_references_formula():
    from hrnet_hip import validate
    sets = _sets(5, batch=2)
    table = _esa_table(sets)
    model = Toy().train()
    ev = validate.evaluate(model, sets, baseline_cpsnrs=table, score_fn=_score)
    assert model.training
    names = [n for s in sets for n in s[4]]
    cps = np.array([float(_score(model(l, a)[:, 0], h, m)[i]) for l, a, h, m, ns in sets for i in range(len(ns))])
    # train.py:209-217: val_score += ESA / shift_cPSNR per imageset, then / len(dataset)
    want = float(np.mean([table[n] / c for n, c in zip(names, cps)]))
    assert ev.names == names and ev.cpsnr.dtype == np.float64 and np.array_equal(ev.cpsnr, cps)
    assert abs(ev.score - want) <= 1e-12 * abs(want), (ev.score, want)
    assert validate.sharded_val_score(model, sets, score_fn=_score, baseline_cpsnrs=table) == ev.score
    # without a table: -mean(cPSNR), with or without names
    plain = validate.evaluate(model, sets, score_fn=_score)
    assert abs(plain.score + float(np.mean(cps))) <= 1e-12 * float(np.mean(cps)) and plain.names == names
    four = [s[:4] for s in sets]
    assert validate.evaluate(model, four, score_fn=_score).score == plain.score
    assert validate.evaluate(model, four, score_fn=_score).names == []


def test_four_tuple_path_is_unchanged():
    """sharded_val_score with both new arguments left alone: the number it returned before they existed, from 4- and 5-tuples."""
    from hrnet_hip import validate
    sets = _sets(4)
    model = Toy().eval()
    total = None
    for l, a, h, m, _ in sets:                                     # the loop as it stood
        sc = _score(model(l, a)[:, 0], h, m).double().sum()
        total = sc if total is None else total + sc
    want = -float(total / len(sets))
    assert validate.sharded_val_score(model, [s[:4] for s in sets], score_fn=_score) == want
    assert validate.sharded_val_score(model, sets, score_fn=_score) == want
    assert validate.sharded_val_score(model, sets, 3, _score, None) == want
    assert not model.training


def test_errors():
    from hrnet_hip import validate
    sets = _sets(3)
    table = _esa_table(sets)
    model = Toy().train()
    with pytest.raises(ValueError, match="names"):
        validate.sharded_val_score(model, [s[:4] for s in sets], score_fn=_score, baseline_cpsnrs=table)
    with pytest.raises(ValueError, match="names"):
        validate.evaluate(model, [s[:4] for s in sets], baseline_cpsnrs=table, score_fn=_score)
    missing = sets[1][4][0]
    del table[missing]
    with pytest.raises(KeyError, match=missing):
        validate.sharded_val_score(model, sets, score_fn=_score, baseline_cpsnrs=table)
    with pytest.raises(KeyError, match=missing):
        validate.evaluate(model, sets, baseline_cpsnrs=table, score_fn=_score)
    assert model.training                                          # restored after a failure too
    with pytest.raises(ValueError):
        validate.evaluate(model, [], score_fn=_score)
    with pytest.raises(ValueError):
        validate.evaluate(model, sets, ensemble="rot90", score_fn=_score)
    with pytest.raises(TypeError, match="forward_ensemble"):
        validate.evaluate(torch.nn.Identity(), sets, ensemble="flip", score_fn=_score)


def test_evaluate_with_ensemble_calls_forward_ensemble():
    from hrnet_hip import validate
    sets = _sets(3)
    model = Toy().eval()
    ev = validate.evaluate(model, sets, ensemble="flip", score_fn=_score, members_per_pass=2)
    assert model.seen == ("flip", 2)
    cps = np.array([float(_score(model.forward_ensemble(l, a, "flip")[:, 0], h, m)[0]) for l, a, h, m, _ in sets])
    assert np.array_equal(ev.cpsnr, cps) and ev.score == -float(torch.from_numpy(cps).sum() / 3)
    assert validate.sharded_val_score(model, sets, score_fn=_score, ensemble="flip") == ev.score
    assert validate.evaluate(model, sets, score_fn=_score).score != ev.score


VAL_WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, os.path.join(%r, "highres-net_amd"))
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    import numpy as np, torch
    from hrnet_hip import dist as hdist, validate
    import util as T
    rank, local_rank, ws = hdist.init(backend="gloo")
    sets = T._sets(7)                                       # 7 imagesets dealt round-robin: rank 0 scores 4, rank 1 scores 3
    table = T._esa_table(sets)
    model = T.Toy().train()
    mine = [sets[i] for i in validate.shard_indices(len(sets), rank, ws)]
    assert len(mine) == (4, 3)[rank]
    got = validate.sharded_val_score(model, mine, score_fn=T._score, baseline_cpsnrs=table)
    assert model.training
    want = validate.evaluate(model, sets, baseline_cpsnrs=table, score_fn=T._score).score          # the single-process score
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    got_e = validate.sharded_val_score(model, mine, score_fn=T._score, baseline_cpsnrs=table, ensemble="dihedral")
    want_e = validate.evaluate(model, sets, baseline_cpsnrs=table, ensemble="dihedral", score_fn=T._score).score
    assert abs(got_e - want_e) <= 1e-12 * abs(want_e) and got_e != got, (got_e, want_e, got)
    hdist.barrier()
    print("esa val score ok", rank, got)
    hdist.finalize()
""") % (ROOT, ROOT, ROOT)


def test_two_rank_esa_validation(tmp_path):
    """The ESA-normalised score sharded over two gloo ranks with ragged shards (4 and 3 imagesets): both ranks return the
    single-process score, plain and self-ensembled."""
    script = tmp_path / "esa_val_worker.py"
    script.write_text(VAL_WORKER)
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=180) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-2000:]
    for rank in range(2):
        assert f"esa val score ok {rank}" in outs[rank][0]
