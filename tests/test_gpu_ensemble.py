"""GPU (-m gpu): the flip / rotate self-ensemble on the device.  hrn_dihedral_expand and hrn_dihedral_mean are pure data movement plus
fp32 adds in a stated order and one multiply, so everything here is compared BIT FOR BIT (torch.equal) with the rule in
hrnet_hip/augment.py: the two kernels on every path (16-byte vectors, LDS tiles for the transposing codes, per element, ragged edge
tiles), HRNet.forward_ensemble end to end in every precision and at every scale, the `ensemble` attribute, and the ESA-normalised
validation score against the numpy oracle's shift_cPSNR."""
import copy

import numpy as np
import pytest
import torch

from hrnet_hip import augment
from oracle import hrnet_np as O
from oracle import synth, weights
import util

pytestmark = pytest.mark.gpu


def _rand(shape, seed):
    return util.dev(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))


# --------------------------------------------------------------------------- the two kernels
MEMBER_LISTS = [[t] for t in range(8)] + [list(range(4)), list(range(8))]


@pytest.mark.parametrize("side", [128, 64, 30, 5])
@pytest.mark.parametrize("codes", MEMBER_LISTS, ids=lambda c: "c" + "".join(map(str, c)))
def test_expand_equals_the_rule(side, codes):
    """128 / 64: whole 32 x 32 tiles; 30 and 5: the per-element path (W % 4 != 0).  N = 3 planes with leading axes (3,) and (1, 3)."""
    from hrnet_hip import binding
    x = _rand((3, side, side), 100 + side)
    got = binding.dihedral_expand(x, codes)
    assert tuple(got.shape) == (len(codes), 3, side, side)
    assert torch.equal(got, augment.expand(x, codes))
    assert torch.equal(torch.ops.hrnet_hip.dihedral_expand(x[None], codes), augment.expand(x[None], codes))


@pytest.mark.parametrize("side", [44, 100])
def test_expand_ragged_edge_tiles_on_the_vector_path(side):
    """W % 4 == 0 but not a multiple of 32: edge tiles of 12 and 4 columns and rows through the vector and LDS paths."""
    from hrnet_hip import binding
    x = _rand((2, side, side), side)
    for codes in (list(range(8)), [7, 2, 5], [6]):
        assert torch.equal(binding.dihedral_expand(x, codes), augment.expand(x, codes))


def test_expand_non_square_without_transposes():
    from hrnet_hip import binding
    for shape in ((3, 24, 40), (2, 40, 24), (2, 7, 9)):
        x = _rand(shape, 7)
        assert torch.equal(binding.dihedral_expand(x, [0, 1, 2, 3]), augment.expand(x, [0, 1, 2, 3]))
        assert torch.equal(binding.dihedral_expand(x, [3, 1]), augment.expand(x, [3, 1]))
        with pytest.raises(binding.HrnetHipError, match="transposes"):
            binding.dihedral_expand(x, [0, 4])
        y = _rand((4,) + shape, 8)
        assert torch.equal(binding.dihedral_mean(y, [2, 0, 3, 1]), augment.mean_inverse(y, [2, 0, 3, 1]))


def test_unaligned_pointers_take_the_per_element_path():
    """A contiguous view that starts 4 bytes into its allocation: W % 4 == 0, but no 16-byte alignment."""
    from hrnet_hip import binding
    codes = [5, 0, 3, 6]
    base = _rand((2 * 32 * 32 + 1,), 3)
    x = base[1:].view(2, 32, 32)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    assert torch.equal(binding.dihedral_expand(x, codes), augment.expand(x, codes))
    ybase = _rand((4 * 2 * 32 * 32 + 1,), 4)
    y = ybase[1:].view(4, 2, 32, 32)
    assert torch.equal(binding.dihedral_mean(y, codes), augment.mean_inverse(y, codes))


SUBSETS = [[0], [5], [6, 1], [3, 4, 0], [7, 2, 5, 1], [1, 0, 6, 3, 4], [2, 7, 4, 0, 5, 3], [6, 5, 4, 3, 2, 1, 0], list(range(8)),
           [4, 5, 6, 7], [0, 1, 2, 3]]


@pytest.mark.parametrize("side", [384, 96, 30])
@pytest.mark.parametrize("codes", SUBSETS, ids=lambda c: "c" + "".join(map(str, c)))
def test_mean_equals_the_rule(side, codes):
    """K = 1 .. 8 with arbitrary distinct codes, transposing and not, in arbitrary order: the sum is taken in list order."""
    from hrnet_hip import binding
    y = _rand((len(codes), 2, side, side), 1000 + side + len(codes))
    got = binding.dihedral_mean(y, codes)
    assert tuple(got.shape) == (2, side, side)
    assert torch.equal(got, augment.mean_inverse(y, codes))
    assert torch.equal(torch.ops.hrnet_hip.dihedral_mean(y[:, :, None], codes), augment.mean_inverse(y[:, :, None], codes))


@pytest.mark.parametrize("side", [44, 100])
def test_mean_ragged_edge_tiles_on_the_vector_path(side):
    """W % 4 == 0 but not a multiple of 32: edge tiles of 12 and 4 columns and rows, through the mirrored loads and, for the
    transposing members, through both LDS tile buffers; mixed lists put both kinds into one accumulator."""
    from hrnet_hip import binding
    for codes in (list(range(8)), [7, 2, 5, 1], [6], [5, 4], [4, 5, 6, 7], [3, 1, 2]):
        y = _rand((len(codes), 2, side, side), 2000 + side + len(codes))
        assert torch.equal(binding.dihedral_mean(y, codes), augment.mean_inverse(y, codes)), codes


@pytest.mark.parametrize("side", [96, 30])
def test_mean_order_is_the_lists(side):
    """Two orders of the same members (each with its own planes): both equal the rule bit for bit, and fp32 addition not being
    associative, they differ from each other somewhere - the kernel adds in the list's order, not in a fixed one."""
    from hrnet_hip import binding
    codes, perm = [0, 5, 2, 7, 1, 6], [4, 2, 0, 5, 3, 1]
    y = _rand((6, 2, side, side), 77)
    codes_p, y_p = [codes[i] for i in perm], y[perm].contiguous()
    a, b = binding.dihedral_mean(y, codes), binding.dihedral_mean(y_p, codes_p)
    assert torch.equal(a, augment.mean_inverse(y, codes)) and torch.equal(b, augment.mean_inverse(y_p, codes_p))
    assert not torch.equal(a, b) and torch.allclose(a, b, rtol=0, atol=1e-5)


def test_mean_of_expand_is_the_identity_up_to_rounding():
    from hrnet_hip import binding
    x = _rand((3, 64, 64), 5)
    codes = list(range(8))
    back = binding.dihedral_mean(binding.dihedral_expand(x, codes), codes)
    assert torch.equal(back, augment.mean_inverse(augment.expand(x, codes), codes)) and torch.allclose(back, x, rtol=1e-6, atol=0)


def test_opcheck():
    ops = torch.ops.hrnet_hip
    x = _rand((2, 3, 16, 16), 1)
    y = _rand((4, 2, 1, 24, 24), 2)
    for args in ((x, [0, 5, 6]), (x, [3])):
        torch.library.opcheck(ops.dihedral_expand.default, args, test_utils=("test_schema", "test_faketensor"))
    for args in ((y, [0, 1, 2, 3]), (y, [7, 5, 0, 2])):
        torch.library.opcheck(ops.dihedral_mean.default, args, test_utils=("test_schema", "test_faketensor"))


# --------------------------------------------------------------------------- HRNet.forward_ensemble
def _model(scale, precision, train=False):
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    st = weights.to_torch_state(weights.hrnet_state(1234))
    if scale != 3:
        rng = np.random.Generator(np.random.PCG64(1234 + 100 * scale))
        w = rng.standard_normal((64, 64, scale, scale)) * float(st["decode.deconv.0.weight"].std())
        st["decode.deconv.0.weight"] = torch.from_numpy(w.astype(np.float32))
    m = HRNet(cfg)
    m.load_state_dict(st)
    m.precision = precision
    m = m.cuda()
    return m.train() if train else m.eval()


def _plain_members(m, x, a, codes):
    """ONE plain forward on the member-major batch built with torch: (K, B, 1, SH, SW)."""
    packed, dt = m.packed_parameters()
    big = augment.expand(x, codes).reshape((-1,) + tuple(x.shape[1:])).contiguous()
    sr = torch.ops.hrnet_hip.hrnet_forward(packed, dt, m._num_layers, bool(m.fuse.alpha_residual), big, a.repeat(len(codes), 1), m._scale)
    return sr.view((len(codes), x.shape[0]) + tuple(sr.shape[1:]))


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_forward_ensemble_end_to_end(scale, prec):
    lrs, alphas, _ = synth.make_batch(60 + scale, 2, 4, 32, [4, 3])
    x, a = util.dev(lrs), util.dev(alphas)
    m = _model(scale, prec)
    for mode in ("dihedral", "flip"):
        codes = augment.ensemble_codes(mode)
        with torch.no_grad():
            want = augment.mean_inverse(_plain_members(m, x, a, codes), codes)
            got = m.forward_ensemble(x, a, mode)
            assert tuple(got.shape) == (2, 1, scale * 32, scale * 32) and not got.requires_grad
            assert torch.equal(got, want), (mode, float((got - want).abs().max()))
            assert torch.equal(m.forward_ensemble(x, a, mode, members_per_pass=1), want)
            assert torch.equal(m.forward_ensemble(x, a, mode, members_per_pass=3), want)
    # the attribute: graph-free forward = forward_ensemble; unset = the plain op, bit for bit
    with torch.no_grad():
        plain = m(x, a)
        packed, dt = m.packed_parameters()
        assert torch.equal(plain, torch.ops.hrnet_hip.hrnet_forward(packed, dt, m._num_layers, bool(m.fuse.alpha_residual), x, a, scale))
        m.ensemble = "flip"
        ens = m(x, a)
        assert torch.equal(ens, m.forward_ensemble(x, a, "flip")) and not torch.equal(ens, plain)
        m.ensemble = None
        assert torch.equal(m(x, a), plain)
    m.ensemble = "dihedral"                                     # .eval() without no_grad is graph-free too
    assert torch.equal(m(x, a), m.forward_ensemble(x, a, "dihedral"))
    # a real difference, not a relabelling: the ensemble is not the plain prediction, but close to it
    assert float((m(x, a) - plain).abs().max()) > 0 and torch.isfinite(m(x, a)).all()


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_training_branch_is_never_ensembled(scale, prec):
    """.train() with grad enabled, in every precision (bf16 is its own path: the bf16 inference kernels, then an fp32 recompute in
    backward) and at every scale: the switch changes neither the output nor the gradients, bit for bit."""
    lrs, alphas, _ = synth.make_batch(9, 2, 3, 32, 3)
    x, a = util.dev(lrs), util.dev(alphas)
    m = _model(scale, prec, train=True)
    base = m(x, a)
    assert base.requires_grad and tuple(base.shape) == (2, 1, scale * 32, scale * 32)
    (base ** 2).sum().backward()
    want = [p.grad.clone() for p in m.parameters()]
    m.zero_grad(set_to_none=True)
    m.ensemble = "dihedral"
    out = m(x, a)
    assert out.requires_grad and torch.equal(out, base)
    (out ** 2).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert all(torch.equal(p.grad, g) for p, g in zip(m.parameters(), want))
    with torch.no_grad():                                       # the same module, graph-free: ensembled
        ens = m(x, a)
        assert torch.equal(ens, m.forward_ensemble(x, a, "dihedral")) and not torch.equal(ens, base)


def test_config_key_sets_the_attribute():
    from DeepNetworks.HRNet import HRNet
    m = HRNet(dict(copy.deepcopy(weights.HRNET_CONFIG), ensemble="flip"))
    m.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
    m = m.cuda().eval()
    lrs, alphas, _ = synth.make_batch(12, 1, 3, 16, 3)
    x, a = util.dev(lrs), util.dev(alphas)
    with torch.no_grad():
        assert torch.equal(m(x, a), m.forward_ensemble(x, a, "flip"))
        assert torch.equal(m(x, a), util.hip_hrnet("fp32").forward_ensemble(x, a, "flip"))


# --------------------------------------------------------------------------- scores
def test_evaluate_and_sharded_val_score_on_device():
    """hrnet_hip.validate with names, a baseline table and ensemble="dihedral" against the numpy oracle's shift_cPSNR of the clipped
    ensembled SR, at the relative 1e-4 of test_sharded_val_score_single_rank_on_device; the training flag is restored."""
    from hrnet_hip import validate
    m = _model(3, "fp32", train=True)
    sets, table = [], {}
    for i in range(3):
        lrs, alphas, hrs = synth.make_batch(40 + i, 2, 4, 32, 4)
        maps = (np.random.Generator(np.random.PCG64(i)).random((2, 96, 96)) > 0.1).astype(np.float32)
        names = [f"imgset{2 * i + j:04d}" for j in range(2)]
        sets.append((util.dev(lrs), util.dev(alphas), util.dev(hrs), util.dev(maps), names))
        table.update({n: 45.0 + 2 * i + j for j, n in enumerate(names)})
    for ensemble in ("dihedral", None):
        ev = validate.evaluate(m, sets, baseline_cpsnrs=table, ensemble=ensemble, members_per_pass=4 if ensemble else None)
        got = validate.sharded_val_score(m, sets, baseline_cpsnrs=table, ensemble=ensemble)
        plain = validate.sharded_val_score(m, sets, ensemble=ensemble)
        assert m.training
        want = []
        m.eval()
        with torch.no_grad():
            for lrs, alphas, hrs, maps, _ in sets:
                sr = (m.forward_ensemble(lrs, alphas, ensemble) if ensemble else m(lrs, alphas))[:, 0].clamp(0, 1).cpu().numpy()
                want += [O.shift_cpsnr(sr[i], hrs.cpu().numpy()[i], maps.cpu().numpy()[i]) for i in range(sr.shape[0])]
        m.train()
        want = np.array(want, np.float64)
        names = [n for s in sets for n in s[4]]
        score = float(np.mean([table[n] / c for n, c in zip(names, want)]))
        print(f"ensemble={ensemble}: score {ev.score:.8f} want {score:.8f}; worst cPSNR rel err {np.abs(ev.cpsnr / want - 1).max():.2e}")
        assert ev.names == names and ev.cpsnr.dtype == np.float64 and ev.cpsnr.shape == (6,)
        assert np.all(np.abs(ev.cpsnr - want) <= 1e-4 * np.abs(want)), (ev.cpsnr, want)
        assert abs(ev.score - score) <= 1e-4 * abs(score), (ev.score, score)
        assert got == ev.score
        assert abs(plain + float(want.mean())) <= 1e-4 * float(want.mean())
    with pytest.raises(KeyError, match="imgset0003"):
        validate.evaluate(m, sets, baseline_cpsnrs={k: v for k, v in table.items() if k != "imgset0003"})
    assert m.training
