"""Flip / rotate augmentation, the part that needs no GPU: the rule itself (hrnet_hip/augment.py), the host collate
(hrn_io_collate_a) against that rule applied to the un-augmented result - bit for bit, the transform moves values and computes
none -, the numpy RNG contract of DataLoader with augmentation off (nothing changes) and on (one extra randint per imageset,
after the views and the corner), and the modes."""
import os

import numpy as np
import pytest
import torch

import DataLoader as DL
import utils as U
from hrnet_hip import augment, io_binding
from scale_ref import restated_read, write_scaled_imageset

N_THREADS = 4
VIEWS = (4, 9, 6, 5)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """{ratio: four imagesets with HR / SM stored at that ratio}, and under "test" two x3 imagesets without HR."""
    root = tmp_path_factory.mktemp("augment")
    out = {}
    for ratio in (2, 3, 4):
        r = str(root / f"x{ratio}")
        os.makedirs(r)
        out[ratio] = [write_scaled_imageset(r, f"imgset{i:04d}", n, ratio, seed=20 + i) for i, n in enumerate(VIEWS)]
    r = str(root / "test")
    os.makedirs(r)
    out["test"] = [write_scaled_imageset(r, f"imgset{9000 + i}", n, 3, with_hr=False, seed=5 + i) for i, n in enumerate((4, 6))]
    return out


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ------------------------------------------------------------------ 1. the helper
def test_apply_gives_eight_distinct_results_and_inverse_undoes_them():
    x = np.arange(7 * 7, dtype=np.int64).reshape(7, 7) ** 2 % 41 + np.arange(7)[:, None] * 100        # no symmetry of the square
    results = [augment.apply(x, c) for c in range(8)]
    assert len({r.tobytes() for r in map(np.ascontiguousarray, results)}) == 8
    assert np.array_equal(results[0], x)
    stack = np.stack([x, x.T + 1, x[::-1] + 2])                       # leading axes are kept
    for c in range(8):
        assert np.array_equal(augment.apply(augment.apply(x, c), augment.inverse(c)), x)
        assert np.array_equal(augment.apply(stack, c), np.stack([augment.apply(p, c) for p in stack]))
        t = augment.apply(torch.from_numpy(x), c)
        assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), results[c])
        assert torch.equal(augment.apply(t, augment.inverse(c)), torch.from_numpy(x))
        # the index map of the header: out[i][j] = in[(j', i') if t & 4 else (i', j')]
        n = 7
        i, j = np.mgrid[0:n, 0:n]
        ip, jp = (n - 1 - i if c & 2 else i), (n - 1 - j if c & 1 else j)
        assert np.array_equal(results[c], x[jp, ip] if c & 4 else x[ip, jp])
    assert [augment.inverse(c) for c in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]
    for bad in (-1, 8, 2.5):
        with pytest.raises(ValueError):
            augment.apply(x, bad)
        with pytest.raises(ValueError):
            augment.inverse(bad)
    with pytest.raises(ValueError):
        augment.apply(np.zeros((3, 4)), 4)                            # a transpose needs a square
    assert augment.apply(np.zeros((3, 4)), 3).shape == (3, 4)


def test_table_of_codes_against_torch_flip_and_rot90():
    x = torch.arange(5 * 5 * 2).reshape(2, 5, 5) ** 2 % 37
    want = {0: x,
            1: torch.flip(x, (-1,)),
            2: torch.flip(x, (-2,)),
            3: torch.rot90(x, 2, (-2, -1)),
            4: x.transpose(-1, -2),
            5: torch.rot90(x, -1, (-2, -1)),                          # a quarter turn clockwise
            6: torch.rot90(x, 1, (-2, -1)),                           # and counter-clockwise
            7: torch.flip(x.transpose(-1, -2), (-2, -1))}
    for c, w in want.items():
        assert torch.equal(augment.apply(x, c), w), c
        assert np.array_equal(augment.apply(x.numpy(), c), w.numpy()), c


# ------------------------------------------------------------------ 2. host collate
def _collate(dirs, scale, min_L, patch, corners, codes, with_hr=True, out=None):
    views = [sorted(os.path.join(d, f) for f in os.listdir(d) if f.startswith("LR")) for d in dirs]
    return io_binding.collate(views, [os.path.join(d, "HR.png") for d in dirs] if with_hr else None, [os.path.join(d, "SM.png") for d in dirs],
                              min_L=min_L, lr_size=128, patch=patch, corners=corners, scale=scale, n_threads=N_THREADS, codes=codes, out=out)


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("patch", [64, 30, 0])                        # S a multiple of 4, S not, whole frames
def test_host_collate_equals_apply_of_the_plain_result(sets, scale, patch):
    dirs = sets[scale]
    min_L = 6                                                         # imageset 0 has 4 views: two padding slots
    hi = 128 - patch                                                  # the last corner that fits
    corner_sets = [[(5, 8), (17, 21), (hi - 24, 2), (hi - 1, 3)], [(0, 0), (1, 1), (2, hi), (hi, hi - 1)]] if patch else [None]
    if patch:
        assert {c % 4 for cs in corner_sets for _, c in cs} == {0, 1, 2, 3}        # all four column alignments
    for corners in corner_sets:
        plain = _collate(dirs, scale, min_L, patch, corners, None)
        assert plain["alphas"][0].tolist() == [1, 1, 1, 1, 0, 0] and not plain["lrs"][0, 4:].any()
        for base in range(0, 8, 4):                                   # codes 0..3, then 4..7: every code, each on a different imageset
            for rot in range(4):
                codes = [(base + (b + rot) % 4) for b in range(4)]
                got = _collate(dirs, scale, min_L, patch, corners, codes)
                assert np.array_equal(got["alphas"], plain["alphas"])
                for b, c in enumerate(codes):
                    for key in ("lrs", "hrs", "maps"):
                        assert np.array_equal(got[key][b], augment.apply(plain[key][b], c)), (key, b, c)
        zeros = _collate(dirs, scale, min_L, patch, corners, [0, 0, 0, 0])
        assert all(np.array_equal(zeros[k], plain[k]) for k in plain)


def test_host_collate_without_hr(sets):
    dirs = sets["test"]
    plain = _collate(dirs, 3, 5, 64, [(3, 9), (50, 61)], None, with_hr=False)
    assert plain["hrs"] is None
    for codes in ([5, 2], [7, 4], [1, 6], [3, 0]):
        got = _collate(dirs, 3, 5, 64, [(3, 9), (50, 61)], codes, with_hr=False)
        assert got["hrs"] is None and np.array_equal(got["alphas"], plain["alphas"])
        for b, c in enumerate(codes):
            assert np.array_equal(got["lrs"][b], augment.apply(plain["lrs"][b], c))
            assert np.array_equal(got["maps"][b], augment.apply(plain["maps"][b], c))


@pytest.mark.parametrize("bad", [-1, 8])
def test_host_collate_refuses_a_bad_code_and_touches_nothing(sets, bad):
    B, min_L, S = 4, 6, 64
    mk = lambda *shape: np.full(shape, 7.0, np.float32)
    out = dict(lrs=mk(B, min_L, S, S), alphas=mk(B, min_L), hrs=mk(B, 3 * S, 3 * S), maps=mk(B, 3 * S, 3 * S))
    with pytest.raises(io_binding.HrnetIoError, match=r"\(-2\)"):
        _collate(sets[3], 3, min_L, S, [(1, 2)] * 4, [0, 3, bad, 1], out=out)
    assert all((a == 7.0).all() for a in out.values())
    with pytest.raises(ValueError):
        _collate(sets[3], 3, min_L, S, [(1, 2)] * 4, [0, 3, 1])      # one code per imageset


def test_old_entry_points_are_the_new_one_without_codes(sets):
    """hrn_io_collate_s and hrn_io_collate still exist and give what hrn_io_collate_a(NULL) gives."""
    import ctypes as c
    lib = io_binding.load_library()
    d = sets[3][1]
    views = sorted(os.path.join(d, f) for f in os.listdir(d) if f.startswith("LR"))[:3]
    want = io_binding.collate([views], [os.path.join(d, "HR.png")], [os.path.join(d, "SM.png")], min_L=3, lr_size=128, patch=32, corners=[(7, 9)])
    for name, extra in (("hrn_io_collate_s", (3,)), ("hrn_io_collate", ())):
        got = dict(lrs=np.empty((1, 3, 32, 32), np.float32), alphas=np.empty((1, 3), np.float32), hrs=np.empty((1, 96, 96), np.float32),
                   maps=np.empty((1, 96, 96), np.float32))
        p = lambda a: a.ctypes.data_as(c.c_void_p)
        rc = getattr(lib, name)(1, io_binding._strs(views), (c.c_int * 1)(3), io_binding._strs([os.path.join(d, "HR.png")]),
                                io_binding._strs([os.path.join(d, "SM.png")]), 3, 128, 32, *extra, (c.c_int * 1)(7), (c.c_int * 1)(9),
                                p(got["lrs"]), p(got["alphas"]), p(got["hrs"]), p(got["maps"]), 2)
        assert rc == 0 and all(np.array_equal(got[k], want[k]) for k in got), name


# ------------------------------------------------------------------ 3. RNG contract, augmentation off
@pytest.mark.parametrize("create_patches,top_k,seed", [(True, 3, None), (True, -1, 5), (False, 3, None)])
def test_augmentation_off_changes_nothing(sets, create_patches, top_k, seed):
    dirs = sets[3]
    cfg = {"create_patches": create_patches, "patch_size": 64}
    old_style = DL.ImagesetDataset(dirs, cfg, seed, top_k, 50.0)                        # the constructor call of before this argument
    variants = [old_style, DL.ImagesetDataset(dirs, cfg, seed=seed, top_k=top_k, beta=50.0, augment=None),
                DL.ImagesetDataset(dirs, dict(cfg, augment=None), seed=seed, top_k=top_k, beta=50.0),
                DL.ImagesetDataset(dirs, dict(cfg, augment="dihedral"), seed=seed, top_k=top_k, beta=50.0, augment=False),
                DL.ImagesetDataset(dirs, cfg, seed=seed, top_k=top_k, beta=50.0, augment="none")]
    results = []
    for ds in variants:
        assert ds.augment is None
        np.random.seed(31)
        batch = ds.load_batch([2, 0, 3], 6, n_threads=N_THREADS)
        item = ds[1]
        plan = DL.ImagesetIndex(ds).plan([2, 0, 3], 6)
        assert ds.last_augment is None
        results.append((batch, item, plan, np.random.get_state()))
    # what the sequence of draws must be, restated: per imageset one choice (top_k > 0) and two randint (patches), nothing else
    np.random.seed(31)
    for _ in range(2):                                                # load_batch, then (after the item) the plan
        for i in ([2, 0, 3, 1] if _ == 0 else [2, 0, 3]):
            restated_read(dirs[i], create_patches, 64, seed, top_k, 50.0, 3, io_binding.png_read)
    want_state = np.random.get_state()
    (batch0, item0, plan0, _), rest = results[0], results[1:]
    for batch, item, plan, state in results:
        assert _same_state(state, want_state)
    for batch, item, plan, _ in rest:
        for a, b in zip(batch0[:4], batch[:4]):
            assert torch.equal(a, b)
        assert batch0[4] == batch[4] and torch.equal(item0["lr"], item["lr"]) and torch.equal(item0["hr"], item["hr"])
        assert np.array_equal(plan0[0], plan[0]) and plan0[1:] == plan[1:]
    # read_imageset: the keyword is last and off by default
    np.random.seed(4)
    a = DL.read_imageset(dirs[0], True, 64, seed, top_k, 50.0, 3)
    s_a = np.random.get_state()
    np.random.seed(4)
    b = DL.read_imageset(dirs[0], True, 64, seed, top_k, 50.0, 3, None)
    assert _same_state(s_a, np.random.get_state()) and np.array_equal(a["lr"], b["lr"]) and np.array_equal(a["hr"], b["hr"])


# ------------------------------------------------------------------ 4. RNG contract, augmentation on
def _restated_draws(dirs, indices, create_patches, patch_size, seed, top_k, beta, scale, mode):
    """The sequence by hand: per imageset the view choice (restated_read: one np.random.choice when top_k > 0), the corner
    (two randint) and then one randint(0, MODES[mode]), each after an optional re-seed.  -> (items, codes)."""
    items, codes = [], []
    for i in indices:
        items.append(restated_read(dirs[i], create_patches, patch_size, seed, top_k, beta, scale, io_binding.png_read))
        if seed is not None:
            np.random.seed(seed)
        codes.append(int(np.random.randint(0, augment.MODES[mode])))
    return items, codes


@pytest.mark.parametrize("create_patches,patch_size", [(True, 64), (True, 30), (False, 64)])
@pytest.mark.parametrize("top_k,seed,mode,scale", [(3, None, "dihedral", 3), (-1, None, "flip", 2), (5, 7, "dihedral", 4), (-1, 11, "dihedral", 3)])
def test_augmentation_on_follows_the_restated_draws(sets, create_patches, patch_size, top_k, seed, mode, scale):
    dirs = sets[scale]
    cfg = {"create_patches": create_patches, "patch_size": patch_size, "scale": scale}
    ds = DL.ImagesetDataset(dirs, cfg, seed=seed, top_k=top_k, beta=50.0, augment=mode)
    plain = DL.ImagesetDataset(dirs, cfg, seed=seed, top_k=top_k, beta=50.0)
    indices, min_L = [2, 0, 3, 1], 6
    np.random.seed(12)
    items, codes = _restated_draws(dirs, indices, create_patches, patch_size, seed, top_k, 50.0, scale, mode)
    want_state = np.random.get_state()
    assert all(0 <= c < augment.MODES[mode] for c in codes)

    # load_batch
    np.random.seed(12)
    lrs, alphas, hrs, maps, names = ds.load_batch(indices, min_L, n_threads=N_THREADS)
    assert _same_state(np.random.get_state(), want_state) and ds.last_augment == codes
    for b, (it, c) in enumerate(zip(items, codes)):
        n = min(min_L, len(it["lr"]))
        assert np.array_equal(lrs[b, :n].numpy(), augment.apply(it["lr"][:n], c)) and not lrs[b, n:].any()
        assert alphas[b].tolist() == [1.0] * n + [0.0] * (min_L - n)
        assert np.array_equal(hrs[b].numpy(), augment.apply(it["hr"], c))
        assert np.array_equal(maps[b].numpy(), augment.apply(it["sm"].astype(np.float32), c))

    # __getitem__ + collateFunction
    np.random.seed(12)
    got = U.collateFunction(min_L=min_L)([ds[i] for i in indices])
    assert _same_state(np.random.get_state(), want_state) and ds.last_augment == codes[-1:]
    for a, b in zip(got[:4], (lrs, alphas, hrs, maps)):
        assert torch.equal(a.float(), b)

    # read_imageset (uint16 arrays and a bool map)
    np.random.seed(12)
    read = [DL.read_imageset(dirs[i], create_patches, patch_size, seed, top_k, 50.0, scale, mode) for i in indices]
    assert _same_state(np.random.get_state(), want_state)
    for r, it, c in zip(read, items, codes):
        assert np.array_equal(r["lr"], augment.apply(it["lr_u16"], c)) and np.array_equal(r["hr"], augment.apply(it["hr_u16"], c))
        assert r["hr_map"].dtype == bool and np.array_equal(r["hr_map"], augment.apply(it["sm"], c))

    # ImagesetIndex: the plan of the un-augmented dataset (same views, same corner), with the codes beside it
    index = DL.ImagesetIndex(ds)
    np.random.seed(12)
    plan, got_codes, p_names, S, have_hr = index.plan_a(indices, min_L)
    assert _same_state(np.random.get_state(), want_state)
    assert got_codes.dtype == np.int32 and got_codes.tolist() == codes == index.last_augment
    np.random.seed(12)
    assert np.array_equal(index.plan(indices, min_L)[0], plan) and _same_state(np.random.get_state(), want_state)
    if seed is not None:                                              # a seeded run: the same views and corner without augmentation
        want_plan = DL.ImagesetIndex(plain).plan(indices, min_L)
        assert np.array_equal(want_plan[0], plan) and want_plan[1:] == (p_names, S, have_hr)
        base = plain.load_batch(indices, min_L, n_threads=N_THREADS)
        for b, c in enumerate(codes):
            for t_aug, t_plain in zip((lrs, hrs, maps), (base[0], base[2], base[3])):
                assert torch.equal(t_aug[b], augment.apply(t_plain[b], c))
            assert torch.equal(alphas[b], base[1][b])

    # BatchPrefetcher on the host: same batches, and the codes of the batch it handed over
    np.random.seed(12)
    pf = DL.BatchPrefetcher(ds, [indices[:2], indices[2:]], min_L, n_threads=N_THREADS)
    taken = [(batch, list(pf.last_augment)) for batch in pf]
    assert [c for _, c in taken] == [codes[:2], codes[2:]]
    assert torch.equal(torch.cat([taken[0][0][0], taken[1][0][0]]), lrs) and torch.equal(torch.cat([taken[0][0][3], taken[1][0][3]]), maps)


def test_augmentation_on_without_hr(sets):
    ds = DL.ImagesetDataset(sets["test"], {"create_patches": True, "patch_size": 64, "augment": "dihedral"}, top_k=3, beta=50.0)
    np.random.seed(8)
    items, codes = _restated_draws(sets["test"], [1, 0], True, 64, None, 3, 50.0, 3, "dihedral")
    np.random.seed(8)
    lrs, alphas, hrs, maps, _ = ds.load_batch([1, 0], 4, n_threads=N_THREADS)
    assert hrs == [] and ds.last_augment == codes
    np.random.seed(8)
    item = ds[1]
    assert item["hr"] is None and item["hr_map"].dtype == bool and ds.last_augment == codes[:1]
    assert np.array_equal(item["hr_map"], augment.apply(items[0]["sm"], codes[0]))
    for b, (it, c) in enumerate(zip(items, codes)):
        assert np.array_equal(lrs[b, :3].numpy(), augment.apply(it["lr"], c)) and np.array_equal(maps[b].numpy(), augment.apply(it["sm"].astype(np.float32), c))


# ------------------------------------------------------------------ 5. modes
def test_modes(sets):
    assert augment.MODES == {"flip": 4, "dihedral": 8}
    assert [augment.check_mode(m) for m in (None, False, "none", True, "flip", "dihedral")] == [None, None, None, "dihedral", "flip", "dihedral"]
    for bad in ("rot", "", 3, 0, 1.0, "None"):
        with pytest.raises(ValueError):
            augment.check_mode(bad)
    cfg = {"create_patches": True, "patch_size": 64}
    mk = lambda config, **kw: DL.ImagesetDataset(sets[3], config, top_k=-1, **kw)
    assert mk(cfg).augment is None and mk(dict(cfg, augment="flip")).augment == "flip" and mk(cfg, augment=True).augment == "dihedral"
    assert mk(dict(cfg, augment="flip"), augment="dihedral").augment == "dihedral"          # the argument wins
    assert mk(dict(cfg, augment="dihedral"), augment="none").augment is None
    for config, kw in ((dict(cfg, augment="spin"), {}), (cfg, dict(augment="spin")), (cfg, dict(augment=8))):
        with pytest.raises(ValueError):
            mk(config, **kw)
    with pytest.raises(ValueError):
        DL.read_imageset(sets[3][0], augment="spin")
    # 200 imageset draws from a fixed seed: "flip" never transposes, "dihedral" reaches all eight codes
    for mode, want in (("flip", {0, 1, 2, 3}), ("dihedral", set(range(8)))):
        index = DL.ImagesetIndex(mk(cfg, augment=mode))
        np.random.seed(2024)
        seen = []
        for _ in range(50):
            index.plan([0, 1, 2, 3], 4)
            seen += index.last_augment
        assert len(seen) == 200 and set(seen) == want
