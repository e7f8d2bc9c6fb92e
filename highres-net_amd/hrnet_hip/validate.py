"""Validation sharded over the ranks (last sentence; reference src/train.py:196-215).

The reference scores every validation imageset on rank 0: `srs = fusion_model(lrs, alphas)[:, 0]`, then per sample
`val_score -= shift_cPSNR(np.clip(srs[i], 0, 1), hrs[i], hr_maps[i])` on the host, finally `val_score /= len(dataset)`.  Here every rank
scores ITS imagesets on the device (`HRNet` in eval mode + `hrn_shift_cpsnr`, 49 shifted cPSNRs per image in one launch; scenes with
H != W go through the forward of the searched loss, `hrn_shift_loss_train` with clip, which takes any aspect ratio) and the two
scalars (sum of scores, number of samples) are all-reduced: one 16-byte collective per validation pass, no image ever leaves its GPU.
Without a process group the result is the single-process score.

With a baseline table (the `norm.csv` of a PROBA-V directory: imageset name -> ESA baseline cPSNR) the score is the reference's
`mean(ESA[name] / shift_cPSNR)` (train.py:213-217), the number that drives its best-checkpoint selection; the batches then carry the
`names` that collateFunction, load_batch, BatchPrefetcher and DeviceImagesetCache.batches produce as their fifth element.  `ensemble`
("flip" / "dihedral") scores the self-ensembled prediction (HRNet.forward_ensemble).  `tile` predicts through HRNet.forward_tiled
(windows of that side; a rectangular scene is scored like a square one).  `evaluate` is the same pass on one rank that also
returns the per-imageset cPSNRs.

The second figure, cSSIM (`losses.shift_cssim`, DESIGN.md section 7k: structural similarity under the same offset search), comes from the
same predictions: `evaluate(..., cssim=True)` adds it per imageset, `sharded_val_score(..., metric="cSSIM")` returns its mean over
all ranks.
"""
import collections

import numpy as np
import torch
import torch.distributed as dist

from . import binding


def shard_indices(n_items, rank, world_size):
    """Imagesets of rank `rank`: every world_size-th one (ragged tails spread over the first ranks)."""
    return list(range(rank, n_items, world_size))


Evaluation = collections.namedtuple("Evaluation", "names cpsnr score")
EvaluationCssim = collections.namedtuple("EvaluationCssim", "names cpsnr score cssim")      # evaluate(..., cssim=True)


def _default_score(srs, hrs, hr_maps, border_w):
    """shift_cPSNR(np.clip(sr, 0, 1), hr, hr_map, border_w) per sample on the device: square batches through hrn_shift_cpsnr, as ever;
    batches with H != W through the searched loss's forward, the same definition on frames of any aspect ratio."""
    if srs.shape[-1] == srs.shape[-2]:
        return binding.shift_cpsnr(srs, hrs, hr_maps, border_w, True)
    return binding.shift_loss_train(srs, hrs, hr_maps, "cPSNR", border_w, True)[0]


def _cssim_score(srs, hrs, hr_maps, border_w):
    """cSSIM of np.clip(sr, 0, 1) per sample on the device, with the defaults of losses.shift_cssim."""
    from . import losses
    return losses.shift_cssim(srs, hrs, hr_maps, border_w=border_w, clip=True)


def _score_batches(fusion_model, batches, baseline_cpsnrs, ensemble, border_w, score_fn, members_per_pass, keep, tile=None, second_fn=None):
    """The validation loop of train.py:196-215 over this rank's batches, (lrs, alphas, hrs, hr_maps) or (..., names): -> (float64
    sum on the device of cPSNR - or of ESA[name] / cPSNR with a baseline table - or None without a batch, the number of samples,
    names, the list of per-batch float64 cPSNR tensors when `keep` - with `second_fn`, of (cPSNR, second_fn(srs, hrs, hr_maps)) pairs).
    The model's training flag is restored."""
    from . import augment
    score_fn = score_fn or (lambda s, h, m: _default_score(s, h, m, border_w))
    mode = augment.check_mode(ensemble)
    if mode is not None and not hasattr(fusion_model, "forward_ensemble"):
        raise TypeError(f"ensemble={ensemble!r} needs a model with forward_ensemble (DeepNetworks.HRNet), got {type(fusion_model).__name__}")
    if tile is not None and not hasattr(fusion_model, "forward_tiled"):
        raise TypeError(f"tile={tile!r} needs a model with forward_tiled (DeepNetworks.HRNet), got {type(fusion_model).__name__}")
    was_training = fusion_model.training
    fusion_model.eval()
    total, count, all_names, kept = None, 0, [], []
    try:
        with torch.no_grad():
            for batch in batches:
                if len(batch) not in (4, 5):
                    raise ValueError(f"a validation batch is (lrs, alphas, hrs, hr_maps) or (..., names); got {len(batch)} elements")
                lrs, alphas, hrs, hr_maps = batch[:4]
                names = list(batch[4]) if len(batch) == 5 else None
                if baseline_cpsnrs is not None and names is None:
                    raise ValueError("a baseline table needs batches with names: (lrs, alphas, hrs, hr_maps, names)")
                if names is not None and len(names) != lrs.shape[0]:
                    raise ValueError(f"{len(names)} names for a batch of {lrs.shape[0]}")
                if tile is not None:
                    srs = fusion_model.forward_tiled(lrs, alphas, tile, ensemble=mode, members_per_pass=members_per_pass)[:, 0]
                elif mode is None:
                    srs = fusion_model(lrs, alphas)[:, 0]
                else:
                    srs = fusion_model.forward_ensemble(lrs, alphas, mode, members_per_pass)[:, 0]
                cpsnr = score_fn(srs, hrs, hr_maps).double()
                if baseline_cpsnrs is None:
                    sc = cpsnr.sum()
                else:       # the batch's ESA values go up as one small tensor; a missing name is the reference's KeyError
                    esa = torch.tensor([float(baseline_cpsnrs[n]) for n in names], dtype=torch.float64).to(cpsnr.device)
                    sc = (esa / cpsnr).sum()
                total = sc if total is None else total + sc
                count += int(srs.shape[0])
                if names is not None:
                    all_names += names
                if keep:
                    kept.append(cpsnr if second_fn is None else (cpsnr, second_fn(srs, hrs, hr_maps).double()))
    finally:
        fusion_model.train(was_training)
    return total, count, all_names, kept


def evaluate(fusion_model, batches, baseline_cpsnrs=None, ensemble=None, border_w=3, score_fn=None, members_per_pass=None, tile=None,
             cssim=False):
    """One rank's evaluation pass over `batches` of (lrs, alphas, hrs, hr_maps, names) (names may be left out without a baseline table):
    -> Evaluation(names, cpsnr, score) with the per-imageset shift_cPSNR as a float64 numpy array in batch order and `score` the
    reference's validation score (train.py:209-217): -mean(cPSNR) without a baseline table, mean(ESA[name] / cPSNR) with one
    (`baseline_cpsnrs`: name -> ESA baseline cPSNR).  ensemble: None, or "flip" / "dihedral" to score
    `fusion_model.forward_ensemble(lrs, alphas, ensemble, members_per_pass)` instead of the plain forward.  The sums stay in float64
    on the device; one read-back at the end.  score_fn as in sharded_val_score.  tile: None, or the window side with which
    `fusion_model.forward_tiled(lrs, alphas, tile, ensemble=ensemble, members_per_pass=members_per_pass)` predicts instead.
    cssim: also score every prediction with `losses.shift_cssim(srs, hrs, hr_maps, border_w, clip=True)` in the same pass; the result is
    then EvaluationCssim(names, cpsnr, score, cssim), `cssim` a float64 numpy array in batch order."""
    second = (lambda s, h, m: _cssim_score(s, h, m, border_w)) if cssim else None
    total, count, names, kept = _score_batches(fusion_model, batches, baseline_cpsnrs, ensemble, border_w, score_fn, members_per_pass, True,
                                               tile, second)
    if count == 0:
        raise ValueError("evaluate: no sample in `batches`")
    mean = float(total / count)
    score = mean if baseline_cpsnrs is not None else -mean
    if not cssim:
        return Evaluation(names, torch.cat(kept).cpu().numpy().astype(np.float64), score)
    return EvaluationCssim(names, torch.cat([c for c, _ in kept]).cpu().numpy().astype(np.float64), score,
                           torch.cat([q for _, q in kept]).cpu().numpy().astype(np.float64))


def baseline_table(batches, border_w=3, a=-0.75, n_ref=9, method="bicubic", **method_kwargs):
    """ESA's baseline for data without ESA's table - "cPSNR of a bicubic upsample of an averaged clear frame": over `batches` of
    (lrs, alphas, hrs, hr_maps, names) -> {name: shift_cPSNR(clip(upsample.baseline(lrs, alphas, scale=S, a=a, n_ref=n_ref), 0, 1), hr,
    hr_map, border_w)}, scored on the device by the scorer `evaluate` uses.  S is taken from the shapes (hrs against lrs: 2, 3 or 4).  The
    result is what `evaluate(..., baseline_cpsnrs=)` takes; `utils.writeBaselineCPSNR` stores it in the format of norm.csv.

    method="shift_add" scores the registered multi-frame baseline instead: `shiftadd.register_and_add(lrs, lr_masks, alphas, scale=S,
    **method_kwargs)` (the views registered against the first one, then shift-and-add over the bicubic base; a and n_ref are not used).
    method="back_projection" scores `observation.register_and_refine(lrs, lr_masks, alphas, scale=S, **method_kwargs)`: the same
    registration, then iterative back-projection against the views (iters, step, init).
    method="robust" scores the same call with robust="welsch" and lam=4e-4 unless method_kwargs set them: `observation.reconstruct`'s
    Welsch-weighted data term and bilateral-TV prior (delta, lam, P, alpha, eps).
    method="joint" scores the same call with joint=True unless method_kwargs set it: `observation.reconstruct_joint`'s Gauss-Newton
    refinement of the shifts beside every data step (for rough registrations; it does not improve on a search that worked).
    A batch may carry lr_masks (B,V,H,W) as a sixth item, which those methods use (None: all clear); the bicubic method does not read
    it."""
    if method not in ("bicubic", "shift_add", "back_projection", "robust", "joint"):
        raise ValueError(f"method must be \"bicubic\", \"shift_add\", \"back_projection\", \"robust\" or \"joint\"; got {method!r}")
    if method == "robust":
        method_kwargs = dict(dict(robust="welsch", lam=4e-4), **method_kwargs)
    if method == "joint":
        method_kwargs = dict(dict(joint=True), **method_kwargs)
    if method == "bicubic" and method_kwargs:
        raise TypeError(f"method=\"bicubic\" takes no further arguments; got {sorted(method_kwargs)}")
    from . import observation, shiftadd, upsample
    table = {}
    with torch.no_grad():
        for batch in batches:
            if len(batch) not in (5, 6):
                raise ValueError(f"a baseline batch is (lrs, alphas, hrs, hr_maps, names[, lr_masks]); got {len(batch)} elements")
            lrs, alphas, hrs, hr_maps, names = batch[:5]
            lr_masks = batch[5] if len(batch) == 6 else None
            names = list(names)
            if len(names) != lrs.shape[0]:
                raise ValueError(f"{len(names)} names for a batch of {lrs.shape[0]}")
            S = hrs.shape[-2] // lrs.shape[-2]
            if tuple(hrs.shape[-2:]) != (S * lrs.shape[-2], S * lrs.shape[-1]):
                raise ValueError(f"hrs {tuple(hrs.shape)} is no integer multiple of lrs {tuple(lrs.shape)}")
            if method == "bicubic":
                srs = upsample.baseline(lrs, alphas, scale=S, a=a, n_ref=n_ref)[:, 0]
            elif method == "shift_add":
                srs = shiftadd.register_and_add(lrs, lr_masks, alphas, scale=S, **method_kwargs)[0]
            else:
                srs = observation.register_and_refine(lrs, lr_masks, alphas, scale=S, **method_kwargs)[0]
            cpsnr = _default_score(srs, hrs, hr_maps, border_w).double().cpu().numpy()
            for name, c in zip(names, cpsnr):
                table[name] = float(c)
    return table


def sharded_val_score(fusion_model, batches, border_w=3, score_fn=None, device=None, baseline_cpsnrs=None, ensemble=None, tile=None,
                      metric="cPSNR"):
    """`batches`: this rank's validation batches of (lrs, alphas, hrs, hr_maps) tensors, or the same with `names` as a fifth element
    (the reference loads them one imageset at a time, train.py:281).  Returns `val_score` of train.py:199-217 over ALL ranks' samples:
    -mean(shift_cPSNR), or with `baseline_cpsnrs` (name -> ESA baseline cPSNR; needs the names) mean(ESA[name] / shift_cPSNR).  Either
    way only (sum, count) is all-reduced.  ensemble: None, or "flip" / "dihedral" to score the model's forward_ensemble.  tile: None, or
    the window side of the model's forward_tiled, which then predicts (with `ensemble`).
    score_fn(srs (B,S,S), hrs, hr_maps) -> (B,) replaces `hrn_shift_cpsnr` in the CPU rehearsal of the collective (tests/test_dist_cpu.py).
    metric: "cPSNR", or "cSSIM" for the mean of `losses.shift_cssim(srs, hrs, hr_maps, border_w, clip=True)` over all ranks' samples
    (returned as it is, not negated: higher is better), through the same collective; a baseline table has no meaning for it."""
    if metric not in ("cPSNR", "cSSIM"):
        raise ValueError(f"metric must be 'cPSNR' or 'cSSIM'; got {metric!r}")
    if metric == "cSSIM":
        if baseline_cpsnrs is not None:
            raise ValueError("baseline_cpsnrs normalises cPSNR; it cannot be combined with metric='cSSIM'")
        score_fn = score_fn or (lambda s, h, m: _cssim_score(s, h, m, border_w))
    total, count, _, _ = _score_batches(fusion_model, batches, baseline_cpsnrs, ensemble, border_w, score_fn, None, False, tile)
    if total is None:
        total = torch.zeros((), dtype=torch.float64, device=device or "cpu")
    acc = torch.stack([total.reshape(()), torch.tensor(float(count), dtype=torch.float64, device=total.device)])
    if dist.is_initialized() and dist.get_world_size() > 1:
        if acc.device.type != "cuda" and dist.get_backend() == "nccl":
            acc = acc.cuda()
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
    if float(acc[1]) == 0:
        raise ValueError("sharded_val_score: no validation sample on any rank")
    mean = float(acc[0] / acc[1])
    return mean if baseline_cpsnrs is not None or metric == "cSSIM" else -mean
