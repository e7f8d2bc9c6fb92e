"""Cloud-free composite reference frame from the views and their quality masks, on device: the link between the
loaders' `lr_masks` / the `valid` planes of `registration.register_*` and the network, which reads neither.

`masked_composite` is one launch of `hrn_masked_composite`.  Its `ref` goes to `HRNet.forward(filled, alphas, ref=ref)` in place of the
network's own frame (the plain lower median of the first nine views, cloudy pixels and the zeros of registered views included), its
`filled` views replace the views.  The result is always one of the input values: exact, bit-reproducible, and a sample does not depend
on its batch.  There is no autograd formula - the frame is data; make `ref` a leaf for its own gradient - and no CPU fallback: tensors
must be on a ROCm device."""
import torch

from . import binding


def masked_composite(lrs, lr_masks=None, alphas=None, n_ref=9, return_count=False, fill=True):
    """lrs (B,V,H,W), lr_masks (B,V,H,W) 0 / non-zero or None (all clear), alphas (B,V) 0 / non-zero or None (every view real)
    -> (ref (B,H,W), filled (B,V,H,W)[, count (B,H,W)]), all f32; `filled` is None with fill=False, `count` comes with return_count.

    Per sample b and pixel p, with n = min(V, n_ref) and 1 <= n_ref <= 32:
      - a view v < n is REAL when alphas is None or alphas[b,v] != 0 (the loaders pad a short imageset with zero views of alpha 0), and
        a CANDIDATE when it is real and lr_masks is None or lr_masks[b,v,p] != 0;
      - with c >= 1 candidates ref[b,p] is their LOWER median - the element at index (c - 1) // 2 in ascending order, the rule of the
        network's own frame (torch.median) - and count[b,p] = c;
      - with c == 0, ref is the lower median over the real views v < n, masks ignored, and count = 0; with no real view either it is
        the lower median over all n views, which is the network's own frame;
      - filled[b,v,p] = lrs[b,v,p] where view v is not real (padding stays as it is), or lr_masks is None, or lr_masks[b,v,p] != 0;
        otherwise ref[b,p].  This covers all V views, not only the first n.
    The inputs must be finite (+inf is the padding key of the selection).  With lr_masks=None, alphas=None and n_ref=9, `ref` is the
    frame the network computes itself, bit for bit."""
    if not torch.is_tensor(lrs):
        raise TypeError(f"lrs must be a torch.Tensor; got {type(lrs).__name__}")
    if lr_masks is not None and not torch.is_tensor(lr_masks):
        raise TypeError(f"lr_masks must be a torch.Tensor or None; got {type(lr_masks).__name__}")
    if alphas is not None and not torch.is_tensor(alphas):
        raise TypeError(f"alphas must be a torch.Tensor or None; got {type(alphas).__name__}")
    if isinstance(n_ref, bool) or not isinstance(n_ref, int):
        raise TypeError(f"n_ref must be an integer; got {n_ref!r}")
    if lrs.dim() != 4 or lrs.numel() == 0:
        raise ValueError(f"lrs must be a non-empty (B,V,H,W); got {tuple(lrs.shape)}")
    if lr_masks is not None and lr_masks.shape != lrs.shape:
        raise ValueError(f"lr_masks must have the shape of lrs, {tuple(lrs.shape)}; got {tuple(lr_masks.shape)}")
    if alphas is not None and tuple(alphas.shape) != tuple(lrs.shape[:2]):
        raise ValueError(f"alphas must be (B,V) = {tuple(lrs.shape[:2])}; got {tuple(alphas.shape)}")
    if not 1 <= n_ref <= binding.COMPOSITE_MAX_REF:
        raise ValueError(f"n_ref must be in 1..{binding.COMPOSITE_MAX_REF}; got {n_ref}")
    for name, t in (("lrs", lrs), ("lr_masks", lr_masks), ("alphas", alphas)):
        if t is not None and not t.is_cuda:
            raise TypeError(f"{name} is on '{t.device}': the composite runs on a ROCm device only (no CPU fallback)")
        if t is not None and t.device != lrs.device:
            raise TypeError(f"{name} is on '{t.device}' but lrs on '{lrs.device}'")
    f32 = lambda t: None if t is None else t.detach().float().contiguous()
    ref, filled, count = torch.ops.hrnet_hip.masked_composite(f32(lrs), f32(lr_masks), f32(alphas), n_ref, bool(return_count), bool(fill))
    out = (ref, filled if fill else None)
    return out + (count,) if return_count else out
