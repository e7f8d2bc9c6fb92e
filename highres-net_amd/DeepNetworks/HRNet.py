"""HRNet on MI355X: same import path, constructor, call signature and state_dict as the reference's
`src/DeepNetworks/HRNet.py` (HRNet :172-211; Encoder :36-74; RecuversiveNet :77-134; Decoder :138-169;
ResidualBlock :7-33), computed by the hand-written gfx950 kernels of libhrnet_hip.so.

The nn.Module tree below only *holds parameters* under the reference's names (so checkpoints load and
`torch.manual_seed` reproduces the reference's default initialisation: the same layer types are created in
the same order).  None of the sub-modules is ever called: `HRNet.forward` hands the tensors to the C ABI
(`hrn_hrnet_forward`), which runs median -> stem -> encoder -> recursive pairwise fusion -> decoder.

Precision (`HRNet.precision`, or key "precision" in the config dict, or env HRNET_HIP_PRECISION):
    "fp32" (default)  exact-fp32 MFMA; matches the reference forward to ~1e-6 relative
    "bf16"            bf16 activations/weights, fp32 accumulation; the throughput path (BASELINE config 3)
    "bf16x3"          split-bf16: every fp32 value as a (hi, lo) pair of bf16, three bf16 MFMAs per product, fp32 accumulation;
                      matches the reference forward to ~1e-5 relative at ~3x the fp32 path's speed

Training precision (`HRNet.train_precision`, or key "train_precision" in the config dict; default None):
    None              today's rules: the training forward and backward follow `precision` ("fp32" / "bf16x3"); with
                      precision "bf16" the forward runs the bf16 inference kernels and a backward recomputes it in fp32
    "fp32" / "bf16" / "bf16x3" (same aliases as `precision`)
                      the training forward and backward run in that precision; `precision` then governs only the forward
                      without a graph (.eval(), no_grad).  "bf16": one bf16 plane per activation and gradient, fp32
                      accumulation; parameters, their gradients and the optimizer state stay fp32

Self-ensemble (`HRNet.ensemble`, or key "ensemble" in the config dict; default None; values as the loaders' `augment`):
    None / False / "none"   off: `forward` is the code path it always was
    "flip" / "dihedral" (True)
                      the forward WITHOUT a graph (.eval(), no_grad) returns `forward_ensemble(lrs, alphas, mode)`: the mean of the
                      4 / 8 predictions from the flipped / rotated view stacks, each transformed back (hrnet_hip/augment.py).  The
                      training branch is never ensembled.

Tiled inference (`HRNet.tile`, or key "tile" in the config dict; default None):
    None              off: `forward` is the code path it always was, square low-res images only
    an integer        the forward WITHOUT a graph routes an input that is not square, or larger than `tile` pixels a side, through
                      `forward_tiled(lrs, alphas, tile, ensemble=self.ensemble)`: overlapping square windows whose cores tile the
                      scene (hrnet_hip/tiling.py).  Scenes of any size and aspect ratio; the training branch is never tiled.

Reference frame (`forward(lrs, alphas, ref=None)`, likewise forward_ensemble and forward_tiled):
    None              the network's own frame, the lower median of lrs[:, :9]: the code path it always was
    a (B,H,W) float tensor on the device
                      that frame is the second input channel of every view instead, e.g. the cloud-free composite of
                      hrnet_hip.composite.masked_composite.  It is data: in training it gets a gradient of its own when it requires one,
                      and nothing flows from it into lrs.  With ref equal to the median every result is bit-identical to ref=None.

Global residual (`HRNet.global_residual`, or key "global_residual" in the config dict; default None):
    None / False      off: every path is the code path it always was
    True              every forward returns net(...) + up(frame) at the model's scale: the network predicts the difference to the
                      bicubic upsample (hrnet_hip/upsample.py, a = -0.75) of `ref` when one is given, else of its own median of
                      lrs[:, :9] (bit for bit, taken as data).  One fused in-place hrn_upsample on the output, in fp32 in every
                      `precision`: after the inference kernels in `forward`, once after the mean in `forward_ensemble`, once on the
                      whole scene after the last scatter in `forward_tiled`.  In training the differentiable op sits around the
                      training op's output: parameter gradients are unchanged, a `ref` that requires grad receives the stem's d_ref
                      plus the adjoint of d_sr; ref=None with lrs.requires_grad raises (pass ref= explicitly).  No new parameters:
                      the state_dict is unchanged, a checkpoint trained with the flag needs the flag, and zeroing decode.final
                      starts such a model exactly at the bicubic baseline.
    base= (forward, forward_ensemble, forward_tiled; None by default)
                      with the flag on, a (B,SH,SW) or (B,1,SH,SW) float tensor on the device that takes the place of up(frame): the
                      model returns net(...) + base, the base added once, at the places the skip is added - e.g. the shift-and-add
                      frame of hrnet_hip.shiftadd.register_and_add, a registered multi-frame base instead of a single upsampled
                      frame.  `ref` keeps its own meaning (the stem's second channel).  In training it is a differentiable add:
                      d_base = d_sr, parameter gradients untouched.  base= with the flag off raises; base=None is the path above.
"""
import os

import torch
import torch.nn as nn

from hrnet_hip import augment, binding, composite, tiling

_PRECISIONS = {"fp32": binding.F32, "f32": binding.F32, "float32": binding.F32, "bf16": binding.BF16, "bfloat16": binding.BF16,
               "bf16x3": binding.BF16X3}
_RESIDUAL_A = -0.75       # the cubic of the global residual's upsampler: torch's and OpenCV's bicubic


class _Holder(nn.Module):
    """Parameter container: exists for state_dict()/parameters()/to(); never executed."""

    def forward(self, *args, **kwargs):
        raise RuntimeError(f"{type(self).__name__} holds parameters only; call HRNet(lrs, alphas)")


class ResidualBlock(_Holder):
    def __init__(self, channel_size=64, kernel_size=3):
        super().__init__()
        pad = kernel_size // 2
        self.block = nn.Sequential(nn.Conv2d(channel_size, channel_size, kernel_size, padding=pad), nn.PReLU(),
                                   nn.Conv2d(channel_size, channel_size, kernel_size, padding=pad), nn.PReLU())


class Encoder(_Holder):
    def __init__(self, config):
        super().__init__()
        cin, layers, k, c = config["in_channels"], config["num_layers"], config["kernel_size"], config["channel_size"]
        self.init_layer = nn.Sequential(nn.Conv2d(cin, c, k, padding=k // 2), nn.PReLU())
        self.res_layers = nn.Sequential(*[ResidualBlock(c, k) for _ in range(layers)])
        self.final = nn.Sequential(nn.Conv2d(c, c, k, padding=k // 2))


class RecuversiveNet(_Holder):
    def __init__(self, config):
        super().__init__()
        self.input_channels = config["in_channels"]
        self.num_layers = config["num_layers"]
        self.alpha_residual = config["alpha_residual"]
        k = config["kernel_size"]
        c = self.input_channels
        self.fuse = nn.Sequential(ResidualBlock(2 * c, k), nn.Conv2d(2 * c, c, k, padding=k // 2), nn.PReLU())


class Decoder(_Holder):
    def __init__(self, config):
        super().__init__()
        d, f = config["deconv"], config["final"]
        self.deconv = nn.Sequential(nn.ConvTranspose2d(d["in_channels"], d["out_channels"], d["kernel_size"], stride=d["stride"]),
                                    nn.PReLU())
        self.final = nn.Conv2d(f["in_channels"], f["out_channels"], f["kernel_size"], padding=f["kernel_size"] // 2)


def _check_config(config):
    """-> the upscale factor.  The kernels take the reference's network (config/config.json:8-34) with any decoder.deconv
    kernel_size == stride in binding.SCALES (non-overlapping: every LR pixel owns its S x S block of SR pixels)."""
    e, r, d = config["encoder"], config["recursive"], config["decoder"]
    ok = (e["in_channels"] == 2 and e["kernel_size"] == 3 and e["channel_size"] == 64 and 0 <= e["num_layers"] <= binding.MAX_RES_LAYERS
          and r["in_channels"] == 64 and r["kernel_size"] == 3
          and d["deconv"]["in_channels"] == 64 and d["deconv"]["out_channels"] == 64
          and d["deconv"]["kernel_size"] == d["deconv"]["stride"] and d["deconv"]["stride"] in binding.SCALES
          and d["final"]["in_channels"] == 64 and d["final"]["out_channels"] == 1 and d["final"]["kernel_size"] == 1)
    if not ok:
        raise NotImplementedError(
            "the gfx950 kernels are specialised for the reference's network (config/config.json:8-34): 2->64 stem, 64-channel "
            f"3x3 convs, a ConvTranspose2d with kernel_size == stride in {binding.SCALES} (the upscale factor), 1x1 final; got "
            + repr(config))
    return d["deconv"]["stride"]


class _HRNetLazyTrainFunction(torch.autograd.Function):
    """`.train()` mode with `precision="bf16"`: the forward runs the bf16 INFERENCE kernels (what `precision` asks for; this is
    the path `src/predict.py` takes, whose `load_model` never calls `.eval()` and whose `get_sr_and_score` does not use
    `no_grad`: predict.py:86-100, :17-49) and keeps nothing; IF a backward pass follows, it re-runs the forward on the fp32
    training kernels first (hrn_hrnet_forward_train) and then hrn_hrnet_backward.  Gradients are those of the fp32 model at the
    same parameters; the one returned tensor carries bf16 rounding."""

    @staticmethod
    def forward(ctx, module, names, lrs, alphas, *params):
        packed, dt = module.packed_parameters()
        ctx.module, ctx.names = module, names
        ctx.versions = tuple(p._version for p in params)
        ctx.save_for_backward(lrs, alphas, *params)
        return binding.hrnet_forward(packed, dt, module._num_layers, module.fuse.alpha_residual, lrs, alphas, scale=module._scale)

    _warned = False

    @staticmethod
    def backward(ctx, d_sr):
        lrs, alphas, *params = ctx.saved_tensors
        m = ctx.module
        if not _HRNetLazyTrainFunction._warned:
            _HRNetLazyTrainFunction._warned = True
            import warnings
            warnings.warn("HRNet(precision='bf16').train(): the forward ran the bf16 inference kernels, this backward recomputes "
                          "the forward on the fp32 training kernels and returns the fp32 model's gradients (two forwards per step, "
                          "loss and gradient ~1e-2 apart). Train with precision='fp32' or 'bf16x3'.", RuntimeWarning, stacklevel=2)
        if tuple(p._version for p in params) != ctx.versions:
            raise RuntimeError("HRNet bf16 train-mode backward: a parameter was modified between forward and backward")
        packed = m._packed_f32()
        _, tws = binding.hrnet_forward_train(packed, lrs, alphas, m._num_layers, m.fuse.alpha_residual, scale=m._scale)
        named = dict(zip(ctx.names, params))
        grads = {k: torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for k, p in named.items()}
        # input gradients from the same fp32 recompute, when asked for (alphas: only through an alpha residual, as in the reference)
        need_lrs = ctx.needs_input_grad[2]
        need_alphas = ctx.needs_input_grad[3] and bool(m.fuse.alpha_residual) and lrs.shape[1] > 1
        d_lrs = torch.empty(lrs.shape, dtype=torch.float32, device=lrs.device) if need_lrs else None
        d_alphas = torch.empty(alphas.shape, dtype=torch.float32, device=alphas.device) if need_alphas else None
        binding.hrnet_backward(packed, named, grads, m._num_layers, m.fuse.alpha_residual, lrs, alphas, d_sr.contiguous(), tws,
                               scale=m._scale, d_lrs=d_lrs, d_alphas=d_alphas)
        return ((None, None, d_lrs.to(lrs.dtype) if need_lrs else None, d_alphas.to(alphas.dtype) if need_alphas else None)
                + tuple(grads[k].to(named[k].dtype) for k in ctx.names))


class HRNet(nn.Module):
    """HRNet(config["network"]); forward(lrs (B,L,H,W), alphas (B,L)) -> (B,1,SH,SW), S = decoder.deconv.stride (2, 3 or 4)."""

    def __init__(self, config):
        super().__init__()
        self._scale = _check_config(config)
        self.encode = Encoder(config["encoder"])
        self.fuse = RecuversiveNet(config["recursive"])
        self.decode = Decoder(config["decoder"])
        self._num_layers = config["encoder"]["num_layers"]
        self.precision = config.get("precision", os.environ.get("HRNET_HIP_PRECISION", "fp32"))
        self.train_precision = config.get("train_precision")
        self.ensemble = config.get("ensemble")
        self.tile = config.get("tile")
        self.global_residual = config.get("global_residual")
        self._packed = {}                   # dtype -> (key, blob): the inference and the training blob do not evict each other

    # -- packed-parameter cache: re-packed whenever a parameter was modified (optimizer step, load_state_dict, .to())
    def _dtype(self):
        try:
            return _PRECISIONS[str(self.precision).lower()]
        except KeyError:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}; got {self.precision!r}")

    def _train_dtype(self):
        """The dtype of the training forward / backward chosen by `train_precision`, or None (then `precision` decides)."""
        if self.train_precision is None:
            return None
        try:
            return _PRECISIONS[str(self.train_precision).lower()]
        except KeyError:
            raise ValueError(f"train_precision must be None or one of {sorted(_PRECISIONS)}; got {self.train_precision!r}")

    def _packed_for(self, dt):
        named = dict(self.named_parameters())
        key = (binding.param_epoch,) + tuple((p.data_ptr(), p._version) for p in named.values())
        hit = self._packed.get(dt)
        if hit is None or hit[0] != key:
            hit = (key, binding.hrnet_pack(named, self._num_layers, dt, self._scale))
            self._packed[dt] = hit
        return hit[1]

    def packed_parameters(self):
        dt = self._dtype()
        return self._packed_for(dt), dt

    # -- the global residual (module docstring): the three public forwards are their `_plain` forms plus one fused add
    def _residual_on(self):
        g = self.global_residual
        if g is None or g is False:
            return False
        if g is True:
            return True
        raise ValueError(f"global_residual must be None, False or True; got {g!r}")

    def _residual_frame(self, lrs, ref):
        """the frame the skip upsamples: `ref` when given, else the network's own median of lrs[:, :9], bit for bit, as data"""
        if ref is not None:
            return binding._ref_frame(ref, lrs)
        return composite.masked_composite(lrs, n_ref=9, fill=False)[0]

    def _add_residual(self, sr, lrs, ref):
        """sr (B,1,SH,SW) -> sr + up(frame).  Without a graph: hrn_upsample in place on sr (no pass of its own over sr beyond the add).
        With one: the differentiable op around the training op's output - d_sr passes through unchanged, a ref that requires grad
        receives the adjoint of d_sr on top of the stem's d_ref."""
        B, _, SH, SW = sr.shape
        frame = self._residual_frame(lrs, ref)
        if sr.requires_grad:                  # the training branch of forward (a ref that requires grad puts sr into a graph too)
            return torch.ops.hrnet_hip.upsample(frame, sr.view(B, SH, SW), self._scale, _RESIDUAL_A).view(B, 1, SH, SW)
        with torch.no_grad():
            plane = sr.view(B, SH, SW)        # the inference outputs are dense: base and out are sr's own memory
            binding.upsample(frame.detach(), plane, self._scale, _RESIDUAL_A, out=plane)
        return sr

    def _add_base(self, sr, base):
        """sr (B,1,SH,SW) -> sr + base, base (B,SH,SW) or (B,1,SH,SW) given by the caller in up(frame)'s place.  Without a graph the add
        is in place on sr (the inference outputs are the model's own memory); with one it is the differentiable add, d_base = d_sr."""
        if not torch.is_tensor(base):
            raise TypeError(f"base must be a torch.Tensor or None; got {type(base).__name__}")
        B, _, SH, SW = sr.shape
        if tuple(base.shape) not in ((B, SH, SW), (B, 1, SH, SW)):
            raise ValueError(f"base must be {(B, SH, SW)} or {(B, 1, SH, SW)}; got {tuple(base.shape)}")
        if not base.is_floating_point():
            raise TypeError(f"base must be a floating-point tensor; got {base.dtype}")
        if base.device != sr.device:
            raise TypeError(f"base is on '{base.device}' but the model's output on '{sr.device}'")
        base = base.float().view(B, 1, SH, SW)
        if torch.is_grad_enabled() and (sr.requires_grad or base.requires_grad):
            return sr + base
        with torch.no_grad():
            return sr.add_(base.detach())

    def _check_base_off(self, base):
        if base is not None:
            raise ValueError("base= needs HRNet(global_residual=True): without the flag the model returns net(...) alone and the base "
                             "would be dropped")

    def forward(self, lrs, alphas, ref=None, base=None):
        if not self._residual_on():
            self._check_base_off(base)
            return self._forward_plain(lrs, alphas, ref)
        if base is not None:
            return self._add_base(self._forward_plain(lrs, alphas, ref), base)
        if ref is None and torch.is_grad_enabled() and torch.is_tensor(lrs) and lrs.requires_grad:
            raise NotImplementedError(
                "HRNet(global_residual=True) with lrs.requires_grad and ref=None: the skip's frame is the median of lrs[:, :9], taken as "
                "data, so its share of the gradient would silently never reach lrs.  Pass ref= explicitly (e.g. "
                "hrnet_hip.composite.masked_composite(lrs)[0], a leaf of its own when it needs a gradient).")
        return self._add_residual(self._forward_plain(lrs, alphas, ref), lrs, ref)

    def forward_ensemble(self, lrs, alphas, mode="dihedral", members_per_pass=None, ref=None, base=None):
        """Self-ensemble at inference: (B,L,H,W), (B,L) -> (B,1,SH,SW), the mean over the K = 4 ("flip") or 8 ("dihedral") members
        of augment.ensemble_codes(mode) of `forward(apply(lrs, code))` transformed back with the inverse code; bit for bit
        `augment.mean_inverse(forward(member-major batch), codes)`.  Always the inference kernels of `precision`, no autograd graph.
        One hrn_dihedral_expand launch builds the (K*B, L, H, W) member-major batch, the forward writes into slices of one
        (K, B, 1, SH, SW) buffer, one hrn_dihedral_mean launch averages.  members_per_pass (1..K, default K): how many members one
        forward takes, which bounds its workspace; a sample's result does not depend on its batch, so this changes no bit.
        ref (B,H,W): the reference frame; every member receives it under the member's own transform (the same expand, as a one-view stack).
        With `global_residual` the skip is added once, on the untransformed frame, after the mean: the filter is symmetric, so in
        exact arithmetic this is the ensemble of the members' own skips, and the ensemble keeps its bits.  base (B,SH,SW): with
        `global_residual`, the frame added in the skip's place (module docstring), once, untransformed, after the mean."""
        if not self._residual_on():
            self._check_base_off(base)
        sr = self._forward_ensemble_plain(lrs, alphas, mode, members_per_pass, ref)
        if base is not None:
            return self._add_base(sr, base)
        return self._add_residual(sr, lrs, ref) if self._residual_on() else sr

    def forward_tiled(self, lrs, alphas, tile=128, windows_per_pass=None, ensemble=None, members_per_pass=None, ref=None, base=None):
        """Inference on a scene of any size and aspect ratio: (B,L,H,W), (B,L) -> (B,1,SH,SW), H, W >= 1, from overlapping square
        windows of side t = min(tile, H, W) (hrnet_hip/tiling.py).  A window is responsible for its core, whose every edge is on the
        scene's border or at least R = tiling.halo(num_layers, L) LR pixels inside the window - the network's receptive field - so
        the result is what a whole-frame forward would give, where one exists.  Always the inference kernels of `precision`, no
        autograd graph.

        The plan's windows go through in chunks of `windows_per_pass` (default max(1, 32 // B): 32 samples per forward): one
        hrn_tile_gather launch builds the (chunk, B, L, t, t) window-major batch, one forward takes it as chunk * B samples, one
        hrn_tile_scatter launch puts the cores into the output.  Peak memory: the output, one chunk of windows (LR and SR) and one
        forward's workspace; all windows are never materialised at once.  A sample's result does not depend on its batch, so the
        chunking changes no bit.  The work grows by the plan's overhead factor n_windows * t * t / (H * W).

        ensemble ("flip" / "dihedral"; None: off): every chunk of windows goes through the self-ensemble of forward_ensemble
        (expand / forward / mean, `members_per_pass` members per forward).  For a square scene this is forward_ensemble of the whole
        frame; for a rectangular one it DEFINES the ensemble, transposing members included: the windows are square.

        A scene that is one window (H == W <= tile) goes straight to the plain forward (or forward_ensemble).

        ref (B,H,W): the reference frame of the scene; every window receives its own cut of it (the same gather, as a one-view stack).

        With `global_residual` the skip is added once, on the whole scene (the upsampler takes rectangular planes), after the last
        scatter: the result stays bit-identical to the whole-frame forward wherever one exists.  base (B,SH,SW): with
        `global_residual`, the scene-sized frame added in the skip's place (module docstring), once, after the last scatter."""
        if not self._residual_on():
            self._check_base_off(base)
        sr = self._forward_tiled_plain(lrs, alphas, tile, windows_per_pass, ensemble, members_per_pass, ref)
        if base is not None:
            return self._add_base(sr, base)
        return self._add_residual(sr, lrs, ref) if self._residual_on() else sr

    def _forward_plain(self, lrs, alphas, ref=None):
        """forward without the global residual: the network's own output"""
        if ref is not None:
            return self._forward_ref(lrs, alphas, ref)
        if lrs.dim() != 4:
            raise ValueError(f"lrs must be (B, L, H, W); got {tuple(lrs.shape)}")
        grad_params = self.training and any(p.requires_grad for p in self.parameters())
        grad_inputs = lrs.requires_grad or alphas.requires_grad
        graph = torch.is_grad_enabled() and (grad_params or grad_inputs)
        if self.tile is not None and not graph and (lrs.shape[2] != lrs.shape[3] or lrs.shape[2] > self._tile_side(self.tile)):
            return self._forward_tiled_plain(lrs, alphas, self.tile, ensemble=self.ensemble)
        if lrs.shape[2] != lrs.shape[3]:
            raise ValueError("square low-res images only: the reference reinterprets (H,W) as (W,H) in its .view() "
                             "(HRNet.py:204), which is the identity only for H == W"
                             + ("" if graph else "; forward_tiled (or the `tile` attribute) takes scenes of any shape at inference"))
        if graph:
            # .train() mode with grad enabled - the training loop (train.py:160-190), but also src/predict.py, which never calls
            # .eval() and uses no no_grad (predict.py:86-100, :17-49).  Autograd cannot tell us whether a backward pass will follow:
            #   precision "fp32" (default) / "bf16x3": the training forward of that precision (torch.ops.hrnet_hip.hrnet_forward_train), which
            #                               keeps its intermediates for the HIP backward (same numbers as the inference kernels of that mode);
            #   precision "bf16":           the bf16 inference kernels, as asked for; a backward pass, if one comes, first
            #                               recomputes the forward on the fp32 training kernels (_HRNetLazyTrainFunction).
            # lrs and alphas go in undetached: autograd asks the backward for their gradients when they require grad (in either mode,
            # frozen parameters included: attribution, learned view weights, input-space optimisation).
            # Otherwise, in .eval() mode (validation, train.py:196-215), the inference kernels run and the result carries no autograd graph.
            # With train_precision set, it alone picks the training forward / backward (bf16 included: no recompute, no warning).
            names = [k for k, _ in self.named_parameters()]
            params = [p for _, p in self.named_parameters()]
            dt = self._train_dtype()
            if dt is None:
                if self._dtype() == binding.BF16:
                    return _HRNetLazyTrainFunction.apply(self, names, lrs, alphas, *params)
                dt = self._dtype()
            # the dispatcher-registered training op (binding.py): hrn_hrnet_forward_train with hrn_hrnet_backward as its autograd formula
            if names != binding.hrnet_param_names(self._num_layers):
                raise RuntimeError("HRNet parameters are not in the reference's registration order")
            # "bf16x3" trains in split-bf16 (conv forward, data and weight gradients on the bf16 matrix cores, ~2^-16 per product), "bf16"
            # in one bf16 plane (one MFMA per product, fp32 accumulation)
            packed = self._packed_for(dt)
            sr, _tws = torch.ops.hrnet_hip.hrnet_forward_train(packed, lrs.float().contiguous(), alphas.float().contiguous(),
                                                               params, self._num_layers, bool(self.fuse.alpha_residual), dt,
                                                               self._scale)
            return sr
        if self.ensemble is not None and augment.check_mode(self.ensemble) is not None:
            return self._forward_ensemble_plain(lrs, alphas, self.ensemble)
        packed, dt = self.packed_parameters()
        return torch.ops.hrnet_hip.hrnet_forward(packed, dt, self._num_layers, bool(self.fuse.alpha_residual), lrs.detach(), alphas.detach(),
                                                 self._scale)

    def _forward_ref(self, lrs, alphas, ref):
        """forward with the reference frame given: the same routing as forward, on the *_ref ops"""
        if lrs.dim() != 4:
            raise ValueError(f"lrs must be (B, L, H, W); got {tuple(lrs.shape)}")
        ref = binding._ref_frame(ref, lrs)
        grad_params = self.training and any(p.requires_grad for p in self.parameters())
        grad_inputs = lrs.requires_grad or alphas.requires_grad or ref.requires_grad
        graph = torch.is_grad_enabled() and (grad_params or grad_inputs)
        if self.tile is not None and not graph and (lrs.shape[2] != lrs.shape[3] or lrs.shape[2] > self._tile_side(self.tile)):
            return self._forward_tiled_plain(lrs, alphas, self.tile, ensemble=self.ensemble, ref=ref)
        if lrs.shape[2] != lrs.shape[3]:
            raise ValueError("square low-res images only: the reference reinterprets (H,W) as (W,H) in its .view() "
                             "(HRNet.py:204), which is the identity only for H == W"
                             + ("" if graph else "; forward_tiled (or the `tile` attribute) takes scenes of any shape at inference"))
        if graph:
            names = [k for k, _ in self.named_parameters()]
            params = [p for _, p in self.named_parameters()]
            dt = self._train_dtype()
            if dt is None:
                if self._dtype() == binding.BF16:
                    raise NotImplementedError(
                        "HRNet(precision='bf16') without train_precision recomputes its forward in fp32 when a backward pass comes; that "
                        "path does not carry a reference frame.  Set train_precision ('fp32', 'bf16' or 'bf16x3') to train with ref=, or "
                        "call under no_grad / .eval() for inference.")
                dt = self._dtype()
            if names != binding.hrnet_param_names(self._num_layers):
                raise RuntimeError("HRNet parameters are not in the reference's registration order")
            packed = self._packed_for(dt)
            sr, _tws = torch.ops.hrnet_hip.hrnet_forward_train_ref(packed, lrs.float().contiguous(), alphas.float().contiguous(), ref,
                                                                   params, self._num_layers, bool(self.fuse.alpha_residual), dt,
                                                                   self._scale)
            return sr
        if self.ensemble is not None and augment.check_mode(self.ensemble) is not None:
            return self._forward_ensemble_plain(lrs, alphas, self.ensemble, ref=ref)
        packed, dt = self.packed_parameters()
        return torch.ops.hrnet_hip.hrnet_forward_ref(packed, dt, self._num_layers, bool(self.fuse.alpha_residual), lrs.detach(),
                                                     alphas.detach(), ref.detach(), self._scale)

    def _forward_ensemble_plain(self, lrs, alphas, mode="dihedral", members_per_pass=None, ref=None):
        """forward_ensemble without the global residual"""
        codes = augment.ensemble_codes(mode)
        K = len(codes)
        per_pass = K if members_per_pass is None else members_per_pass
        if not isinstance(per_pass, int) or not 1 <= per_pass <= K:
            raise ValueError(f"members_per_pass must be an integer in 1..{K}, got {members_per_pass!r}")
        if lrs.dim() != 4:
            raise ValueError(f"lrs must be (B, L, H, W); got {tuple(lrs.shape)}")
        if lrs.shape[2] != lrs.shape[3]:
            # the forward's restriction, not the ensemble's: the two kernels take non-square planes when no member transposes ("flip")
            raise ValueError(f"square low-res images only, as in forward (every member is one); got {tuple(lrs.shape)}")
        if tuple(alphas.shape) != tuple(lrs.shape[:2]):
            raise ValueError(f"alphas must be {tuple(lrs.shape[:2])}; got {tuple(alphas.shape)}")
        B, V, H, W = lrs.shape
        S = self._scale
        if ref is not None:
            ref = binding._ref_frame(ref, lrs)
        packed, dt = self.packed_parameters()
        with torch.no_grad():
            members = torch.ops.hrnet_hip.dihedral_expand(lrs.detach().float().contiguous(), codes)         # (K,B,V,H,W)
            refs = None if ref is None else torch.ops.hrnet_hip.dihedral_expand(ref.detach().view(B, 1, H, W), codes)      # (K,B,1,H,W)
            alphas = alphas.detach().float().contiguous()
            srs = torch.empty((K, B, 1, S * H, S * W), dtype=torch.float32, device=members.device)
            for k0 in range(0, K, per_pass):
                k1 = min(K, k0 + per_pass)
                binding.hrnet_forward(packed, dt, self._num_layers, self.fuse.alpha_residual, members[k0:k1].view(-1, V, H, W),
                                      alphas.repeat(k1 - k0, 1), out=srs[k0:k1].view(-1, 1, S * H, S * W), scale=S,
                                      ref=None if refs is None else refs[k0:k1].view(-1, H, W))
            return torch.ops.hrnet_hip.dihedral_mean(srs, codes)

    @staticmethod
    def _tile_side(tile):
        if isinstance(tile, bool) or not isinstance(tile, int) or tile < 1:
            raise ValueError(f"tile must be a positive integer, got {tile!r}")
        return tile

    def _forward_tiled_plain(self, lrs, alphas, tile=128, windows_per_pass=None, ensemble=None, members_per_pass=None, ref=None):
        """forward_tiled without the global residual"""
        tile = self._tile_side(tile)
        if lrs.dim() != 4 or lrs.numel() == 0:
            raise ValueError(f"lrs must be a non-empty (B, L, H, W); got {tuple(lrs.shape)}")
        if tuple(alphas.shape) != tuple(lrs.shape[:2]):
            raise ValueError(f"alphas must be {tuple(lrs.shape[:2])}; got {tuple(alphas.shape)}")
        mode = augment.check_mode(ensemble)
        B, V, H, W = lrs.shape
        S = self._scale
        if ref is not None:
            ref = binding._ref_frame(ref, lrs).detach()
        per_pass = max(1, 32 // B) if windows_per_pass is None else windows_per_pass
        if isinstance(per_pass, bool) or not isinstance(per_pass, int) or per_pass < 1:
            raise ValueError(f"windows_per_pass must be a positive integer, got {windows_per_pass!r}")
        codes = augment.ensemble_codes(mode) if mode is not None else None
        K = len(codes) if codes else 1
        m_pass = K if members_per_pass is None else members_per_pass
        if codes and (isinstance(m_pass, bool) or not isinstance(m_pass, int) or not 1 <= m_pass <= K):
            raise ValueError(f"members_per_pass must be an integer in 1..{K}, got {members_per_pass!r}")
        if H == W and H <= tile:
            if mode is not None:
                return self._forward_ensemble_plain(lrs, alphas, mode, members_per_pass, ref=ref)
            packed, dt = self.packed_parameters()
            if ref is not None:
                return torch.ops.hrnet_hip.hrnet_forward_ref(packed, dt, self._num_layers, bool(self.fuse.alpha_residual), lrs.detach(),
                                                             alphas.detach(), ref, S)
            return torch.ops.hrnet_hip.hrnet_forward(packed, dt, self._num_layers, bool(self.fuse.alpha_residual), lrs.detach(),
                                                     alphas.detach(), S)
        R = tiling.halo(self._num_layers, V)
        p = tiling.plan(H, W, tile, R)
        t, n = p.t, len(p.windows)
        packed, dt = self.packed_parameters()
        ops = torch.ops.hrnet_hip
        with torch.no_grad():
            lrs = lrs.detach().float().contiguous()
            alphas = alphas.detach().float().contiguous()
            out = torch.empty((B, 1, S * H, S * W), dtype=torch.float32, device=lrs.device)
            for w0 in range(0, n, per_pass):
                w1 = min(n, w0 + per_pass)
                c = w1 - w0
                wins = ops.tile_gather(lrs, t, R, w0, w1)                                                   # (c,B,V,t,t)
                rwin = None if ref is None else ops.tile_gather(ref.view(B, 1, H, W), t, R, w0, w1).view(-1, t, t)          # (c*B,t,t)
                a = alphas.repeat(c, 1)
                if codes is None:
                    srs = binding.hrnet_forward(packed, dt, self._num_layers, self.fuse.alpha_residual, wins.view(-1, V, t, t), a, scale=S,
                                                ref=rwin)
                else:                                                                                       # forward_ensemble on c * B samples
                    members = ops.dihedral_expand(wins.view(-1, V, t, t), codes)                            # (K,c*B,V,t,t)
                    rmem = None if rwin is None else ops.dihedral_expand(rwin.view(-1, 1, t, t), codes)      # (K,c*B,1,t,t)
                    srs = torch.empty((K, c * B, 1, S * t, S * t), dtype=torch.float32, device=lrs.device)
                    for k0 in range(0, K, m_pass):
                        k1 = min(K, k0 + m_pass)
                        binding.hrnet_forward(packed, dt, self._num_layers, self.fuse.alpha_residual, members[k0:k1].view(-1, V, t, t),
                                              a.repeat(k1 - k0, 1), out=srs[k0:k1].view(-1, 1, S * t, S * t), scale=S,
                                              ref=None if rmem is None else rmem[k0:k1].view(-1, t, t))
                    srs = ops.dihedral_mean(srs, codes)
                    del members, rmem
                ops.tile_scatter(out, srs.view(c, B, 1, S * t, S * t), t, R, S, w0, w1)
                del wins, srs                     # before the next chunk is allocated: one chunk at a time, as the bound says
            return out

    def _packed_f32(self):
        return self._packed_for(binding.F32)

    # -- staged access for parity tests / profiling (channels-last tensors in the storage dtype)
    def encode_views(self, lrs):
        packed, dt = self.packed_parameters()
        return binding.hrnet_encoder(packed, dt, self._num_layers, lrs)

    def fuse_views(self, emb, alphas):
        packed, dt = self.packed_parameters()
        return binding.hrnet_fuse(packed, dt, self._num_layers, self.fuse.alpha_residual, emb, alphas)

    def decode_state(self, fused):
        packed, dt = self.packed_parameters()
        return binding.hrnet_decoder(packed, dt, self._num_layers, fused, self._scale)
