"""Flip / rotate augmentation of the input pipeline: the eight symmetries of the square, one code per sample.  Pure Python,
no GPU and no native library: this module states the rule that hrn_io_collate_a (host path) and hrn_collate_device_a (HBM cache)
implement inside their gathers, it is the reference their tests compare against, and it lets a user undo a transform.  The
self-ensemble at test time (HRNet.forward_ensemble; hrn_dihedral_expand / hrn_dihedral_mean on the device) is stated here too:
`ensemble_codes`, `expand` and `mean_inverse`, which those kernels are compared against bit for bit.

A code t in 0..7 acts on the last two axes of a square array:

    if t & 4: x = x.transpose(-1, -2)
    if t & 2: x = x.flip(-2)          # rows
    if t & 1: x = x.flip(-1)          # columns

i.e. on a side-n square  out[i][j] = x[(j', i') if t & 4 else (i', j')]  with  i' = n-1-i if t & 2 else i  and
j' = n-1-j if t & 1 else j.  As rotations (torch.rot90 counts counter-clockwise): 0 identity, 3 rot 180, 5 rot 90 clockwise,
6 rot 90 counter-clockwise, 1 / 2 the mirror images left-right / up-down, 4 the transpose, 7 the anti-transpose.

The loaders draw one code per imageset with `np.random.randint(0, MODES[mode])` (DataLoader.py gives the place of that draw
in the RNG sequence) and apply it to the cropped window of every LR view and to the HR / SM windows alike, so the LR / HR
geometry of a sample, sub-pixel shifts included, stays that of a valid sample."""
import numpy as np

MODES = {"flip": 4, "dihedral": 8}        # mode -> number of codes drawn from: "flip" never transposes


def check_mode(mode):
    """Normalise an `augment` argument: None, False and "none" -> None (off), True -> "dihedral", a key of MODES -> itself;
    anything else is a ValueError."""
    if mode is None or mode is False or (isinstance(mode, str) and mode == "none"):
        return None
    if mode is True:
        return "dihedral"
    if isinstance(mode, str) and mode in MODES:
        return mode
    raise ValueError(f"augment must be None, False, True, 'none' or one of {sorted(MODES)}, got {mode!r}")


def check_code(code):
    code_int = int(code)
    if code_int != code or not 0 <= code_int <= 7:
        raise ValueError(f"augmentation code must be an integer in 0..7, got {code!r}")
    return code_int


def apply(x, code):
    """`x` (numpy array or torch tensor, at least 2-D, square in its last two axes when the code transposes) under `code`.
    Returns a view where the library gives one (numpy) or a new tensor (torch.flip copies)."""
    code = check_code(code)
    if x.ndim < 2:
        raise ValueError("apply needs at least two axes")
    is_numpy = isinstance(x, np.ndarray)
    if code & 4:
        if x.shape[-1] != x.shape[-2]:
            raise ValueError(f"codes 4..7 transpose: the last two axes must be equal, got {tuple(x.shape[-2:])}")
        x = np.swapaxes(x, -1, -2) if is_numpy else x.transpose(-1, -2)
    for bit, axis in ((2, -2), (1, -1)):
        if code & bit:
            x = np.flip(x, axis) if is_numpy else x.flip(axis)
    return x


def inverse(code):
    """The code that undoes `code`: apply(apply(x, c), inverse(c)) == x.  Every code is its own inverse except the two quarter
    turns, 5 and 6, which undo each other (with a transpose, the row flip of one is the column flip of the other)."""
    code = check_code(code)
    return {5: 6, 6: 5}.get(code, code)


# --------------------------------------------------------------------------- self-ensemble: the rule of hrn_dihedral_expand / _mean
def ensemble_codes(mode):
    """The members of a self-ensemble: [0, 1, 2, 3] for "flip", [0 .. 7] for "dihedral" (True).  A mode that `check_mode` refuses, or
    one that means "off", is a ValueError: an ensemble needs members."""
    mode = check_mode(mode)
    if mode is None:
        raise ValueError(f"an ensemble needs a mode, one of {sorted(MODES)}")
    return list(range(MODES[mode]))


def check_codes(codes):
    """A member list: 1..8 distinct codes in 0..7 -> list of int."""
    codes = [check_code(c) for c in codes]
    if not 1 <= len(codes) <= 8:
        raise ValueError(f"a member list holds 1..8 codes, got {len(codes)}")
    if len(set(codes)) != len(codes):
        raise ValueError(f"the codes of a member list must be distinct, got {codes}")
    return codes


def expand(x, codes):
    """x (..., H, W) -> (K, ..., H, W), member-major: out[k] = apply(x, codes[k])."""
    parts = [apply(x, c) for c in check_codes(codes)]
    if isinstance(x, np.ndarray):
        return np.stack(parts)
    import torch
    return torch.stack(parts)


def mean_inverse(y, codes):
    """y (K, ..., H, W) -> (..., H, W): every member transformed back and averaged, with the summation rule of hrn_dihedral_mean:

        m_k = apply(y[k], inverse(codes[k]));   out = r * ((..((m_0 + m_1) + m_2)..) + m_{K-1}),   r = 1 / K rounded to y's dtype

    adds in member order in y's own dtype, then ONE multiply - no division - so fp32 arrays give the kernel's bits."""
    codes = check_codes(codes)
    if len(y) != len(codes):
        raise ValueError(f"y has {len(y)} members for {len(codes)} codes")
    total = apply(y[0], inverse(codes[0]))
    for k in range(1, len(codes)):
        total = total + apply(y[k], inverse(codes[k]))
    if isinstance(y, np.ndarray):
        return total * y.dtype.type(1.0 / len(codes))
    import torch
    return total * torch.tensor(1.0 / len(codes), dtype=y.dtype).item()
