"""The depth-window dispatch table: Conv3d(3x3x3, pad 1) as the 2-D convolution kernels over the D slices of a [D + 2][C][H][W]
volume (include/uz_api.h, volumes section), the only call with more view channels (Cin = 3 C) than its buffer has (CinTot = C).

A case is (math mode, C, Cout, D, H, W) and, per direction, what the host-side queries of tests/_conv_routes.py answer for the 2-D
call the plans emit (unet_zoo_amd/_plan.py _conv_fwd / _conv_bwd):
  fwd    (Cin, Cout, N) = (3 C, Cout, D)   -> (route, parts, cot, bn)
  dgrad  (Cin, Cout, N) = (C, 3 Cout, D)   -> (route, parts, cot)      the dy volume read through a window of 3 Cout channels
  wgrad  (Cin, Cout, N) = (3 C, Cout, D)   -> (route, slabs)           weight-gradient target 256 (dispatch_state)
A direction a case does not claim is None.  tests/test_conv3d_routes_cpu.py pins the claims and proves that the cases tell the
five addressing defects below apart; tests/test_conv3d_routes_gpu.py runs every case with gpu=True.

The fp64 reference is F.conv3d / its two gradients on the (1, C, D, H, W) tensor.  The defects are wrong evaluations of that same
reference, one function each: what a kernel would compute if it addressed the window or the Conv3d parameter wrongly."""
import collections
import functools

import torch
import torch.nn.functional as F

from tests import _conv_routes as R

Vol = collections.namedtuple("Vol", "mode C Cout D H W fwd dgrad wgrad gpu")
DIRECTIONS = R.DIRECTIONS
_KEYS = {"fwd": ("route", "parts", "cot", "bn"), "dgrad": ("route", "parts", "cot"), "wgrad": ("route", "slabs")}


def V(mode, C, Cout, D, H, W, fwd=None, dgrad=None, wgrad=None, gpu=True):
    assert mode in (0, 1, 2, 3)
    claims = [None if v is None else dict(zip(_KEYS[d], v, strict=True)) for d, v in zip(DIRECTIONS, (fwd, dgrad, wgrad))]
    return Vol(mode, C, Cout, D, H, W, *claims, gpu)


def case_id(c):
    return f"m{c.mode}-{c.C}x{c.Cout}x{c.D}x{c.H}x{c.W}"


def directions(c):
    return [d for d in DIRECTIONS if getattr(c, d) is not None]


def as2d(c, direction):
    """The 2-D call of one direction as a case of tests/_conv_routes.py (what _check and case_id of the 2-D table take)."""
    cin, cout = (c.C, 3 * c.Cout) if direction == "dgrad" else (3 * c.C, c.Cout)
    return R.R(direction, c.mode, c.D, cin, cout, c.H, c.W, 3, gpu=c.gpu, **(getattr(c, direction) or {}))


def queries(L, c):
    """What the host-side queries answer per claimed direction in the current dispatch state (the caller enters dispatch_state)."""
    out = {}
    for d in directions(c):
        q = R.queries(L, as2d(c, d))
        out[d] = {k: q[k] for k in _KEYS[d]}
    return out


CASES = [
    # ---- fp32 MFMA kernels (conv_mfma.hip, conv_wgrad.hip): the window over the zero slices and across the images of a batch tile
    V(0, 5, 7, 1, 5, 3, (0, 1, 32, 0), (0, 1, 32), (0, 4)),                  # D = 1: both neighbours are the zero slices
    V(0, 6, 8, 2, 6, 10, (0, 1, 32, 0), (0, 1, 32), (0, 4)),                 # D = 2
    V(0, 5, 7, 3, 4, 4, (0, 1, 32, 0), (0, 1, 32), (0, 4)),                  # batch tiles (TB = 4) over 3 slices: the window crosses the images of one tile
    V(0, 5, 7, 5, 2, 2, (0, 1, 32, 0), (0, 1, 32), (0, 4)),                  # two batch tiles, the second ragged
    V(0, 2, 3, 140, 4, 4, (0, 1, 32, 0), (0, 1, 32), (0, 140)),              # 140 slabs > 64: two-stage reduce, then the volC write (conv_wgrad.hip wgrad_reduce_kernel)
    V(0, 23, 7, 2, 5, 3, (0, 1, 32, 0), (0, 1, 32), (0, 2)),                # added: 3 C = 69 > 64, the kd = 2 slab is cut by a channel tile of the fp32 kernels too (the rows below have that on the split path only)
    # ---- split-fp16 forced (mode 2): where kd falls in the 16-channel chunks of conv_split.hip, the weight-gradient tiles of conv_wgrad_split.hip
    V(2, 5, 7, 3, 13, 9, (1, 1, 32, 3), (1, 1, 32), (0, 12)),                # Kc = 15: all three kd in one chunk
    V(2, 6, 7, 3, 13, 9, (1, 1, 32, 3), (1, 1, 32), (0, 12)),                # Kc = 18: kd = 2 straddles the chunk boundary
    V(2, 11, 40, 3, 8, 32, (1, 1, 32, 6), (1, 2, 32), (1, 6)),               # Kc = 33 (K tail 1); 64-channel weight-gradient tile, ragged on both sides
    V(2, 4, 32, 3, 8, 32, (1, 1, 32, 6), (1, 2, 32), (1, 6)),                # Cin = 12 on the 32-channel weight-gradient tile
    V(2, 11, 40, 3, 16, 16, (1, 1, 32, 3), (1, 2, 32), (1, 6)),              # W = 16 tiles
    V(2, 5, 11, 1, 8, 32, (1, 1, 32, 2), (1, 1, 32), (1, 2)),                # D = 1 on the split kernels
    V(2, 27, 7, 3, 8, 32, (1, 2, 32, 0), (1, 1, 32), (1, 6)),                # forward chunk loop split in 2 over a window (Kc = 81)
    V(2, 22, 65, 2, 8, 32, (1, 1, 32, 4), (1, 4, 32), (1, 4)),               # dgrad split in 4; second ci tile holds 2 channels (kd = 2, ci 20..21); Cout overhang 1
    V(2, 3, 5, 70, 8, 32, (1, 1, 32, 140), (1, 1, 32), (1, 140)),            # split weight gradient with 140 slabs, Conv3d layout behind the group stage
    # ---- default policy (mode 1): the thresholds a volume meets
    V(1, 1, 32, 4, 128, 128, (2, 1, 32, 0), (0, 1, 32), (2, 256)),           # 1-channel volume: thin forward and thin weight gradient on a window (65 536 px)
    V(1, 1, 32, 3, 128, 128, (0, 1, 32, 0), (0, 1, 32), (0, 384)),           # ... one slice less: off the thin path
    V(1, 2, 64, 16, 128, 128, (1, 1, 32, 1024), (1, 1, 32), (0, 512)),       # the latent input (6 -> 64) at 262 144 px
    V(1, 2, 64, 15, 128, 128, (0, 1, 32, 0), (0, 1, 32), (0, 480), gpu=False),   # ... below it
    V(1, 4, 32, 32, 128, 128, (1, 1, 32, 2048), (1, 1, 32), (1, 256)),       # the image layer (12 -> 32) at 524 288 px: lomin
    V(1, 4, 32, 16, 128, 128, None, None, (0, 512), gpu=False),              # ... below it
    V(1, 22, 64, 8, 16, 16, (0, 1, 32, 0), (0, 4, 32), (1, 16)),             # 2 048 px = pxmin, W = 16
    V(1, 11, 33, 20, 16, 32, (1, 1, 32, 40), (0, 2, 32), (0, 160)),          # default policy on the 16 x 16 geometry
    V(1, 11, 33, 20, 16, 33, (0, 1, 64, 0), (0, 1, 32), (0, 160)),           # ... and off it
    V(1, 32, 32, 40, 16, 16, (1, 2, 32, 0), (1, 2, 32), (0, 160)),           # chunk split 2 in both directions under the default policy
    # ---- single-piece bf16 (mode 3)
    V(3, 22, 65, 16, 16, 128, (1, 1, 128, 128), (0, 1, 32), (1, 55)),        # 128-channel tile overhanging by 63
    V(3, 32, 16, 16, 16, 128, (0, 1, 32, 0), (1, 1, 32), (0, 256)),          # bf16 data gradient on a dy window (Kc = 48)
    V(3, 11, 32, 8, 128, 128, (1, 1, 32, 512), (0, 1, 32), (1, 128)),        # 32-channel weight-gradient tile
    V(3, 22, 65, 20, 16, 32, (1, 1, 32, 40), (0, 4, 32), (1, 32)),           # 16 x 16 geometry
]
GPU_CASES = [(i, c) for i, c in enumerate(CASES) if c.gpu]
# (index, case, direction) of everything the GPU tier runs
GPU_RUNS = [(i, c, d) for i, c in GPU_CASES for d in directions(c)]
# (math mode, direction, route) keys the 2-D table's GATE never needed: the fp32 MFMA kernels under another mode, compared with the
# un-rounded reference and gated as in mode 0
GATE_ALIAS = {(2, "wgrad", 0): (0, "wgrad", 0), (3, "fwd", 0): (0, "fwd", 0), (3, "wgrad", 0): (0, "wgrad", 0)}
# Keys gated for this table alone, at no more than 4x the worst ratio of the materialised 2-D twin on the MI355X (in the comment).
# (2, "wgrad", 1): the 2-D table meets the forced-split weight gradient from 32 768 pixels on (3e-8, 1.1e-8 observed); here a sum has
# 256 - 768 terms, and its error - a sum of signed per-product errors of at most 3 * 2^-22 |ab| = 7.2e-7 |ab| (split_f16.h) - averages
# out over that many fewer terms.  The twin, the same kernel on a real 3 C-channel tensor, is bit-equal and so shows the same ratio:
# the arithmetic at this term count is the cause, not the addressing.  The gate stays under the worst-case bound of one product.
WINDOW_GATE = {
    (2, "wgrad", 1): 4e-7,       # 1.3e-7 (m2-22x65x2x8x32: 512 terms)
}
PROOF_SLICES = 4        # the cases of 262 144 px or more are proved on their first four slices (an fp64 Conv3d of the whole case is slow on a CPU)


# ----------------------------------------------------------------------------- operands
def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _act(shape, seed, nonneg):
    """[D][C][H][W]: the structure of test_conv_routes_gpu._act (an offset block of rows, one quiet channel at 2^-12, non-negative in
    every other case) and a depth ramp, so that no two slices look alike to a window that starts one slice off."""
    D, C, H, W = shape
    t = _rnd(*shape, seed=seed)
    r0 = H // 4
    t[:, :, r0:r0 + max(1, H // 4)] += 3.0
    if C > 1:
        t[:, 1] *= 2.0 ** -12
    if nonneg:
        t = torch.relu(t)
    return t * (1.0 + 0.5 * torch.arange(D, dtype=torch.float32) / D)[:, None, None, None]


_KD = torch.tensor([0.6, 1.0, 1.5])     # no symmetry in kd: the three depth taps differ in scale as well as in value


@functools.lru_cache(maxsize=None)
def _operands(idx):
    c = CASES[idx]
    C, Co, D, H, W = c.C, c.Cout, c.D, c.H, c.W
    nonneg = idx % 2 == 1
    ops = {}
    w = _rnd(Co, C, 3, 3, 3, seed=2000 + idx, scale=1.0 / (27 * C) ** 0.5) * _KD[None, None, :, None, None]
    w[0] -= w[0].mean()                              # output channel 0 cancels on the offset block
    ops["fwd"] = (_act((D, C, H, W), 1000 + idx, nonneg), w)
    wd = _rnd(Co, C, 3, 3, 3, seed=5000 + idx, scale=1.0 / (27 * Co) ** 0.5) * _KD[None, None, :, None, None]
    wd[:, 0] -= wd[:, 0].mean()                      # input channel 0 of the gradient cancels on the offset block
    ops["dgrad"] = (_act((D, Co, H, W), 4000 + idx, nonneg), wd)
    dy = _rnd(D, Co, H, W, seed=8000 + idx)
    if Co > 1:
        dy[:, Co - 1] *= 2.0 ** -12
    ops["wgrad"] = (_act((D, C, H, W), 7000 + idx, nonneg), dy)
    ops["bias"] = _rnd(Co, seed=3000 + idx)
    ops["prev"] = _rnd(D, C, H, W, seed=6000 + idx)
    return ops


def operands(idx, direction):
    """(a, b) fp32 on the CPU, shared and not to be written to: fwd (x [D][C][H][W], w [Cout][C][3][3][3]), dgrad (dy [D][Cout][H][W],
    w), wgrad (x, dy).  direction "bias" / "prev": the forward's bias, the tensor the data gradient accumulates onto."""
    return _operands(idx)[direction]


def rounds_operands(c, direction):
    """Mode 3 on route 1 multiplies RNE-bf16 operands; everything else is compared with the un-rounded fp64 sum."""
    return c.mode == 3 and getattr(c, direction)["route"] == 1


def _bf16(t):
    return t.to(torch.bfloat16).float()


def ref_operands(idx, direction, slices=None):
    """The operands as the reference sees them: fp64, bf16-rounded first where the kernel rounds, cut to the first `slices` slices."""
    c = CASES[idx]
    a, b = operands(idx, direction)
    if rounds_operands(c, direction):
        a, b = _bf16(a), _bf16(b)
    if slices is not None and slices < c.D:
        a = a[:slices]
        b = b[:slices] if direction == "wgrad" else b
    return a.double(), b.double()


# ----------------------------------------------------------------------------- the fp64 reference
def _v5(t):          # [D][C][H][W] -> (1, C, D, H, W)
    return t.permute(1, 0, 2, 3)[None]


def _v4(t):
    return t[0].permute(1, 0, 2, 3)


def conv3d(direction, a, b):
    """fwd: y [D][Cout][H][W] of (x, w); dgrad: dx [D][C][H][W] of (dy, w); wgrad: dw [Cout][C][3][3][3] of (x, dy).  No bias."""
    if direction == "fwd":
        return _v4(F.conv3d(_v5(a), b, None, padding=1))
    if direction == "dgrad":
        return _v4(F.conv_transpose3d(_v5(a), b, None, padding=1))
    wshape = (b.shape[1], a.shape[1], 3, 3, 3)
    return torch.nn.grad.conv3d_weight(_v5(a), wshape, _v5(b), padding=1)


def terms(c, direction):
    return {"fwd": 27 * c.C, "dgrad": 27 * c.Cout, "wgrad": c.D * c.H * c.W}[direction]


def floor_of(c, direction, a, b, slices=None):
    T = terms(c, direction) if slices is None or direction != "wgrad" else min(slices, c.D) * c.H * c.W
    return 2.0 ** -39 * float(a.abs().max()) * float(b.abs().max()) * T


@functools.lru_cache(maxsize=None)
def reference(idx, direction):
    """(ref, den, floor) of a case: the fp64 result, the same operation on |a|, |b|, and the absolute floor of test_conv_routes_gpu.
    Computed once and shared: do not write to the tensors."""
    a, b = ref_operands(idx, direction)
    return conv3d(direction, a, b), conv3d(direction, a.abs(), b.abs()), floor_of(CASES[idx], direction, a, b)


# ----------------------------------------------------------------------------- wrong evaluations of the same reference
def _next_slice(t):
    """Slice d of the result is slice d + 1 of t; behind the last one comes the zero slice."""
    s = torch.zeros_like(t)
    s[:-1] = t[1:]
    return s


def _without_kd(w, kd):
    w = w.clone()
    w[:, :, kd] = 0
    return w


def _kd_major(w):
    """The [co][ci][kd] parameter's memory read as [co][kd][ci]: element (co, ci, kd) comes from flat position kd C + ci."""
    Co, C = w.shape[:2]
    return w.reshape(Co, 3, C, 3, 3).permute(0, 2, 1, 3, 4)


def defect_kd_flipped(direction, a, b):
    """1: kd flipped in the forward and the weight gradient, not flipped in the data gradient (whose window runs kd = 2 - j)."""
    if direction == "wgrad":
        return conv3d(direction, a, b).flip(2)
    return conv3d(direction, a, b.flip(2))


def defect_window_starts_at_d(direction, a, b):
    """2: the window starts at slice d instead of d - 1 (the window is over x in fwd / wgrad, over dy in dgrad)."""
    return conv3d(direction, _next_slice(a), b)


def defect_next_slice_zero(direction, a, b):
    """3: slice d + 1 reads as zeros - a buffer resource sized with CinTot ends behind slice d.  That slice meets kd = 2 in the
    forward and the weight gradient, j = 2 (kd = 0) in the data gradient."""
    if direction == "wgrad":
        return _without_kd(conv3d(direction, a, b), 2)
    return conv3d(direction, a, _without_kd(b, 2 if direction == "fwd" else 0))


def defect_weight_read_kd_major(direction, a, b):
    """4: the weight read as [co][kd][ci] where the parameter is [co][ci][kd] (forward and data gradient)."""
    return None if direction == "wgrad" else conv3d(direction, a, _kd_major(b))


def defect_wgrad_written_kd_major(direction, a, b):
    """5: the weight gradient written as [co][kd][ci] into the Conv3d-shaped tensor."""
    if direction != "wgrad":
        return None
    dw = conv3d(direction, a, b)
    return dw.permute(0, 2, 1, 3, 4).reshape(dw.shape)


DEFECTS = {1: defect_kd_flipped, 2: defect_window_starts_at_d, 3: defect_next_slice_zero, 4: defect_weight_read_kd_major,
           5: defect_wgrad_written_kd_major}


def defect_is_identity(n, c, direction):
    """Where a defect is no defect: with D = 1 only the centre tap meets a real slice, so zeroing slice d + 1 (3) or flipping kd (1)
    changes nothing; with C = 1 the layouts [co][ci][kd] and [co][kd][ci] are the same memory (4, 5).  The CPU test asserts that
    the defective evaluation EQUALS the true one there, so these are facts about the operation and not holes in the table."""
    return (c.D == 1 and n in (1, 3)) or (c.C == 1 and n in (4, 5))


def defects_of(direction):
    return [n for n in DEFECTS if (n != 4 or direction != "wgrad") and (n != 5 or direction == "wgrad")]
