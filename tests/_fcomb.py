"""Shared by tests/test_fcomb_cpu.py and tests/test_fcomb_gpu.py: the op-level cases of uz_fcomb_sample_fwd (csrc/fcomb.hip) with
their inputs, a direct fp64 evaluation, an fp32 torch-CPU evaluation (what the logit gate is derived from) and a numpy twin in
the kernel's own decomposition; and the model-level cases of ProbabilisticUnet.predict with the CPU oracle's answer.  Everything
is computed once per process and read-only."""
import contextlib
import ctypes as C
import functools
import json
import os
import types

import numpy as np

from tests import _golden as G

FC = 32                                                                # feature / hidden channels, fixed by the model
BN_EPS = 1e-3                                                          # the model's (torchlayers.py:20)
CANARY = -777.0

# ---- the issue's op-level values
PLANES = ((1, 1), (7, 9), (16, 16), (1, 257), (64, 64))               # H*W = 1, 63, 256, 257, 64*64
BS = ((1, 1), (1, 17), (3, 2))
ROUTE_PROBE_S = 17                                                     # the S whose samples-per-workgroup the three extra S sit around
KS, LS, UNITS, CTOTS = (1, 2, 3, 8), (1, 2, 6), (1, 2, 3), (32, 38)
# six cases per plane - the three (B, S) and S one below / at / one above the route's samples per workgroup -, the other values
# rotated through them so that every value meets every plane; the fifth case starts every device buffer one float off 16 bytes
_ROT = dict(K=(1, 2, 3, 8, 2, 3), L=(1, 2, 6, 6, 1, 2), U=(1, 2, 3, 3, 2, 1), Ctot=(32, 38, 32, 38, 38, 32), shift=(0, 0, 0, 0, 1, 0))
# ... and the sizes at which the launch changes kernel: two pixels per thread once that still gives 256 workgroups.  On the
# 257-pixel plane (one pixel block, B = 1, four samples per workgroup) that is S = 1021: 1020 is the last one-pixel launch, 1021
# the first pair launch, with a ragged last sample group and a second pixel of every thread but one beyond the plane; 64 x 64 at
# B = 3, S = 44 is a pair launch of eight pixel blocks.
# The kernel walks its samples in chunks of 8 whose z terms share one LDS array: with 512 pixel workgroups (B = 512 on the 63-pixel
# plane) the samples are not split, so S = 7, 8, 9 are one below, at and one above a chunk and 13 is a full chunk and a ragged
# one; B = 256, S = 26 is two sample groups of 13.  The route gives these to the pair kernel; px = 1 forces the one-pixel kernel
# onto the same inputs (UZ_FCOMB_PX, the only way to more than four samples per workgroup there), px = 2 the pair kernel onto one
# small case of every plane.  px = 0 everywhere else: the route's own choice, with the variable unset.
EXTRA = (dict(H=1, W=257, B=1, S=1020, K=2, L=2, U=2, Ctot=32, shift=0, px=0, ppw=256, spw=4),
         dict(H=1, W=257, B=1, S=1021, K=3, L=6, U=3, Ctot=38, shift=1, px=0, ppw=512, spw=4),
         dict(H=64, W=64, B=3, S=44, K=8, L=1, U=2, Ctot=38, shift=0, px=0, ppw=512, spw=4))
EXTRA += tuple(dict(H=7, W=9, B=512, S=S, K=2, L=2, U=2, Ctot=32, shift=0, px=px, ppw=256 if px == 1 else 512, spw=S)
               for S in (7, 8, 9, 13) for px in (0, 1))
EXTRA += tuple(dict(H=7, W=9, B=256, S=26, K=3, L=6, U=3, Ctot=38, shift=1, px=px, ppw=256 if px == 1 else 512, spw=13) for px in (0, 1))
EXTRA += tuple(dict(H=H, W=W, B=1, S=2, K=2, L=2, U=2, Ctot=38, shift=0, px=2, ppw=512, spw=2) for H, W in PLANES)
CHUNK = 8                                                              # samples per z-term chunk of the kernel

# Logits: no gate in the project to borrow.  Measured on the op-level cases below: an fp32 torch-CPU evaluation of the same chain
# (cat, conv2d, eval batch_norm, relu; logits_f32_error, asserted in test_fcomb_cpu.py to stay at this figure) is within 1.35e-6 of
# fp64 (measured 1.340e-6, on the B = 512 cases, whose logits reach 5.3; 8.50e-7 over the cases with logits up to 3.6); the device adds
# in another order, so the gate is 4 x that.
LOGITS_F32_ERROR = 1.35e-6
LOGITS_TOL = 4 * LOGITS_F32_ERROR


@contextlib.contextmanager
def forced_px(px):
    """UZ_FCOMB_PX for the calls inside (the library reads it at every call): 1 or 2 forces that many pixels per thread, 0 unsets
    the variable - whatever the process was started with is put back afterwards, so no claim depends on it."""
    old = os.environ.pop("UZ_FCOMB_PX", None)
    if px:
        os.environ["UZ_FCOMB_PX"] = str(px)
    try:
        yield
    finally:
        os.environ.pop("UZ_FCOMB_PX", None)
        if old is not None:
            os.environ["UZ_FCOMB_PX"] = old


def route(L, K, U, B, S, H, W, px=0):
    """uz_fcomb_sample_route -> (pixels per workgroup, samples per workgroup, grid x, y, z)."""
    from unet_zoo_amd import _ffi
    o = (C.c_int * 5)()
    with forced_px(px):
        rc = _ffi.lib().uz_fcomb_sample_route(L, K, U, B, S, H, W, o)
    assert rc == 0, _ffi.lib().uz_last_error()
    return tuple(o)


def case_route(c):
    return route(c.L, c.K, c.U, c.B, c.S, c.H, c.W, c.px)


def extra_case(e):
    return types.SimpleNamespace(**{k: v for k, v in e.items() if k not in ("ppw", "spw")})


@functools.lru_cache(maxsize=None)
def cases(H, W):
    """The op-level cases of one plane as namespaces (H, W, B, S, K, L, U, Ctot, shift, px)."""
    out = []
    for i in range(6):
        K, L, U = _ROT["K"][i], _ROT["L"][i], _ROT["U"][i]
        if i < 3:
            B, S = BS[i]
        else:
            B, S = 1, route(L, K, U, 1, ROUTE_PROBE_S, H, W)[1] + (i - 4)
        out.append(types.SimpleNamespace(H=H, W=W, B=B, S=S, K=K, L=L, U=U, Ctot=_ROT["Ctot"][i], shift=_ROT["shift"][i], px=0))
    out += [extra_case(e) for e in EXTRA if (e["H"], e["W"]) == (H, W)]
    return tuple(out)


def case_key(c):
    """What the inputs and the reference of a case depend on (px only chooses the kernel: such cases share both)."""
    return (c.H, c.W, c.B, c.S, c.K, c.L, c.U, c.Ctot, c.shift)


def case_id(c):
    return case_key(c) + (c.px,)


def _inputs(c):
    rng = np.random.Generator(np.random.PCG64(list(case_key(c))))
    f32 = np.float32
    d = dict(feat=rng.standard_normal((c.B, FC, c.H, c.W)).astype(f32), eps=rng.standard_normal((c.S * c.B, c.L)).astype(f32),
             mu=rng.standard_normal((c.B, c.L)).astype(f32), sigma=rng.uniform(0.2, 1.2, (c.B, c.L)).astype(f32), units=[])
    for u in range(c.U):
        cin = FC + c.L if u == 0 else FC
        d["units"].append(dict(w=(rng.standard_normal((FC, cin)) / np.sqrt(cin)).astype(f32), b=(rng.standard_normal(FC) / np.sqrt(cin)).astype(f32),
                               gamma=rng.uniform(0.5, 1.5, FC).astype(f32), beta=rng.uniform(-0.5, 0.5, FC).astype(f32),
                               rm=rng.uniform(-0.5, 0.5, FC).astype(f32), rv=rng.uniform(0.5, 2.0, FC).astype(f32)))
    d["w_last"] = (rng.standard_normal((c.K, FC)) / np.sqrt(FC)).astype(f32)
    d["b_last"] = (rng.standard_normal(c.K) / np.sqrt(FC)).astype(f32)
    return d


def _conv1x1(w, x):
    """(O, C) x (N, C, H, W) -> (N, O, H, W) at the operands' precision (BLAS: the sums are not in channel order)."""
    return np.tensordot(w, x, axes=([1], [1])).transpose(1, 0, 2, 3)


def fcomb_f64(c, d, drop_bn=False, swap=None):
    """Fcomb in eval mode evaluated directly in fp64: (z (S*B, L), logits (S*B, K, H, W), per unit the pre-ReLU activations).
    drop_bn skips every BatchNorm; swap = (u, v) gives unit u the statistics of unit v and the reverse."""
    f = np.float64
    mu, sg, eps = d["mu"].astype(f), d["sigma"].astype(f), d["eps"].astype(f)
    z = np.tile(mu, (c.S, 1)) + np.tile(sg, (c.S, 1)) * eps
    x = np.concatenate([np.tile(d["feat"].astype(f), (c.S, 1, 1, 1)), np.broadcast_to(z[:, :, None, None], (c.S * c.B, c.L, c.H, c.W))], axis=1)
    order = list(range(c.U))
    if swap is not None:
        order[swap[0]], order[swap[1]] = order[swap[1]], order[swap[0]]
    pre = []
    for u in range(c.U):
        p, s = d["units"][u], d["units"][order[u]]
        y = _conv1x1(p["w"].astype(f), x) + p["b"].astype(f)[None, :, None, None]
        if not drop_bn:
            rstd = 1.0 / np.sqrt(s["rv"].astype(f) + BN_EPS)
            y = ((y - s["rm"].astype(f)[None, :, None, None]) * rstd[None, :, None, None] * p["gamma"].astype(f)[None, :, None, None]
                 + p["beta"].astype(f)[None, :, None, None])
        pre.append(y)
        x = np.maximum(y, 0.0)
    logits = _conv1x1(d["w_last"].astype(f), x) + d["b_last"].astype(f)[None, :, None, None]
    return z, logits, pre


def fcomb_twin(c, d):
    """uz_fcomb_sample_fwd in numpy, fp32 throughout and in the kernel's decomposition: base = W0[:, :32] f + b0 once per image, the
    z term W0[:, 32:] z once per (sample, image), then per sample BatchNorm as (y - rm) * rstd * gamma + beta with
    rstd = 1 / sqrt(rv + eps), ReLU, the 32 x 32 units and the head.  -> (z, logits) fp32."""
    f32 = np.float32
    u0 = d["units"][0]
    base = _conv1x1(u0["w"][:, :FC], d["feat"]).astype(f32) + u0["b"][None, :, None, None]
    z = (np.tile(d["mu"], (c.S, 1)) + np.tile(d["sigma"], (c.S, 1)) * d["eps"]).astype(f32)
    zt = (z @ u0["w"][:, FC:].T).astype(f32)                                           # (S*B, 32)
    x = np.tile(base, (c.S, 1, 1, 1)) + zt[:, :, None, None]
    for u in range(c.U):
        p = d["units"][u]
        if u:
            x = _conv1x1(p["w"], x).astype(f32) + p["b"][None, :, None, None]
        rstd = (f32(1.0) / np.sqrt(p["rv"] + f32(BN_EPS))).astype(f32)
        x = (x - p["rm"][None, :, None, None]) * rstd[None, :, None, None] * p["gamma"][None, :, None, None] + p["beta"][None, :, None, None]
        x = np.maximum(x, f32(0)).astype(f32)
    logits = _conv1x1(d["w_last"], x).astype(f32) + d["b_last"][None, :, None, None]
    return z, logits.astype(f32)


def logits_f32_error(c, d, ref_logits):
    """max |fp32 torch-CPU evaluation - fp64| of the logits of one case: what LOGITS_TOL is derived from."""
    import torch
    import torch.nn.functional as F
    def t(a):
        return torch.from_numpy(np.array(a))                           # (the shared inputs are read-only)
    z = t(d["mu"]).repeat(c.S, 1) + t(d["sigma"]).repeat(c.S, 1) * t(d["eps"])
    x = torch.cat([t(d["feat"]).repeat(c.S, 1, 1, 1), z[:, :, None, None].expand(c.S * c.B, c.L, c.H, c.W)], dim=1)
    for p in d["units"]:
        x = F.conv2d(x, t(p["w"])[:, :, None, None], t(p["b"]))
        x = F.relu(F.batch_norm(x, t(p["rm"]), t(p["rv"]), t(p["gamma"]), t(p["beta"]), training=False, eps=BN_EPS))
    y = F.conv2d(x, t(d["w_last"])[:, :, None, None], t(d["b_last"]))
    return G.maxabs(y.numpy(), ref_logits)


@functools.lru_cache(maxsize=None)
def _case_data(key):
    c = types.SimpleNamespace(**dict(zip(("H", "W", "B", "S", "K", "L", "U", "Ctot", "shift"), key)))
    d = _inputs(c)
    z, logits, pre = fcomb_f64(c, d)
    live = [(bool((p > 0).any()), bool((p < 0).any())) for p in pre]
    for a in [d["feat"], d["eps"], d["mu"], d["sigma"], d["w_last"], d["b_last"], z, logits] + [v for p in d["units"] for v in p.values()]:
        a.setflags(write=False)
    return d, types.SimpleNamespace(z=z, logits=logits, live=live)


def case_data(c):
    """(inputs, fp64 reference with .z, .logits and per unit (some pre-ReLU value > 0, some < 0)) of one op-level case."""
    return _case_data(case_key(c))


def z_tol(d, c):
    """One rounded multiply-add: 2^-23 (|mu| + |sigma eps|), elementwise (S*B, L)."""
    return 2.0 ** -23 * (np.abs(np.tile(d["mu"], (c.S, 1)).astype(np.float64))
                         + np.abs(np.tile(d["sigma"], (c.S, 1)).astype(np.float64) * d["eps"].astype(np.float64)))


# ------------------------------------------------------------------------------------------ model level
with open(os.path.join(G.GOLDEN, "probunet_small.json")) as _f:
    _META = json.load(_f)
FILTERS, LATENT = _META["filters"], _META["latent_dim"]
H0 = 2 ** (len(FILTERS) - 1)                                           # six poolings: 64 puts the deepest plane at 1 x 1
SHAPES = ((1, 4, H0, H0), (3, 2, H0, H0), (2, 3, H0, 2 * H0))         # (B, S, H, W)
NO_CONVS = (3, 4)
LOGIT_TOL_MODEL = 1e-4                                                 # the project's logit gate
MARGIN = 2e-4                                                          # labels are compared where the oracle's top two logits differ by more
# seeds of the synthetic batch per (no_convs_fcomb, shape): ones for which the oracle leaves no pixel within MARGIN of a tie and
# half of the S*B label maps come out as either class (the deterministic weights give nearly flat maps; test_fcomb_cpu.py asserts both)
DATA_SEEDS = {(3, SHAPES[0]): 83, (3, SHAPES[1]): 85, (3, SHAPES[2]): 87, (4, SHAPES[0]): 77, (4, SHAPES[1]): 83, (4, SHAPES[2]): 81}


def model_state(no_convs, seed=1236):
    import torch
    import oracle
    from unet_zoo_amd.models.probabilistic_unet import probunet_spec
    sd = oracle.deterministic_state_dict(probunet_spec(1, 2, FILTERS, LATENT, no_convs), seed=seed + no_convs)
    for k, v in sd.items():                                             # eval-mode BatchNorm far from the identity
        n = torch.arange(v.numel(), dtype=torch.float32).reshape(v.shape)
        if k.endswith("running_mean"):
            v += 0.3 * torch.cos(1.7 * n + 0.3)
        elif k.endswith("running_var"):
            v *= 1.0 + 0.6 * torch.sin(2.3 * n + 1.1)
    return sd


@functools.lru_cache(maxsize=None)
def model_case(no_convs, B, S, H, W):
    """State dict, patch, eps (S*B, L) and the CPU oracle's mu, sigma, z and logits (S*B, K, H, W) of one model-level case."""
    import torch
    import oracle
    from oracle import refgraph as R
    sd = model_state(no_convs)
    x, _, eps = oracle.synthetic_batch(B, H, W, seed=DATA_SEEDS[(no_convs, (B, S, H, W))], eps_shapes=[(S * B, LATENT)])
    patch, e = torch.from_numpy(x), torch.from_numpy(eps[0])
    with torch.no_grad():
        out = R.probunet_forward(sd, patch, None, bn_train=False)
        z = out["prior_mu"].repeat(S, 1) + out["prior_sigma"].repeat(S, 1) * e
        logits = R.probunet_fcomb(sd, out["unet_features"].repeat(S, 1, 1, 1), z, bn_train=False)
    top = torch.sort(logits, dim=1).values
    sure = (top[:, -1] - top[:, -2]) > MARGIN                           # (S*B, H, W)
    return types.SimpleNamespace(sd=sd, patch=patch, eps=e, mu=out["prior_mu"], sigma=out["prior_sigma"], z=z, logits=logits,
                                 labels=torch.argmax(logits, dim=1), sure=sure)
