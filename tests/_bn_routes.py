"""The BatchNorm dispatch table: cases on both sides of every size limit of csrc/bn.hip (small_ept 512 | 513 and 2048 | 2049,
SMALL_LIMIT 4096, MID_HALF_LIMIT 8192, MID_LIMIT 32768, CHUNK 16384, reduction_groups' images per workgroup), each with the route it
claims, stated only through the library's host-side query uz_bn_route - the function the entry points themselves dispatch on.

A case is (N, C, H, W), training, `off` (floats between a 256-byte boundary and the start of every buffer a view lives in: 1 breaks
the 16-byte alignment the float4 kernels need), the storage (fp32, or bf16 for the *_b16 entry points), options and the claims
  fwd / bwd = (path, instance, parts, nb, ngrp, vec)
with path 0 small / 1 mid / 2 large / 3 large with bf16 storage, instance = elements per thread (small) or threads per workgroup
(mid), parts = chunks per plane, nb x ngrp = images per reduction workgroup x image groups, vec = the float4 instance.  The claims
hold with UZ_BN_MID, UZ_BN_MID_FWD and UZ_BN_MID_HALF unset (each read once per process).

Operands are those of tests/test_ops_gpu.py::test_bn_relu_fwd_bwd (y = randn * 2 + 0.7, gamma = |randn| + 0.5, beta = 0.3 randn),
and the reference is fp64 tensor arithmetic on them.  The ReLU knife edge: the kernels' mask is fmaf(y, alpha, beta') > 0 in fp32,
the reference's is fp64, and a pre-activation within rounding of zero may fall on either side - so the incoming gradient dA is set
to 0 wherever the fp64 pre-activation has |o| < RELU_EDGE.  dz is then 0 whichever way the mask falls, every element is still
compared and every other element still exercises the mask.  At most RELU_EDGE_SHARE of a case's elements may be zeroed that way
(expected 2e-4 at gamma >= 0.5 and unit variance); a case that exceeds it gets another seed offset, the cap stays.
tests/test_bn_routes_cpu.py checks claims and cap; tests/test_bn_routes_gpu.py runs every case against the reference."""
import collections
import ctypes
import functools

import torch


class Case(collections.namedtuple("Case", "N C H W training off b16 seed opt claims")):
    """opt: sorted (name, value) pairs (hashable: the operands and the reference of a case are cached); claims: (direction, route) pairs."""
    __slots__ = ()

    def o(self, name):
        return dict(self.opt).get(name)


SMALL, MID, LARGE, LARGE_ST = 0, 1, 2, 3
F_CONV_PARTIALS, F_OUT_PACKED, F_DBIAS_PARTIALS, F_SLABS, F_B16 = 1, 2, 4, 8, 16
EPS, MOMENTUM = 1e-3, 0.01
RELU_EDGE, RELU_EDGE_SHARE = 1e-4, 1e-3
C0 = 1                        # first channel of every view; the buffers hold C + 2 channels
SWITCHES = ("UZ_BN_MID", "UZ_BN_MID_FWD", "UZ_BN_MID_HALF")


def small(ept):
    return (SMALL, ept, 1, 0, 0, 0)


def mid(nt):
    return (MID, nt, 1, 0, 0, 1)


def large(parts, nb, ngrp, vec, st=False):
    return (LARGE_ST if st else LARGE, 0, parts, nb, ngrp, vec)


def B(N, H, W, fwd, bwd="same", C=3, training=1, off=0, b16=0, seed=0, **opt):
    claims = [("fwd", fwd)]
    if training:
        claims.append(("bwd", fwd if bwd == "same" else bwd))
    return Case(N, C, H, W, training, off, b16, seed, tuple(sorted(opt.items())), tuple(claims))


def case_id(c):
    x = "".join(f"-{k}{v}" for k, v in c.opt)
    return f"{c.N}x{c.C}x{c.H}x{c.W}" + ("" if c.training else "-eval") + (f"-off{c.off}" if c.off else "") + ("-b16" if c.b16 else "") + x


def aligned(c):
    """Whether the views of the case - channels [C0, C0 + C) of a buffer `off` floats past a 256-byte boundary - start on 16-byte boundaries."""
    return (c.off + C0 * c.H * c.W) % 4 == 0


def query(L, c, direction, flags=0):
    out = (ctypes.c_int * 6)()
    rc = L.uz_bn_route(direction, c.N, c.C, c.H, c.W, c.training if direction == 0 else 1, int(aligned(c)), flags | (F_B16 if c.b16 else 0), out)
    assert rc == 0, L.uz_last_error()
    return tuple(out)


def queries(L, c):
    return tuple((k, query(L, c, 0 if k == "fwd" else 1)) for k, _ in c.claims)


CASES = [
    # ---- small_ept 2 | 8 (512 | 513 values per channel); 1 x 27 x 19 is also the batch of one
    B(2, 16, 16, small(2)), B(1, 27, 19, small(8)),
    # ---- small_ept 8 | 16 (2048 | 2049)
    B(2, 32, 32, small(8)), B(3, 1, 683, small(16)),
    # ---- SMALL_LIMIT with H W % 4 == 0: 4096 small | 4100 the 512-thread mid instance (hw4 = 41: a thread's float4 index crosses images)
    B(4, 32, 32, small(16)), B(25, 2, 82, mid(512)),
    # ---- SMALL_LIMIT with H W % 4 != 0: 4097 goes to the scalar large path
    B(1, 17, 241, large(1, 1, 1, 0)),
    # ---- MID_HALF_LIMIT: 8192 <512, 4> | 8196 <1024, 8>
    B(8, 32, 32, mid(512)), B(3, 4, 683, mid(1024)),
    # ---- MID_LIMIT: 32768 mid | 32772 large
    B(8, 64, 64, mid(1024)), B(3, 4, 2731, large(1, 1, 3, 1)),
    # ---- a mid size whose views start 4 bytes past a 16-byte boundary: scalar large path (workspace required)
    B(8, 32, 32, large(1, 1, 8, 0), off=1),
    # ---- eval mode at a mid size: the large apply pass alone
    B(8, 32, 32, large(1, 1, 8, 1), training=0), B(3, 4, 683, large(1, 1, 3, 1), training=0),
    # ---- CHUNK = 16384: one chunk exactly | two chunks, the last of 4 (float4) | two chunks, the last of 1 (scalar)
    B(3, 128, 128, large(1, 1, 3, 1)), B(3, 68, 241, large(2, 1, 3, 1)), B(3, 145, 113, large(2, 1, 3, 0)),
    # ---- reduction_groups: nb = 2 with a ragged last group (9 = 4 x 2 + 1), nb = 8 with a last group of one image (17 = 2 x 8 + 1), scalar;
    # nb = 2 on the float4 kernels.  The largest cases (2 - 8 M floats): relu = 1 and the plain entry points only
    B(9, 27, 17, large(1, 2, 5, 0), C=512, big=1), B(17, 27, 9, large(1, 8, 3, 0), C=1024, big=1), B(17, 4, 482, large(1, 2, 9, 1), C=256, big=1),
    # ---- the minimum batch; one value per channel (refused in training mode before any launch)
    B(2, 1, 1, small(2)), B(1, 1, 1, small(2), refused=1),
    # ---- null gamma, beta and running buffers, one case per path
    B(2, 32, 32, small(8), null=1), B(8, 32, 32, mid(512), null=1), B(3, 68, 241, large(2, 1, 3, 1), null=1),
    # ---- C = 1 and C = 5 on every path: the ceil(C / 4) grid of chan_partial_sum and the one-channel grids
    B(1, 27, 19, small(8), C=1), B(25, 2, 82, mid(512), C=1), B(3, 68, 241, large(2, 1, 3, 1), C=1),
    B(2, 32, 32, small(8), C=5), B(3, 4, 683, mid(1024), C=5), B(3, 145, 113, large(2, 1, 3, 0), C=5),
    # ---- bf16 storage (*_b16): the smallest legal size, two chunks, and nb > 1
    B(3, 4, 2731, large(1, 1, 3, 1, st=True), b16=1), B(3, 68, 241, large(2, 1, 3, 1, st=True), b16=1),
    B(17, 4, 482, large(1, 2, 9, 1, st=True), C=256, b16=1, big=1),
]

# ---- folded inputs, synthesised on the host by the GPU tier: which cases, and what the query answers with the flag set
PARTIAL_ROWS = [1, 255, 256, 257]
PARTIAL_CASES = [c for c in CASES if (c.N, c.C, c.H, c.W, c.off, c.training, c.b16) in
                 {(25, 3, 2, 82, 0, 1, 0), (3, 3, 68, 241, 0, 1, 0), (3, 3, 145, 113, 0, 1, 0)} and not c.opt]
# with conv_partials (forward) / conv_partials + dbias_partials (backward) the mid-size case leaves the one-launch path
PARTIAL_CLAIMS = {(25, 2, 82): large(1, 1, 25, 1), (3, 68, 241): large(2, 1, 3, 1), (3, 145, 113): large(2, 1, 3, 0)}
SLAB_COUNTS = [2, 5]
SLAB_CASES = [c for c in CASES if (c.N, c.C, c.H, c.W) in {(2, 3, 16, 16), (1, 3, 27, 19), (4, 3, 32, 32)} and not c.opt]
PACKED_CASES = [c for c in CASES if (c.N, c.C, c.H, c.W, c.off, c.training, c.b16) in
                {(8, 3, 32, 32, 0, 1, 0), (3, 3, 68, 241, 0, 1, 0)} and not c.opt]
UNBIASED_CASES = [c for c in CASES if (c.N, c.C, c.H, c.W) in {(2, 3, 1, 1), (2, 3, 16, 16), (1, 3, 27, 19)}]


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).float()


def _rb(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=2)
def operands(c):
    """fp32 CPU operands of a case (bf16-representable where the case stores bf16); gamma / beta / running buffers None for a null case."""
    s = 100 * c.seed
    y = _rnd(c.N, c.C, c.H, c.W, seed=5 + s) * 2 + 0.7
    da = _rnd(c.N, c.C, c.H, c.W, seed=10 + s)
    if c.b16:
        y, da = _rb(y), _rb(da)
    if c.o("null"):
        return dict(y=y, da=da, gamma=None, beta=None, rm=None, rv=None)
    return dict(y=y, da=da, gamma=_rnd(c.C, seed=6 + s).abs() + 0.5, beta=_rnd(c.C, seed=7 + s) * 0.3,
                rm=_rnd(c.C, seed=8 + s) * 0.1, rv=_rnd(c.C, seed=9 + s).abs() + 0.5)


def _ch(v):
    return v.view(1, -1, 1, 1)


def reference_of(y, da, gamma, beta, rm, rv, relu):
    """fp64 BatchNorm (+ ReLU) forward and backward of fp32 operands in plain tensor arithmetic (gamma / beta / rm / rv may be None).
    `da` in the answer is the incoming gradient with the knife-edge elements zeroed (module docstring), `edge_share` the share of
    elements that were, `dz` = da under the ReLU mask, `xh` the normalised input."""
    N, C, H, W = y.shape
    n = N * H * W
    y = y.double()
    gamma = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    beta = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    mean = y.mean((0, 2, 3))
    var = ((y - _ch(mean)) ** 2).mean((0, 2, 3))
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (y - _ch(mean)) * _ch(rstd)
    o = _ch(gamma) * xh + _ch(beta)
    a = o.clamp_min(0.0) if relu else o
    r = dict(mean=mean, var=var, rstd=rstd, a=a, alpha=gamma * rstd, beta_=beta - mean * gamma * rstd, xh=xh)
    if rm is not None:
        r["rm"] = (1 - MOMENTUM) * rm.double() + MOMENTUM * mean
        r["rv"] = (1 - MOMENTUM) * rv.double() + MOMENTUM * var * (n / (n - 1.0) if n > 1 else 1.0)
        oe = _ch(gamma) * (y - _ch(rm.double())) / torch.sqrt(_ch(rv.double()) + EPS) + _ch(beta)
        r["a_eval"] = oe.clamp_min(0.0) if relu else oe
    edge = o.abs() < RELU_EDGE
    r["edge"] = edge
    r["edge_share"] = float(edge.double().mean())
    r["da"] = torch.where(edge, torch.zeros((), dtype=torch.float32), da)
    dz = r["da"].double() * (o > 0) if relu else r["da"].double()
    r["dz"] = dz
    r["dbeta"] = dz.sum((0, 2, 3))
    r["dgamma"] = (dz * xh).sum((0, 2, 3))
    r["dy"] = _ch(gamma * rstd) * (dz - _ch(r["dbeta"] / n) - xh * _ch(r["dgamma"] / n))
    return r


@functools.lru_cache(maxsize=2)
def reference(c, relu):
    """reference_of the case's operands, computed once per (case, relu) and shared by the tests that need it."""
    op = operands(c)
    return reference_of(op["y"], op["da"], op["gamma"], op["beta"], op["rm"], op["rv"], relu)
