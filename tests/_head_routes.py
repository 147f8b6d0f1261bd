"""The heads dispatch table: cases at the kernel-choice thresholds of csrc/conv1x1_small.hip - the 1x1 heads with at most 8 outputs
(uz_conv_fwd / uz_conv_bwd_data / uz_conv_bwd_weight at ks = 1, uz_conv1x1_*_b16) and the fused latent heads (uz_latent_heads_*) -
each with the launch it claims, stated only through the library's host-side query uz_heads_route, which answers from the
predicates the entry points themselves dispatch through.

A case is a kind ("c1" the 1x1 head, "c1_b16" the same through the bf16-storage entry points, "lat" the latent heads), a shape
(N, Cin, Cout or L, H, W), the view offsets and the claims per direction
  fwd   = (form, pix)                    form: 0 scalar, 1 float4, 2 channel-parallel, 3 not covered (the MFMA kernels run)
  dgrad = (form, pix, groups, cgroup)    pix: workgroups of 1 024 pixels per image (form 2: QPB, pixel quads per workgroup)
  wgrad = (form, nchunk)                 groups x cgroup: channel groups of the data gradient; nchunk: chunks of 16 384 pixels
A direction without a claim is not run for the case.  The claims hold with UZ_HEADS_PAR unset.

Views: the many-channel operand (x / h / dx / dh) is channels [C0, C0 + Cin) of a buffer of Cin + 2 channels that starts off[0]
floats into a NaN-filled allocation; the few-channel operands of a 1x1 head (y / dy) are channels [C0, C0 + Cout) of a buffer of
Cout + 2 channels that starts off[1] floats in; the latent heads' contiguous tensors (mu, pre_sigma, sigma, z, eps, dy_a, dy_b)
start GUARD + off[1] floats in; the bf16 operand of a "c1_b16" case is channels [0, Cin) of its buffer, B16_LEAD + off[0] elements
in (a plane of 2-byte elements need not be a multiple of 16 bytes).  An offset of 1 breaks the 16-byte alignment the float4 kernels need.  Cases come in pairs, one
on each side of a threshold; the comment of a group names the line it pins.  tests/test_head_routes_cpu.py checks the claims,
tests/test_head_routes_gpu.py runs every case against fp64."""
import collections
import ctypes

Case = collections.namedtuple("Case", "kind N Cin Cout H W off opt claims")
DIRECTIONS = ("fwd", "dgrad", "wgrad")
OPS = dict(c1=(0, 1, 2), c1_b16=(0, 1, 2), lat=(3, 4, 5))
SCALAR, VEC, PAR, MFMA = 0, 1, 2, 3
# every form uz_heads_route can answer per (kind, direction)
FORMS = {("c1", "fwd"): {SCALAR, VEC, MFMA}, ("c1", "dgrad"): {SCALAR, VEC, MFMA}, ("c1", "wgrad"): {SCALAR, VEC, MFMA},
         ("lat", "fwd"): {SCALAR, VEC, PAR}, ("lat", "dgrad"): {SCALAR, VEC}, ("lat", "wgrad"): {SCALAR, VEC}}
C0 = 1          # first channel of every view; the buffers hold C + 2 channels
GUARD = 4       # NaN floats in front of a contiguous tensor
B16_LEAD = 8    # NaN elements (16 bytes) in front of a bf16 buffer
NOT_COVERED = dict(fwd=(MFMA, 0), dgrad=(MFMA, 0, 0, 0), wgrad=(MFMA, 0))


def Hd(kind, N, Cin, Cout, H, W, fwd=None, dgrad=None, wgrad=None, off=(0, 0), **opt):
    claims = {k: v for k, v in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)) if v is not None}
    assert kind in OPS and claims
    return Case(kind, N, Cin, Cout, H, W, tuple(off), tuple(sorted(opt.items())), claims)


def opt(c, name, default=None):
    return dict(c.opt).get(name, default)


def case_id(c):
    o = "" if c.off == (0, 0) else f"-off{c.off[0]}{c.off[1]}"
    x = "".join(f"-{k}{v}" for k, v in c.opt)
    return f"{c.kind}-{c.N}x{c.Cin}x{c.Cout}x{c.H}x{c.W}{o}{x}"


def aligned(c):
    """Whether every view of the case starts on a 16-byte boundary, as the buffers of the GPU tier place them."""
    hw = c.H * c.W
    wide = c.off[0] % 8 == 0 if c.kind == "c1_b16" else (c.off[0] + C0 * hw) % 4 == 0
    narrow = (GUARD + c.off[1]) % 4 == 0 if c.kind == "lat" else (c.off[1] + C0 * hw) % 4 == 0
    return wide and narrow


def queries(L, c):
    got = {}
    for d, op in zip(DIRECTIONS, OPS[c.kind]):
        if d not in c.claims:
            continue
        o = (ctypes.c_int * 5)()
        rc = L.uz_heads_route(op, c.Cin, c.Cout, c.N, c.H, c.W, int(aligned(c)), o)
        assert rc == 0, L.uz_last_error()
        got[d] = {"fwd": (o[0], o[1]), "dgrad": (o[0], o[1], o[2], o[3]), "wgrad": (o[0], o[4])}[d]
    return got


def all3(form, pix=1, groups=1, cgroup=None, nchunk=1, Cin=5):
    return dict(fwd=(form, pix), dgrad=(form, pix, groups, Cin if cgroup is None else cgroup), wgrad=(form, nchunk))


CASES = [
    # ---- covered output counts (heads_outputs_covered = the instances of C1_DISPATCH / C1_W): 1, 2, 3, 4, 6, 8 stream; 5, 7 and 9 do not
    *[Hd("c1", 2, 5, co, 4, 8, **all3(VEC)) for co in (1, 2, 3, 4, 6, 8)],
    *[Hd("c1", 2, 5, co, 4, 8, **NOT_COVERED) for co in (5, 7, 9)],
    # ---- CIN_MAX = 512 (8 outputs x 512 channels fill the LDS image exactly) | 513
    Hd("c1", 2, 512, 8, 4, 8, fwd=(VEC, 1), dgrad=(VEC, 1, 64, 8), wgrad=(VEC, 1)),
    Hd("c1", 2, 513, 8, 4, 8, **NOT_COVERED),
    # ---- PIX = 1024 pixels per workgroup: one block | a second block of one float4 | 1 023 and 1 025, scalar by shape
    Hd("c1", 2, 5, 2, 32, 32, **all3(VEC)),
    Hd("c1", 2, 5, 2, 4, 257, **all3(VEC, pix=2)),
    Hd("c1", 2, 5, 2, 3, 341, **all3(SCALAR)),
    Hd("c1", 2, 5, 2, 25, 41, **all3(SCALAR, pix=2)),
    # ---- a view one float off (heads_vec): scalar by alignment, the many-channel side and the few-channel side in turn; 4 x 257 = two
    # pixel blocks, 68 x 241 = two weight-gradient chunks
    Hd("c1", 2, 5, 2, 4, 257, off=(1, 0), **all3(SCALAR, pix=2)),
    Hd("c1", 2, 5, 2, 4, 257, off=(0, 1), **all3(SCALAR, pix=2)),
    Hd("c1", 1, 5, 2, 68, 241, off=(1, 0), wgrad=(SCALAR, 2)),
    Hd("c1", 1, 5, 2, 68, 241, off=(0, 1), wgrad=(SCALAR, 2)),
    # ---- data gradient channel groups (heads_dgrad_groups): groups = ceil(1024 / pixblk) capped at ceil(Cin / 8); Cin 8 | 9: one | two
    # groups (5 + 4); Cin 25: 7 + 7 + 7 + 4; pixblk 1 023 | 1 024: two groups | one
    Hd("c1", 2, 8, 2, 4, 8, dgrad=(VEC, 1, 1, 8)),
    Hd("c1", 2, 9, 2, 4, 8, dgrad=(VEC, 1, 2, 5)),
    Hd("c1", 2, 25, 3, 4, 8, dgrad=(VEC, 1, 4, 7)),
    Hd("c1", 1023, 9, 2, 2, 2, dgrad=(VEC, 1, 2, 5)),
    Hd("c1", 1024, 9, 2, 2, 2, dgrad=(VEC, 1, 1, 9)),
    # ---- weight gradient chunks (heads_nchunk, WCHUNK = 16 384): 16 384 | 16 388 on the float4 sweep, 16 383 | 16 385 on the scalar one
    Hd("c1", 1, 5, 2, 128, 128, wgrad=(VEC, 1)),
    Hd("c1", 1, 5, 2, 68, 241, wgrad=(VEC, 2)),
    Hd("c1", 1, 5, 2, 127, 129, wgrad=(SCALAR, 1)),
    Hd("c1", 1, 5, 2, 145, 113, wgrad=(SCALAR, 2)),
    # ... a last chunk of two float4: 245 768 pixels = 16 chunks of `per` = 16 384, the last holds 8 pixels
    Hd("c1", 1, 3, 2, 248, 991, wgrad=(VEC, 16)),
    # ... WCHUNK_MAX = 64: 4 x 512 x 512 = 64 chunks exactly | 5 x 512 x 512 capped (per = 20 480); without db
    Hd("c1", 4, 3, 2, 512, 512, wgrad=(VEC, 64)),
    Hd("c1", 5, 3, 2, 512, 512, wgrad=(VEC, 64), db=0),
    # ---- null bias in the forward, no bias gradient
    Hd("c1", 2, 5, 3, 4, 8, fwd=(VEC, 1), wgrad=(VEC, 1), bias=0, db=0),
    Hd("c1", 2, 5, 3, 5, 7, fwd=(SCALAR, 1), wgrad=(SCALAR, 1), bias=0, db=0),
    # ---- bf16 storage of the many-channel operand (uz_conv1x1_*_b16): two pixel blocks, two chunks
    Hd("c1_b16", 2, 5, 2, 4, 257, **all3(VEC, pix=2)),
    Hd("c1_b16", 1, 5, 3, 68, 241, wgrad=(VEC, 2)),
    # ---- latent heads, channel-parallel forward (heads_par): a power-of-two number of quads, N * quads <= PAR_QUADS_MAX = 16 384;
    # QPB = min(quads, 64): quads 1 (255 of 256 channel groups idle at Cin 7; CG = 256 > Cin), 64 (one workgroup), 128 (two), 36 (sequential)
    Hd("lat", 3, 7, 2, 2, 2, fwd=(PAR, 1), dgrad=(VEC, 1, 1, 7), wgrad=(VEC, 1)),
    Hd("lat", 3, 192, 2, 2, 2, fwd=(PAR, 1), dgrad=(VEC, 1, 24, 8), wgrad=(VEC, 1)),
    Hd("lat", 2, 24, 3, 16, 16, fwd=(PAR, 64), dgrad=(VEC, 1, 3, 8), wgrad=(VEC, 1)),
    Hd("lat", 2, 24, 1, 16, 32, fwd=(PAR, 64), dgrad=(VEC, 1, 3, 8), wgrad=(VEC, 1), act=1),
    Hd("lat", 2, 24, 2, 12, 12, fwd=(VEC, 1), dgrad=(VEC, 1, 3, 8), wgrad=(VEC, 1)),
    Hd("lat", 64, 6, 2, 32, 32, fwd=(PAR, 64)),
    Hd("lat", 65, 6, 2, 32, 32, fwd=(VEC, 1)),
    # ... z / eps null, biases null, exp instead of softplus
    Hd("lat", 2, 24, 2, 16, 16, fwd=(PAR, 64), wgrad=(VEC, 1), z=0, bias=0, db=0, act=1),
    Hd("lat", 2, 24, 2, 12, 12, fwd=(VEC, 1), z=0, bias=0, act=1),
    # ... L = 4 at Cin = 512: the 2 L x Cin weights fill the LDS image
    Hd("lat", 2, 512, 4, 4, 4, fwd=(PAR, 4), dgrad=(VEC, 1, 64, 8), wgrad=(VEC, 1)),
    Hd("lat", 2, 512, 4, 5, 5, fwd=(SCALAR, 1), dgrad=(SCALAR, 1, 64, 8), wgrad=(SCALAR, 1)),
    # ... pixel blocks, a misaligned view, ragged channel groups and two weight-gradient chunks on the latent kernels
    Hd("lat", 2, 5, 2, 4, 257, **all3(VEC, pix=2)),
    Hd("lat", 2, 5, 2, 25, 41, **all3(SCALAR, pix=2)),
    Hd("lat", 2, 5, 2, 4, 257, off=(1, 0), **all3(SCALAR, pix=2)),
    Hd("lat", 2, 5, 2, 16, 16, off=(0, 1), **all3(SCALAR)),
    Hd("lat", 2, 25, 3, 4, 8, dgrad=(VEC, 1, 4, 7)),
    Hd("lat", 1, 5, 2, 68, 241, wgrad=(VEC, 2)),
    Hd("lat", 1, 5, 2, 68, 241, off=(1, 0), wgrad=(SCALAR, 2)),
    Hd("lat", 1, 5, 2, 145, 113, wgrad=(SCALAR, 2)),
]

# calls the entry points refuse with an error return before any launch: (entry, N, Cin, Cout or L, H, W)
REFUSED = [
    ("lat", 2, 513, 2, 4, 4),           # Cin past the LDS image
    ("lat", 2, 8, 0, 4, 4), ("lat", 2, 8, 5, 4, 4),
    ("c1_b16", 2, 5, 2, 25, 41),        # bf16 storage off the float4 shape
    ("c1_b16", 2, 5, 5, 4, 8),          # ... and at an output count the streaming kernels do not cover
]

# ---- the four convolution queries at ks = 1 on both sides of the covered output counts and of CIN_MAX, in every math mode:
# (Cin, Cout, N, H, W) -> uz_conv_route for the three kinds, uz_conv_bwd_weight_slabs, uz_conv_splitk_parts, uz_conv_bwd_splitk_parts.
# A streaming head writes no slabs and splits nothing; an uncovered one runs the fp32 MFMA kernels with their own slabs and split-K
# (32 x 192 x 4 x 4: 32 slabs, 24 forward parts)
CONV_QUERY_STREAMING = [(192, co, 32, 4, 4) for co in (1, 2, 3, 4, 6, 8)] + [(512, 8, 32, 4, 4)]
CONV_QUERY_MFMA = [((192, co, 32, 4, 4), dict(routes=(0, 0, 0), slabs=32, parts=24, bwd_parts=1)) for co in (5, 7, 9)]
CONV_QUERY_MFMA.append(((513, 8, 32, 4, 4), dict(routes=(0, 0, 0), slabs=32, parts=65, bwd_parts=1)))
