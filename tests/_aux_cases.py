"""Case tables, operands and fp64 references for the kernels beside the timed step that decide what the model is trained on and how
it is scored: the validation metrics (csrc/metrics.hip), the batch assembly and augmentation (csrc/augment.hip), the latent-noise
stream and step counters, and the posterior input (csrc/pointwise.hip).  numpy only: tests/test_aux_cases_cpu.py checks the
references, the gate tables and that the cases discriminate (a deliberately wrong twin changes an expected output beyond its gate);
tests/test_aux_cases_gpu.py runs every case through the C ABI on views inside guarded allocations.

Gates that are "4 x the fp32 twin" are 4 x the distance between the same formulas evaluated in numpy float32 and the fp64 reference
on the same case, of max(1, max |ref|).  The *_F32 tables hold those distances as measured on the CPU; the CPU tier recomputes them."""
import collections

import numpy as np

from oracle import augment as OA

# ================================================================================================ validation metrics
# ---- uz_label_pair_counts: 256 threads stride one map pair, four wave sums, out indexed with gridDim.y
PC_HW = [1, 63, 64, 65, 255, 256, 257, 1000, 16385]          # no full wave / one wave +- 1 / one workgroup +- 1 / ragged / 64 trips + 1
PC_NANB = [(1, 1), (3, 5), (5, 3)]
PC_LABELS = [0, 1, 3, 255, 7]                                 # 7 is in neither map; 3 only in a, 255 only in b (except the shared map)
PC_OFFSETS = [(0, 0), (1, 3)]                                 # byte offsets of the a / b views: 16-byte aligned, odd addresses


def pc_maps(HW, Na, Nb):
    """a over {0, 1, 3}, b over {0, 1, 255}; the last map of b is a copy of a[0] (identical maps: intersection = both counts)."""
    rs = np.random.default_rng(7000 + 64 * HW + 8 * Na + Nb)
    a = np.array([0, 1, 3], np.uint8)[rs.integers(0, 3, (Na, HW))]
    b = np.array([0, 1, 255], np.uint8)[rs.integers(0, 3, (Nb, HW))]
    b[Nb - 1] = a[0]
    return a, b


def pc_ref(a, b, label, stride=None):
    """Flat int64 image of `out` as the kernel writes it: (i * Nb + j) * 3 + {intersection, |a == l|, |b == l|}.
    stride: the row stride in pairs (Nb; a wrong kernel might use Na) - rows then overlap or leave holes (-1)."""
    Na, Nb = a.shape[0], b.shape[0]
    stride = Nb if stride is None else stride
    out = np.full((max(Na * Nb, (Na - 1) * stride + Nb)) * 3, -1, np.int64)
    for i in range(Na):
        for j in range(Nb):
            x, y = a[i] == label, b[j] == label
            out[(i * stride + j) * 3:(i * stride + j) * 3 + 3] = [np.count_nonzero(x & y), np.count_nonzero(x), np.count_nonzero(y)]
    return out[:Na * Nb * 3]


# ---- uz_ncc_maps: one thread per pixel, 256 per workgroup
NM_HW = [1, 255, 256, 257, 1000]
NM_NMK = [(1, 1, 1), (1, 1, 2), (6, 4, 2), (5, 3, 3), (3, 2, 4)]


# HW = 1 has 1 + M output values.  The float32 distance of so few roundings is nearly nothing for most draws, and 4 x nearly nothing
# asks for more than an fp32 output can hold: half an ulp of the value (up to 6e-8 of it) plus an ulp of each logf.  These cases take
# the first draw whose two float32 distances reach 4.5e-8 (tests/test_aux_cases_cpu.py checks both that they do and that it is the first).
NM_DRAW = {(6, 4, 2, 1): 6, (5, 3, 3, 1): 16, (3, 2, 4, 1): 4}
NM_DRAW_FLOOR = 4.5e-8


def nm_id(N, M, K, HW):
    return f"{N}x{M}x{K}x{HW}"


def nm_operands(N, M, K, HW):
    """Softmax samples (N, K, HW) fp32 with exact one-hot pixels (exact 0 and exact 1: the + 1e-8 decides the value) at the first,
    middle and last pixel; one-hot ground truth (M, K, HW) fp32 whose first annotator marks, at those pixels, a class the sample has at
    exactly 0 (E_sy = -log(1e-8) / N there) and whose last annotator, where M > 1, has an empty mask (all label 0)."""
    rs = np.random.default_rng(9000 + 1000 * HW + 100 * N + 10 * M + K + 100000 * NM_DRAW.get((N, M, K, HW), 0))
    z = rs.standard_normal((N, K, HW)) * 2
    soft = np.exp(z - z.max(1, keepdims=True))
    soft = soft / soft.sum(1, keepdims=True) if K > 1 else rs.uniform(0.05, 1.0, (N, K, HW))
    soft = soft.astype(np.float32)
    for t, p in enumerate(sorted({0, HW // 2, HW - 1})):
        i, k = t % N, t % K
        soft[i, :, p] = 0
        soft[i, k, p] = 1 if K > 1 else (t + 1) % 2
    lab = rs.integers(0, K, (M, HW))
    for t, p in enumerate(sorted({0, HW // 2, HW - 1})):
        lab[0, p] = (t % K + 1) % K                                # the first annotator marks a class that sample has at exactly 0
    if M > 1:
        lab[M - 1] = 0
    gt = np.stack([(lab == k) for k in range(K)], axis=1).astype(np.float32)
    return soft, gt


def nm_ref(soft, gt, dtype=np.float64, tail=True):
    """E_ss (HW) and E_sy (M, HW) as oracle/metrics.py variance_ncc_dist writes them, every operation and the result in `dtype`:
    float64 is the reference, float32 the same formulas in the number format of the kernel's outputs (the oracle itself takes the
    mean over the samples in double and never rounds it back; E_ss and E_sy are fp32 arrays, so half an ulp of each value is
    part of any fp32 evaluation).  tail=False leaves the pixels behind the last full 256 unwritten (NaN)."""
    s, g = soft.astype(dtype), gt.astype(dtype)

    def xent(m_samp, m_gt, eps=1e-8):
        return -1.0 * np.sum(m_gt * np.log(m_samp + dtype(eps)), axis=0)
    mean_seg = np.mean(s, axis=0)
    ess = np.mean(np.stack([xent(s[i], mean_seg) for i in range(s.shape[0])]), axis=0)
    esy = np.stack([np.mean(np.stack([xent(s[i], g[j]) for i in range(s.shape[0])]), axis=0) for j in range(g.shape[0])])
    assert ess.dtype == esy.dtype == dtype
    if not tail:
        full = soft.shape[-1] // 256 * 256
        ess[full:], esy[:, full:] = np.nan, np.nan
    return ess, esy


def rel_err(got, ref):
    """max |got - ref| of max(1, max |ref|); NaN (an unwritten element) counts as infinite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    return float("inf") if np.isnan(d).any() else float(d.max()) / max(1.0, float(np.abs(ref).max()))


def nm_f32_error(N, M, K, HW):
    soft, gt = nm_operands(N, M, K, HW)
    (e32, y32), (e64, y64) = nm_ref(soft, gt, np.float32), nm_ref(soft, gt)
    return rel_err(e32, e64), rel_err(y32, y64)


# numpy float32 against fp64 on nm_operands, (E_ss, E_sy); the GPU gate is 4 x these
NM_F32 = {
    "1x1x1x1": (1.000e-08, 1.000e-08), "1x1x1x255": (4.757e-08, 1.389e-08), "1x1x1x256": (4.316e-08, 1.389e-08), "1x1x1x257": (5.707e-08, 1.389e-08), "1x1x1x1000": (5.452e-08, 1.389e-08),
    "1x1x2x1": (1.000e-08, 1.389e-08), "1x1x2x255": (9.150e-08, 2.391e-08), "1x1x2x256": (9.217e-08, 1.440e-08), "1x1x2x257": (8.981e-08, 1.389e-08), "1x1x2x1000": (9.178e-08, 1.884e-08),
    "6x4x2x1": (1.556e-07, 5.066e-08), "6x4x2x255": (9.653e-08, 1.144e-07), "6x4x2x256": (9.430e-08, 8.387e-08), "6x4x2x257": (1.522e-07, 1.063e-07), "6x4x2x1000": (9.228e-08, 1.051e-07),
    "5x3x3x1": (1.174e-07, 7.869e-08), "5x3x3x255": (7.527e-08, 7.863e-08), "5x3x3x256": (7.531e-08, 8.604e-08), "5x3x3x257": (9.342e-08, 8.539e-08), "5x3x3x1000": (8.703e-08, 1.081e-07),
    "3x2x4x1": (5.139e-08, 7.950e-08), "3x2x4x255": (5.090e-08, 5.372e-08), "3x2x4x256": (8.916e-08, 6.420e-08), "3x2x4x257": (8.821e-08, 7.401e-08), "3x2x4x1000": (7.290e-08, 6.866e-08),
}

# ---- uz_ncc: one workgroup per map pair, fp64 one-pass sums
NCC_M = [1, 4]
NCC_HW = NM_HW                          # HW = 1 is a constant map by necessity: reference and kernel are both 0 / 0
NCC_GATE = 4 * 2.0 ** -24               # one fp32 rounding of a value in [-1, 1] is 2^-25; the one-pass variance loses ~ 1e-16 (mean / std)^2


def ncc_operands(M, HW):
    """a (HW) and v (M, HW) fp32 with unit spread on offsets up to 1e3 (|mean| / std up to 1e3) and correlations 0.9, -0.5, 0, 1."""
    rs = np.random.default_rng(11000 + 10 * HW + M)
    z0 = rs.standard_normal(HW)
    a = ((1000.0 if M == 4 else 3.0) + z0).astype(np.float32)
    rho, off = [0.9, -0.5, 0.0, 1.0], [0.0, 1000.0, -30.0, 5.0]
    v = np.stack([off[j] + rho[j] * z0 + np.sqrt(1 - rho[j] ** 2) * rs.standard_normal(HW) for j in range(M)]).astype(np.float32)
    return a, v


def ncc_ref(a, v):
    """Two-pass Pearson correlation in fp64 of the fp32 maps (oracle/metrics.py ncc: centre, divide by the deviations, correlate)."""
    a = a.astype(np.float64)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for vj in v.astype(np.float64):
            da, dv = a - a.mean(), vj - vj.mean()
            out.append(np.mean(da * dv) / (np.sqrt(np.mean(da * da)) * np.sqrt(np.mean(dv * dv))))
    return np.array(out)


# ---- end to end through unet_zoo_amd.metrics: 24 x 20, three labels, one annotator with an empty mask
def e2e_operands():
    rs = np.random.default_rng(31)
    H, W, N, M, K = 24, 20, 5, 4, 3
    yy, xx = np.mgrid[0:H, 0:W]

    def blobs(n):
        out = np.zeros((n, H, W), np.int64)
        for i in range(n):
            for lbl in (1, 2):
                cy, cx, r = rs.uniform(5, H - 5), rs.uniform(5, W - 5), rs.uniform(2, 6)
                out[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = lbl
        return out
    samples, gts = blobs(N), blobs(M)
    gts[2] = 0                                                    # the empty mask
    samples[3][samples[3] == 2] = 0                               # a sample without label 2
    z = rs.standard_normal((N, K, H, W)) * 2
    soft = np.exp(z - z.max(1, keepdims=True))
    soft = (soft / soft.sum(1, keepdims=True)).astype(np.float32)
    return samples, gts, soft


# ================================================================================================ batch assembly
AugCase = collections.namedtuple("AugCase", "name H W A nlabels rows idx ann")
AUG_ROWS = 7                                                      # dataset rows per case
DEG10 = (float(np.float32(np.cos(np.pi / 18))), float(np.float32(np.sin(np.pi / 18))))


def prm(rot=None, scale=None, flips=0):
    """One parameter row: rot = (cos, sin) or None, scale = (p_x, p_y, r) or None, flips bit 0 left-right, bit 1 up-down."""
    c, s = rot if rot else (1.0, 0.0)
    px, py, r = scale if scale else (0, 0, 0)
    return [float(rot is not None), c, s, float(scale is not None), float(px), float(py), float(r), float(flips)]


def _rows(H, W, r, far):
    """The eight rows of a non-square or tiny shape: four un-resampled flips, rotation, crop at the origin / far corner, both."""
    c, s = DEG10
    return [prm(flips=0), prm(flips=1), prm(flips=2), prm(flips=3), prm(rot=(c, s)), prm(scale=(0, 0, r), flips=1),
            prm(scale=(far[0], far[1], r), flips=2), prm(rot=(c, -s), scale=(far[0], far[1], r), flips=3)]


IDX = [5, 2, 6, 2, 0, 4, 3, 1]                                     # unsorted, row 2 twice
ANN4 = [1, 3, 2, 1, 3, 2, 0, 3]
C10, S10 = DEG10
AUG_CASES = [
    # every row exact by construction: integer source coordinates and weights 0 / 1 in any precision
    AugCase("sq128-exact", 128, 128, 4, 3,
            [prm(flips=0), prm(flips=1), prm(flips=2), prm(flips=3), prm(rot=(1.0, 0.0), flips=1), prm(scale=(0, 0, 128), flips=2),
             prm(rot=(0.0, 1.0)), prm(rot=(1.0, 0.0), scale=(0, 0, 128), flips=3)], IDX, ANN4),
    # +-10 degrees, r = min(H, W) - 30 at the origin and the far corner, r = 1, each branch alone and both
    AugCase("sq128-resample", 128, 128, 4, 3,
            [prm(rot=(C10, S10)), prm(rot=(C10, -S10), flips=3), prm(scale=(0, 0, 98)), prm(scale=(30, 30, 98), flips=1),
             prm(rot=(C10, S10), scale=(30, 30, 98), flips=1), prm(rot=(C10, -S10), scale=(10, 50, 64), flips=2),
             prm(scale=(127, 127, 1)), prm(rot=(C10, S10), scale=(64, 60, 1), flips=3)], IDX, ANN4),
    # H W = 21 760 > 64 x 256: the grid-stride loop takes a second, partial trip; H != W
    AugCase("136x160", 136, 160, 4, 8, _rows(136, 160, 106, (54, 30)), IDX, ANN4),
    AugCase("160x136", 160, 136, 1, 2, _rows(160, 136, 106, (30, 54)), IDX, [0] * 8),
    AugCase("5x7", 5, 7, 4, 3, _rows(5, 7, 3, (4, 2)), IDX, ANN4),
    AugCase("1x300", 1, 300, 4, 8, _rows(1, 300, 1, (299, 0)), IDX, ANN4),
    AugCase("sq128-one-label", 128, 128, 1, 1, [prm(flips=3), prm(rot=(C10, S10)), prm(scale=(30, 30, 98)), prm(rot=(C10, -S10), scale=(0, 0, 98), flips=1)],
            [3, 0, 3, 6], [0] * 4),
]
AUG_MARGIN = 1e-4                 # labels are compared where the fp64 margin is at least this
AUG_MARGIN_CAP = 1e-3             # at most this share of a case's pixels may lie below it
AUG_IMAGE_FLOOR = 2e-5            # the image gate is never looser than the gate of test_device_batch_assembly_matches_the_numpy_twin


def aug_dataset(case):
    """X (rows, H, W) fp32 noise; Y (rows, H, W, A) uint8 label maps whose regions (nearest of ~ 4 seeds per label, a Voronoi
    partition) touch one another, so three and more labels meet inside a 2 x 2 tap window.  The data hold nlabels labels; with
    nlabels = 1 three, of which the resampling stages drop two (all weights 0: label 0) and the plain gather keeps all."""
    rs = np.random.default_rng(500 + case.H * 1000 + case.W + case.A)
    H, W, A, nl = case.H, case.W, case.A, case.nlabels if case.nlabels > 1 else 3
    X = (rs.standard_normal((AUG_ROWS, H, W)) * 0.2).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    Y = np.zeros((AUG_ROWS, H, W, A), np.uint8)
    for i in range(AUG_ROWS):
        for a in range(A):
            n = 4 * nl
            cy, cx = rs.uniform(0, H, n), rs.uniform(0, W, n)
            d = (yy[..., None] - cy) ** 2 + (xx[..., None] - cx) ** 2
            Y[i, ..., a] = (np.argmin(d, axis=-1) % nl).astype(np.uint8)
    return X, Y


def aug_row_exact(case, row):
    """A row whose result is exact by construction: nothing resampled, or rotation by a multiple of 90 degrees with cos / sin
    exactly 0 / +-1 (integer source coordinates), and / or the identity crop r = W = H at the origin."""
    do_rot, c, s, do_scale, px, py, r, _ = row
    rot_ok = not do_rot or (c, s) == (1.0, 0.0) or (case.H == case.W and c == 0.0 and abs(s) == 1.0)
    scale_ok = not do_scale or (case.H == case.W == int(r) and px == 0 and py == 0)
    return rot_ok and scale_ok


def aug_ref(case, dtype=np.float64, defects=(), X=None, Y=None):
    """The twin on every row of the case: images (B, H, W), labels (B, H, W) and, for float64, margins (B, H, W).
    defects: those of oracle/augment.py plus "flips" (bits swapped) and "annotator" (offset ignored)."""
    if X is None:
        X, Y = aug_dataset(case)
    inner = tuple(d for d in defects if d in ("centre", "scale", "argmax"))
    outs = []
    for b, row in enumerate(case.rows):
        row = list(row)
        if "flips" in defects:
            row[7] = float((int(row[7]) & 1) << 1 | (int(row[7]) >> 1) & 1)
        ann = 0 if "annotator" in defects else case.ann[b]
        outs.append(OA.augment(X[case.idx[b]], Y[case.idx[b], ..., ann], np.asarray(row, np.float32), case.nlabels, dtype=dtype, defects=inner))
    return [np.stack([o[k] for o in outs]) for k in range(len(outs[0]))]


def aug_f32_error(case):
    """max |fp32 twin - fp64 twin| over the case's images, of max(1, max |ref|)."""
    X, Y = aug_dataset(case)
    return rel_err(aug_ref(case, np.float32, X=X, Y=Y)[0], aug_ref(case, X=X, Y=Y)[0])


# fp32 twin against fp64 twin, image; the GPU gate is min(4 x this, AUG_IMAGE_FLOOR)
AUG_F32 = {
    "sq128-exact": 0.000e+00, "sq128-resample": 5.839e-06, "136x160": 7.354e-06, "160x136": 9.486e-06, "5x7": 9.163e-08, "1x300": 1.922e-06, "sq128-one-label": 5.385e-06,
}


# ================================================================================================ latent noise
M32 = np.uint64(0xFFFFFFFF)
VGRID_QUADS = 2048 * 256                                          # quads one pass of the capped grid covers (pointwise.hip vgrid)


def philox4x32(ctr, key, rounds=10):
    """Philox4x32 (Salmon et al., SC'11): ctr four and key two arrays of 32-bit words held in uint64; returns the four output words."""
    c = [np.asarray(w, np.uint64) & M32 for w in ctr]
    k0, k1 = [np.asarray(w, np.uint64) & M32 for w in key]
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def noise_words(seed, offset, n, defects=()):
    """The (quads, 4) output words of uz_randn_fill's counters {lo(offset + q), hi(offset + q), 0x5A5A5A5A, 0}, key {lo, hi}(seed).
    defects: "ctr_hi" / "key_hi" (that word forced to 0), "rounds" (nine)."""
    quads = (n + 3) // 4
    ctr = (np.uint64(offset & (2 ** 64 - 1)) + np.arange(quads, dtype=np.uint64))              # wraps mod 2^64 like the kernel
    seed = np.uint64(seed & (2 ** 64 - 1))
    chi = np.zeros(quads, np.uint64) if "ctr_hi" in defects else ctr >> np.uint64(32)
    khi = np.uint64(0) if "key_hi" in defects else seed >> np.uint64(32)
    w = philox4x32([ctr & M32, chi, np.full(quads, 0x5A5A5A5A, np.uint64), np.zeros(quads, np.uint64)], [seed & M32, khi],
                   9 if "rounds" in defects else 10)
    return np.stack(w, axis=1)


def noise_ref(seed, offset, n, dtype=np.float64, defects=()):
    """Box-Muller on the uniforms ((w >> 8) + 0.5) 2^-24 of noise_words: per quad r1 cos, r1 sin, r2 cos, r2 sin.  float32 evaluates the
    kernel's formulas (2 pi rounded to fp32 included) in numpy float32.  "stride": nothing behind the first pass of the grid (NaN)."""
    T = dtype
    w = noise_words(seed, offset, n, defects)
    u = ((w >> np.uint64(8)).astype(T) + T(0.5)) * T(2.0 ** -24)
    two_pi = T(np.float32(6.283185307179586)) if T is np.float32 else T(2 * np.pi)
    out = np.empty(w.shape, T)
    for h in (0, 1):
        r = np.sqrt(T(-2.0) * np.log(u[:, 2 * h]))
        a = two_pi * u[:, 2 * h + 1]
        out[:, 2 * h], out[:, 2 * h + 1] = r * np.cos(a), r * np.sin(a)
    if "stride" in defects:
        out[VGRID_QUADS:] = np.nan
    return out.reshape(-1)[:n]


SEED2 = 0x9E3779B97F4A7C15                                        # both words non-zero, the high one with its top bit set
NOISE_CASES = [(12345, 0, n) for n in range(1, 10)] + [          # ragged tails of one and two quads and the first element of a third
    (0xDEADBEEF12345678, 0, 1025),                               # high key word; two workgroups, ragged
    (SEED2, 2 ** 32 - 2, 16),                                    # the counter carries into its high word inside the call
    (SEED2, 2 ** 40 + 7, 64),                                    # high counter word
    (SEED2, 3, 4 * VGRID_QUADS + 5),                             # beyond the capped grid: every thread strides once, then a ragged tail
]


def noise_id(case):
    return f"{case[0]:x}-{case[1]:x}-{case[2]}"


def noise_f32_error(case):
    d = np.abs(noise_ref(*case, dtype=np.float32).astype(np.float64) - noise_ref(*case))
    return float(d.max())


# numpy float32 Box-Muller against fp64 on the case's integers, max |difference| (absolute: the values are O(1))
NOISE_F32 = {
    "3039-0-1": 4.127e-08, "3039-0-2": 4.127e-08, "3039-0-3": 4.127e-08,
    "3039-0-4": 1.090e-07, "3039-0-5": 1.090e-07, "3039-0-6": 1.090e-07,
    "3039-0-7": 3.134e-07, "3039-0-8": 3.134e-07, "3039-0-9": 3.134e-07,
    "deadbeef12345678-0-1025": 1.134e-06, "9e3779b97f4a7c15-fffffffe-16": 4.482e-07, "9e3779b97f4a7c15-10000000007-64": 9.881e-07,
    "9e3779b97f4a7c15-3-2097157": 1.842e-04,
}
NOISE_GATE = None                                                 # None: 4 x NOISE_F32 of the case
NOISE_GATE_CAP = 1e-5                                             # a wrong counter or key word is an O(1) error

# ---- uz_step_counters
COUNTERS_N, COUNTERS_IDX = 300, 257                               # 257 distinct indices: two workgroups, the second with one thread

# ================================================================================================ posterior input
PI_HW = [(1, 1), (15, 17), (16, 16), (31, 33), (32, 32), (25, 41), (17, 241)]      # 1, 255, 256, 1 023, 1 024, 1 025, 4 097: ceil(HW / 1 024) workgroups
PI_CH = [(1, 2), (3, 4)]                                           # (in_ch, nlabels)
PI_N = 2


def pi_operands(H, W, in_ch, nlabels):
    rs = np.random.default_rng(13000 + H * W + in_ch)
    patch = rs.standard_normal((PI_N, in_ch, H, W)).astype(np.float32)
    mask = rs.integers(0, nlabels + 1, (PI_N, H, W)).astype(np.float32)           # nlabels itself: outside [0, nlabels)
    mask.reshape(-1)[0] = nlabels
    mask.reshape(-1)[-1] = -1.0
    ref = np.concatenate([patch, np.stack([(mask == k) for k in range(nlabels)], axis=1).astype(np.float32) - np.float32(0.5)], axis=1)
    return patch, mask, ref
