"""Shared by tests/test_volwindow_cpu.py and tests/test_volwindow_gpu.py: whole volumes from blended windows
(PHISeg3D.predict_volume; uz_vol_window_gather / _accum / _finish, csrc/volwindow.hip).  A numpy restatement of the window grid and
the blend weights, a numpy twin of accum + finish in the kernels' order of operations, a direct evaluation in extended precision,
the rule that says where labels must agree, and the op-level cases.

Logits are integers / 4 in [-8, 8] (tests/_vol_stats.py): the fp32 level sums are exact.  Independent random logits per window
would make an exact tie of a voxel's blended classes - and a near tie that an fp32 rounding closes - vanishingly rare once a
voxel is covered twice, so both are planted, block-wise (a block = g^3 voxels of the padded volume; origins are multiples of g, so
a block is a block of every window that covers it):
  * tie blocks: in EVERY covering window two classes are set to the element's maximum over the classes at every level - a structural
    tie at the top, first maximum wins: classes (0, 1) in block 0, (K-2, K-1) in the others;
  * near-tie blocks (K >= 3, covered at least twice): as above for classes (0, 1) in every covering window but the last one visited;
    there class 2 is +8, class 0 -8, class 1 -7.75 and the rest -8 at the finest level and every class 0 at the coarser ones: class 1
    leads class 0 by about 1e-8 of their blended value - plain in fp64, mostly gone after a rounding to fp32."""
import collections
import functools
import itertools

import numpy as np

from tests import _predict as P

STATS_K = (1, 2, 3, 8)
STATS_S = (1, 3)
BLENDS = ("gaussian", "uniform")
REL_GAP = 1e-12                     # labels must agree where the two largest blended values differ by more than this share of the larger
EXEMPT_CAP = 0.01                   # ... or tie structurally; the voxels left over are at most this share of a case, per sample

# volume, window, stride (None: the default), g, per level (f, fz) finest first, channels beside the classes, channel offset
Case = collections.namedtuple("Case", "dhw window stride g factors extra c0")


def _pow2(L):
    return tuple((1 << l, 1 << l) for l in range(L))


CASES = [
    Case((13, 10, 19), (8, 8, 8), (4, 4, 4), 4, _pow2(3), 0, 0),                  # 24 windows, overhang on all axes, up to 8-fold overlap, odd W
    Case((5, 7, 9), (8, 8, 8), (4, 4, 4), 4, _pow2(1), 0, 0),                     # shrunk and overhanging windows, two along W
    Case((16, 16, 16), (8, 8, 8), (8, 8, 8), 4, _pow2(3), 3, 2),                  # disjoint cover; Ctot = K + 3, channel offset 2
    Case((9, 20, 33), (8, 16, 16), (4, 8, 4), 4, ((1, 1), (2, 1)), 0, 0),         # non-cubic; f and fz differ
    Case((8, 8, 24), (8, 8, 16), (8, 8, 8), 8, _pow2(3), 0, 0),                   # overlap on one axis
    Case((1, 1, 1), (4, 4, 4), None, 4, _pow2(1), 0, 0),                          # a single voxel
]
WINDOW_COUNTS = (24, 2, 8, 24, 2, 1)


def case_id(c):
    return "x".join(map(str, c.dhw)) + "-w" + "x".join(map(str, c.window)) + f"-L{len(c.factors)}" + (f"-c{c.c0}of+{c.extra}" if c.extra else "")


# ------------------------------------------------------------------------------------------ grid and weights, restated
def default_stride(window, g):
    return tuple(max(g, (w // 2) // g * g) for w in window)


def window_grid(dhw, window, stride, g):
    """(padded, extent, origins): the issue's rule, written per axis."""
    stride = default_stride(window, g) if stride is None else stride
    padded, extent, axes = [], [], []
    for n, w, s in zip(dhw, window, stride):
        P_ = (n + g - 1) // g * g
        padded.append(P_)
        if P_ <= w:
            extent.append(P_)
            axes.append([0])
        else:
            o, k = [], 0
            while k * s < P_ - w:
                o.append(k * s)
                k += 1
            extent.append(w)
            axes.append(o + [P_ - w])
    return tuple(padded), tuple(extent), list(itertools.product(*axes))


def blend_tables(extent, blend):
    out = []
    for w in extent:
        i = np.arange(w, dtype=np.float64)
        out.append(np.exp(-0.5 * ((i - (w - 1) / 2.0) / (w / 8.0)) ** 2) if blend == "gaussian" else np.ones(w, np.float64))
    return out


def gather_twin(src, origin, extent):
    """uz_vol_window_gather: the window of src (C, D, H, W), zero beyond the volume -> (C, wd, wh, ww)."""
    out = np.zeros((src.shape[0], *extent), src.dtype)
    hi = [min(n - o, e) for n, o, e in zip(src.shape[1:], origin, extent)]
    if min(hi) > 0:
        out[:, :hi[0], :hi[1], :hi[2]] = src[:, origin[0]:origin[0] + hi[0], origin[1]:origin[1] + hi[1], origin[2]:origin[2] + hi[2]]
    return out


# ------------------------------------------------------------------------------------------ accum + finish
DEFECTS = ("drop_last_window", "uniform_for_gaussian", "divide_by_count", "overhang_modulo", "order_transposed", "labels_after_rounding")


def _resized(lv, f, fz):
    return lv.repeat(fz, axis=-3).repeat(f, axis=-2).repeat(f, axis=-1)


def summed_logits(levels, factors, dt):
    """One window: the levels (S, K, d_l, h_l, w_l) resized to the window and summed at precision dt, last level first."""
    a = _resized(levels[-1], *factors[-1]).astype(dt)
    for lv, fac in zip(levels[:-1], factors[:-1]):
        a = a + _resized(lv, *fac).astype(dt)
    return a


def evaluate(dhw, extent, origins, tables, factors, win_levels, S, prec, defect=None):
    """Accum over the windows in the order given, then finish.  win_levels[i] are the levels of the i-th window VISITED.
    prec = "twin": the kernels' arithmetic - fp32 level sums, then fp64: max-shifted softmax added in class order, weight
    (tz ty) tx, product and sum rounded separately, labels from the unnormalised accumulators, one division by the weight sum, the
    samples added in order, one division by S; soft / mean_soft / entropy rounded to fp32.  prec = "ref": the same quantities with
    everything in extended precision (np.longdouble), returned as fp64.  defect: one of DEFECTS - a deliberately wrong evaluation."""
    D, H, W = dhw
    dt = np.float64 if prec == "twin" else np.longdouble
    K = win_levels[0][0].shape[1]
    origins = list(origins)
    if defect == "drop_last_window":
        last = [max(o[a] for o in origins) for a in range(3)]
        origins = [o if not any(o[a] == last[a] and last[a] > 0 for a in range(3)) else None for o in origins]
    if defect == "order_transposed":
        axes = [sorted({o[a] for o in origins}) for a in range(3)]
        origins = [(z, y, x) for x in axes[2] for y in axes[1] for z in axes[0]]
    if defect == "uniform_for_gaussian":
        tables = [np.ones_like(t) for t in tables]
    wt = ((tables[0].astype(dt)[:, None, None] * tables[1].astype(dt)[None, :, None]) * tables[2].astype(dt)[None, None, :])
    acc, wsum, count = np.zeros((S, K, D, H, W), dt), np.zeros((D, H, W), dt), np.zeros((D, H, W), dt)
    for o, levels in zip(origins, win_levels):
        if o is None:
            continue
        a = summed_logits(levels, factors, np.float32 if prec == "twin" else np.longdouble).astype(dt)
        e = np.exp(a - a.max(axis=1, keepdims=True))
        se = np.zeros_like(e[:, 0])
        for k in range(K):
            se = se + e[:, k]
        sv = e / se[:, None]
        if defect == "overhang_modulo":
            idx = np.ix_((o[0] + np.arange(extent[0])) % D, (o[1] + np.arange(extent[1])) % H, (o[2] + np.arange(extent[2])) % W)
            for s in range(S):
                for k in range(K):
                    acc[s, k][idx] = acc[s, k][idx] + wt * sv[s, k]
            wsum[idx] = wsum[idx] + wt
            count[idx] += 1
            continue
        hi = [min(n - q, w) for n, q, w in zip(dhw, o, extent)]
        if min(hi) <= 0:
            continue
        vol = (slice(o[0], o[0] + hi[0]), slice(o[1], o[1] + hi[1]), slice(o[2], o[2] + hi[2]))
        win = (slice(0, hi[0]), slice(0, hi[1]), slice(0, hi[2]))
        acc[(slice(None), slice(None)) + vol] += wt[win] * sv[(slice(None), slice(None)) + win]
        wsum[vol] += wt[win]
        count[vol] += 1
    div = count if defect == "divide_by_count" else wsum
    with np.errstate(invalid="ignore", divide="ignore"):
        p = acc / div
        m = np.zeros((K, D, H, W), dt)
        for s in range(S):
            m = m + p[s]
        m = m / dt(S)
        ent = -np.where(m > 0, m * np.log(np.where(m > 0, m, 1.0)), 0.0).sum(axis=0)
    out_dt = np.float32 if prec == "twin" else np.float64
    labels = np.argmax(p.astype(np.float32) if defect == "labels_after_rounding" else acc, axis=1).astype(np.uint8)
    return dict(soft=p.astype(out_dt), labels=labels, mean_soft=m.astype(out_dt), mean_label=np.argmax(m, axis=0).astype(np.uint8),
                entropy=ent.astype(out_dt), blend=p.astype(np.float64), mean=m.astype(np.float64), count=count.astype(np.int64))


def _top_two(v):
    """v (K, ...) -> indices of the largest and the second largest class (first maximum first) and their relative gap."""
    order = np.argsort(-v, axis=0, kind="stable")
    i1, i2 = order[0], order[1]
    a, b = np.take_along_axis(v, i1[None], 0)[0], np.take_along_axis(v, i2[None], 0)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(a > 0, (a - b) / a, 0.0)
    return i1, i2, gap


def must_match(dhw, extent, origins, factors, win_levels, S, ref, dt=np.float64):
    """Where labels (S, D, H, W) and mean_label (D, H, W) are pinned: the reference's two largest blended values differ by more than
    REL_GAP of the larger, or the two classes have identical summed logits in every covering window (for the mean: in every sample
    too) - a structural tie, first maximum.  K = 1: everywhere.  dt: the precision the logits are summed at (np.float32 for logits
    whose fp32 sums are not exact: the kernel's own sum)."""
    D, H, W = dhw
    K = win_levels[0][0].shape[1]
    if K == 1:
        return np.ones((S, D, H, W), bool), np.ones((D, H, W), bool), np.zeros((S, D, H, W), bool)
    tops = [_top_two(ref["blend"][s]) for s in range(S)]
    mtop = _top_two(ref["mean"])
    struct, mstruct = np.ones((S, D, H, W), bool), np.ones((S, D, H, W), bool)
    for o, levels in zip(origins, win_levels):
        hi = [min(n - q, w) for n, q, w in zip(dhw, o, extent)]
        if min(hi) <= 0:
            continue
        a = summed_logits(levels, factors, dt)[:, :, :hi[0], :hi[1], :hi[2]]
        vol = (slice(o[0], o[0] + hi[0]), slice(o[1], o[1] + hi[1]), slice(o[2], o[2] + hi[2]))
        for s in range(S):
            for dst, (i1, i2, _) in ((struct, tops[s]), (mstruct, mtop)):
                same = np.take_along_axis(a[s], i1[vol][None], 0)[0] == np.take_along_axis(a[s], i2[vol][None], 0)[0]
                dst[(s,) + vol] &= same
    pin = np.stack([tops[s][2] > REL_GAP for s in range(S)]) | struct
    return pin, (mtop[2] > REL_GAP) | mstruct.all(axis=0), struct


def gates(got, twin, ref, pins, S, against=None):
    """What a result has to meet: (failures, figures).  Labels and mean_label equal the twin's on the pinned voxels; soft, mean_soft
    and entropy lie within the project's gates (tests/_predict.py) of `against` (default: the extended-precision reference)."""
    against = ref if against is None else against
    pin, mpin = pins[0], pins[1]
    fig = dict(labels=int(np.sum((np.asarray(got["labels"]) != twin["labels"]) & pin)),
               mean_label=int(np.sum((np.asarray(got["mean_label"]) != twin["mean_label"]) & mpin)))
    tol = dict(soft=P.SOFT_TOL, mean_soft=P.mean_soft_tol(S), entropy=P.ENTROPY_TOL)
    for k in tol:
        if got.get(k) is not None:
            d = np.abs(np.asarray(got[k], np.float64) - np.asarray(against[k], np.float64))
            fig[k] = float("inf") if not np.all(np.isfinite(d)) else float(d.max())
    failed = [k for k in ("labels", "mean_label") if fig[k]] + [k for k in tol if k in fig and not fig[k] <= tol[k]]
    return failed, fig


# ------------------------------------------------------------------------------------------ the case set
def level_shape(extent, fac):
    f, fz = fac
    assert extent[0] % fz == 0 and extent[1] % f == 0 and extent[2] % f == 0
    return extent[0] // fz, extent[1] // f, extent[2] // f


def _blocks(c, padded, extent, origins):
    """The planted blocks of a case: {block index: ("tie", (a, b)) | ("near", last covering window)} - see the module docstring."""
    g = c.g
    nb = tuple(p // g for p in padded)
    cover = collections.defaultdict(list)
    for i, o in enumerate(origins):
        for b in itertools.product(*[range(o[a] // g, (o[a] + extent[a]) // g) for a in range(3)]):
            cover[b].append(i)
    inside = [b for b in itertools.product(*map(range, nb)) if all(b[a] * g < c.dhw[a] for a in range(3))]
    plan = {b: "tie_first" if b == (0, 0, 0) else "tie_last" for b in inside if b == (0, 0, 0) or sum(b) % 5 == 2}
    twice = [b for b in inside if len(cover[b]) >= 2 and b not in plan]
    for b in ([twice[0], twice[-1]] if twice else []):
        plan[b] = "near"
    return plan, cover


def window_logits(c, K, S):
    """Per window visited, per level (S, K, d_l, h_l, w_l) fp32: random integers / 4 in [-8, 8] with the planted blocks."""
    padded, extent, origins = window_grid(c.dhw, c.window, c.stride, c.g)
    rng = np.random.Generator(np.random.PCG64(1000 * K + 100 * len(c.factors) + S + 7919 * int(np.prod(c.dhw)) + 31 * c.c0))
    wins = [[(rng.integers(-32, 33, size=(S, K, *level_shape(extent, fac))) / 4.0).astype(np.float32) for fac in c.factors] for _ in origins]
    plan, cover = _blocks(c, padded, extent, origins)
    g = c.g
    for b, kind in plan.items():
        if K < 2 or (kind == "near" and K < 3):
            continue
        for i in cover[b]:
            for l, (f, fz) in enumerate(c.factors):
                lo = [(b[a] * g - origins[i][a]) // q for a, q in enumerate((fz, f, f))]
                n = [g // fz, g // f, g // f]
                el = (slice(None), slice(None), slice(lo[0], lo[0] + n[0]), slice(lo[1], lo[1] + n[1]), slice(lo[2], lo[2] + n[2]))
                blk = wins[i][l][el]
                if kind == "near" and i == cover[b][-1]:
                    blk[:] = 0.0
                    if l == 0:
                        blk[:] = -8.0
                        blk[:, 2] = 8.0
                        blk[:, 1] = -7.75
                else:
                    pair = (K - 2, K - 1) if kind == "tie_last" else (0, 1)
                    top = blk.max(axis=1)
                    blk[:, pair[0]] = top
                    blk[:, pair[1]] = top
                wins[i][l][el] = blk
    return wins


@functools.lru_cache(maxsize=None)
def case(i, K, S, blend):
    """Everything the tests need of CASES[i], computed once and shared (read-only): grid, weight tables, logits per window, twin,
    reference, and where the labels are pinned."""
    c = CASES[i]
    padded, extent, origins = window_grid(c.dhw, c.window, c.stride, c.g)
    tables = blend_tables(extent, blend)
    wins = window_logits(c, K, S)
    for w in wins:
        for lv in w:
            lv.setflags(write=False)
    args = (c.dhw, extent, origins, tables, c.factors, wins, S)
    ref = evaluate(*args, "ref")
    return dict(c=c, padded=padded, extent=extent, origins=origins, tables=tables, wins=wins, args=args, twin=evaluate(*args, "twin"), ref=ref,
                pins=must_match(c.dhw, extent, origins, c.factors, wins, S, ref))


def all_keys():
    return [(i, K, S, b) for i in range(len(CASES)) for K in STATS_K for S in STATS_S for b in BLENDS]
