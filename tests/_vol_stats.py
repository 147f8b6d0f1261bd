"""Shared by tests/test_vol_stats_cpu.py and tests/test_vol_stats_gpu.py: the op-level cases of the streamed volume statistics
(uz_vol_sample_accum / uz_vol_sample_finish, csrc/predict.hip), their numpy twin and their fp64 reference.  Both are the 2-D
kernel's (tests/_predict.py) on the nearest-resized levels with B = 1 and H W := D H W - which is the contract of the pair."""
import collections
import functools

import numpy as np

from tests import _predict as P

STATS_K = (1, 2, 3, 8)
STATS_S = (1, 3)

# (D, H, W), per level (f, fz) finest first, channels beside the K classes, channel offset of the classes
Case = collections.namedtuple("Case", "dhw factors extra c0")


def _pow2(L):
    return tuple((1 << l, 1 << l) for l in range(L))


CASES = [
    Case((1, 1, 1), _pow2(1), 0, 0),                      # a single voxel
    Case((4, 4, 4), _pow2(3), 0, 0),                      # the coarsest level is 1 x 1 x 1
    Case((2, 6, 10), _pow2(2), 0, 0),                     # 120 voxels: a ragged last wave; W % 4 != 0
    Case((3, 8, 33), _pow2(1), 0, 0),                     # odd W
    Case((16, 16, 16), _pow2(5), 0, 0),                   # five levels
    Case((8, 16, 24), _pow2(3), 3, 2),                    # Ctot = K + 3, channel offset 2: a slice of a wider buffer
    Case((4, 8, 8), ((1, 1), (2, 1)), 0, 0),              # factors that differ: level 1 at f = 2, fz = 1
]


def case_id(c):
    return "x".join(map(str, c.dhw)) + f"-L{len(c.factors)}" + (f"-c{c.c0}of+{c.extra}" if c.extra else "")


def level_shape(c, l):
    (D, H, W), (f, fz) = c.dhw, c.factors[l]
    assert D % fz == 0 and H % f == 0 and W % f == 0
    return D // fz, H // f, W // f


def vol_logits(c, K, S):
    """Per level (S, K, D_l, H_l, W_l): integers / 4 in [-8, 8] like tests/_predict.stats_logits - fp32 sums are exact, ties occur."""
    D, H, W = c.dhw
    rng = np.random.Generator(np.random.PCG64(1000 * K + 100 * len(c.factors) + S + 7919 * D * H * W + 31 * c.c0))
    return [(rng.integers(-32, 33, size=(S, K, *level_shape(c, l))) / 4.0).astype(np.float32) for l in range(len(c.factors))]


def resize(c, levels):
    """Nearest resize of every level to the full volume (index od // fz, oy // f, ox // f), flattened to (S, K, 1, D H W)."""
    out = []
    for lv, (f, fz) in zip(levels, c.factors):
        full = lv.repeat(fz, axis=2).repeat(f, axis=3).repeat(f, axis=4)
        assert full.shape[2:] == tuple(c.dhw)
        out.append(np.ascontiguousarray(full.reshape(full.shape[0], full.shape[1], 1, -1)))
    return out


def _unflatten(c, r, S):
    D, H, W = c.dhw
    K = r["soft"].shape[1]
    return dict(soft=r["soft"].reshape(S, K, D, H, W), labels=r["labels"].reshape(S, D, H, W), mean_soft=r["mean_soft"].reshape(K, D, H, W),
                mean_label=r["mean_label"].reshape(D, H, W), entropy=r["entropy"].reshape(D, H, W))


def vol_stats_twin(c, levels, S):
    """The pair in numpy: uz_sample_stats's twin on the resized levels."""
    return _unflatten(c, P.sample_stats_twin(resize(c, levels), 1, S), S)


def vol_stats_f64(c, levels, S):
    return _unflatten(c, P.sample_stats_f64(resize(c, levels), 1, S), S)


@functools.lru_cache(maxsize=None)
def vol_case(i, K, S):
    """(levels, resized levels, fp64 reference) of CASES[i]; computed once and shared between the tests - read-only."""
    c = CASES[i]
    levels = vol_logits(c, K, S)
    flat = resize(c, levels)
    for a in levels + flat:
        a.setflags(write=False)
    return levels, flat, vol_stats_f64(c, levels, S)
