"""Shared by tests/test_score_cpu.py and tests/test_score_gpu.py: the op-level cases of uz_score_samples (csrc/score.hip) and their
expected values.  The expected GED, NCC and Dice come from oracle.metrics - pinned to the reference's own functions by
tests/golden/metrics.* - applied per image; the expected pair counts are numpy integer counts.  Nothing here restates a metric:
ged_from_counts exists only to show that the case set discriminates (test_score_cpu.py ties it to the oracle's GED first, then
mutates it)."""
import functools
import types

import numpy as np

from oracle import metrics as OM

PS = (1, 63, 64, 65, 127, 1024, 4097)              # below, at and above one word and one 64-word stretch of a wave
KS = (2, 3, 8)
BSA = ((1, 1, 1), (1, 7, 4), (3, 2, 4), (2, 6, 3))
CONSTANT_SOFT = (64, 2, 1, 7, 4)                   # the one case whose soft is constant: its NCC is not finite
CASES = [(P, K, B, S, A) for P in PS for K in KS for (B, S, A) in BSA]


def has_soft(case):
    """A map of one pixel has no variance, so its NCC is 0 / 0 whatever the inputs: the P = 1 cases carry no `soft` (and so cover the
    soft = null route); every other case has one."""
    return case[0] > 1


def n_pairs(S, A):
    return S * A + S * S + A * A


@functools.lru_cache(maxsize=None)
def case(P, K, B, S, A):
    """Seeded inputs of one case (read-only): labels (S, B, P), ann (B, A, P), mean_label (B, P) uint8, soft (S, B, K, P) fp32 or None.
    By (B, S, A) the label maps are bent so that the set holds what the kernels can get wrong:
      (1, 7, 4)  the last label is absent from every sample and every annotator (both empty), and sample 0 also lacks label 1, which
                 the annotators carry from P >= 63 on (exactly one empty)
      (3, 2, 4)  sample 0 of image 1 lacks label 1 (exactly one empty); annotator 2 of image 2 is empty of every label but 0
      (2, 6, 3)  the last P % 64 pixels of sample 0 and annotator 0 of image 0 carry label 1 (a ragged last word that is all ones)
      (1, 1, 1)  from P >= 63 on, pixel 0 of the sample holds K and pixel 1 of the annotator 255: values >= K set no bit"""
    rng = np.random.Generator(np.random.PCG64(7919 * P + 101 * K + 17 * B + 5 * S + A))
    p = rng.dirichlet(np.ones(K) * 2.0)            # uneven label densities
    draw = lambda *shape: rng.choice(K, size=shape, p=p).astype(np.uint8)
    labels, ann, mean_label = draw(S, B, P), draw(B, A, P), draw(B, P)
    if (B, S, A) == (1, 7, 4):
        for m in (labels, ann, mean_label):
            m[m == K - 1] = 0
        if K > 2:                                    # (K = 2: label 1 IS the last label and stays absent everywhere)
            labels[0][labels[0] == 1] = 0
            if P >= 63:
                ann[0, :, 5] = 1
    elif (B, S, A) == (3, 2, 4):
        labels[0, 1][labels[0, 1] == 1] = 0
        if P >= 63:
            ann[1, :, 3] = 1
        ann[2, 2] = 0
    elif (B, S, A) == (2, 6, 3):
        if P % 64:
            labels[0, 0, P - P % 64:] = 1
            ann[0, 0, P - P % 64:] = 1
    elif P >= 63:
        labels[0, 0, 0] = K
        ann[0, 0, 1] = 255
    soft = None
    if has_soft((P, K, B, S, A)):
        if (P, K, B, S, A) == CONSTANT_SOFT:
            soft = np.full((S, B, K, P), 1.0 / K, np.float32)
        else:
            z = rng.standard_normal((S, B, K, P)) * 2.0
            e = np.exp(z - z.max(axis=2, keepdims=True))
            soft = (e / e.sum(axis=2, keepdims=True)).astype(np.float32)
        soft.setflags(write=False)
    for m in (labels, ann, mean_label):
        m.setflags(write=False)
    return types.SimpleNamespace(P=P, K=K, B=B, S=S, A=A, labels=labels, ann=ann, mean_label=mean_label, soft=soft)


def np_counts(labels, ann, K, tail_bits=False):
    """(B, K, S*A + S*S + A*A, 3) int64 in uz_score_samples' layout: per image and label the matrices samples x annotators, samples x
    samples, annotators x annotators, each [i][j] -> intersection, |first|, |second|.  tail_bits=True is the MUTANT of a kernel that
    leaves the bits from P to the end of the last word set in every plane."""
    S, B, P = labels.shape
    A = ann.shape[1]
    pad = (-P) % 64 if tail_bits else 0
    out = np.zeros((B, K, n_pairs(S, A), 3), np.int64)
    for b in range(B):
        for k in range(K):
            s, y = (labels[:, b] == k), (ann[b] == k)
            t = 0
            for first, second in ((s, y), (s, s), (y, y)):
                for u in first:
                    for v in second:
                        out[b, k, t] = (np.count_nonzero(u & v) + pad, np.count_nonzero(u) + pad, np.count_nonzero(v) + pad)
                        t += 1
    return out


def ged_from_counts(counts, S, A, both_empty=1.0):
    """GED per image from a counts array - NOT the expected value (that is oracle.metrics'), only the handle by which
    test_score_cpu.py mutates the both-empty convention and the counts."""
    B, K = counts.shape[:2]
    c = counts[:, 1:].astype(np.float64)
    inter, ca, cb = c[..., 0], c[..., 1], c[..., 2]
    iou = np.where((ca == 0) & (cb == 0), both_empty, np.where((ca == 0) | (cb == 0), 0.0, inter / np.maximum(ca + cb - inter, 1)))
    d = 1 - iou.sum(axis=1) / (K - 1)                                                  # (B, NP)
    sy, ss, yy = d[:, :S * A].sum(axis=1), d[:, S * A:S * A + S * S].sum(axis=1), d[:, S * A + S * S:].sum(axis=1)
    return (2.0 / (S * A)) * sy - (1.0 / S ** 2) * ss - (1.0 / A ** 2) * yy


def expected_from(labels, ann, mean_label, soft, K):
    """oracle.metrics per image: ged (B), dice (B, A, K), ncc (B) or None; counts from numpy."""
    S, B, P = labels.shape
    A = ann.shape[1]
    li, ai, mi = labels.astype(np.int64), ann.astype(np.int64), mean_label.astype(np.int64)
    ged = np.array([OM.generalised_energy_distance(li[:, b], ai[b], nlabels=K - 1, label_range=range(1, K)) for b in range(B)])
    dice = np.array([[OM.per_label_dice(mi[b], ai[b, j], K) for j in range(A)] for b in range(B)], np.float64)
    ncc = None
    if soft is not None:
        with np.errstate(all="ignore"):
            ncc = np.array([float(np.asarray(OM.variance_ncc_dist(soft[:, b], np.stack([(ai[b] == k) for k in range(K)], axis=1).astype(np.int64))).reshape(-1)[0])
                            for b in range(B)])
    return types.SimpleNamespace(ged=ged, dice=dice, ncc=ncc, counts=np_counts(labels, ann, K))


@functools.lru_cache(maxsize=None)
def expected(P, K, B, S, A):
    """Expected values of one case, computed once per process and shared: treat as read-only."""
    c = case(P, K, B, S, A)
    return expected_from(c.labels, c.ann, c.mean_label, c.soft, K)


def golden_batches(arrays):
    """tests/golden/metrics.*'s m0, m1, m2 as batches: m0 and m1 share S = 6, A = 4 and stack to B = 2; m2 (S = 4, A = 3) is a batch
    of one.  -> list of (names, labels (S, B, P), ann (B, A, P), soft (S, B, K, P))."""
    out = []
    for names in (("m0", "m1"), ("m2",)):
        labels = np.stack([arrays[f"{n}_samples"].reshape(arrays[f"{n}_samples"].shape[0], -1) for n in names], axis=1)
        ann = np.stack([arrays[f"{n}_gts"].reshape(arrays[f"{n}_gts"].shape[0], -1) for n in names], axis=0)
        soft = np.stack([arrays[f"{n}_soft"].reshape(*arrays[f"{n}_soft"].shape[:2], -1) for n in names], axis=1)
        out.append((names, np.ascontiguousarray(labels), np.ascontiguousarray(ann), np.ascontiguousarray(soft)))
    return out
