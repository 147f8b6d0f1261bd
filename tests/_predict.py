"""Shared by tests/test_predict_cpu.py and tests/test_predict_gpu.py: numpy twins of the two kernels of csrc/predict.hip
(uz_batch_repeat_fwd, uz_sample_stats), a direct fp64 evaluation of the statistics, and the op-level cases with their references,
computed once per process."""
import functools

import numpy as np

# ---- the issue's op-level cases
STATS_K = (1, 2, 3, 8)
STATS_L = (1, 5)
STATS_BS = ((1, 1), (1, 17), (3, 2))
STATS_HW = ((1, 1), (7, 9), (16, 16), (1, 257), (64, 64))            # H*W = 1, 63, 256, 257, 64*64
REPEAT_BS = ((1, 1), (1, 5), (3, 2))
REPEAT_PLANES = ((1, 1), (2, 2), (3, 3), (4, 4), (32, 32))
REPEAT_SIDES = ((8, 0), (13, 0), (13, 3))                            # (Ctot, channel offset) of a C = 8 slice, for x and y alike
REPEAT_C = 8

SOFT_TOL = 1e-6                                                        # the gate of test_accumulate_softmax_argmax


def mean_soft_tol(S):
    """Each of the S terms within SOFT_TOL of fp64, one rounding per ordered fp32 add behind the division."""
    return SOFT_TOL + S * 2.0 ** -24


# Entropy of the mean probabilities: no gate in the project to borrow.  Measured on the op-level cases below: an fp32 torch-CPU
# evaluation of the same formula (entropy_f32_error, asserted in test_predict_cpu.py to stay at or below this figure) is within
# 3.7e-7 of fp64 (measured 3.67e-7); the device's exp / log are not libm's, so the gate is 4 x that.
ENTROPY_F32_ERROR = 3.7e-7
ENTROPY_TOL = 4 * ENTROPY_F32_ERROR


def batch_repeat_twin(x, S):
    """uz_batch_repeat_fwd: y[s*B + b] = x[b]."""
    return np.concatenate([x] * S, axis=0)


def stats_logits(K, L, B, S, H, W, seed=0):
    """L level logits (S*B, K, H, W): integers / 4 in [-8, 8] - sums and argmax are exact in fp32 and ties do occur."""
    rng = np.random.Generator(np.random.PCG64(1000 * K + 100 * L + 10 * B + S + 7919 * H * W + seed))
    return [(rng.integers(-32, 33, size=(S * B, K, H, W)) / 4.0).astype(np.float32) for _ in range(L)]


def _stats(levels, B, S, dt):
    """The statistics in the kernel's order of operations: the levels summed at precision `dt`, last level first; behind the sum
    everything in fp64 - max-shifted softmax, the samples of an image added in the order s = 0 .. S-1, one division, the entropy -
    and rounded to `dt` on the way out; mean_label from the unrounded means; both argmax take the first maximum."""
    acc = levels[-1].astype(dt)
    for lv in levels[:-1]:
        acc = acc + lv.astype(dt)
    labels = np.argmax(acc, axis=1).astype(np.uint8)
    acc = acc.astype(np.float64)
    e = np.exp(acc - acc.max(axis=1, keepdims=True))
    soft = e / e.sum(axis=1, keepdims=True)
    N, K, H, W = soft.shape
    assert N == S * B
    m = np.zeros((B, K, H, W), np.float64)
    for s in range(S):
        m = m + soft[s * B:(s + 1) * B]
    m = m / np.float64(S)
    mean_label = np.argmax(m, axis=1).astype(np.uint8)
    ent = -np.where(m > 0, m * np.log(np.where(m > 0, m, 1.0)), 0.0).sum(axis=1)
    return dict(soft=soft.astype(dt), labels=labels, mean_soft=m.astype(dt), mean_label=mean_label, entropy=ent.astype(dt))


def sample_stats_twin(levels, B, S):
    """uz_sample_stats in numpy: fp32 where the kernel is fp32, fp64 where it is fp64."""
    return _stats(levels, B, S, np.float32)


def sample_stats_f64(levels, B, S):
    """The same quantities evaluated directly in fp64: the reference of the op-level gates."""
    return _stats(levels, B, S, np.float64)


def entropy_f32_error(levels, B, S):
    """max |fp32 torch-CPU evaluation - fp64| of the entropy on one case: what ENTROPY_TOL is derived from."""
    import torch
    acc = torch.from_numpy(levels[-1]).clone()
    for lv in levels[:-1]:
        acc = acc + torch.from_numpy(lv)
    soft = torch.softmax(acc, dim=1)
    m = soft.reshape(S, B, *soft.shape[1:]).sum(dim=0) / S
    ent = -(torch.where(m > 0, m * torch.log(torch.where(m > 0, m, torch.ones_like(m))), torch.zeros_like(m))).sum(dim=1)
    return float(np.max(np.abs(ent.numpy().astype(np.float64) - sample_stats_f64(levels, B, S)["entropy"])))


@functools.lru_cache(maxsize=None)
def stats_case(K, L, B, S, H, W):
    """(levels, fp64 reference) of one op-level case; computed once and shared between the tests - treat both as read-only."""
    levels = stats_logits(K, L, B, S, H, W)
    for lv in levels:
        lv.setflags(write=False)
    return levels, sample_stats_f64(levels, B, S)


def stats_cases(K, L):
    return [(B, S, H, W) for B, S in STATS_BS for H, W in STATS_HW]


def has_tie(levels):
    """Does some pixel's accumulated logit have two classes sharing the maximum?"""
    acc = np.sum(np.stack([lv.astype(np.float64) for lv in levels]), axis=0)
    if acc.shape[1] < 2:
        return False
    top = np.sort(acc, axis=1)
    return bool(np.any(top[:, -1] == top[:, -2]))
