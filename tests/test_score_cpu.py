"""CPU tier of the scoring path (uz_score_samples, metrics.score_prediction, UNetModel.score): the op-level case set of
tests/_score.py has the properties the kernels can get wrong, its expected values reproduce the reference's golden metrics, the
cases tell a kernel without the both-empty convention or with dirty tail bits from a right one, and UNetModel.score's chunk
arithmetic covers a split exactly once."""
import numpy as np
import pytest

from tests import _golden as G
from tests import _score as SC


def test_case_set_spans_the_sizes_the_issue_names():
    assert len(SC.CASES) == len(set(SC.CASES)) == 7 * 3 * 4
    assert {c[0] for c in SC.CASES} == {1, 63, 64, 65, 127, 1024, 4097} and {c[1] for c in SC.CASES} == {2, 3, 8}
    assert {c[2:] for c in SC.CASES} == {(1, 1, 1), (1, 7, 4), (3, 2, 4), (2, 6, 3)}
    assert SC.CONSTANT_SOFT in SC.CASES
    for c in SC.CASES:
        v = SC.case(*c)
        P, K, B, S, A = c
        assert v.labels.shape == (S, B, P) and v.ann.shape == (B, A, P) and v.mean_label.shape == (B, P)
        assert v.labels.dtype == v.ann.dtype == v.mean_label.dtype == np.uint8
        assert (v.soft is None) == (P == 1)
        if v.soft is not None:
            assert v.soft.shape == (S, B, K, P) and v.soft.dtype == np.float32
            assert np.allclose(v.soft.sum(axis=2), 1.0, atol=1e-6) and v.soft.min() > 0


def test_case_set_holds_empty_pairs_ragged_words_and_out_of_range_labels():
    both = one = ragged = big = 0
    for c in SC.CASES:
        P, K, B, S, A = c
        v = SC.case(*c)
        for b in range(B):
            for l in range(1, K):
                s_has = (v.labels[:, b] == l).any(axis=1)
                y_has = (v.ann[b] == l).any(axis=1)
                both += int((~s_has).any() and (~y_has).any())
                one += int((s_has.any() and (~y_has).any()) or ((~s_has).any() and y_has.any()))
        if P % 64:
            t = P - P % 64
            ragged += int(any((v.labels[s, b, t:] == 1).all() and (v.ann[b, j, t:] == 1).all()
                              for s in range(S) for b in range(B) for j in range(A)))
        big += int((v.labels >= K).any() and (v.ann >= K).any())
    print(f"both-empty {both}, exactly-one-empty {one}, ragged all-ones tail {ragged}, values >= K {big}")
    assert both > 0 and one > 0 and ragged > 0 and big > 0


def test_only_the_constant_soft_case_has_a_non_finite_ncc():
    for c in SC.CASES:
        e = SC.expected(*c)
        if not SC.has_soft(c):
            assert e.ncc is None
        elif c == SC.CONSTANT_SOFT:
            assert not np.isfinite(e.ncc).any(), c
        else:
            assert np.isfinite(e.ncc).all(), (c, e.ncc)
        assert np.isfinite(e.ged).all() and np.isfinite(e.dice).all()


def test_expected_values_reproduce_the_golden_metrics_as_a_batch():
    arrays, meta = G.load("metrics")
    seen = []
    for names, labels, ann, soft in SC.golden_batches(arrays):
        mean_label = labels[0]                                          # any map: the golden file holds no Dice
        e = SC.expected_from(labels, ann, mean_label, soft, 2)
        for b, n in enumerate(names):
            assert abs(e.ged[b] - meta[f"{n}_ged"]) <= 1e-12, n
            assert abs(e.ncc[b] - meta[f"{n}_ncc"]) <= 1e-6, n
            seen.append(n)
    assert seen == ["m0", "m1", "m2"]
    (_, labels, ann, _), _ = SC.golden_batches(arrays)
    assert labels.shape[:2] == (6, 2) and ann.shape[:2] == (2, 4)
    assert not (labels[:, 1] == 1).any(axis=1).all() and not (ann[1] == 1).any(axis=1).all()      # m1: an empty sample, an empty annotator


def test_cases_tell_the_both_empty_convention_and_dirty_tail_bits():
    """ged_from_counts on numpy's counts IS the oracle's GED (1e-12) on every case; with the both-empty IoU dropped to 0, or with
    the bits beyond P set in every plane, the GED (or the counts) of at least one case moves."""
    moved_empty = moved_tail_ged = moved_tail_counts = 0
    for c in SC.CASES:
        P, K, B, S, A = c
        v, e = SC.case(*c), SC.expected(*c)
        assert np.abs(SC.ged_from_counts(e.counts, S, A) - e.ged).max() <= 1e-12, c
        moved_empty += int(np.abs(SC.ged_from_counts(e.counts, S, A, both_empty=0.0) - e.ged).max() > 1e-6)
        dirty = SC.np_counts(v.labels, v.ann, K, tail_bits=True)
        assert (P % 64 == 0) == np.array_equal(dirty, e.counts)
        moved_tail_counts += int(not np.array_equal(dirty, e.counts))
        moved_tail_ged += int(np.abs(SC.ged_from_counts(dirty, S, A) - e.ged).max() > 1e-6)
    print(f"cases moved: both-empty dropped {moved_empty}, tail bits: counts {moved_tail_counts}, GED {moved_tail_ged}")
    assert moved_empty > 0 and moved_tail_counts > 0 and moved_tail_ged > 0


@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("per_call", [1, 2, 8])
def test_score_chunks_cover_every_image_once_and_pad_only_the_last_call(n, per_call):
    from unet_zoo_amd.train_model import score_chunks
    chunks = score_chunks(n, per_call)
    size = min(per_call, n)
    assert len(chunks) == -(-n // size)
    kept = []
    for i, (idx, keep) in enumerate(chunks):
        assert len(idx) == size and 1 <= keep <= size                   # one call shape
        assert keep == size or i == len(chunks) - 1                     # only the last call is padded
        assert idx[keep:] == [idx[keep - 1]] * (size - keep)            # ... with copies of its last image
        kept += idx[:keep]
    assert kept == list(range(n))                                       # every image once, in order; exactly the padding dropped
    with pytest.raises(ValueError):
        score_chunks(0, per_call)
    with pytest.raises(ValueError):
        score_chunks(n, 0)


def test_default_images_per_call_follows_the_row_budget():
    from unet_zoo_amd.train_model import SCORE_IMAGES_PER_CALL, default_images_per_call
    from unet_zoo_amd.models import PHISeg, ProbabilisticUnet
    assert SCORE_IMAGES_PER_CALL == 8
    assert [default_images_per_call(S) for S in (1, 10, 100)] == [8, 8, 8]                  # no budget: ProbabilisticUnet
    assert not hasattr(ProbabilisticUnet, "predict_rows_budget")
    budget = PHISeg.predict_rows_budget
    assert [default_images_per_call(S, budget) for S in (1, 10, 16, 17, 64, 100, 1000)] == [8, 8, 8, 7, 2, 1, 1]
