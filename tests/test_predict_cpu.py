"""CPU tier of mask-free inference (PHISeg.predict): the two plans it runs, built on a structure-only model, the plans of
forward() against the op lists recorded before _encoder was split, the new symbols, and the numpy twins of the two kernels
against a direct fp64 evaluation - the twins are the reference of the wiring checks in tests/test_predict_gpu.py."""
import json
import os

import numpy as np
import pytest

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi
from tests import _golden as G
from tests import _predict as P

FILTERS = [4, 8, 8, 8, 8, 8, 8]


def _net():
    from unet_zoo_amd.models.phiseg import PHISeg
    return PHISeg(1, 2, FILTERS, image_size=(1, 64, 64), device="cpu")


def _param_names(op):
    return [r[1] for r in op["p"] if isinstance(r, tuple) and r and r[0] in ("param", "pgrad", "buffer")]


def test_the_two_entry_points_are_declared_and_exported():
    L, protos = _ffi.lib(), _ffi.prototypes()
    assert {"uz_batch_repeat_fwd", "uz_sample_stats"} <= set(_ffi.header_symbols())
    assert hasattr(L, "uz_batch_repeat_fwd") and hasattr(L, "uz_sample_stats")
    assert len(protos["uz_batch_repeat_fwd"][1]) == 10 and len(protos["uz_sample_stats"][1]) == 13
    assert not any("REPEAT" in c or "STATS" in c for c in _ffi.op_codes())           # called through the ABI, never a tape op


def test_predict_builds_a_trunk_plan_and_a_draw_plan():
    B, S = 2, 3
    net = _net()
    trunk = net._build_predict(B, 64, 64, "trunk")
    draw = net._build_predict(B * S, 64, 64, "draw")
    assert trunk.N == B and draw.N == B * S and not trunk.bn_training and not draw.bn_training
    codes = [o["code"] for o in trunk.fwd_ops]
    assert codes.count("UZ_OP_CONV_FWD") == 21 and codes.count("UZ_OP_BN_RELU_FWD") == 21 and codes.count("UZ_OP_AVGPOOL_FWD") == 6
    assert all(o.i("N") == B for o in trunk.fwd_ops if o["code"] == "UZ_OP_CONV_FWD")
    assert all(o.i("N") == B * S for o in draw.fwd_ops if o["code"] == "UZ_OP_CONV_FWD")
    for plan in (trunk, draw):
        names = [n for o in plan.fwd_ops for n in _param_names(o)]
        assert names and not any(n.startswith("posterior.") for n in names)
        assert not plan.loss_ops and not plan.bwd_ops and not plan.extra_ops
        assert "mask" not in plan.io and "loss_mask" not in plan.io
    assert all(n.startswith("prior.contracting_path.") for o in trunk.fwd_ops for n in _param_names(o))
    assert not any(n.startswith("prior.contracting_path") for o in draw.fwd_ops for n in _param_names(o))
    dcodes = [o["code"] for o in draw.fwd_ops]
    assert dcodes.count("UZ_OP_LATENT_HEADS_FWD") == 5 and dcodes.count("UZ_OP_NEAREST_FWD") == 5
    # the hand-over: five views of equal shape in both plans, levels 2 .. 5 and the deepest; in the draw plan nothing writes them
    assert len(trunk.io["feats"]) == len(draw.io["feats"]) == 5
    for src, dst, lvl in zip(trunk.io["feats"], draw.io["feats"], (2, 3, 4, 5, 6)):
        assert (src.C, src.H, src.W) == (dst.C, dst.H, dst.W) == (FILTERS[lvl], 64 >> lvl, 64 >> lvl)
        assert (src.N, dst.N) == (B, B * S)
        writers, readers = draw._users_of(dst)
        assert not writers and readers
    # ... and no bound slot covers the mixed concat buffers: the split convolutions that read them measure the tensor themselves
    for dst in draw.io["feats"][:4]:
        whole = dst.buf
        from unet_zoo_amd._plan import View
        assert draw.amax_in(View(whole)) is None and draw.amax_in(View(whole, 0, 2 * FILTERS[0])) is not None
    assert draw.amax_in(draw.io["feats"][4]) is None
    assert draw.span(draw.io["eps"]) is not None                                   # the five noise buffers fill in one launch
    full = net._build(B * S, 64, 64, False, False)
    assert len(trunk.fwd_ops) + len(draw.fwd_ops) < len(full.fwd_ops)
    assert len(draw.fwd_ops) < len(full.fwd_ops) - len(trunk.fwd_ops)              # (the posterior is gone as well, not just the trunk)


def test_forward_plans_are_op_for_op_what_they_were():
    """(code, i, n) of every op of _build(2, 64, 64, True, True), in tape order, against the lists recorded from the commit before
    _encoder was split into its contracting and its latent half (tests/golden/phiseg_plan_ops.json, default arithmetic mode)."""
    with open(os.path.join(G.GOLDEN, "phiseg_plan_ops.json")) as f:
        want = json.load(f)
    assert want["filters"] == FILTERS and want["build"] == [2, 64, 64, True, True]
    L = _ffi.lib()
    mode = L.uz_get_conv_math()
    L.uz_set_conv_math(1)
    try:
        plan = _net()._build(2, 64, 64, True, True)
    finally:
        L.uz_set_conv_math(-1 if os.environ.get("UZ_CONV_MATH") is None else mode)
    for tape, ops in (("fwd", plan.fwd_ops), ("loss", plan.loss_ops), ("bwd", plan.bwd_ops)):
        got = [[o["code"], [int(v) for v in o["i"]], int(o["n"])] for o in ops]
        assert len(got) == len(want[tape]), tape
        for k, (g, w) in enumerate(zip(got, want[tape])):
            assert g == w, (tape, k, g, w)


def test_predict_refuses_what_it_cannot_do_before_touching_the_device():
    import torch
    from unet_zoo_amd.models.phiseg import PHISeg
    net = _net()
    net.eval()
    with pytest.raises(_ffi.UzError):                                               # structure-only model: no fallback
        net.predict(torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError):
        net._build_predict(1, 96, 96, "trunk")
    assert hasattr(PHISeg, "predict")


@pytest.mark.parametrize("K", P.STATS_K)
@pytest.mark.parametrize("L", P.STATS_L)
def test_sample_stats_twin_agrees_with_fp64(K, L):
    for B, S, H, W in P.stats_cases(K, L):
        levels, ref = P.stats_case(K, L, B, S, H, W)
        tw = P.sample_stats_twin(levels, B, S)
        assert tw["soft"].dtype == np.float32 and tw["labels"].dtype == np.uint8 and tw["labels"].shape == (S * B, H, W)
        assert np.array_equal(tw["labels"], ref["labels"]) and np.array_equal(tw["mean_label"], ref["mean_label"])
        assert G.maxabs(tw["soft"], ref["soft"]) <= P.SOFT_TOL
        assert G.maxabs(tw["mean_soft"], ref["mean_soft"]) <= P.mean_soft_tol(S)
        assert G.maxabs(tw["entropy"], ref["entropy"]) <= P.ENTROPY_TOL
        assert np.all(ref["entropy"] >= 0) and np.all(ref["entropy"] <= np.log(K) + 1e-12)
        assert np.allclose(ref["mean_soft"].sum(axis=1), 1.0, atol=1e-12)


def test_the_op_level_inputs_hold_ties_and_the_entropy_gate_is_what_was_measured():
    ties, worst = 0, 0.0
    for K in P.STATS_K:
        for L in P.STATS_L:
            for B, S, H, W in P.stats_cases(K, L):
                levels, _ = P.stats_case(K, L, B, S, H, W)
                assert all(np.array_equal(lv * 4, np.round(lv * 4)) and np.abs(lv).max() <= 8 for lv in levels)
                ties += P.has_tie(levels)
                worst = max(worst, P.entropy_f32_error([lv.copy() for lv in levels], B, S))
    assert ties >= 1
    print(f"entropy: fp32 torch-CPU evaluation within {worst:.3e} of fp64 on the op-level cases; gate {P.ENTROPY_TOL:.3e}")
    # (the recorded figure, not this host's: another libm or vector width moves the last digit, the gate stays what was written down)
    assert 0.25 * P.ENTROPY_F32_ERROR <= worst <= 1.5 * P.ENTROPY_F32_ERROR and P.ENTROPY_TOL == 4 * P.ENTROPY_F32_ERROR


def test_first_maximum_wins_and_a_zero_probability_adds_no_entropy():
    lv = [np.array([[[[1.0]], [[2.5]], [[2.5]], [[-1.0]]]], np.float32)]             # (1, 4, 1, 1): classes 1 and 2 tie
    tw = P.sample_stats_twin(lv, 1, 1)
    assert tw["labels"].item() == 1 and tw["mean_label"].item() == 1
    for big in (60.0, 500.0):                                                       # p = 7.7e-53, and 0 exactly
        lv = [np.array([[[[big]], [[-big]]]], np.float32)]
        for f in (P.sample_stats_twin, P.sample_stats_f64):
            r = f(lv, 1, 1)
            assert np.isfinite(r["entropy"]).all() and float(np.abs(r["entropy"]).max()) <= 1e-40 and r["mean_label"].item() == 0
    assert P.sample_stats_f64([np.array([[[[500.0]], [[-500.0]]]], np.float32)], 1, 1)["mean_soft"][0, 1, 0, 0] == 0.0


def test_batch_repeat_twin_is_patch_repeat():
    import torch
    x = np.arange(3 * 2 * 2 * 2, dtype=np.float32).reshape(3, 2, 2, 2)
    assert np.array_equal(P.batch_repeat_twin(x, 4), torch.from_numpy(x).repeat(4, 1, 1, 1).numpy())
