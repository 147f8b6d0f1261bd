"""CPU tier of mask-free inference on volumes (PHISeg3D.predict): the two streamed statistics entry points, their numpy twin
against a direct fp64 evaluation, their refusals, the two plans predict() runs - built on structure-only
models - and the plans of forward() against the op-code lists recorded from the commit before the predict builder was lifted
into models/_hier.py (tests/golden/phiseg3d_plan_ops.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi
from tests import _golden as G
from tests import _predict as P
from tests import _vol_stats as VS

LAYOUTS = [([8, 16, 16], 3), ([8, 16, 16], 2), ([8, 16, 16, 16], 2)]               # level difference 0, 1, 2
CIN, K3, DHW = 4, 3, (16, 32, 32)


def _net(filters, latent_levels, **kw):
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    return PHISeg3D(CIN, K3, filters, latent_levels=latent_levels, device="cpu", **kw)


def _param_names(op):
    return [r[1] for r in op["p"] if isinstance(r, tuple) and r and r[0] in ("param", "pgrad", "buffer")]


def _touching(plan, v, write):
    """The ops of every tape with an operand on v's channels that they write / only read - a 3x3x3 convolution reads a volume
    through its depth window, which Plan._users_of does not follow."""
    from unet_zoo_amd import _ops
    from unet_zoo_amd._plan import View, _buf_of
    hits = []
    for _, ops in plan._all_tapes():
        for o in ops:
            wr = _ops.writes(o)
            for j, r in enumerate(o["p"]):
                if _buf_of(r) is not v.buf:
                    continue
                q = r[1] if isinstance(r, tuple) else getattr(r, "view", None) or r
                if not isinstance(q, View) or (q.c0 < v.c0 + v.C and v.c0 < q.c0 + q.C):
                    if (j in wr) == write:
                        hits.append(o)
    return hits


def test_the_entry_points_are_declared_and_exported():
    L, protos = _ffi.lib(), _ffi.prototypes()
    names = {"uz_vol_sample_accum", "uz_vol_sample_finish"}
    assert names <= set(_ffi.header_symbols()) and all(hasattr(L, n) for n in names)
    assert len(protos["uz_vol_sample_accum"][1]) == 14 and len(protos["uz_vol_sample_finish"][1]) == 10
    assert not any("SAMPLE" in c or "STATS" in c for c in _ffi.op_codes())          # called through the ABI, never a tape op


@pytest.mark.parametrize("K", VS.STATS_K)
@pytest.mark.parametrize("S", VS.STATS_S)
def test_vol_stats_twin_agrees_with_fp64(K, S):
    for i, c in enumerate(VS.CASES):
        levels, flat, ref = VS.vol_case(i, K, S)
        tw = VS.vol_stats_twin(c, levels, S)
        D, H, W = c.dhw
        assert tw["soft"].dtype == np.float32 and tw["labels"].dtype == np.uint8 and tw["labels"].shape == (S, D, H, W)
        assert np.array_equal(tw["labels"], ref["labels"]) and np.array_equal(tw["mean_label"], ref["mean_label"])
        assert G.maxabs(tw["soft"], ref["soft"]) <= P.SOFT_TOL
        assert G.maxabs(tw["mean_soft"], ref["mean_soft"]) <= P.mean_soft_tol(S)
        assert G.maxabs(tw["entropy"], ref["entropy"]) <= P.ENTROPY_TOL
        assert np.all(ref["entropy"] >= 0) and np.all(ref["entropy"] <= np.log(K) + 1e-12)
        assert np.allclose(ref["mean_soft"].sum(axis=0), 1.0, atol=1e-12)


def test_the_resize_is_torchs_nearest_and_the_inputs_are_exact_in_fp32():
    import torch
    import torch.nn.functional as F
    for i, c in enumerate(VS.CASES):
        levels, flat, _ = VS.vol_case(i, 3, 3)
        for lv, fl in zip(levels, flat):
            assert np.array_equal(lv * 4, np.round(lv * 4)) and np.abs(lv).max() <= 8
            want = F.interpolate(torch.from_numpy(lv.copy()), size=list(c.dhw), mode="nearest").numpy()
            assert np.array_equal(fl.reshape(want.shape), want), VS.case_id(c)


@pytest.mark.parametrize("K", [k for k in VS.STATS_K if k >= 2])
def test_every_class_count_has_a_case_with_a_tie(K):
    """First maximum wins is exercised: some voxel's accumulated logits share their maximum between two classes."""
    assert any(P.has_tie(VS.vol_case(i, K, S)[1]) for i in range(len(VS.CASES)) for S in VS.STATS_S)


def test_the_entry_points_refuse_bad_arguments_on_the_host():
    """Every refusal is decided before anything is launched, so it shows without a GPU (tests/test_vol_stats_gpu.py adds that nothing
    was written)."""
    L = _ffi.lib()
    cell = (ctypes.c_double * 64)()
    p = ctypes.addressof(cell)

    def accum(ptrs=(p, p), ctot=(3, 3), f=(1, 2), fz=(1, 2), Lv=2, K=3, dhw=(2, 4, 4), labels=p, acc=p, tables=True):
        n = len(ptrs)
        arr = [(ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*ctot), (ctypes.c_int * n)(*f), (ctypes.c_int * n)(*fz)]
        if not tables:
            arr[0] = None
        return L.uz_vol_sample_accum(*arr, Lv, K, *dhw, labels, None, acc, 1, None)
    for bad in (dict(K=0), dict(K=9), dict(Lv=0), dict(Lv=9), dict(ptrs=(p, None)), dict(tables=False), dict(labels=None), dict(acc=None),
                dict(f=(1, 0)), dict(fz=(0, 2)), dict(ctot=(3, 2)), dict(dhw=(3, 4, 4)), dict(dhw=(2, 4, 6)), dict(dhw=(2, 6, 4)),
                dict(dhw=(0, 4, 4)), dict(dhw=(2048, 1024, 1024))):
        assert accum(**bad) != 0, bad
        assert b"vol_sample_accum" in L.uz_last_error()
    for args in ((None, 3, 2, 2, 4, 4, p, p, p), (p, 3, 2, 2, 4, 4, None, p, p), (p, 0, 2, 2, 4, 4, p, p, p), (p, 9, 2, 2, 4, 4, p, p, p),
                 (p, 3, 0, 2, 4, 4, p, p, p), (p, 3, 2, 2, 0, 4, p, p, p), (p, 3, 2, 2048, 1024, 1024, p, p, p)):
        assert L.uz_vol_sample_finish(*args, None) != 0, args
        assert b"vol_sample_finish" in L.uz_last_error()


# ------------------------------------------------------------------------------------------ the two plans of predict()
@pytest.mark.parametrize("filters,latent_levels", LAYOUTS)
def test_predict_builds_a_trunk_plan_and_a_draw_plan(filters, latent_levels):
    net = _net(filters, latent_levels)
    R, nl, (D, H, W) = len(filters), latent_levels, DHW
    trunk, draw = net._build_predict(D, H, W, "trunk"), net._build_predict(D, H, W, "draw")
    for plan in (trunk, draw):
        assert plan.N == D and not plan.bn_training
        names = [n for o in plan.fwd_ops for n in _param_names(o)]
        assert names and not any(n.startswith("posterior.") for n in names)
        assert not plan.loss_ops and not plan.bwd_ops and not plan.extra_ops
        assert "loss_mask" not in plan.io and "input" not in plan.io
        assert not any(b.b16 for b in plan.bufs)
    assert all(n.startswith("prior.contracting_path.") for o in trunk.fwd_ops for n in _param_names(o))
    assert not any(n.startswith("prior.contracting_path") for o in draw.fwd_ops for n in _param_names(o))
    tcodes, dcodes = [o["code"] for o in trunk.fwd_ops], [o["code"] for o in draw.fwd_ops]
    assert tcodes.count("UZ_OP_AVGPOOL3D_FWD") == R - 1 and tcodes.count("UZ_OP_BN_RELU_FWD") == 3 * R
    assert dcodes.count("UZ_OP_LATENT_FWD") == nl and "UZ_OP_LATENT_FWD" not in tcodes
    assert "UZ_OP_NEAREST3D_FWD" not in dcodes and "UZ_OP_NEAREST3D_FWD" not in tcodes and "UZ_OP_AVGPOOL3D_FWD" not in dcodes
    # the draw plan ends at the un-resized level logits: level l is the volume halved l times, whatever the level difference
    assert draw.io["s"] is None and len(draw.io["s_in"]) == nl and len(draw.io["eps"]) == nl
    assert [(v.N, v.C, v.H, v.W) for v in draw.io["s_in"]] == [(D >> l, K3, H >> l, W >> l) for l in range(nl)]
    # the hand-over: views of equal shape in both plans, levels R-L .. R-2 and the deepest; in the draw plan nothing writes them
    lvls = list(range(R - nl, R - 1)) + [R - 1]
    assert len(trunk.io["feats"]) == len(draw.io["feats"]) == len(lvls) == nl
    for src, dst, lvl in zip(trunk.io["feats"], draw.io["feats"], lvls):
        assert (src.N, src.C, src.H, src.W) == (dst.N, dst.C, dst.H, dst.W) == (D >> lvl, filters[lvl], H >> lvl, W >> lvl)
        assert not draw._users_of(dst)[0] and not _touching(draw, dst, True) and _touching(draw, dst, False)
        assert trunk._users_of(src)[0] and _touching(trunk, src, True)
    full = net._build(D, H, W, False, False)
    assert len(draw.fwd_ops) < len(full.fwd_ops) - len(trunk.fwd_ops)              # (the posterior is gone as well, not just the trunk)
    assert [o["code"] for o in full.fwd_ops].count("UZ_OP_NEAREST3D_FWD") == nl - 1


def test_predict_refuses_what_it_cannot_do_before_touching_the_device():
    import torch
    net = _net([8, 16, 16], 2)
    net.eval()
    with pytest.raises(_ffi.UzError):                                               # structure-only model: no fallback
        net.predict(torch.zeros(1, CIN, 16, 32, 32))
    with pytest.raises(ValueError):
        net._build_predict(10, 32, 32, "trunk")
    with pytest.raises(ValueError):
        net._build_predict(16, 32, 30, "draw")


def test_forward_plans_hold_the_ops_they_held():
    """The op codes of every tape of _build(16, 32, 32, True, True) and (..., False, False), in tape order, for the three layouts."""
    with open(os.path.join(G.GOLDEN, "phiseg3d_plan_ops.json")) as f:
        want = json.load(f)
    assert (want["input_channels"], want["num_classes"], tuple(want["dhw"])) == (CIN, K3, DHW)
    assert [(e["filters"], e["latent_levels"]) for e in want["layouts"]] == LAYOUTS
    L = _ffi.lib()
    mode = L.uz_get_conv_math()
    L.uz_set_conv_math(1)
    try:
        for e in want["layouts"]:
            net = _net(e["filters"], e["latent_levels"])
            for rec in e["plans"]:
                plan = net._build(*rec["build"])
                for tape, ops in (("fwd", plan.fwd_ops), ("loss", plan.loss_ops), ("bwd", plan.bwd_ops)):
                    assert [o["code"] for o in ops] == rec[tape], (e["filters"], e["latent_levels"], rec["build"], tape)
    finally:
        L.uz_set_conv_math(-1 if os.environ.get("UZ_CONV_MATH") is None else mode)
