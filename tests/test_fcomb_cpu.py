"""CPU tier of ProbabilisticUnet.predict: the two new symbols, what predict() refuses before it touches a device, the launch
uz_fcomb_sample_route reports for the op-level shapes, what the entry point refuses without a launch, the op-level inputs (every
unit's BatchNorm must matter), the numpy twin and the recorded fp32 figure against a direct fp64 evaluation, and the oracle's
margins on the model-level cases - tests/test_fcomb_gpu.py compares the device with these references."""
import ctypes as C

import numpy as np
import pytest

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi
from tests import _fcomb as F
from tests import _golden as G

ALL_CASES = [c for H, W in F.PLANES for c in F.cases(H, W)]
UNIQUE_INPUTS = list({F.case_key(c): c for c in ALL_CASES}.values())              # cases that differ by the forced kernel only share inputs


def test_the_two_entry_points_are_declared_and_exported():
    L, protos = _ffi.lib(), _ffi.prototypes()
    assert {"uz_fcomb_sample_fwd", "uz_fcomb_sample_route"} <= set(_ffi.header_symbols())
    assert hasattr(L, "uz_fcomb_sample_fwd") and hasattr(L, "uz_fcomb_sample_route")
    assert len(protos["uz_fcomb_sample_fwd"][1]) == 18 and len(protos["uz_fcomb_sample_route"][1]) == 8
    assert protos["uz_fcomb_sample_fwd"][1][8] is C.c_float                         # bn_eps
    assert not any("FCOMB" in c for c in _ffi.op_codes())                           # called through the ABI, never a tape op


def _cpu_net(**kw):
    from unet_zoo_amd.models.probabilistic_unet import ProbabilisticUnet
    return ProbabilisticUnet(1, 2, F.FILTERS, latent_dim=F.LATENT, no_convs_fcomb=3, image_size=(1, F.H0, F.H0), device="cpu", **kw)


def test_predict_refuses_what_it_cannot_do_before_touching_the_device():
    import torch
    from unet_zoo_amd.models.probabilistic_unet import ProbabilisticUnet
    from unet_zoo_amd.models.phiseg import Prediction  # noqa: F401
    assert hasattr(ProbabilisticUnet, "predict")
    x = torch.zeros(1, 1, F.H0, F.H0)
    net = _cpu_net()
    net.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        net.predict(x)
    net.eval()
    for bad in (0, -3):
        with pytest.raises(ValueError):
            net.predict(x, n_samples=bad)
    rev = _cpu_net(reversible=True)
    rev.eval()
    with pytest.raises(NotImplementedError):
        rev.predict(x)
    with pytest.raises(_ffi.UzError, match="no GPU"):                               # structure-only model: no fallback
        net.predict(x, n_samples=2)
    refs = net._fcomb_param_refs()
    assert len(refs) == 6 * 2 + 2 and refs[0][1] == "fcomb.layers.0.convolution.0.weight" and refs[-1][1] == "fcomb.last_layer.bias"
    assert [r[1].rsplit(".", 1)[1] for r in refs[6:12]] == ["weight", "bias", "weight", "bias", "running_mean", "running_var"]
    assert net._ptab.shape[refs[0][1]] == (32, 32 + F.LATENT, 1, 1)


def test_every_value_of_the_issue_meets_every_plane():
    for H, W in F.PLANES:
        cs = F.cases(H, W)
        assert {(c.B, c.S) for c in cs} >= set(F.BS)
        spw = F.route(1, 1, 1, 1, F.ROUTE_PROBE_S, H, W)[1]
        assert {c.S for c in cs if c.B == 1} >= {spw - 1, spw, spw + 1} and spw - 1 >= 1
        assert {c.K for c in cs} >= set(F.KS) and {c.L for c in cs} >= set(F.LS) and {c.U for c in cs} >= set(F.UNITS)
        assert {c.Ctot for c in cs} == set(F.CTOTS) and {c.shift for c in cs} == {0, 1}
    assert sum(len(F.cases(H, W)) for H, W in F.PLANES) == 6 * len(F.PLANES) + len(F.EXTRA)


def test_route_covers_every_pixel_and_every_sample_exactly_once():
    seen = set()
    for c in ALL_CASES:
        ppw, spw, gx, gy, gz = F.case_route(c)
        HW = c.H * c.W
        assert ppw in (256, 512) and spw >= 1
        assert (gx - 1) * ppw < HW <= gx * ppw, F.case_id(c)                        # disjoint pixel blocks, the last one ragged
        assert gy == c.B
        assert (gz - 1) * spw < c.S <= gz * spw, F.case_id(c)                       # disjoint sample groups, the last one ragged
        if c.px:
            assert ppw == 256 * c.px, F.case_id(c)
        seen.add((ppw, spw))
    for e in F.EXTRA:                                                               # the kernel switch is where the cases say it is
        assert F.case_route(F.extra_case(e))[:2] == (e["ppw"], e["spw"]), e
    # both kernels walk one sample below, at and one above a chunk of 8 and a chunk plus a ragged one; the pair kernel meets every plane
    for ppw in (256, 512):
        assert {(ppw, F.CHUNK - 1), (ppw, F.CHUNK), (ppw, F.CHUNK + 1), (ppw, 13)} <= seen
        assert any(F.case_route(c)[:2] == (ppw, 13) and F.case_route(c)[4] == 2 for c in ALL_CASES)
    for H, W in F.PLANES:
        assert any(F.case_route(c)[0] == 512 for c in F.cases(H, W)), (H, W)
    with F.forced_px(0):
        _route_figures()


def _route_figures():
    # two pixels per thread only while that leaves a workgroup per CU; the samples are split to fill the chip, four at least each
    assert F.route(6, 2, 3, 1, 16, 128, 128) == (256, 4, 64, 1, 4)
    assert F.route(6, 2, 3, 1, 100, 128, 128) == (512, 7, 32, 1, 15)
    assert F.route(6, 2, 3, 32, 16, 128, 128) == (512, 16, 32, 32, 1)


def test_bad_arguments_are_refused_without_a_launch():
    """Every refusal is decided on the host before the first device call, so it can be asked for without a device; the pointers
    are never followed."""
    L = _ffi.lib()
    o = (C.c_int * 5)()
    good = dict(L=6, K=2, U=3, B=1, S=4, H=8, W=8)

    def route(**kw):
        a = {**good, **kw}
        return L.uz_fcomb_sample_route(a["L"], a["K"], a["U"], a["B"], a["S"], a["H"], a["W"], o)
    assert route() == 0
    for kw in (dict(K=9), dict(K=0), dict(L=0), dict(L=9), dict(U=0), dict(U=9), dict(B=0), dict(S=0), dict(H=0), dict(B=65536)):
        assert route(**kw) != 0, kw
        assert L.uz_last_error()
    assert L.uz_fcomb_sample_route(6, 2, 3, 1, 4, 8, 8, None) != 0
    p = 4096                                                                        # a non-null address nothing reads

    def fwd(C_=32, Ctot=32, L_=6, K=2, U=3, ptrs=(p,) * 7):
        feat, mu, sigma, eps, params, z, logits = ptrs
        return L.uz_fcomb_sample_fwd(feat, C_, Ctot, mu, sigma, eps, params, U, 1e-3, L_, K, 1, 4, 8, 8, z, logits, None)
    for kw in (dict(C_=31), dict(C_=33, Ctot=33), dict(K=9), dict(L_=0), dict(U=0), dict(Ctot=31)):
        assert fwd(**kw) != 0, kw
    for i in range(7):
        assert fwd(ptrs=tuple(None if j == i else p for j in range(7))) != 0, i
    assert b"fcomb_sample" in L.uz_last_error()


def test_op_level_inputs_make_every_batchnorm_matter():
    """Every unit has live and dead ReLU outputs, and a kernel that drops BatchNorm or uses another unit's statistics is off by
    more than 100 x the gate."""
    swapped = 0
    for c in UNIQUE_INPUTS:
        d, ref = F.case_data(c)
        assert len(ref.live) == c.U and all(pos and neg for pos, neg in ref.live), F.case_id(c)
        assert G.maxabs(F.fcomb_f64(c, d, drop_bn=True)[1], ref.logits) > 100 * F.LOGITS_TOL, F.case_id(c)
        for u in range(c.U - 1):
            assert G.maxabs(F.fcomb_f64(c, d, swap=(u, u + 1))[1], ref.logits) > 100 * F.LOGITS_TOL, (F.case_id(c), u)
            swapped += 1
    assert swapped >= len(F.PLANES)


def test_twin_agrees_with_fp64_and_the_logit_gate_is_what_was_measured():
    worst = 0.0
    for c in UNIQUE_INPUTS:
        d, ref = F.case_data(c)
        z, logits = F.fcomb_twin(c, d)
        assert z.dtype == np.float32 and logits.dtype == np.float32 and logits.shape == (c.S * c.B, c.K, c.H, c.W)
        assert np.all(np.abs(z.astype(np.float64) - ref.z) <= F.z_tol(d, c)), F.case_id(c)
        assert G.maxabs(logits, ref.logits) <= F.LOGITS_TOL, F.case_id(c)
        worst = max(worst, F.logits_f32_error(c, d, ref.logits))
    print(f"logits: fp32 torch-CPU evaluation within {worst:.3e} of fp64 on the op-level cases; gate {F.LOGITS_TOL:.3e}")
    # the recorded figure still holds, and is no loose one; the gate stays what was written down
    assert 0.5 * F.LOGITS_F32_ERROR <= worst <= F.LOGITS_F32_ERROR and F.LOGITS_TOL == 4 * F.LOGITS_F32_ERROR


@pytest.mark.parametrize("no_convs", F.NO_CONVS)
def test_the_oracle_decides_the_labels_of_the_model_level_cases(no_convs):
    """Labels are compared on the device only where the oracle's top two logits are more than 2e-4 apart: at most 1 % of the
    pixels may be left out, and both classes must occur."""
    for shape in F.SHAPES:
        m = F.model_case(no_convs, *shape)
        B, S, H, W = shape
        assert m.logits.shape == (S * B, 2, H, W) and m.z.shape == (S * B, F.LATENT)
        assert 1.0 - float(m.sure.float().mean()) <= 0.01, shape
        assert 0.2 <= float(m.labels.float().mean()) <= 0.8, shape
        assert float(m.sigma.min()) > 0.1
        rows = m.logits.reshape(S, B, 2, H, W)
        assert all(not bool((rows[s] == rows[0]).all()) for s in range(1, S))      # the draws differ
