"""The operand schema of the tape ops (include/uz_ops.def as unet-zoo_amd/_ops.py reads it) against the header, the wire struct, the plans and - for the two parts the
lane scheduler and the bf16-storage pass depend on - literal copies of the tables the plan builder carried before the schema."""
import pytest

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import _ffi, _ops


def test_every_op_code_of_the_header_has_a_schema_and_nothing_else_has():
    codes = set(_ffi.op_codes()) - {"UZ_OP__COUNT"}
    assert set(_ops.SCHEMA) == codes
    assert set(_ops.WRITES) == codes and set(_ops.CONV_KIND) | set(_ops.SPLIT_WRITERS) | set(_ops.SPLIT_READERS) <= codes


def test_every_schema_fits_the_wire_struct():
    n_i, n_f, n_p = (dict((nm, tp._length_) for nm, tp, *_ in _ffi.uz_op._fields_ if hasattr(tp, "_length_"))[k] for k in "ifp")
    assert (n_i, n_f, n_p) == (15, 4, 12)
    for code, s in _ops.SCHEMA.items():
        assert len(s.i) <= n_i and len(s.p) <= n_p and len(s.f) <= n_f, code
        for names, index in ((s.i, s.ix), (s.p, s.px), (s.f, s.fx)):
            assert len(set(names)) == len(names) and [index[nm] for nm in names] == list(range(len(names))), code
        assert all(0 <= j < len(s.p) for j in s.writes) and all(nm in s.ix for nm in s.opts) and all(nm in s.px for nm in s.b16), code
        if s.b16:
            assert s.ix["b16"] == _ops.B16_SLOT == 13 and "b16" not in s.opts, code
    for table in (_ops.SPLIT_WRITERS, _ops.SPLIT_READERS):
        for code, (view, *rest) in table.items():
            s = _ops.SCHEMA[code]
            assert view in s.px and all(nm in s.px or nm in s.ix for nm in rest), code


def test_make_pads_to_the_schema_and_takes_operands_by_name():
    a = _ops.make("UZ_OP_CONV_FWD", p=["x", "w"], i=[3, 4], n=7, gid=2)
    b = _ops.make("UZ_OP_CONV_FWD", p={"w": "w", "x": "x"}, i={"ctot_x": 4, "cin": 3}, n=7, gid=2)
    assert a == b and type(a["i"]) is list and type(a["p"]) is list
    assert a["i"] == [3, 4] + [0] * 12 and a["p"] == ["x", "w"] + [None] * 10 and a["f"] == [] and a["n"] == 7 and a["gid"] == 2
    assert a.i("cin") == 3 and a.i("cin", "ctot_x") == [3, 4] and a.p("w") == "w" and a.base_form()
    a.set(i={"x_packed": 1, "x_seg2_c0": 32}, p={"x_amax2": "s2"})
    assert a["i"][10:12] == [1, 32] and a["p"][10] == "s2" and not a.base_form() and b["i"][10] == 0
    assert _ops.make("UZ_OP_BN_RELU_FWD", f=[1e-3, 0.01]).f("eps", "momentum") == [1e-3, 0.01]
    with pytest.raises(AssertionError):
        _ops.make("UZ_OP_SCALE", p=["a", "b"])                       # more operands than the op has
    with pytest.raises(KeyError):
        a.i("no_such_slot")


def _headline(which, monkeypatch):
    from unet_zoo_amd.models.phiseg import PHISeg
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    from unet_zoo_amd.models.probabilistic_unet import ProbabilisticUnet
    from unet_zoo_amd.models.unet import Unet
    nf7 = [32, 64, 128, 192, 192, 192, 192]
    if which == "phiseg":
        return PHISeg(1, 2, nf7, image_size=(1, 128, 128), device="cpu")._build(32, 128, 128, True, True)
    if which == "unet":
        return Unet(1, 2, [32, 64, 128, 192], device="cpu")._build(32, 128, 128)
    if which == "probunet":
        return ProbabilisticUnet(1, 2, nf7, latent_dim=6, no_convs_fcomb=3, image_size=(1, 128, 128), device="cpu")._build(32, 128, 128, True, True)
    monkeypatch.setenv("UZ_STORE_B16", "1")
    L = _ffi.lib()
    L.uz_set_conv_math(3)
    try:
        return PHISeg3D(4, 3, [32, 64, 64], latent_levels=2, device="cpu")._build(32, 64, 64, True, True)
    finally:
        L.uz_set_conv_math(-1)


@pytest.mark.parametrize("which", ["phiseg", "unet", "probunet", "phiseg3d_b16"])
def test_every_emitted_op_has_exactly_the_schemas_lengths(which, monkeypatch):
    plan = _headline(which, monkeypatch)
    tapes = [plan.fwd_ops, plan.loss_ops, plan.bwd_ops, *plan.extra_ops.values()]
    assert sum(len(t) for t in tapes) > 80
    if which == "phiseg3d_b16":
        assert plan.b16_info["ops"] >= 40
    for ops in tapes:
        for o in ops + [q for c in ops if c["code"] == "UZ_OP_CHAIN" for q in c["_acc_ops"]]:
            s = _ops.SCHEMA[o["code"]]
            assert isinstance(o, _ops.Op) and (len(o["i"]), len(o["p"]), len(o["f"])) == (len(s.i), len(s.p), len(s.f)), o["code"]
            assert all(type(v) is int for v in o["i"]) and all(type(v) is float for v in o["f"]), o["code"]


# What the plan builder's lane scheduler used as its write table before the schema existed (Plan._WRITES and the two exceptions of
# Plan._op_writes), copied literally: the schedule of every plan depends on exactly these sets.
_WRITES_BEFORE = {
    "UZ_OP_CONV_FWD": (3, 9), "UZ_OP_CONV_BWD_DATA": (2, 8, 9), "UZ_OP_CONV_BWD_WEIGHT": (2, 3, 8),
    "UZ_OP_BN_RELU_FWD": (3, 4, 5, 6), "UZ_OP_BN_RELU_BWD": (5, 6, 7, 8), "UZ_OP_RELU_BWD": (2, 3),
    "UZ_OP_AVGPOOL_FWD": (1,), "UZ_OP_AVGPOOL_BWD": (1, 3, 4), "UZ_OP_BILINEAR_FWD": (1,), "UZ_OP_BILINEAR_BWD": (1, 3, 4),
    "UZ_OP_NEAREST_FWD": (1,), "UZ_OP_NEAREST_BWD": (1,), "UZ_OP_SPATIAL_MEAN_FWD": (1,), "UZ_OP_SPATIAL_MEAN_BWD": (1,),
    "UZ_OP_POSTERIOR_INPUT": (2,), "UZ_OP_LATENT_FWD": (3, 4), "UZ_OP_LATENT_BWD": (5, 6),
    "UZ_OP_LATENT_HEADS_FWD": (6, 7, 8, 9), "UZ_OP_LATENT_HEADS_BWD_DATA": (4,), "UZ_OP_LATENT_HEADS_BWD_WEIGHT": (3, 4, 5, 6),
    "UZ_OP_KL_FWD": (4,), "UZ_OP_KL_BWD": (5, 6, 7, 8), "UZ_OP_CE_FWD": (2,), "UZ_OP_CE_BWD": (1,),
    "UZ_OP_SUM_TERMS": (1,), "UZ_OP_SCALE": (0,), "UZ_OP_COPY": (0,), "UZ_OP_MEMSET": (0,),
    "UZ_OP_L2_NORMS": (2,), "UZ_OP_L2_NORMS_BWD": (4,),
    "UZ_OP_BCAST_CHANNELS": (1,), "UZ_OP_BCAST_CHANNELS_BWD": (1,), "UZ_OP_EVENT_RECORD": (0,), "UZ_OP_ABSMAX": (1,),
    "UZ_OP_ADD_VIEWS": (2,), "UZ_OP_W3D_PERMUTE": (1,), "UZ_OP_AVGPOOL3D_FWD": (1,), "UZ_OP_AVGPOOL3D_BWD": (1,),
    "UZ_OP_DEPTH_LERP_FWD": (1,), "UZ_OP_DEPTH_LERP_BWD": (1,), "UZ_OP_NEAREST3D_FWD": (1,), "UZ_OP_NEAREST3D_BWD": (1,),
    "UZ_OP_ABSMAX_COPY": (), "UZ_OP_PACK_WEIGHTS": (2,), "UZ_OP_CHAIN_PACK": (2,), "UZ_OP_CHAN_SUM_PARTIALS": (1,), "UZ_OP_CHAN_SUM_TABLE": (1,), "UZ_OP_WGRAD_REDUCE_TABLE": (1,),
}


def _writes_before(o):
    if o["code"] == "UZ_OP_CONV_BWD_DATA" and len(o["i"]) > 10 and o["i"][10] == 3:
        return (7,)
    if o["code"] == "UZ_OP_BN_RELU_FWD" and len(o["i"]) > 11 and o["i"][11]:
        return (3, 4, 5) if o["i"][11] == 1 else (6,)
    return _WRITES_BEFORE[o["code"]]


def test_written_slots_equal_the_table_the_scheduler_used_before():
    # the codes the old table did not know never appear in a plan's tape (optimiser / metric ops) or are handled apart (the chain launch)
    assert set(_ops.SCHEMA) - set(_WRITES_BEFORE) == {"UZ_OP_ACC_SOFTMAX_ARGMAX", "UZ_OP_ADAM", "UZ_OP_AXPY", "UZ_OP_CHAIN"}
    assert _ops.SCHEMA["UZ_OP_CHAIN"].writes == ()
    for code, want in _WRITES_BEFORE.items():
        assert tuple(sorted(_ops.SCHEMA[code].writes)) == want == tuple(sorted(_ops.WRITES[code])), code
        assert tuple(sorted(_ops.writes(_ops.make(code)))) == want, code
    for fold in (0, 1, 2, 3):
        o = _ops.make("UZ_OP_CONV_BWD_DATA", i={"fold": fold})
        assert tuple(sorted(_ops.writes(o))) == _writes_before(o) == ((7,) if fold == 3 else (2, 8, 9))
    for phase in (0, 1, 2):
        o = _ops.make("UZ_OP_BN_RELU_FWD", i={"phase": phase})
        assert tuple(sorted(_ops.writes(o))) == _writes_before(o) == {0: (3, 4, 5, 6), 1: (3, 4, 5), 2: (6,)}[phase]
    from unet_zoo_amd._plan import Plan
    assert Plan._WRITES is _ops.WRITES


# The bf16-storage pass's operand table before the schema (Plan._B16_SLOTS and the special cases of Plan._b16_slots), copied literally:
# p[] slots in the order of the bits of i[13].
_B16_SLOTS_BEFORE = {
    "UZ_OP_CONV_FWD": (0, 3), "UZ_OP_CONV_BWD_DATA": (0, 2), "UZ_OP_CONV_BWD_WEIGHT": (0, 1),
    "UZ_OP_BN_RELU_FWD": (0, 6), "UZ_OP_BN_RELU_BWD": (0, 1, 5),
    "UZ_OP_AVGPOOL3D_FWD": (0, 1), "UZ_OP_AVGPOOL3D_BWD": (0, 1), "UZ_OP_DEPTH_LERP_FWD": (0, 1), "UZ_OP_DEPTH_LERP_BWD": (0, 1),
    "UZ_OP_BILINEAR_FWD": (0, 1), "UZ_OP_BILINEAR_BWD": (0, 1),
}


def _b16_slots_before(o):
    c = o["code"]
    slots = _B16_SLOTS_BEFORE.get(c)
    if not slots:
        return ()
    if c.startswith("UZ_OP_CONV_") and o["i"][7] == 1:
        return {"UZ_OP_CONV_FWD": ((0, 0),), "UZ_OP_CONV_BWD_DATA": ((2, 1),), "UZ_OP_CONV_BWD_WEIGHT": ((0, 0),)}[c]
    if c == "UZ_OP_BILINEAR_FWD":
        return ((1, 1),)
    if c == "UZ_OP_BILINEAR_BWD":
        return ((0, 0),)
    return tuple((j, k) for k, j in enumerate(slots))


def test_bf16_format_bit_order_equals_the_table_the_storage_pass_used_before():
    assert {c for c, s in _ops.SCHEMA.items() if s.b16} == set(_B16_SLOTS_BEFORE)
    for code, s in _ops.SCHEMA.items():
        assert tuple(s.px[nm] for nm in s.b16) == _B16_SLOTS_BEFORE.get(code, ()), code
        for ks in ((1, 3, 5) if code in _ops.CONV_KIND else (0,)):
            o = _ops.make(code, i={"ks": ks} if ks else ())
            assert _ops.b16_slots(o) == _b16_slots_before(o), (code, ks)
