"""The UZ_* switches of the Python package (unet_zoo_amd/_knobs.py): every read goes through the one table, the table is what
INTEGRATION.md section 4 documents and what tools/plan_dump.py flips, values parse as the table says, a model's defaults sit between
the environment and the table's, and a plan keeps the switches it was built under."""
import importlib.util
import os
import re

import pytest

from unet_zoo_amd import _knobs
from unet_zoo_amd._plan import ParamTable, Plan
from tests import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.abspath(_knobs.__file__))
NAMES = {k.name for k in _knobs.TABLE}
PLAN = [k for k in _knobs.TABLE if k.scope == "plan"]


def _sources():
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py") and f != "_knobs.py":
                with open(os.path.join(d, f)) as fh:
                    yield os.path.relpath(os.path.join(d, f), PKG), fh.read()


def test_table_is_well_formed():
    assert len(PLAN) == 28 and len(NAMES) == len(_knobs.TABLE) == len({k.attr for k in _knobs.TABLE})
    assert {k.scope for k in _knobs.TABLE} == {"plan", "engine", "dp", "train", "lib"} and all(k.doc for k in _knobs.TABLE)
    assert not any("HW_QUEUES" in k.name or "GRAPH_QUEUES" in k.name for k in _knobs.TABLE)      # the import-time queue setup is not a switch


def test_every_read_of_a_switch_goes_through_the_table():
    attrs = {k.attr for k in PLAN} | {"from_env"}
    n_get = n_attr = 0
    for path, text in _sources():
        for no, line in enumerate(text.splitlines(), 1):
            assert not (re.search(r"\benviron\b|getenv", line) and "UZ_" in line), f"{path}:{no} reads a UZ_ variable past _knobs"
        for name in re.findall(r"""["'](UZ_[A-Z0-9_]+)["']""", text):
            if not name.startswith(("UZ_OP_", "UZ_CH_")):                  # (tape-op and chain sub-op codes)
                assert name in NAMES, f"{path}: {name} is not a row of _knobs.TABLE"
        for name in re.findall(r"_knobs\.get\(\s*[\"'](\w+)", text):
            n_get += 1
            assert name in NAMES, f"{path}: _knobs.get({name!r})"
        for attr in re.findall(r"\bknobs\.([A-Za-z_]\w*)", text):
            n_attr += 1
            assert attr in attrs, f"{path}: knobs.{attr} is not a plan-scope attribute"
    assert n_get >= 7 and n_attr >= 28
    for f in ("_plan.py", "_passes.py", "_chain_plan.py"):
        assert not re.search(r"\benviron\b|getenv|^import os$", dict(_sources())[f], re.M), f


def _doc_default(k):
    d = k.default
    if d is None:
        return "unset"
    if d == ():
        return "none"
    return "`%s`" % (int(d) if isinstance(d, (bool, int)) else f"{d:g}" if isinstance(d, float) else d)


def test_every_switch_is_documented_with_its_default():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        sec = f.read().split("## 4. Environment switches")[1]
    rows = [line.split("|") for line in sec.splitlines() if line.startswith("| `UZ_")]
    for k in _knobs.TABLE:
        mine = [r for r in rows if f"`{k.name}`" in r[1]]
        assert len(mine) == 1, k.name
        assert _doc_default(k) in mine[0][2], (k.name, _doc_default(k), mine[0][2])


def test_plan_dump_flips_every_plan_switch():
    spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    flipped = set().union(*(c["env"] for _, c in mod.configurations(ROOT)))
    assert flipped <= NAMES and flipped >= {k.name for k in PLAN}
    for _, c in mod.configurations(ROOT):
        _knobs.read(environ=c["env"])                                      # every value it sets is in its switch's domain


def test_parsing():
    k = _knobs.read(environ={})
    assert all(getattr(k, r.attr) == r.default for r in PLAN) and k.from_env == frozenset()
    assert (k.chain_wgs, k.chain_wgs_bwd, k.lanes, k.fold_bn_bwd, k.wgrad_table, k.chain_nets) == (256, 80, 2, False, True, None)
    assert all(_knobs.get(r.name, environ={}) == r.default for r in _knobs.TABLE)
    with pytest.raises(AttributeError):
        k.lanes = 3
    bare = lambda env: Plan(1, ParamTable([], "cpu"), True, "cpu", _knobs.read(environ=env))
    assert bare({"UZ_LANES": "99"}).n_lanes == 8 and bare({"UZ_LANES": "0"}).n_lanes == 1 and bare({}).n_lanes == 2      # (the Plan clamps)
    assert _knobs.read(environ={"UZ_DECOUPLE_PREFIX": ""}).decouple_wgrad_prefixes == ()
    assert _knobs.read(environ={"UZ_DECOUPLE_PREFIX": "a,,b"}).decouple_wgrad_prefixes == ("a", "b")
    assert _knobs.read(environ={"UZ_CHAIN_NETS": "fwd,prior"}).chain_nets == ("fwd", "prior")
    on = _knobs.read(environ={"UZ_WGRAD_TABLE": "0", "UZ_FOLD_BN_BWD": "1", "UZ_CHAIN": "8192", "UZ_SCHED_HEAVY": "12.5", "UZ_SCHED_COST": "beside"})
    assert (on.wgrad_table, on.fold_bn_bwd, on.chain_px, on.sched_heavy, on.sched_cost) == (False, True, 8192, "12.5", "beside")
    assert on.from_env == {"wgrad_table", "fold_bn_bwd", "chain_px", "sched_heavy", "sched_cost"}
    assert _knobs.read(environ={"UZ_SCHED_HEAVY": "off"}).sched_heavy == "off"
    for name, bad in (("UZ_WGRAD_TABLE", "true"), ("UZ_CHAIN", "abc"), ("UZ_SCHED_COST", "fast"), ("UZ_SCHED_HEAVY", "on"), ("UZ_LANES", "two"),
                      ("UZ_FOLD_BN_BWD", "")):
        with pytest.raises(ValueError, match=name):
            _knobs.read(environ={name: bad})
    # the readers of the other scopes: the value at the moment of the call
    assert _knobs.get("UZ_DP_BUCKET_MB", environ={"UZ_DP_BUCKET_MB": "1.5"}) == 1.5 and _knobs.get("UZ_TUNE_SCHEDULE", environ={"UZ_TUNE_SCHEDULE": "0"}) == 0
    assert _knobs.get("UZ_TRAIN_REPLAY", environ={"UZ_TRAIN_REPLAY": "no"}) == "no" and _knobs.get("UZ_REPLAY", environ={"UZ_REPLAY": "graph"}) == "graph"
    for name, bad in (("UZ_REPLAY", "hip"), ("UZ_DP_BUCKET_MB", "big"), ("UZ_DP_STREAM_PRIORITY", "high")):
        with pytest.raises(ValueError, match=name):
            _knobs.get(name, environ={name: bad})
    with pytest.raises(KeyError):
        _knobs.get("UZ_NO_SUCH_SWITCH")


def test_model_defaults_sit_between_the_environment_and_the_table():
    model = dict(chain_px=8192, decouple_wgrad_prefixes=("likelihood",))
    k = _knobs.read(defaults=model, environ={})
    assert (k.chain_px, k.decouple_wgrad_prefixes, k.chain_wgs) == (8192, ("likelihood",), 256) and not k.from_env
    k = _knobs.read(defaults=model, environ={"UZ_CHAIN": "0", "UZ_DECOUPLE_PREFIX": "prior,posterior"})
    assert (k.chain_px, k.decouple_wgrad_prefixes) == (0, ("prior", "posterior")) and k.from_env == {"chain_px", "decouple_wgrad_prefixes"}
    assert _knobs.read(defaults=model, environ={"UZ_DECOUPLE_PREFIX": ""}).decouple_wgrad_prefixes == ()


def test_models_hand_their_defaults_to_the_plan(monkeypatch):
    from unet_zoo_amd.models.phiseg import PHISeg
    for name in NAMES:
        monkeypatch.delenv(name, raising=False)
    _, meta = G.load("phiseg_small")
    net = PHISeg(1, 2, meta["filters"], image_size=(1, 64, 64), device="cpu")
    k = net._build(2, 64, 64, True, True).knobs
    lanes = net.replay_mode == "lanes"
    assert k.lanes == net.default_lanes_by_mode.get(net.replay_mode, net.default_lanes) and k.chain_px == net.chain_px == 0
    assert (k.sched_cost, k.sched_heavy) == (("beside", "off") if lanes else ("alone", "r4"))
    assert (k.decouple_wgrad_px, k.decouple_wgrad_prefixes) == (8192, ("likelihood",)) and not k.from_env
    monkeypatch.setenv("UZ_DECOUPLE_WGRAD", "0")
    monkeypatch.setenv("UZ_LANES", "2")
    net = PHISeg(1, 2, meta["filters"], image_size=(1, 64, 64), device="cpu")
    plan = net._build(2, 64, 64, True, True)
    assert (plan.knobs.decouple_wgrad_px, plan.n_lanes, plan.sched_cost) == (0, 2, k.sched_cost) and plan.knobs.from_env == {"decouple_wgrad_px", "lanes"}


def _bwd_record(plan):
    return ([(o["code"], o["lane"]) for o in plan.bwd_ops],
            [(s.lane, s.signal, s.n_wait, tuple(s.wait)[:s.n_wait]) for s in plan.scheds["bwd"]])


def test_a_plan_is_rescheduled_under_the_switches_it_was_built_with(monkeypatch):
    """reschedule() - minutes after the build, inside the tuner - must not pick up a cost model from the environment of that moment.
    The two cost models schedule this fixture differently (asserted), so a reschedule that read the environment would show."""
    from unet_zoo_amd.models.phiseg import PHISeg
    _, meta = G.load("phiseg_small")

    def build(cost):
        monkeypatch.setenv("UZ_LANES", "3")
        monkeypatch.setenv("UZ_SCHED_HEAVY", "off")
        monkeypatch.setenv("UZ_SCHED_COST", cost)
        return PHISeg(1, 2, meta["filters"], image_size=(1, 64, 64), device="cpu")._build(2, 64, 64, True, True)
    other = _bwd_record(build("alone"))
    plan = build("beside")
    first = _bwd_record(plan)
    assert first != other
    monkeypatch.setenv("UZ_SCHED_COST", "alone")
    monkeypatch.setenv("UZ_SCHED_HEAVY", "r4")
    plan.reschedule("bwd")
    assert _bwd_record(plan) == first and plan.sched_cost == plan.knobs.sched_cost == "beside"
