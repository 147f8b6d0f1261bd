"""Canonical dump of built plans: one JSON per configuration plus its SHA-256.

A refactor of the plan builder must leave every materialised tape, schedule and buffer layout as it was.  This tool builds the
plans of a fixed list of configurations (models, sizes, math modes, lanes, data-parallel buckets, every pass knob flipped once)
and writes, per configuration, everything the device would see: per tape and op in final scheduled order the code, i (padded
to 16), f (padded to 4), n, p (padded to 12, as symbolic refs) and lane; the sub-ops of the chain launches; the schedule arrays;
every buffer's placement; the pointer tables; the summary dicts of the passes.  It reads ops only as plain dicts and lists
(o["code"], o["i"][k], ...), so the same file runs against any commit:

    python tools/plan_dump.py --out /tmp/new                       # this tree
    python tools/plan_dump.py --out /tmp/old --root <other tree>   # e.g. a git worktree of the parent commit
    diff /tmp/old/DIGESTS.txt /tmp/new/DIGESTS.txt

--device cuda builds the same plans with their arenas on the GPU (plan decisions query the library; the device must not change
them), --only NAME[,NAME] / --list select configurations, --time N prints N build times of the headline PHiSeg plan.
"""
import argparse
import hashlib
import json
import os
import sys
import time

NF7 = [32, 64, 128, 192, 192, 192, 192]
KNOBS = {"UZ_FOLD_BN_BWD": "1", "UZ_BN_FOLD_DGRAD": "0", "UZ_PACK_DY": "0", "UZ_PACK_ACT": "0", "UZ_BN_OFFCHAIN": "1",
         "UZ_FOLD_RELU_BWD": "0", "UZ_WGRAD_TABLE": "0", "UZ_DBIAS_TABLE": "0", "UZ_CHAIN": "0"}       # each flipped from its default
# (UZ_CHAIN=0 is the default spelled out - phiseg7@chain8192 is the configuration that turns it on; UZ_FOLD_RELU_BWD bites on unet only)
FLIPS = {"phiseg7": {"UZ_PREPACK": "0", "UZ_BN_FUSE_STATS": "0", "UZ_BN_FOLD_REDUCE": "0", "UZ_PACK_OWN_GROUP": "0", "UZ_WGRAD_TABLE_CHUNK": "8",
                     "UZ_DECOUPLE_WGRAD": "0", "UZ_DECOUPLE_PREFIX": "", "UZ_SCHED_COST": "alone", "UZ_SCHED_HEAVY": "r4", "UZ_FUSE_HEADS": "0"},
         "phiseg3d_mid": {"UZ_WGRAD_TABLE_VOL": "0", "UZ_BN_FUSE_STATS_VOL": "0"},
         "phiseg7@chain8192": {"UZ_CHAIN_BWD": "0", "UZ_CHAIN_WGS": "128", "UZ_CHAIN_WGS_BWD": "40", "UZ_CHAIN_NETS": "fwd"}}


def golden_meta(root, name):
    with open(os.path.join(root, "tests", "golden", name + ".json")) as f:
        return json.load(f)


def configurations(root):
    """[(name, dict(model=..., env=..., mode=..., dp=..., resched=..., method=...))]: `model` is (kind, constructor kwargs, arguments
    of the builder `method`: _build, or PHISeg._build_predict)."""
    ps, us, pus, p3s = (golden_meta(root, n) for n in ("phiseg_small", "unet_small", "probunet_small", "phiseg3d_small"))
    models = {
        "unet": ("unet", dict(num_filters=[32, 64, 128, 192]), (32, 128, 128)),
        "phiseg7": ("phiseg", dict(num_filters=NF7, image_size=(1, 128, 128)), (32, 128, 128, True, True)),
        "probunet7": ("probunet", dict(num_filters=NF7, latent_dim=6, no_convs_fcomb=3, image_size=(1, 128, 128)), (32, 128, 128, True, True)),
        "unet_small": ("unet", dict(num_filters=us["filters"]), (2, 64, 64)),
        "phiseg_small": ("phiseg", dict(num_filters=ps["filters"], image_size=(1, 64, 64)), (2, 64, 64, True, True)),
        "probunet_small": ("probunet", dict(num_filters=pus["filters"], latent_dim=pus["latent_dim"], no_convs_fcomb=3), (2, 64, 64, True, True)),
        "phiseg3d_tiny": ("phiseg3d", dict(ch=(4, 3), num_filters=[8, 16, 16], latent_levels=2), (16, 32, 32, True, True)),
        "phiseg3d_tiny_rev": ("phiseg3d", dict(ch=(4, 3), num_filters=[8, 16, 16], latent_levels=2, reversible=True), (16, 32, 32, True, True)),
        "phiseg3d_mid": ("phiseg3d", dict(ch=(4, 3), num_filters=[32, 64, 64], latent_levels=2), (32, 64, 64, True, True)),
        "phiseg3d_golden": ("phiseg3d", dict(ch=(p3s["input_channels"], p3s["num_classes"]), num_filters=p3s["filters"],
                                             latent_levels=p3s["latent_levels"]), (*p3s["dhw"], True, True)),
        "phiseg3d_golden_rev": ("phiseg3d", dict(ch=(p3s["input_channels"], p3s["num_classes"]), num_filters=p3s["filters"],
                                                 latent_levels=p3s["latent_levels"], reversible=True), (*p3s["dhw"], True, True)),
    }
    dp_small = ("phiseg", dict(num_filters=[4, 8, 8, 8, 8, 8, 8], image_size=(1, 64, 64)), (2, 64, 64, True, True))
    out = []

    def add(name, model, env=None, mode=None, dp=None, resched=False, method="_build"):
        out.append((name, dict(model=models[model] if isinstance(model, str) else model, env=env or {}, mode=mode, dp=dp, resched=resched, method=method)))
    for m in models:
        add(m, m)
    # the hierarchical builder shared by PHISeg and PHISeg3D: 2-D reversible, the two predict() plans, and the 3-D level layouts
    # with as many latent as resolution levels (l3) and with a level difference of two (d2); train / eval / decode / reversible each
    add("phiseg_small_rev", (dp_small[0], dict(dp_small[1], reversible=True), dp_small[2]))
    add("phiseg_small@trunk", ("phiseg", models["phiseg_small"][1], (2, 64, 64, "trunk")), method="_build_predict")
    add("phiseg_small@draw", ("phiseg", models["phiseg_small"][1], (6, 64, 64, "draw")), method="_build_predict")
    for tag, nf, lat in (("l3", [8, 16, 16], 3), ("d2", [8, 16, 16, 16], 2)):
        kw = dict(ch=(4, 3), num_filters=nf, latent_levels=lat)
        add(f"phiseg3d_{tag}", ("phiseg3d", kw, (16, 32, 32, True, True)))
        add(f"phiseg3d_{tag}@eval", ("phiseg3d", kw, (16, 32, 32, False, False)))
        add(f"phiseg3d_{tag}@decode", ("phiseg3d", kw, (16, 32, 32, False, False, True)))
        add(f"phiseg3d_{tag}_rev", ("phiseg3d", dict(kw, reversible=True), (16, 32, 32, True, True)))
    for mode in (0, 1, 2, 3):
        for m in ("unet", "phiseg7", "probunet7", "phiseg_small", "phiseg3d_mid", "phiseg3d_tiny_rev"):
            add(f"{m}@math{mode}", m, mode=mode)
    add("phiseg3d_mid@math3+b16", "phiseg3d_mid", env={"UZ_STORE_B16": "1"}, mode=3)
    add("phiseg3d_golden@math3+b16", "phiseg3d_golden", env={"UZ_STORE_B16": "1"}, mode=3)
    # eval plans (bn_training off; PHiSeg: the prior draws its own samples), sampling / decode tapes
    for m in ("phiseg7", "phiseg_small", "probunet7", "probunet_small", "phiseg3d_tiny"):
        kind, kw, args = models[m]
        add(m + "@eval", (kind, kw, args[:3] + (False, False)))
    for m in ("phiseg7", "phiseg_small", "phiseg3d_tiny", "phiseg3d_tiny_rev"):
        kind, kw, args = models[m]
        add(m + "@decode", (kind, kw, args[:3] + (False, False, True)))
    for lanes in ("1", "2", "3"):
        for m in ("unet", "phiseg7", "probunet7", "phiseg_small", "phiseg3d_tiny"):
            add(f"{m}@lanes{lanes}", m, env={"UZ_LANES": lanes})
    add("phiseg7@lanes3+offchain+foldbn", "phiseg7", env={"UZ_LANES": "3", "UZ_BN_OFFCHAIN": "1", "UZ_FOLD_BN_BWD": "1"})
    for tables in ("1", "0"):
        add(f"dp_small@tables{tables}", dp_small, env={"UZ_DP_TABLES": tables}, dp=3000)
        add(f"phiseg7+dp@tables{tables}", "phiseg7", env={"UZ_DP_TABLES": tables}, dp="default")
    add("unet+dp", "unet", dp="default")
    for k, v in KNOBS.items():
        for m in ("phiseg7", "unet", "probunet7", "phiseg_small"):
            add(f"{m}@{k}={v}", m, env={k: v})
        add(f"phiseg3d_mid@math3+b16@{k}={v}", "phiseg3d_mid", env={"UZ_STORE_B16": "1", k: v}, mode=3)
    add("phiseg7@chain8192", "phiseg7", env={"UZ_CHAIN": "8192"})
    # the remaining plan switches, each away from its default on a model where that changes the plan (name: <base configuration>@<switch>=<value>)
    for base, flips in FLIPS.items():
        for k, v in flips.items():
            add(f"{base}@{k}={v}", base.split("@")[0], env={**dict(out)[base]["env"], k: v})
    add("phiseg_small@heads_unfused", "phiseg_small", env={"UZ_FUSE_HEADS": "0"})
    add("phiseg_small@lanes3+resched", "phiseg_small", env={"UZ_LANES": "3", "UZ_SCHED_HEAVY": "off", "UZ_SCHED_COST": "beside"}, resched=True)
    add("phiseg7@resched", "phiseg7", resched=True)
    return out


def build_plan(cfg, device):
    from unet_zoo_amd import _ffi, dp
    from unet_zoo_amd.models.phiseg import PHISeg
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    from unet_zoo_amd.models.probabilistic_unet import ProbabilisticUnet
    from unet_zoo_amd.models.unet import Unet
    kind, kw, args = cfg["model"]
    kw = dict(kw)
    saved = {k: os.environ.get(k) for k in cfg["env"]}
    os.environ.update(cfg["env"])
    L = _ffi.lib()
    if cfg["mode"] is not None:
        assert L.uz_set_conv_math(cfg["mode"]) == 0
    try:
        if kind == "phiseg3d":
            cin, k = kw.pop("ch")
            net = PHISeg3D(cin, k, kw.pop("num_filters"), device=device, **kw)
        else:
            net = {"unet": Unet, "phiseg": PHISeg, "probunet": ProbabilisticUnet}[kind](1, 2, kw.pop("num_filters"), device=device, **kw)
        net.train()
        if cfg["dp"] is not None:
            buckets = dp.param_buckets(net._ptab) if cfg["dp"] == "default" else dp.param_buckets(net._ptab, target_floats=cfg["dp"])
            net._dp = type("S", (), dict(overlap=True, buckets=buckets))()
        plan = getattr(net, cfg["method"])(*args)
        if cfg["resched"]:
            # deterministic "measured" durations, then one reschedule() per tape (Engine.tune_schedule does this with real ones)
            for which in ("fwd", "bwd"):
                for k, o in enumerate(plan._program_order[which]):
                    o["cost_us"] = (3.0, 30.0, 300.0)[(7 * k + 3) % 3] + (k % 5)
                plan.reschedule(which)
        return plan
    finally:
        if cfg["mode"] is not None:
            L.uz_set_conv_math(-1)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def canon(r):
    """Symbolic form of one operand ref: JSON-able, without addresses or object identities."""
    if r is None or isinstance(r, (bool, int, float, str)):
        return r
    if isinstance(r, (tuple, list)):
        return [canon(q) for q in r]
    name = type(r).__name__
    if name == "View":
        return {"view": [r.buf.name, r.c0, r.C, r.b0, r.nb]}
    if name == "_ScratchView":
        return {"scratch": dict(N=r.N, C=r.C, H=r.H, W=r.W, amax=r.amax, off=r.off, nb=r.nb, view=canon(r.view), zkey=canon(r.zkey))}
    raise TypeError(f"operand ref of type {name}")


def pad(lst, n, fill):
    lst = list(lst)
    assert len(lst) <= n, (len(lst), n)
    return lst + [fill] * (n - len(lst))


def dump_op(o):
    return dict(code=o["code"], i=pad(o["i"], 16, 0), f=pad(o["f"], 4, 0.0), n=o["n"], p=pad([canon(r) for r in o["p"]], 12, None), lane=o.get("lane"))


def dump_plan(plan):
    tapes = [("fwd", plan.fwd_ops), ("loss", plan.loss_ops), ("bwd", plan.bwd_ops)] + sorted(plan.extra_ops.items())
    d = {"tapes": {nm: [dump_op(o) for o in ops] for nm, ops in tapes}}
    d["scheds"] = {nm: [[s.lane, s.signal, s.n_wait, list(s.wait)[:s.n_wait]] for s in plan.scheds[nm]] for nm, _ in tapes}
    d["chains"] = [dict(which=ch["which"], net=ch["net"], n_wgs=ch["n_wgs"],
                        sub=[dict(code=e["code"], i=pad(e["i"], 16, 0), f=pad(e["f"], 4, 0.0), p=pad([canon(r) for r in e["p"]], 12, None), level=e["level"])
                             for e in ch["sub"]]) for ch in getattr(plan, "_chains", [])]
    d["bufs"] = [dict(name=b.name, off=b.off, packed=b.packed, b16=b.b16, alias=None if b.alias is None else dict(b.alias), shape=[b.N, b.C, b.H, b.W])
                 for b in plan.bufs]
    d["ptr_tables"] = [[canon(r) for r in t] for t in plan.ptr_tables]
    d["layout"] = dict(arena_floats=plan.arena_floats, n_amax=plan.n_amax, n_amax_fwd=plan.n_amax_fwd, amax_off=plan.amax_off, scratch=plan.scratch,
                       gy_off=plan.gy_off, scratch_off=plan.scratch_off, gyz_off=[sorted([canon(k), v] for k, v in z.items()) for z in plan.gyz_off],
                       amax_remap=sorted(plan._amax_remap.items()), n_lanes=plan.n_lanes, grad_buckets=canon(plan.grad_buckets))
    d["round4"], d["b16_info"], d["bn_offchain"] = plan.round4, plan.b16_info, plan.bn_offchain
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="directory for <name>.json and DIGESTS.txt")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose package is dumped")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--only", default=None)
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--time", type=int, default=0, help="print N build times (s) of the headline PHiSeg plan and exit")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import __graft_entry__  # noqa: F401  (puts the tree on the path the way the driver does)
    import unet_zoo_amd
    assert os.path.abspath(unet_zoo_amd.__file__).startswith(root + os.sep), unet_zoo_amd.__file__
    cfgs = configurations(root)
    if a.only:
        cfgs = [c for c in cfgs if c[0] in set(a.only.split(","))]
    if a.list:
        print("\n".join(n for n, _ in cfgs))
        return
    if a.time:
        cfg = dict(configurations(root))["phiseg7"]
        ts = []
        for _ in range(a.time):
            t0 = time.perf_counter()
            build_plan(cfg, a.device)
            ts.append(round(time.perf_counter() - t0, 3))
        print("phiseg7 _build seconds:", ts)
        return
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    lines = []
    for name, cfg in cfgs:
        plan = build_plan(cfg, a.device)
        text = json.dumps(dump_plan(plan), sort_keys=True, separators=(",", ":"))
        digest = hashlib.sha256(text.encode()).hexdigest()
        n_ops = sum(len(ops) for ops in (plan.fwd_ops, plan.loss_ops, plan.bwd_ops, *plan.extra_ops.values()))
        lines.append(f"{digest}  {n_ops:5d} ops  {name}")
        print(lines[-1], flush=True)
        if a.out:
            with open(os.path.join(a.out, name.replace("/", "_") + ".json"), "w") as f:
                f.write(text)
    if a.out:
        with open(os.path.join(a.out, "DIGESTS.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
