"""The deep-level chain (csrc/chain.hip; UZ_CHAIN / NativeModel.chain_px, off by default): the plan pass that collects the small-plane
ops of a tape into persistent UZ_OP_CHAIN launches (_chain_pass, the last of the four rewrites Plan.finalize() runs), the device
tables of such a launch (_chain_tables, built when Plan._resolve first meets a "chaintab" ref) and its status query.  Functions of the plan.
"""
import ctypes as C

import torch

from . import _ffi, _ops
from ._ops import conv_dims
from ._plan import View, _ScratchView


def _chain_limit(plan):
    """Largest N*H*W whose ops run inside the persistent chain launch (0: off).  Only with two-piece operands (the chain's
    convolutions are split-fp16: UZ_CONV_MATH=f32 keeps every convolution on the fp32 matrix pipe, bf16 is the volume path) and
    training-mode BatchNorm."""
    px = plan.knobs.chain_px
    if px <= 0 or not plan.bn_training or plan.L.uz_get_conv_math() in (0, 3) or plan.extra_ops:
        return 0
    return px


def _chain_net(o):
    """The sub-network an op belongs to (first component of the name of the tensor / parameter it is about): backward chains are
    built per sub-network, so that the prior's deep levels - which only wait for the KL gradients - run beside the likelihood's
    device-filling kernels instead of behind them."""
    c = o["code"]
    if c in ("UZ_OP_CONV_BWD_DATA", "UZ_OP_CONV_FWD"):
        w = o.p("w")
        return w[1].split(".")[0] if isinstance(w, tuple) else None          # w = ("param", key, offset)
    slot = {"UZ_OP_BN_RELU_BWD": "y", "UZ_OP_BN_RELU_FWD": "y", "UZ_OP_AVGPOOL_BWD": "dy", "UZ_OP_BILINEAR_BWD": "dy",
            "UZ_OP_LATENT_BWD": "dmu", "UZ_OP_LATENT_HEADS_BWD_DATA": "dy_a"}.get(c)
    if slot is None or not isinstance(o.p(slot), View):
        return None
    nm = o.p(slot).buf.name
    return (nm[5:] if nm.startswith("grad:") else nm).split(".")[0]


def _chain_eligible_fwd(o, px):
    c = o["code"]
    if c == "UZ_OP_CONV_FWD":
        _, cin, cout, N, H, W, ks = conv_dims(o)
        x = o.p("x")
        if o.i("b16") or ks != 3 or N * H * W > px or o.i("relu") or o.i("x_packed") or o.p("bn_partials") is not None or not isinstance(x, View) or x.nb is not None:
            return False
        if cin <= 4:
            return True
        return cin % 16 == 0 and cout % 32 == 0 and o.p("x_amax") is not None
    if c == "UZ_OP_BN_RELU_FWD":
        N, H, W = o.i("N", "H", "W")
        y = o.p("y")
        return not o.i("b16") and o.i("training") == 1 and o.i("npart") == 0 and not o.i("a_packed") and N * H * W <= px and isinstance(y, View) and y.nb is None
    if c == "UZ_OP_AVGPOOL_FWD":
        N, H, W = o.i("N", "H", "W")
        return N * ((H + 1) // 2) * ((W + 1) // 2) <= px and not o.i("y_packed") and o.p("x").nb is None
    if c == "UZ_OP_BILINEAR_FWD":
        N, H, W = o.i("N", "H", "W")
        return not o.i("b16") and N * 4 * H * W <= px and not o.i("y_packed") and o.p("x").nb is None
    if c == "UZ_OP_LATENT_HEADS_FWD":
        N, H, W = o.i("N", "H", "W")
        return o.i("L") == 2 and N * H * W <= px
    return False


def _chain_eligible_bwd(o, px):
    c = o["code"]
    own_dy = lambda r: isinstance(r, _ScratchView) and r.view is not None and r.zkey is None
    if c == "UZ_OP_BN_RELU_BWD":
        N, H, W = o.i("N", "H", "W")
        da, y = o.p("da", "y")
        return (not o.i("b16") and N * H * W <= px and not any(o.i("npart", "dy_packed", "dbias_rows")) and own_dy(o.p("dy"))
                and isinstance(da, View) and da.nb is None and isinstance(y, View) and not y.buf.packed)
    if c == "UZ_OP_CONV_BWD_DATA":
        _, cin, cout, N, H, W, ks = conv_dims(o)
        fold = o.i("fold")
        if o.i("b16") or ks != 3 or N * H * W > px or not own_dy(o.p("dy")) or fold not in (0, 3) or o.i("dy_packed") or o.p("dx").nb is not None:
            return False
        if cin <= 4:
            return fold == 0
        return cout % 16 == 0 and cin % 32 == 0 and o.p("dy_amax") is not None
    if c == "UZ_OP_AVGPOOL_BWD":
        N, H, W = o.i("N", "H", "W")
        return N * H * W <= px and o.p("a") is None and o.p("dy").nb is None
    if c == "UZ_OP_BILINEAR_BWD":
        N, H, W = o.i("N", "H", "W")
        return not o.i("b16") and N * 4 * H * W <= px and o.p("a") is None and o.p("dy").nb is None
    if c == "UZ_OP_LATENT_BWD":
        dmu = o.p("dmu")
        return isinstance(dmu, View) and dmu.C == 2 and dmu.N * dmu.H * dmu.W <= px
    if c == "UZ_OP_LATENT_HEADS_BWD_DATA":
        N, H, W = o.i("N", "H", "W")
        return o.i("L") == 2 and N * H * W <= px
    return False


def _chain_pass(plan):
    """Collects the small-plane ops of a tape into UZ_OP_CHAIN ops (uz_chain_run): a sub-DAG is levelled into phases of independent
    sub-ops, every 3 x 3 convolution gets a split-K factor and a slab buffer of its own, its weights a fragment-ordered image packed
    once per tape (UZ_OP_CHAIN_PACK).  Forward tape: one chain; backward tape: one chain per sub-network (_chain_net).  The tape
    keeps a valid program order: [every op the chain depends on] [chain] [the rest]; a chain's set must be convex in the dependency
    DAG (an op outside may not sit between two inside) - offenders and what hangs behind them stay per-op launches."""
    plan.chain_info = {}
    px = _chain_limit(plan)
    if px <= 0:
        return
    only = plan.knobs.chain_nets                          # diagnostics: "fwd,prior" = the forward chain and the prior's backward chain only
    jobs = [("fwd", plan.fwd_ops, _chain_eligible_fwd, None)] if (only is None or "fwd" in only) else []
    if plan.bwd_ops and plan.knobs.chain_bwd:
        nets = []
        for o in plan.bwd_ops:
            if _chain_eligible_bwd(o, px):
                nt = _chain_net(o)
                if nt not in nets:
                    nets.append(nt)
        jobs += [("bwd", plan.bwd_ops, _chain_eligible_bwd, nt) for nt in nets if only is None or nt in only]
    for which, ops, elig, net in jobs:
        if ops:
            _chain_build(plan, which, ops, elig, net, px)
    # the chains' weight images: one buffer and one packing launch per tape, a scheduling group of its own behind the parameter bound
    for which, imgs in plan._chain_imgs.items():
        if not imgs:
            continue
        off = blk = 0
        refs = []
        for wkey, e in imgs.items():
            e["off"], e["blk0"] = off, blk
            refs += [plan.P(wkey), ("chainimg", which, wkey), ("raw", e["mc"]), ("raw", e["kc"]), ("raw", e["cin"]), ("raw", e["dgrad"]), ("raw", blk)]
            off += e["bytes"]
            blk += e["blocks"]
        plan._chain_imgbuf[which] = plan.vec("chain_weights:" + which, off // 4)
        tape = plan.fwd_ops if which == "fwd" else plan.bwd_ops
        pos = next(k for k, o in enumerate(tape) if o["code"] == "UZ_OP_CHAIN")
        tape.insert(pos, _ops.make("UZ_OP_CHAIN_PACK", p=[plan.ptr_table(refs), ("amaxw", 0), plan._chain_imgbuf[which]], i=[len(imgs), blk],
                                   gid=("chainpack", which)))


def _chain_build(plan, which, ops, elig, net, px):
    fwd = which == "fwd"
    E = [k for k, o in enumerate(ops) if elig(o, px) and (net is None or _chain_net(o) == net)]
    if len(E) < 8:
        return
    deps = plan._hazard_deps(ops)
    vkey = lambda v: (id(v.buf), v.c0) if isinstance(v, View) else (id(v.view.buf), v.view.c0)
    # pairing tables
    ywriter, bn_of_y, dgrad_of_dx, bn_of_da = {}, {}, {}, {}
    for k, o in enumerate(ops):
        c = o["code"]
        if c == "UZ_OP_CONV_FWD" and isinstance(o.p("y"), View):
            ywriter[vkey(o.p("y"))] = k
        elif c == "UZ_OP_BN_RELU_FWD":
            bn_of_y[vkey(o.p("y"))] = k
        elif c == "UZ_OP_CONV_BWD_DATA" and isinstance(o.p("dx"), View):
            dgrad_of_dx.setdefault(vkey(o.p("dx")), []).append(k)
        elif c == "UZ_OP_BN_RELU_BWD" and isinstance(o.p("da"), View):
            bn_of_da[vkey(o.p("da"))] = k
    Es = set(E)
    changed = True
    while changed:
        changed = False
        for k in sorted(Es):
            o = ops[k]
            c = o["code"]
            if c == "UZ_OP_BN_RELU_FWD" and o.i("nslab") > 0 and ywriter.get(vkey(o.p("y"))) not in Es:
                Es.discard(k); changed = True                 # its convolution leaves slabs for it outside the chain
            elif c == "UZ_OP_CONV_FWD" and o.i("slabs_only") and bn_of_y.get(vkey(o.p("y"))) not in Es:
                Es.discard(k); changed = True
            elif c == "UZ_OP_BN_RELU_BWD" and o.i("nslab") > 0:
                dg = dgrad_of_dx.get(vkey(o.p("da")), [])
                if len(dg) != 1 or dg[0] not in Es:
                    Es.discard(k); changed = True             # dA arrives as slabs of a data gradient that is not in the chain
            elif c == "UZ_OP_CONV_BWD_DATA" and o.i("fold") == 3 and bn_of_da.get(vkey(o.p("dx"))) not in Es:
                Es.discard(k); changed = True
            elif c == "UZ_OP_LATENT_BWD" and not (k + 1 < len(ops) and ops[k + 1]["code"] == "UZ_OP_LATENT_HEADS_BWD_DATA" and (k + 1) in Es):
                Es.discard(k); changed = True
            elif c == "UZ_OP_LATENT_HEADS_BWD_DATA" and not (k >= 1 and ops[k - 1]["code"] == "UZ_OP_LATENT_BWD" and (k - 1) in Es):
                Es.discard(k); changed = True
        # convexity: no op outside may both depend on the set and be depended on by it
        desc = set()
        for k in range(len(ops)):
            if any(d in Es or d in desc for d in deps[k]):
                desc.add(k)
        bad = {k for k in Es if any((d not in Es) and (d in desc) for d in deps[k])}
        if bad:
            drop = set(bad)
            for k in sorted(Es):
                if any(d in drop for d in deps[k]):
                    drop.add(k)
            Es -= drop
            changed = True
    if len(Es) < 8:
        return
    anc = set()
    for k in reversed(range(len(ops))):
        if k in Es or k in anc:
            anc.update(d for d in deps[k] if d not in Es)
    # a scheduling group (one unit's ops, same gid, back to back) shares the lane's scratch - a unit's dy, a convolution's split-K
    # slabs - which the dependency analysis does not see: a group moves in front of the chain as a whole or not at all
    runs, a0 = [], 0
    for k in range(1, len(ops) + 1):
        if k == len(ops) or ops[k]["gid"] != ops[a0]["gid"]:
            runs.append((a0, k)); a0 = k
    grew = True
    while grew:
        grew = False
        for a0, b0 in runs:
            if any(k in anc for k in range(a0, b0)):
                for k in range(a0, b0):
                    if k not in Es and k not in anc:
                        anc.add(k); grew = True
        for k in sorted(anc, reverse=True):
            for d in deps[k]:
                if d not in Es and d not in anc:
                    anc.add(d); grew = True
    desc = set()
    for k in range(len(ops)):
        if any(d in Es or d in desc for d in deps[k]):
            desc.add(k)
    if any(k in desc for k in anc):
        return                                            # a group straddles the chain: leave this tape / sub-network per-op
    level = {}
    for k in sorted(Es):
        level[k] = 1 + max((level[d] for d in deps[k] if d in Es), default=-1)
    imgs = plan._chain_imgs.setdefault(which, {})
    G = plan.knobs.chain_wgs if fwd else plan.knobs.chain_wgs_bwd
    sub, flops = [], 0.0

    def emit(k, code, p, i, f=(), lvl=None):
        sub.append(dict(code=code, p=list(p), i=[int(v) for v in i], f=list(f), level=level[k] if lvl is None else lvl, orig=ops[k], k=k))

    def image(wkey, mc, kc, cin, dgrad):
        if wkey not in imgs:
            imgs[wkey] = dict(mc=mc, kc=kc, cin=cin, dgrad=dgrad, bytes=plan.L.uz_chain_packed_bytes(kc, mc), blocks=plan.L.uz_chain_pack_blocks(kc, mc))
        return ("chainimg", which, wkey)

    def weight_key(w):
        kind, wkey, offset = w
        assert kind == "param" and offset == 0, w
        return wkey

    extra_levels = {}            # op index -> 1 when a slab-sum phase was put behind it (shifts everything that depends on it)
    slab_of = {}
    for k in sorted(Es, key=lambda k: (level[k], k)):
        o = ops[k]
        c, I, P = o["code"], o.i, o.p
        if c == "UZ_OP_CONV_FWD":
            _, cin, cout, N, H, W, _ = conv_dims(o)
            x, w, bias, y = P("x", "w", "bias", "y")
            if cin <= 4:
                emit(k, "UZ_CH_CONV3_SMALL", [x, w, bias, y], [cin, I("ctot_x"), cout, I("ctot_y"), N, H, W])
                continue
            bk = bn_of_y.get(vkey(y))
            S = plan.L.uz_chain_conv_ksplit(cin, cout, N, H, W, G) if (bk in Es) else 1
            wkey = weight_key(w)
            slab = plan.vec(wkey + ":chslab", S * N * cout * H * W) if S > 1 else None
            if slab is not None:
                slab_of[vkey(y)] = (slab, S)
            emit(k, "UZ_CH_CONV3", [x, image(wkey, cout, cin, cin, 0), bias if S == 1 else None, y if S == 1 else None, slab, P("x_amax"), P("w_amax")],
                 [cin, I("ctot_x"), cout, I("ctot_y"), N, H, W, S, 0])
            flops += 2.0 * N * H * W * cin * cout * 9
            plan._packs["fwd"].pop(wkey, None)          # the image replaces the per-tape LDS image of the split kernels
        elif c == "UZ_OP_BN_RELU_FWD":
            slab, S = slab_of.get(vkey(P("y")), (None, 1))
            cbias = ops[ywriter[vkey(P("y"))]].p("bias") if S > 1 else None
            emit(k, "UZ_CH_BN_FWD", [*P("y", "gamma", "beta", "running_mean", "running_var", "save", "a"), slab, P("a_amax"), cbias],
                 [*I("C", "ctot_y", "ctot_a", "N"), I("H") * I("W"), I("relu"), S], o.f("eps", "momentum"))
        elif c == "UZ_OP_AVGPOOL_FWD":
            emit(k, "UZ_CH_AVGPOOL_FWD", P("x", "y", "x_amax", "y_amax"), I("C", "ctot_x", "ctot_y", "N", "H", "W"))
        elif c == "UZ_OP_BILINEAR_FWD":
            emit(k, "UZ_CH_BILINEAR_FWD", P("x", "y", "x_amax", "y_amax"), I("C", "ctot_x", "ctot_y", "N", "H", "W", "align_corners"))
        elif c == "UZ_OP_LATENT_HEADS_FWD":
            emit(k, "UZ_CH_HEADS_FWD", o["p"], [*I("cin", "ctot_h", "N"), I("H") * I("W"), I("act")])
        elif c == "UZ_OP_BN_RELU_BWD":
            slab, S = slab_of.get(("da",) + vkey(P("da")), (None, 1))
            emit(k, "UZ_CH_BN_BWD", [*P("da", "y", "gamma", "save"), P("dy").view, *P("dgamma", "dbeta", "dbias", "dy_amax"), slab, P("beta")],
                 [*I("C", "ctot_da", "ctot_y", "N"), I("H") * I("W"), I("relu"), S])
        elif c == "UZ_OP_CONV_BWD_DATA":
            _, cin, cout, N, H, W, _ = conv_dims(o)
            acc, dy, dx = I("accumulate"), P("dy").view, P("dx")
            wkey = weight_key(P("w"))
            if cin <= 4:
                emit(k, "UZ_CH_CONV3_SMALL_BWD_DATA", [dy, P("w"), dx], [cin, I("ctot_dx"), cout, I("ctot_dy"), N, H, W, acc])
                continue
            S = plan.L.uz_chain_conv_ksplit(cout, cin, N, H, W, G)
            folded = I("fold") == 3                           # the consumer's BatchNorm backward adds the slabs (the only reader of a dA this op alone writes)
            slab = plan.vec(wkey + ":chdslab", S * N * cin * H * W) if S > 1 else None
            emit(k, "UZ_CH_CONV3", [dy, image(wkey, cin, cout, cin, 1), None, dx if S == 1 else None, slab, P("dy_amax"), P("w_amax")],
                 [cout, I("ctot_dy"), cin, I("ctot_dx"), N, H, W, S, acc if S == 1 else 0])
            flops += 2.0 * N * H * W * cout * cin * 9
            if S > 1 and folded:
                slab_of[("da",) + vkey(dx)] = (slab, S)
            elif S > 1:
                # other writers / readers of dx: a reduction phase of its own right behind the convolution
                extra_levels[k] = 1
                emit(k, "UZ_CH_SLAB_SUM", [slab, dx], [S, N, cin, I("ctot_dx"), H * W, acc], lvl=level[k] + 0.5)
            plan._packs["bwd"].pop(wkey, None)
        elif c == "UZ_OP_AVGPOOL_BWD":
            emit(k, "UZ_CH_AVGPOOL_BWD", P("dy", "dx"), I("C", "ctot_dy", "ctot_dx", "N", "H", "W", "accumulate"))
        elif c == "UZ_OP_BILINEAR_BWD":
            emit(k, "UZ_CH_BILINEAR_BWD", P("dy", "dx"), I("C", "ctot_dy", "ctot_dx", "N", "H", "W", "align_corners", "accumulate"))
        elif c == "UZ_OP_LATENT_BWD":
            h = ops[k + 1]
            # (head a = the sigma head: LATENT_HEADS_BWD_DATA p = g_pre, g_mu, w_sigma, w_mu, dh)
            emit(k, "UZ_CH_LATENT_HEADS_BWD", [*o["p"], *h.p("w_a", "w_b", "dh")],
                 [*h.i("cin", "ctot_h", "N"), h.i("H") * h.i("W"), I("act"), h.i("accumulate")], lvl=level[k + 1])
        elif c == "UZ_OP_LATENT_HEADS_BWD_DATA":
            pass                                              # fused into the sub-op of the LATENT_BWD in front of it
        else:
            raise AssertionError(c)
    # a slab-sum phase sits at level + 0.5: renumber the levels densely, keeping the order
    if extra_levels:
        # everything that depends (inside the set) on an op with a slab-sum must come after the half level: recompute levels with that op one deeper
        lv2 = {}
        for k in sorted(Es):
            lv2[k] = max((lv2[d] + 1 + extra_levels.get(d, 0) for d in deps[k] if d in Es), default=0)
        for e in sub:
            e["level"] = lv2[e["k"]] + (1 if e["code"] == "UZ_CH_SLAB_SUM" else 0)
            if e["code"] == "UZ_CH_LATENT_HEADS_BWD":
                e["level"] = lv2[e["k"] + 1]
    sub.sort(key=lambda e: (e["level"], e["k"], e["code"] == "UZ_CH_SLAB_SUM"))
    dense = {lv: n for n, lv in enumerate(sorted({e["level"] for e in sub}))}
    for e in sub:
        e["level"] = dense[e["level"]]
    idx = len(plan._chains)
    plan._chains.append(dict(sub=sub, which=which, n_wgs=G, net=net))
    # access of the whole launch = the union of what its sub-ops touch (the packed images instead of the split kernels' ones)
    acc_ops = []
    for k in sorted(Es):
        q = ops[k].clone()
        if q["code"] in ("UZ_OP_CONV_FWD", "UZ_OP_CONV_BWD_DATA"):
            q.set(p={"w_image": None})
        acc_ops.append(q)
    n_ph = 1 + max(e["level"] for e in sub)
    chain_op = _ops.make("UZ_OP_CHAIN", p=[("chaintab", idx, "ops"), ("chaintab", idx, "phases"), ("chaintab", idx, "state")],
                         i=[n_ph, G, len(sub)], gid=("chain", idx), _acc_ops=acc_ops, _which=which,
                         _cost_s=n_ph * 12e-6 + flops / 100e12)   # (flops: the chain's 3 x 3 convolutions; first guess for the lane scheduler, tune_schedule measures it)
    new_ops = [ops[k] for k in range(len(ops)) if k in anc] + [chain_op] + [ops[k] for k in range(len(ops)) if k not in anc and k not in Es]
    ops[:] = new_ops
    plan.chain_info.setdefault(which, []).append(dict(net=net, ops=len(sub), phases=n_ph, convs=sum(e["code"] == "UZ_CH_CONV3" for e in sub), workgroups=G))


def _chain_tables(plan, idx):
    """Device tables of chain `idx` (built once, when the arena exists): the sub-ops in phase order with their tile ranges, the
    phase table, the barrier state."""
    ch = plan._chains[idx]
    if "dev" in ch:
        return ch["dev"]
    codes = _ffi.chain_codes()
    sub = ch["sub"]
    arr = (_ffi.uz_chain_op * len(sub))()
    phases, tile0, cur = [], 0, None
    for k, e in enumerate(sub):
        a = arr[k]
        a.code = codes[e["code"]]
        assert len(e["i"]) <= 16 and len(e["p"]) <= 12
        for j, v in enumerate(e["i"]):
            a.i[j] = int(v)
        for j, v in enumerate(e["f"]):
            a.f[j] = float(v)
        for j, r in enumerate(e["p"]):
            a.p[j] = plan._resolve(r, 0)
        nt = plan.L.uz_chain_op_tiles(C.byref(a))
        if nt <= 0:
            raise RuntimeError(f"chain sub-op {e['code']} {e['i']} is not covered by uz_chain_run")
        if e["level"] != cur:
            cur, tile0 = e["level"], 0
            phases.append([k, 0])
        # the op's tiles are dealt to the workgroups round-robin from workgroup tile0 on: behind a short op the next one starts
        # on the workgroups the first left idle
        a.tile0, a.ntiles = tile0 % ch["n_wgs"], nt
        tile0 += nt
        phases[-1][1] += 1
        e["tile0"], e["ntiles"] = a.tile0, nt
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
    dev = dict(ops=raw.to(plan.device), phases=torch.tensor(phases, dtype=torch.int32).reshape(-1).to(plan.device),
               state=torch.zeros(plan.L.uz_chain_state_bytes() // 4, dtype=torch.int32, device=plan.device), n_phases=len(phases))
    ch["dev"] = dev
    return dev


def chain_status(plan, stream_ptr):
    """0 when every chain launch of the last replay completed, else 1 + the phase whose grid barrier timed out (synchronises)."""
    worst = 0
    for idx, ch in enumerate(plan._chains):
        if "dev" in ch:
            out = C.c_int(0)
            _ffi.check(plan.L.uz_chain_status(C.c_void_p(ch["dev"]["state"].data_ptr()), C.byref(out), C.c_void_p(stream_ptr)), "chain_status")
            worst = max(worst, out.value)
    return worst
