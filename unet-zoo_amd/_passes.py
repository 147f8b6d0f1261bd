"""Plan-time rewrites of the emitted tapes, run by Plan.finalize() in this order: split storage (_split_storage_passes), BatchNorm's
apply pass off the forward chain (_bn_offchain_pass, off by default), bf16 storage of the volume path (_b16_pass); the fourth, the
deep-level chain, is _chain_plan.py.  Each is a function of the plan: it reads the ops the emitters left (Plan._units, Plan._vol_units,
the tapes), rewrites them in place and leaves a summary dict on the plan (round4, bn_offchain, b16_info).
"""
from . import _chain_plan, _ops
from ._ops import conv_dims
from ._plan import View, _ScratchView, _buf_of


def _users_of(plan, v):
    """(writers, readers) of the channels of view `v` across all tapes, each a list of (op, slot name, ref)."""
    writers, readers = [], []
    for _, ops in plan._all_tapes():
        for o in ops:
            wr = _ops.writes(o)
            for j, r in enumerate(o["p"]):
                if isinstance(r, View) and r.buf is v.buf and r.c0 < v.c0 + v.C and v.c0 < r.c0 + r.C:
                    (writers if j in wr else readers).append((o, _ops.SCHEMA[o["code"]].p[j], r))
    return writers, readers


def _sole_dgrad(plan, u, tabbed):
    """The plain data gradient that is the ONLY writer of unit `u`'s dA, which nothing but the unit's BatchNorm backward reads;
    None when there is no such op."""
    B, ga = u.get("bn_bwd"), u.get("ga")
    if B is None or not isinstance(ga, View) or ga.nb is not None or id(ga.buf) in tabbed:
        return None
    writers, readers = _users_of(plan, ga)
    if len(writers) != 1 or len(readers) != 1 or readers[0][0] is not B:
        return None
    W, nm, r = writers[0]
    if W["code"] != "UZ_OP_CONV_BWD_DATA" or nm != "dx" or (r.c0, r.C, r.nb) != (ga.c0, ga.C, None) or W.p("fold_arg") is not None or W.i("accumulate"):
        return None
    return W


def _split_storage_passes(plan):
    """Plan-time rewrites on the Conv2D units (torchlayers.py:18-21) of the large planes, all decided from the emitted ops:
      1. folded backward reduction - where the ONLY writer of a unit's dA is an unsplit split-path data gradient, that launch masks
         dA with the unit's ReLU and leaves the BatchNorm-backward sums in its epilogue; the unit's backward runs a per-channel
         finalise instead of the reduction pass over dA and y (off unless UZ_FOLD_BN_BWD=1);
      2. dY in split storage - where both consumers of a unit's dy (its weight and data gradient) run on the split path, the
         BatchNorm-backward apply pass writes the operand pieces instead of fp32 values (UZ_PACK_DY=0);
      3. activations in split storage - a buffer written only by BatchNorm-apply / pooling / interpolation launches that know
         their bound beforehand and read only by split-path convolutions (forward + weight gradient) is kept as operand pieces;
         a concat buffer's (at most two) producers each scale from a slot of their own (UZ_PACK_ACT=0).
    Returns a summary dict (also kept as plan.round4)."""
    info = dict(folded=0, dy_packed=0, act_packed=0, act_views=0)
    plan.round4 = info
    units = [u for u in plan._units if "bn_bwd" in u or "bn_fwd" in u]
    if plan.L.uz_get_conv_math() in (0, 3) or not plan.bn_training:
        return info                              # fp32-only / bf16 modes have no two-piece operands
    knobs = plan.knobs
    large = lambda u: u["N"] * u["H"] * u["W"] > 4096 and (u["H"] * u["W"]) % 4 == 0
    tabbed = {id(q.buf) for t in plan.ptr_tables for q in t if isinstance(q, View)}
    # ---- 1. folded backward reduction
    # (off by default: measured on MI355X the epilogue's extra read of y is exposed - the 64-channel-tile kernel keeps ONE
    #  workgroup per CU, so its memory phase overlaps nothing: data gradient of 128 -> 128 @ 128 x 128 451 -> 573 us against
    #  269 -> 170 us for the unit's BatchNorm backward; step +-0)
    if knobs.fold_bn_bwd and plan.bwd_ops:
        for u in units:
            if not large(u) or u["npart"] <= 0:
                continue
            W = _sole_dgrad(plan, u, tabbed)
            if W is None:
                continue
            _, cin_w, cout_w, N, H, Wd, ks = conv_dims(W)
            if ks != 3:
                continue
            rows = plan.L.uz_conv_bwd_relu_partials(cin_w, cout_w, N, H, Wd, 3)
            if rows <= 0 or cin_w != u["C"]:
                continue
            part = plan.vec(u["name"] + ":bwdpart", 4 * u["C"] * rows)
            y = u["y"]
            W.set(p={"fold_arg": y, "partials": part, "bn_stats": u["save"]}, i={"ctot_fold": y.Ctot, "fold": 2, "fold_relu": u["relu"]})
            u["bn_bwd"].set(p={"da_partials": part}, i={"npart": rows})
            info["folded"] += 1
    # ---- 1b. small planes: the data gradient's split-K reduce folded into the consumer's BatchNorm backward (the mirror of the
    # forward's uz_conv_fwd_slabs / uz_bn_relu_fwd_slabs): where the ONLY writer of a unit's dA is a split-K fp32 data gradient, that
    # launch leaves its partial sums in a buffer of the layer's own and the unit's one-workgroup-per-channel backward adds them
    # itself - one reduction launch less on the backward chains of the 8 x 8 ... 2 x 2 levels (UZ_BN_FOLD_DGRAD=0 switches it off)
    info["dgrad_folded"] = 0
    if knobs.bn_fold_dgrad and plan.bwd_ops:
        for u in units:
            if u["N"] * u["H"] * u["W"] > 4096:
                continue
            W = _sole_dgrad(plan, u, tabbed)
            if W is None:
                continue
            _, cin_w, cout_w, N, H, Wd, ksw = conv_dims(W)
            parts = plan.L.uz_conv_bwd_splitk_parts(cin_w, cout_w, N, H, Wd, ksw)
            if parts <= 1 or cin_w != u["C"]:
                continue
            slabs = plan.vec(u["name"] + ":daslabs", parts * N * cin_w * H * Wd)
            W.set(p={"fold_arg": slabs}, i={"fold": 3})
            u["bn_bwd"].set(p={"da_partials": slabs}, i={"nslab": parts})
            info["dgrad_folded"] += 1
    # ---- 2. dY in split storage
    if knobs.pack_dy and plan.bwd_ops:
        for u in units:
            B, wg, dg = u.get("bn_bwd"), u.get("wgrad"), u.get("dgrad")
            if B is None or wg is None or not large(u) or u["ks"] != 3 or u["W"] % 4:
                continue
            if u["N"] * u["H"] * u["W"] <= plan.L.uz_bn_bwd_fused_limit(u["H"], u["W"]):
                continue                         # one-launch backward (channel's batch on chip): no tensor-wide bound before the first write
            if plan.L.uz_conv_route(2, u["cin"], u["C"], u["N"], u["H"], u["W"], 3) != 1:
                continue
            if dg is not None and (plan.L.uz_conv_route(1, u["cin"], u["C"], u["N"], u["H"], u["W"], 3) != 1 or dg.i("fold") == 1):
                continue
            for o in (B, wg, dg):
                if o is not None:
                    o.set(i={"dy_packed": 1})
            info["dy_packed"] += 1
    # ---- 3. activations in split storage
    if knobs.pack_act and not plan.extra_ops:
        named = {id(v.buf) for v in plan.named.values() if isinstance(v, View)}
        for b in plan.bufs:
            if b.alias is not None or id(b) in tabbed or id(b) in named or (b.H * b.W) % 4 or b.N * b.H * b.W <= max(4096, _chain_plan._chain_limit(plan)):
                continue                                 # (planes of the deep-level chain stay fp32: its convolutions split on the fly)
            wr_list, rd_list, ok = [], [], True
            for tape, ops in plan._all_tapes():
                for o in ops:
                    c = o["code"]
                    writer, reader = _ops.SPLIT_WRITERS.get(c), _ops.SPLIT_READERS.get(c)
                    for nm, r in zip(_ops.SCHEMA[c].p, o["p"]):
                        if _buf_of(r) is not b:
                            continue
                        if not isinstance(r, View) or r.nb is not None:
                            ok = False
                        elif writer and nm == writer[0]:
                            if c == "UZ_OP_BN_RELU_FWD":
                                N, H, W = o.i("N", "H", "W")
                                one_launch = 4096 < N * H * W <= plan.L.uz_bn_fwd_fused_limit(H, W)      # mid path: a-priori bound from the parameters
                                if not (o.i("training") and o.i("nslab") == 0 and (o.i("npart") > 0 or one_launch)):
                                    ok = False           # needs the bound before the first word is written
                            elif o.p("x_amax") is None:
                                ok = False               # pooling / interpolation forward their INPUT's bound
                            wr_list.append((o, r))
                        elif reader and nm == reader[0]:
                            kind, cin, cout, N, H, W, ks = conv_dims(o)
                            if ks != 3 or plan.L.uz_conv_route(kind, cin, cout, N, H, W, 3) != 1 or (kind == 0 and o.i("slabs_only")):
                                ok = False
                            rd_list.append((o, r))
                        else:
                            ok = False
            if not ok or not wr_list or not rd_list:
                continue
            wr_list.sort(key=lambda t: t[1].c0)
            segs = [(r.c0, r.c0 + r.C) for _, r in wr_list]
            if any(a[1] > b2[0] for a, b2 in zip(segs, segs[1:])):
                continue                                 # overlapping producers
            plan_rd = []
            for o, r in rd_list:
                cov = [sg for sg in segs if sg[0] < r.c0 + r.C and r.c0 < sg[1]]
                tiled = cov and cov[0][0] <= r.c0 and cov[-1][1] >= r.c0 + r.C and all(a[1] == b2[0] for a, b2 in zip(cov, cov[1:]))
                if not tiled or len(cov) > 2 or (len(cov) == 2 and (cov[1][0] - r.c0) % 16):
                    ok = False
                    break
                plan_rd.append((o, r, cov))
            if not ok:
                continue
            slot_of = {}
            for o, r in wr_list:
                _, bound, flag = _ops.SPLIT_WRITERS[o["code"]]
                slot = slot_of[(r.c0, r.c0 + r.C)] = ("amax", plan._new_amax())
                o.set(p={bound: slot + ("acc",)}, i={flag: 1})
            for o, r, cov in plan_rd:
                _, bound, bound2, seg2_c0, flag = _ops.SPLIT_READERS[o["code"]]
                two = len(cov) == 2
                o.set(p={bound: slot_of[cov[0]], bound2: slot_of[cov[1]] if two else None}, i={flag: 1, seg2_c0: cov[1][0] - r.c0 if two else 0})
            b.packed = True
            info["act_packed"] += 1
            info["act_views"] += len(wr_list)
    return info


def _bn_offchain_pass(plan):
    """Takes BatchNorm's apply pass out of the forward's dependency chain (round 6; UZ_BN_OFFCHAIN=1, off by default).  For a Conv -> BatchNorm -> ReLU
    unit on the large planes whose activation is kept in split storage and read, in the forward tape, by exactly ONE 3 x 3 split-path
    convolution (the middle layers of every three-convolution block; the weight gradient of that convolution reads it too, in the
    backward tape): the unit's BatchNorm op becomes two - the statistics launch, which stays in the unit's group, and the apply pass, a
    group of its own - and the consumer reads the unit's PRE-normalisation output with its statistics table and applies BatchNorm +
    ReLU in its staging (uz_conv_fwd_bn_ex: the same operand pieces the apply pass stores).  The consumer then depends on the
    statistics launch only; the apply pass still writes the activation for the weight gradient, beside the chain instead of in it."""
    info = dict(units=0)
    plan.bn_offchain = info
    if not plan.knobs.bn_offchain or plan.L.uz_get_conv_math() in (0, 3) or not plan.bn_training or plan.extra_ops:
        return info
    ops = plan.fwd_ops
    for u in [u for u in plan._units if "bn_fwd" in u]:
        B = u["bn_fwd"]
        if not (B.i("a_packed") == 1 and B.i("npart") > 0 and B.i("nslab") == 0 and B.i("training") == 1) or B.i("phase") or B.i("b16"):
            continue                                             # large path, statistics from the convolution's partials, split-storage output
        N, H, W = B.i("N", "H", "W")
        if N * H * W <= plan.L.uz_bn_fwd_fused_limit(H, W) or not any(o is B for o in ops):
            continue
        y, a = B.p("y", "a")
        if not (isinstance(a, View) and isinstance(y, View)) or a.nb is not None or y.nb is not None or not a.contiguous:
            continue
        readers = [(o, nm, r) for o in ops for nm, r in zip(_ops.SCHEMA[o["code"]].p, o["p"]) if o is not B and isinstance(r, View) and r.buf is a.buf]
        if len(readers) != 1 or any(isinstance(r, View) and r.buf is a.buf for o in plan.loss_ops for r in o["p"]):
            continue
        R, nm, rv = readers[0]
        if R["code"] != "UZ_OP_CONV_FWD" or nm != "x" or R.i("ks") != 3 or R.i("x_packed") != 1 or any(R.i("relu", "x_seg2_c0", "slabs_only", "bn_in", "b16")) or \
                (rv.c0, rv.C, rv.nb) != (0, a.buf.C, None):
            continue
        k = next(n for n, o in enumerate(ops) if o is B)
        fin = B.clone().set(p={"y": None, "a": None}, i={"phase": 1})
        plan._detached += 1
        kind, slot, _acc = B.p("a_amax")                         # the apply pass reads the bound the statistics launch published
        app = B.clone(gid=("bnapply", plan._detached)).set(p={"running_mean": None, "running_var": None, "bn_partials": None, "a_amax": (kind, slot)},
                                                                i={"phase": 2})
        ops[k:k + 1] = [fin, app]
        u["bn_fwd"] = fin
        R.set(p={"x": y, "x_amax2": None, "bn_stats": B.p("save")}, i={"ctot_x": y.Ctot, "x_packed": 0, "bn_in": 1 | (B.i("relu") << 1)})
        info["units"] += 1
    return info


# ------------------------------------------------------------------ bf16 storage (BASELINE config 5: PHiSeg3D "bf16")
def _b16_slots(plan, o):
    """(p[] slot, format bit) of the tensor operands of op `o` that may be bf16; () = no bf16-storage form.  A pass-through to
    _ops.b16_slots, kept because callers outside this module ask the plan (Plan._b16_slots)."""
    return _ops.b16_slots(o)


def _b16_ok(plan, o):
    """Can op `o` run through its bf16-storage entry point (whatever the formats of its operands turn out to be)?  Only the base
    form of a kernel has one (Op.base_form: the format bits themselves are what this pass sets, they do not count)."""
    c = o["code"]
    if c in _ops.CONV_KIND:
        kind, cin, cout, N, H, W, ks = conv_dims(o)
        base = o.base_form() and (kind != 1 or o.p("fold_arg") is None)
        if ks == 1:
            return cout in (1, 2, 3, 4, 6, 8) and cin <= 512 and (H * W) % 4 == 0 and base
        if ks != 3 or W % 32:
            return False
        if kind == 2:
            # (a weight gradient may leave its slabs to the table launch - slabs_only / nslab - in either storage: uz_conv_bwd_weight_b16 takes slabs_out)
            if any(o.i("x_packed", "x_seg2_c0", "dy_packed")) or o.p("db") is not None:
                return False
        elif not base:
            return False
        if kind != 2 and plan.L.uz_conv_split_parts(kind, cin, cout, N, H, W) != 1:
            return False
        return plan.L.uz_conv_route(kind, cin, cout, N, H, W, 3) == 1
    if c == "UZ_OP_BN_RELU_FWD":
        N, H, W = o.i("N", "H", "W")
        return N * H * W > 32768 and (H * W) % 4 == 0 and o.i("training") == 1 and o.base_form()
    if c == "UZ_OP_BN_RELU_BWD":
        N, H, W = o.i("N", "H", "W")
        return N * H * W > 32768 and (H * W) % 4 == 0 and o.base_form() and o.p("da_partials") is None
    if c in ("UZ_OP_AVGPOOL3D_FWD", "UZ_OP_AVGPOOL3D_BWD"):
        return o.i("W") % 4 == 0 and o.i("H") % 2 == 0
    if c in ("UZ_OP_DEPTH_LERP_FWD", "UZ_OP_DEPTH_LERP_BWD"):
        return (o.i("H") * o.i("W")) % 4 == 0
    if c == "UZ_OP_BILINEAR_FWD":                          # the band kernel's shapes
        return o.i("W") % 4 == 0 and o.i("W") <= 128 and o.i("H") >= 4 and o.base_form() and (o.p("x_amax") is None or True)
    if c == "UZ_OP_BILINEAR_BWD":
        return 2 * o.i("W") <= 128 and o.i("H") >= 4 and 256 % o.i("W") == 0 and o.p("a") is None and o.base_form()
    return False


def _b16_pass(plan):
    """Which volume tensors are kept in bf16 (UZ_STORE_B16=1, single-piece bf16 arithmetic only): a buffer whose
    EVERY reader and writer - in every tape - is an op with a bf16-storage form on a shape that form serves (the 3x3x3
    convolutions on the matrix pipe with planes wider than 32, the large-plane BatchNorm path, AvgPool3d, the depth stage of the
    trilinear interpolation).  The decision is per buffer, every op carries one format bit per tensor operand (its b16 slot), so the
    two formats mix freely: what some other op touches (the 1x1x1 heads' inputs, the in-plane interpolation's operands, the
    latent and loss tensors, the image) stays fp32.  A unit's dy moves to a bf16 twin of the zero-bordered scratch class when
    its three backward ops all qualify.  Returns / keeps a summary in plan.b16_info."""
    info = plan.b16_info = dict(buffers=0, grads=0, dy=0, bytes_saved=0, ops=0)
    on = plan.knobs.store_b16
    if not on or plan.L.uz_get_conv_math() != 3 or not plan.bn_training or plan.extra_ops:
        return info
    all_ops = [o for ops in (plan.fwd_ops, plan.loss_ops, plan.bwd_ops) for o in ops]
    tabbed = {id(q.buf) for t in plan.ptr_tables for q in t if isinstance(q, View)}
    named = {id(v.buf) for v in plan.named.values() if isinstance(v, View)}
    ok_cache = {}
    bad, seen = set(), set()
    for o in all_ops:
        slots = [j for j, _ in _b16_slots(plan, o)]
        if id(o) not in ok_cache:
            ok_cache[id(o)] = bool(slots) and _b16_ok(plan, o)
        for j, r in enumerate(o["p"]):
            b = _buf_of(r)
            if b is None:
                continue
            seen.add(id(b))
            if not (ok_cache[id(o)] and j in slots):
                bad.add(id(b))
    for b in plan.bufs:
        if not b.vol or b.alias is not None or id(b) in tabbed or id(b) in named or id(b) in bad or id(b) not in seen:
            continue
        if b.W % 32 or (b.N - 2) * b.H * b.W <= 32768:
            continue
        b.b16 = True
        info["grads" if b.name.startswith("grad:") else "buffers"] += 1
        info["bytes_saved"] += 2 * b.numel
    # dy of the units: the lane's zero-bordered scratch class (slices, elements per slice) -> its bf16 twin
    for u in plan._vol_units:
        B, Wg, Dg, gyv = u["bn_bwd"], u["wgrad"], u["dgrad"], u["gyv"]
        if Wg is None or gyv.zkey is None or gyv.view is not None:
            continue
        if not (_b16_ok(plan, B) and _b16_ok(plan, Wg) and (Dg is None or _b16_ok(plan, Dg))):
            continue
        old = gyv.zkey
        new = (old[0], old[1], 16)
        plan._gyz[new] = max(plan._gyz.get(new, 0), (plan._gyz[old] + 1) // 2)
        gyv.zkey = new
        assert B.p("dy") == ("gyvol", old)
        B.set(p={"dy": ("gyvol", new)})
        B["b16_dy"] = Wg["b16_dy"] = True
        if Dg is not None:
            assert Dg.p("dy") == ("gywin", old)
            Dg.set(p={"dy": ("gywin", new)})
            Dg["b16_dy"] = True
        info["dy"] += 1
    used = set()
    for o in all_ops:
        for q in o["p"]:
            if isinstance(q, _ScratchView) and q.zkey is not None:
                used.add(q.zkey)
            elif isinstance(q, tuple) and q and q[0] in ("gyvol", "gywin"):
                used.add(q[1])
    for k in [k for k in plan._gyz if k not in used]:
        del plan._gyz[k]                                   # an fp32 class every unit has left
    # format bits
    for o in all_ops:
        slots = _b16_slots(plan, o)
        if not slots or not ok_cache.get(id(o)):
            continue
        dy_slot = _ops.SCHEMA[o["code"]].px["dy"] if o.get("b16_dy") else None
        bits = 0
        for j, k in slots:
            b = _buf_of(o["p"][j])
            bits |= int((b is not None and b.b16) or j == dy_slot) << k
        if bits:
            o.set(i={"b16": bits})
            info["ops"] += 1
    return info
