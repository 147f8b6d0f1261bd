"""Lane scheduling of a tape: hazard analysis, cost models and the list scheduler.

Plain functions over ops and access triples - nothing here knows the plan.  `Plan._schedule` calls `schedule` with its
`_access`; `Plan._hazard_deps` (the chain pass, tests) calls `hazard_deps` per op.  Which resources an op reads, writes or
accumulates into is the plan's business (`Plan._access`, `Plan._resources`).
"""
from . import _ffi, _ops
from ._ops import conv_dims


def hazard_deps(accesses):
    """Per node of `accesses` (program order; each a (reads, writes, accumulates) triple of (space, lo, hi) half-open ranges) the
    set of earlier nodes it must follow - RAW, WAR and WAW; accumulators (bound slots only) commute with each other."""
    hist, deps = {}, []                                 # space -> list of [lo, hi, last writer, readers since, accumulators since]
    for k, (reads, writes, accs) in enumerate(accesses):
        d = set()
        for space, lo, hi in reads:                     # after the last writer and every accumulator since
            for e in hist.get(space, ()):
                if e[0] < hi and lo < e[1]:
                    if e[2] is not None:
                        d.add(e[2])
                    d.update(e[4])
        for space, lo, hi in accs:                      # after the last writer and every reader since (not after other accumulators)
            for e in hist.get(space, ()):
                if e[0] < hi and lo < e[1]:
                    if e[2] is not None:
                        d.add(e[2])
                    d.update(e[3])
        for space, lo, hi in writes:
            for e in hist.get(space, ()):
                if e[0] < hi and lo < e[1]:
                    if e[2] is not None:
                        d.add(e[2])
                    d.update(e[3])
                    d.update(e[4])
        d.discard(k)
        deps.append(d)
        for space, lo, hi in reads:
            for e in hist.setdefault(space, []):
                if e[0] < hi and lo < e[1]:
                    e[3].add(k)
            hist[space].append([lo, hi, None, {k}, set()])
        for space, lo, hi in accs:
            for e in hist.setdefault(space, []):
                if e[0] < hi and lo < e[1]:
                    e[4].add(k)
            hist[space].append([lo, hi, None, set(), {k}])
        for space, lo, hi in writes:
            lst = hist.setdefault(space, [])
            keep = [e for e in lst if not (lo <= e[0] and e[1] <= hi)]     # fully covered entries are superseded
            keep.append([lo, hi, k, set(), set()])
            hist[space] = keep
    return deps


def _op_cost(o):
    """Rough duration (s) of one op on MI355X - only the RELATIVE sizes matter: the list scheduler
    below uses them to decide which chains can share a lane."""
    c = o["code"]
    if "_cost_s" in o:
        return o["_cost_s"]
    if c in _ops.CONV_KIND:
        kind, cin, cout, N, H, W, ks = conv_dims(o)
        flop = 2.0 * N * H * W * cin * cout * ks * ks
        # measured fp32-equivalent TFLOP/s per plane size at batch 32 (tools/op_profile.py), forward / data
        # gradient and weight gradient; small channel counts and 1x1 kernels run far below these
        px = N * H * W
        table = ((262144, 180, 150), (65536, 190, 159), (16384, 148, 122), (4096, 97, 85), (1024, 37, 31), (256, 11, 9), (0, 3, 2.2))
        rate = next((f if kind != 2 else w) for lim, f, w in table if px >= lim) * 1e12
        if min(cin, cout) < 32 or ks == 1:
            rate = min(rate, 20e12)
        return flop / rate + 4e-6
    if c == "UZ_OP_BN_RELU_FWD" and o.i("phase") == 1:
        return 6e-6                                              # statistics from the convolution's partials: one small launch
    if c in ("UZ_OP_BN_RELU_FWD", "UZ_OP_BN_RELU_BWD", "UZ_OP_RELU_BWD"):
        C_, N, H, W = o.i("C", "N", "H", "W")
        if c == "UZ_OP_BN_RELU_FWD":
            return C_ * N * H * W * 12.0 / 4e12 + 10e-6
        return C_ * N * H * W * 20.0 / 4e12 + 14e-6
    if c in ("UZ_OP_AVGPOOL_FWD", "UZ_OP_AVGPOOL_BWD", "UZ_OP_BILINEAR_FWD", "UZ_OP_BILINEAR_BWD", "UZ_OP_NEAREST_FWD", "UZ_OP_NEAREST_BWD"):
        C_, N, H, W = o.i("C", "N", "H", "W")
        return C_ * N * H * W * 24.0 / 2e12 + 6e-6
    return 6e-6


def _op_cost_beside(o):
    """Duration (s) of one op as the lane replay REALISES it beside the other lanes' kernels (round 5: fitted per op class to the
    per-op lane traces profiles/r5_lane_trace_{fwd,bwd}.json of the headline configuration, tools/sched_calibrate.py prints the fit).
    The isolated model above is 2 - 6x short for the small launches (a 7-us convolution takes 33 - 45 us beside a device-filling
    kernel) and 1.4 - 10x long for the large ones: the list scheduler then queued off-critical weight gradients in front of a
    critical chain on the same lane and the chain started 2 ms late."""
    c = o["code"]
    if "_cost_s" in o:
        return o["_cost_s"]
    m = _op_cost(o) * 1e6
    if c in ("UZ_OP_CONV_FWD", "UZ_OP_CONV_BWD_DATA"):
        us = 28.0 + 0.62 * m
    elif c == "UZ_OP_CONV_BWD_WEIGHT":
        us = 25.0 + 0.70 * m
    elif c == "UZ_OP_BN_RELU_FWD":
        us = 20.0 + 0.50 * m
    elif c in ("UZ_OP_BN_RELU_BWD", "UZ_OP_RELU_BWD"):
        us = 25.0 + 0.80 * m
    elif c in ("UZ_OP_AVGPOOL_FWD", "UZ_OP_AVGPOOL_BWD"):
        us = 12.0 + 0.06 * m
    elif c in ("UZ_OP_BILINEAR_FWD", "UZ_OP_BILINEAR_BWD", "UZ_OP_NEAREST_FWD", "UZ_OP_NEAREST_BWD"):
        us = 18.0 + 0.42 * m
    elif c == "UZ_OP_WGRAD_REDUCE_TABLE":
        us = 8.0 + 0.0031 * o.i("total_blocks")       # HBM-bound: PHiSeg's 106 layers = 95 301 blocks take 300 us
    elif c in ("UZ_OP_MEMSET",):
        us = 8.0
    elif c in ("UZ_OP_W3D_PERMUTE", "UZ_OP_AVGPOOL3D_FWD", "UZ_OP_AVGPOOL3D_BWD", "UZ_OP_DEPTH_LERP_FWD", "UZ_OP_DEPTH_LERP_BWD",
               "UZ_OP_NEAREST3D_FWD", "UZ_OP_NEAREST3D_BWD", "UZ_OP_ADD_VIEWS"):
        # volume ops stream whole volumes: a flat 25 us was wrong by orders of magnitude (PHiSeg3D's static schedule)
        us = 12.0 + _vol_bytes(o) / 3.0e6                  # ~3 TB/s realised beside the other lanes' kernels
    else:
        us = 25.0
    return us * 1e-6


def _vol_bytes(o):
    """Bytes a volume / view op moves (input + output once)."""
    c = o["code"]
    if c == "UZ_OP_W3D_PERMUTE":
        return 8.0 * o.i("cout") * o.i("cin") * 27
    if c == "UZ_OP_ADD_VIEWS":
        C_, N, H, W = o.i("C", "N", "H", "W")
        return 12.0 * C_ * N * H * W
    C_, D, H, W = o.i("C", "D", "H", "W")
    n = float(C_) * D * H * W
    if c in ("UZ_OP_AVGPOOL3D_FWD", "UZ_OP_AVGPOOL3D_BWD"):
        return 4.0 * n * (1.0 + 0.125)
    if c in ("UZ_OP_DEPTH_LERP_FWD", "UZ_OP_DEPTH_LERP_BWD"):
        return 4.0 * n * 3.0
    return 4.0 * n * (1.0 + float(o.i("factor")) * o.i("factor") * o.i("factor_z"))          # nearest-neighbour 3-D


def _op_heavy(o):
    """True for ops that fill the chip on their own (only one of those is simulated in flight at a time)."""
    c = o["code"]
    if c in _ops.CONV_KIND:
        _, cin, cout, N, H, W, _ = conv_dims(o)
        return N * H * W >= 2048 and cin * cout >= 32 * 32      # measured: 512..8192 pixels all within 1 %
    if c in ("UZ_OP_BN_RELU_FWD", "UZ_OP_BN_RELU_BWD", "UZ_OP_RELU_BWD"):
        C_, N, H, W = o.i("C", "N", "H", "W")
        return C_ * N * H * W >= 4.0e6
    if c in ("UZ_OP_AVGPOOL_FWD", "UZ_OP_AVGPOOL_BWD", "UZ_OP_BILINEAR_FWD", "UZ_OP_BILINEAR_BWD", "UZ_OP_NEAREST_FWD", "UZ_OP_NEAREST_BWD"):
        C_, N, H, W = o.i("C", "N", "H", "W")
        return C_ * N * H * W >= 2.0e6
    return False


def schedule(ops, access, n_lanes, cost_model, heavy_mode):
    """Turns the tape into a DAG schedule for uz_graph_create_lanes and REORDERS `ops` in place.  access(op) gives the op's
    (reads, writes, accumulates); cost_model: "alone" = the isolated-launch model (_op_cost), "beside" = the model fitted to the lane
    replay's realised durations (_op_cost_beside); heavy_mode: which groups count as device-filling - "r4" = the round-4 rule (any op
    of the group above the size thresholds of _op_heavy), a number = groups whose modelled duration reaches that many microseconds,
    "off" = no group is heavy (plain critical-path list scheduling).

    1. Hazard analysis in program order: a group (one layer's forward, or one layer's backward;
       its ops stay back to back) depends on every earlier group it has a RAW, WAR or WAW conflict
       with (buffer channel ranges, gradient ranges, BN running buffers).
    2. Event-driven list scheduling in simulated time (cost model above) on n_lanes lanes (a lane is a
       scratch copy, so the groups of a lane stay ordered): among the groups that are ready, the one
       with the longest remaining critical path starts first; at most ONE device-filling ("heavy")
       group is in flight at a time, light groups start whenever a lane is free.  This staggers the
       independent chains (posterior / prior encoders, likelihood branches) so that the latency-bound
       deep levels of one run beside the device-filling layers of another, instead of both being
       deep - and the chip idle - at the same time.
    3. The tape is rewritten in simulated start order (a topological order of the DAG, so the
       eager runner stays correct) and every group gets: its lane, and the cross-lane groups it
       must wait for that are not already implied by its lane predecessor.
    Returns the ctypes uz_sched array (indexed like the reordered ops) and the scheduled DAG for diagnostics
    (tools/critical_path.py): per group in schedule order its op range, lane and predecessors."""
    n, K = len(ops), n_lanes
    sched = (_ffi.uz_sched * max(n, 1))()
    if n == 0:
        return sched, []
    groups = []                                         # [first, last] op index per group, program order
    for k, o in enumerate(ops):
        if groups and ops[groups[-1][1]]["gid"] == o["gid"]:
            groups[-1][1] = k
        else:
            groups.append([k, k])
    G = len(groups)
    # ---- 1. hazards between the groups: a group accesses what its ops access
    accesses = []
    for a, b in groups:
        reads, writes, accs = [], [], []
        for o in ops[a:b + 1]:
            r_, w_, a_ = access(o)
            reads.extend(r_); writes.extend(w_); accs.extend(a_)
        accesses.append((reads, writes, accs))
    deps = hazard_deps(accesses)
    # ---- 2. list scheduling in simulated time
    assert cost_model in ("alone", "beside"), cost_model
    op_cost = _op_cost_beside if cost_model == "beside" else _op_cost
    cost = [sum((o["cost_us"] * 1e-6 if "cost_us" in o else op_cost(o)) for o in ops[a:b + 1]) for a, b in groups]    # cost_us: measured (tune_schedule)
    succ = [[] for _ in range(G)]
    indeg = [len(d) for d in deps]
    for gi, d in enumerate(deps):
        for e in d:
            succ[e].append(gi)
    ready_at = [0.0] * G
    ready = [gi for gi in range(G) if indeg[gi] == 0]
    free = [0.0] * K
    tail = [None] * K
    finish = [0.0] * G
    order, lane_of = [], [None] * G
    # one device-filling group at a time (critical path first); light groups start whenever a lane is free
    if heavy_mode == "r4":
        heavy = [any(_op_heavy(o) for o in ops[a:b + 1]) for a, b in groups]
    elif heavy_mode == "off":
        heavy = [False] * G
    else:
        heavy = [c >= float(heavy_mode) * 1e-6 for c in cost]
    # (round 5, measured under the lane replay and removed - commit 0cbd7b7 has the code: device-filling groups on a lane of their own
    #  -7 %, weight-gradient-only groups on a low-priority lane -11 %, heavy weight gradients deferred behind the data-gradient chain -2 %;
    #  profiles/NOTES_r5.md section 3)
    blevel = [0.0] * G
    for gi in reversed(range(G)):
        blevel[gi] = cost[gi] + max((blevel[sg] for sg in succ[gi]), default=0.0)
    for gi, (a, b) in enumerate(groups):
        if any(o["code"] == "UZ_OP_EVENT_RECORD" for o in ops[a:b + 1]):
            blevel[gi], cost[gi] = 1e9, 1e-7      # bucket-final markers cost nothing and must fire the moment their bucket is done
            # ... and so must the bucket's deferred reductions (slab / bias-row tables): they are the last writers of the bucket, they
            # have no other successor, and left at their own bottom level the list scheduler runs them LAST - all buckets final at 98 %
            # of the tape, nothing of the exchange overlapped (headline plan under the round-5 cost model; 84 % under the old one)
            for d in deps[gi]:
                if any(o["code"] in ("UZ_OP_WGRAD_REDUCE_TABLE", "UZ_OP_CHAN_SUM_TABLE") for o in ops[groups[d][0]:groups[d][1] + 1]):
                    blevel[d] = 1e8
    t, running = 0.0, []
    while len(order) < G:
        running = [(f, g) for f, g in running if f > t + 1e-12]
        busy_lanes = {lane_of[g] for _, g in running}
        heavy_busy = any(heavy[g] for _, g in running)
        started = False
        for gi in sorted((g for g in ready if ready_at[g] <= t + 1e-12), key=lambda g: (-blevel[g], g)):
            lanes_free = [l for l in range(K) if l not in busy_lanes]
            if not lanes_free or (heavy[gi] and heavy_busy):
                continue
            pref = [l for l in lanes_free if tail[l] is not None and tail[l] in deps[gi]]
            lane = pref[0] if pref else min(lanes_free, key=lambda l: (free[l], l))
            lane_of[gi] = lane
            finish[gi] = t + cost[gi]
            free[lane] = finish[gi]
            tail[lane] = gi
            order.append(gi)
            ready.remove(gi)
            running.append((finish[gi], gi))
            busy_lanes.add(lane)
            heavy_busy = heavy_busy or heavy[gi]
            started = True
            for sgi in succ[gi]:
                indeg[sgi] -= 1
                ready_at[sgi] = max(ready_at[sgi], finish[gi])
                if indeg[sgi] == 0:
                    ready.append(sgi)
        if not started:
            nxt = [f for f, _ in running] + [ready_at[g] for g in ready if ready_at[g] > t + 1e-12]
            assert nxt, "dependency cycle in the tape"
            t = min(nxt)
    assert len(order) == G, "dependency cycle in the tape"
    # ---- 3. rewrite the tape in schedule order, compute waits
    new_ops, first, last = [], [0] * G, [0] * G
    for gi in order:
        a, b = groups[gi]
        first[gi] = len(new_ops)
        new_ops.extend(ops[a:b + 1])
        last[gi] = len(new_ops) - 1
    ops[:] = new_ops
    sched = (_ffi.uz_sched * max(n, 1))()
    anc = [0] * G                                       # bitset of transitive predecessors (incl. lane order)
    ltail = [None] * K
    for gi in order:
        lane = lane_of[gi]
        mask = 0
        for d in deps[gi]:
            mask |= anc[d] | (1 << d)
        implied = 0
        if ltail[lane] is not None:
            implied = anc[ltail[lane]] | (1 << ltail[lane])
            mask |= implied
        per_lane = {}
        for d in deps[gi]:
            if lane_of[d] != lane and not (implied >> d) & 1:
                cur = per_lane.get(lane_of[d])
                if cur is None or first[d] > first[cur]:
                    per_lane[lane_of[d]] = d
        waits = list(per_lane.values())
        waits = [d for d in waits if not any(d != e and (anc[e] >> d) & 1 for e in waits)]
        anc[gi] = mask
        ltail[lane] = gi
        k0 = first[gi]
        sched[k0].n_wait = len(waits)
        for w, d in enumerate(sorted(waits, key=lambda d: first[d])):
            sched[k0].wait[w] = last[d]
            sched[last[d]].signal = 1
        for k in range(first[gi], last[gi] + 1):
            sched[k].lane = lane
            ops[k]["lane"] = lane
    pos = {gi: n_ for n_, gi in enumerate(order)}
    dag = [dict(first=first[gi], last=last[gi], lane=lane_of[gi], deps=sorted(pos[d] for d in deps[gi]),
                sim_start=finish[gi] - cost[gi], sim_cost=cost[gi], blevel=blevel[gi]) for gi in order]
    return sched, dag
