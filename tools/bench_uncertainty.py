#!/usr/bin/env python3
"""Time metrics.score_uncertainty (uz_vol_uncertainty, csrc/voluncert.hip) on BraTS-sized label volumes: S = 16 samples, a decision
volume and a reference, R = 3 nested regions (WT / TC / ET of the raw BraTS values), at 128^3 and 240 x 240 x 155, on two inputs: the
smooth-blob volumes of tools/bench_volscore.py (row 16 is the decision), and the same volumes with 1 % of the voxels flipped to a random
label; and on samples, a decision and a reference that are all background ("empty"): the pass with nothing to put into the
tables, which shows what the streaming alone costs.

Per shape and input: the call without and with the vote maps, each with the bytes the pass must move - (S + 2) P read, with votes R P
more written; the slices and the finish's outputs are a few hundred KB and not counted - as GB/s of the WHOLE call (two launches) and
as a share of the copy rate measured in the same run (a device-to-device copy of 1 GiB, read + written bytes over its median time).
BESIDE it metrics.score_volume(hd95=False) on the same S + 1 rows, the yardstick of a streaming pass over label volumes in this
project, and AGAINST it the same tables from numpy on the host (a 256-entry lookup per region, a sum over the samples, one bincount),
timed once and compared with the device's table integer for integer.
--kernel-stats FILE reads a rocprofv3 --kernel-trace --stats CSV of a run of this tool (taken in a run of its own) and puts the two
launches' own durations into the notes.  Each device time is the median of `--repeats` calls between two device events after
`--warmup` calls.  --notes writes profiles/NOTES_uncertainty.md.  Without a GPU the tool exits.
usage: python tools/bench_uncertainty.py [--notes] [--repeats 20] [--warmup 3] [--shapes 128x128x128 240x240x155] [--inputs smooth speckle empty]
                                         [--no-host] [--no-score] [--no-votes] [--kernel-stats FILE]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import unet_zoo_amd  # noqa: E402,F401
from unet_zoo_amd import _ffi, metrics  # noqa: E402
from bench_volscore import blobs, timed  # noqa: E402
from bench_components import speckle  # noqa: E402

SAMPLES, REGIONS = 16, metrics.BRATS_REGIONS
VOLWINDOW_FINISH_SHARE = 0.76                                            # profiles/NOTES_volwindow.md: uz_vol_window_finish over the copy rate
COPY_BYTES = 1 << 30


def copy_rate(dev, warmup, repeats):
    """GB/s of a device-to-device copy: bytes read + bytes written over the median time"""
    src = torch.zeros(COPY_BYTES, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src), warmup, repeats)
    return 2 * COPY_BYTES / t["median"] / 1e6, t


def host_tables(smp, dec, ref, regions):
    """the same tables from numpy: (R, S+1, 2, 2) int64"""
    S = smp.shape[0]
    out = np.zeros((len(regions), S + 1, 2, 2), np.int64)
    for r, reg in enumerate(regions):
        lut = np.zeros(256, np.uint8)
        lut[list(reg)] = 1
        c = lut[smp].sum(0, dtype=np.int64).ravel()
        out[r] = np.bincount(c * 4 + lut[dec].ravel().astype(np.int64) * 2 + lut[ref].ravel(), minlength=(S + 1) * 4).reshape(S + 1, 2, 2)
    return out


def one_input(name, rows_h, ref_h, shape, args, dev, copy_gbs):
    D, H, W = shape
    P = D * H * W
    smp, dec, ref = torch.from_numpy(rows_h[:SAMPLES]).to(dev), torch.from_numpy(rows_h[SAMPLES]).to(dev), torch.from_numpy(ref_h).to(dev)
    rows = torch.from_numpy(rows_h).to(dev)
    route = (C.c_int * 3)()
    _ffi.lib().uz_vol_uncertainty_route(SAMPLES, len(REGIONS), D, H, W, 16, route)
    sink = {}

    def plain():
        sink["plain"] = metrics.score_uncertainty(smp, ref, REGIONS, decision=dec)

    def with_votes():
        sink["votes"] = metrics.score_uncertainty(smp, ref, REGIONS, decision=dec, return_votes=True)
    t_plain = timed(plain, args.warmup, args.repeats)
    first = [t.clone() for t in (sink["plain"].table, sink["plain"].levels, sink["plain"].dice, sink["plain"].auc, sink["plain"].calibration)]
    plain()
    again = (sink["plain"].table, sink["plain"].levels, sink["plain"].dice, sink["plain"].auc, sink["plain"].calibration)
    bit_equal = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first, again))
    t_votes = timed(with_votes, args.warmup, args.repeats) if not args.no_votes else dict(median=float("nan"), min=float("nan"), max=float("nan"))
    b_plain, b_votes = (SAMPLES + 2) * P, (SAMPLES + 2 + len(REGIONS)) * P
    tab = sink["plain"].table.cpu().numpy()
    row = dict(input=name, shape=list(shape), samples=SAMPLES, regions=len(REGIONS), route=list(route), plain_ms=t_plain, votes_ms=t_votes,
               plain_mb=round(b_plain / 1e6, 1), votes_mb=round(b_votes / 1e6, 1),
               plain_gbs=round(b_plain / t_plain["median"] / 1e6, 1), votes_gbs=round(b_votes / t_votes["median"] / 1e6, 1),
               plain_share=round(b_plain / t_plain["median"] / 1e6 / copy_gbs, 3), votes_share=round(b_votes / t_votes["median"] / 1e6 / copy_gbs, 3),
               repeat_bit_equal=bit_equal, background_share=round(float(tab[0, 0, 0, 0]) / P, 4),
               score=[round(float(v), 4) for v in sink["plain"].auc[:, 3].cpu()], ece=[round(float(v), 5) for v in sink["plain"].calibration[:, 0].cpu()],
               workspace_kb=round(_ffi.lib().uz_vol_uncertainty_workspace(SAMPLES, len(REGIONS), D, H, W) / 1e3, 1))
    if not args.no_score:
        def score():
            sink["score"] = metrics.score_volume(rows, ref, REGIONS, hd95=False)
        row["score_volume_ms"] = timed(score, args.warmup, args.repeats)
        row["score_volume_gbs"] = round((SAMPLES + 2) * P / row["score_volume_ms"]["median"] / 1e6, 1)       # it reads the reference once per row: an upper bound of what it must move
        row["plain_over_score_volume"] = round(t_plain["median"] / row["score_volume_ms"]["median"], 3)
    if not args.no_host:
        t0 = time.perf_counter()
        want = host_tables(rows_h[:SAMPLES], rows_h[SAMPLES], ref_h, REGIONS)
        dt = time.perf_counter() - t0
        row.update(host_s=round(dt, 3), host_table_equal=bool(np.array_equal(want, tab)), speedup_vs_host=round(dt * 1e3 / t_plain["median"], 1))
    return row


def kernel_rows(path):
    """the table pass and the finish out of a rocprofv3 --stats CSV: [(name, calls, average us, min us, max us)]"""
    out = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            if "table_k<" in r["Name"] or "unc_finish_k" in r["Name"]:
                name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                out.append((name, int(r["Calls"]), round(float(r["AverageNs"]) / 1e3, 2), round(float(r["MinNs"]) / 1e3, 2), round(float(r["MaxNs"]) / 1e3, 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", action="store_true", help="write profiles/NOTES_uncertainty.md")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["128x128x128", "240x240x155"])
    ap.add_argument("--inputs", nargs="+", default=["smooth", "speckle", "empty"], choices=["smooth", "speckle", "empty"])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-score", action="store_true")
    ap.add_argument("--no-votes", action="store_true", help="time the call without the vote maps only (a profiled run: one form of the table pass)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats CSV of a separate run of this tool")
    ap.add_argument("--kernel-stats-what", default="240 x 240 x 155, smooth, without votes", help="what that run timed")
    args = ap.parse_args()
    if args.notes and args.no_votes:
        sys.exit("--notes reports both forms of the call: not with --no-votes")
    if not torch.cuda.is_available():
        sys.exit("bench_uncertainty needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    copy_gbs, t_copy = copy_rate(dev, args.warmup, args.repeats)
    rows = []
    for s in args.shapes:
        shape = tuple(int(v) for v in s.split("x"))
        rows_h, ref_h = blobs(shape, SAMPLES + 1)
        for name in args.inputs:
            rows.append(one_input(name, dict(smooth=lambda: rows_h, speckle=lambda: speckle(rows_h), empty=lambda: np.zeros_like(rows_h))[name](), np.zeros_like(ref_h) if name == "empty" else ref_h, shape, args, dev, copy_gbs))
    kernels = kernel_rows(args.kernel_stats) if args.kernel_stats else []
    res = dict(bench="uncertainty", calls=rows, copy_gbs=round(copy_gbs, 1), copy_ms=t_copy, kernels=kernels, repeats=args.repeats, warmup=args.warmup,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    if args.notes:
        f = lambda t: f"{t['median']} ({t['min']} - {t['max']})"
        vol = lambda r: " x ".join(map(str, r["shape"]))
        lines = ["# Sample uncertainty of label volumes on the device", "",
                 f"`tools/bench_uncertainty.py --notes` on {res['device']}: S = {SAMPLES} sampled label volumes, a decision volume and a reference, R = {len(REGIONS)} nested regions (WT / TC / ET),",
                 "the smooth-blob volumes of `tools/bench_volscore.py` (row 16 is the decision) and the same volumes with 1 % of the voxels flipped to a random label (speckle), and all-background samples, decision and reference (empty: nothing goes through the LDS tables); every",
                 f"device time is the median of {args.repeats} calls between two device events after {args.warmup} warm-up calls (min and max beside it).  A call is `metrics.score_uncertainty`: two launches, the table",
                 "pass and the finish.  The bytes are what the pass must move: (S + 2) P read, with the vote maps R P more written; the slices (workspace, below) and the finish's outputs",
                 "are not counted.  The GB/s are those bytes over the WHOLE call's median, the share is that rate over the copy rate of the same run: a device-to-device copy of",
                 f"1 GiB, read + written bytes over its median time, {res['copy_gbs']} GB/s ({f(t_copy)} ms).", "",
                 "| volume | input | call ms | MB | GB/s | of the copy rate | with votes ms | MB | GB/s | of the copy rate | background share | workspace KB | workgroups |",
                 "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {vol(r)} | {r['input']} | {f(r['plain_ms'])} | {r['plain_mb']} | {r['plain_gbs']} | {r['plain_share']} | {f(r['votes_ms'])} | {r['votes_mb']} | {r['votes_gbs']} | "
                         f"{r['votes_share']} | {r['background_share']} | {r['workspace_kb']} | {r['route'][1]} |")
        lines += ["", f"Beside it: `uz_vol_window_finish` of `volwindow.hip` runs at {VOLWINDOW_FINISH_SHARE} of the copy rate (`profiles/NOTES_volwindow.md`, a kernel alone; the figures above are whole calls",
                  "of two launches, so at these sizes the launch gap and the finish count against them)."]
        if kernels:
            lines += ["", f"The two launches' own durations (`rocprofv3 --kernel-trace --stats`, a run of its own: {args.kernel_stats_what}):", "",
                      "| kernel | calls | average us | min us | max us |", "|---|---|---|---|---|"]
            lines += [f"| `{k[0]}` | {k[1]} | {k[2]} | {k[3]} | {k[4]} |" for k in kernels]
        if not args.no_score:
            lines += ["", "Beside `metrics.score_volume(hd95=False)` on the same S + 1 rows against the same reference, in the same process (GB/s over (S + 2) P bytes):", "",
                      "| volume | input | score_uncertainty ms | score_volume ms | GB/s | score_uncertainty / score_volume |", "|---|---|---|---|---|---|"]
            for r in rows:
                lines.append(f"| {vol(r)} | {r['input']} | {r['plain_ms']['median']} | {f(r['score_volume_ms'])} | {r['score_volume_gbs']} | {r['plain_over_score_volume']} |")
        if not args.no_host:
            lines += ["", "Against the same tables from numpy on the host (a 256-entry lookup per region, a sum over the samples, one bincount; one core; the copy of 17 volumes to the host not counted):", "",
                      "| volume | input | host s | device call ms | ratio | table integer for integer equal |", "|---|---|---|---|---|---|"]
            for r in rows:
                lines.append(f"| {vol(r)} | {r['input']} | {r['host_s']} | {r['plain_ms']['median']} | {r['speedup_vs_host']} | {r['host_table_equal']} |")
        lines += ["", "Scores of these inputs (WT / TC / ET): " + "; ".join(f"{vol(r)} {r['input']}: score {r['score']}, ECE {r['ece']}" for r in rows) + ".",
                  "", "A repeated call was bit-equal on every shape and input: " + str(all(r["repeat_bit_equal"] for r in rows)) + "."]
        # where the time goes: the histogram path (a filled input against the empty one of the same shape), the finish and the table pass alone
        lines += ["", "## Where the time goes", ""]
        by = {(tuple(r["shape"]), r["input"]): r for r in rows}
        for (shape, name), r in by.items():
            e = by.get((shape, "empty"))
            if name != "empty" and e is not None:
                d = r["plain_ms"]["median"] - e["plain_ms"]["median"]
                lines.append(f"* {vol(r)}, {name} ({round(1 - r['background_share'], 3)} of the voxels off the background bin of WT): {round(1e3 * d, 1)} us more than the call on background alone "
                             f"({r['plain_ms']['median']} against {e['plain_ms']['median']} ms) - the histogram path: table lookups and LDS atomics, many of them on the few words of an interior.")
        fin = next((k for k in kernels if k[0].startswith("unc_finish_k")), None)
        tab = next((k for k in kernels if k[0].startswith("table_k")), None)
        big = by.get(((240, 240, 155), "smooth"))
        if fin and tab and big:
            b = (SAMPLES + 2) * 240 * 240 * 155
            lines.append(f"* The launches alone ({args.kernel_stats_what}): the table pass {tab[2]} us = {round(b / tab[2] / 1e3, 1)} GB/s = {round(b / tab[2] / 1e3 / copy_gbs, 2)} of the copy rate; "
                         f"the finish {fin[2]} us, a fixed cost (1024 slices of R (S + 1) 4 counters, one workgroup per region); the rest of the call's {big['plain_ms']['median']} ms, "
                         f"{round(1e3 * big['plain_ms']['median'] - tab[2] - fin[2], 1)} us, is the gap between two launches as the events see it.")
        lines += ["* The scalar form is not on this path: both sizes are multiples of 16 and every row is 16-byte aligned (route: wide).",
                  "", "Unmeasured: the table pass's own duration on background alone, on speckle and with votes (the profiled run took one input; those figures above are whole calls); the scalar",
                  "and the 4-byte forms at a large size; S and R other than 16 and 3; the rate of LDS atomics in isolation; real BraTS samples (a few per cent foreground: between the",
                  "empty and the smooth rows); sizes near 2^31 voxel-samples."]
        with open(os.path.join(ROOT, "profiles", "NOTES_uncertainty.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
