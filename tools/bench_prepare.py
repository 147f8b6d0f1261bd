#!/usr/bin/env python3
"""Time data.prepare_case (uz_vol_prepare) and data.restore_volume (uz_vol_restore, csrc/volprep.hip) on a BraTS-sized case: a synthetic
240 x 240 x 155 x 4 head (an ellipsoid of integer intensities with holes, zero outside; its box is about 150 x 180 x 140) into
(160, 192, 160) - the box is padded - and into 128^3 - the box is cropped -, centred, with the mask.  Restore: N = 17 uint8 rows (16
samples and the mean label) of target extent back into 240 x 240 x 155 with the BraTS lut, and one fp32 row (the entropy).

Per call: the median of `--repeats` calls between two device events after `--warmup` calls, the bytes the call must move - prepare:
one read of raw for the bounds, two reads of the placed block for the statistics, one read of the block and one write of the target for
the store, plus the mask; restore: the placed block read, the native volumes written - as GB/s of the WHOLE call and as a share of
the copy rate measured in the same run (a device-to-device copy of 1 GiB, read + written bytes over its median time).  AGAINST it the
restated reference functions of tests/_volprep.py in numpy on the host, timed once, and the device's image compared with theirs.
--kernel-stats FILE reads a rocprofv3 --kernel-trace --stats CSV of a run of this tool (taken in a run of its own, one shape) and puts
every launch's own duration into the notes.  --notes writes profiles/NOTES_prepare.md.  Without a GPU the tool exits.
usage: python tools/bench_prepare.py [--notes] [--repeats 20] [--warmup 3] [--sizes 160x192x160 128x128x128] [--no-host] [--no-restore] [--kernel-stats FILE]"""
import argparse
import csv
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
from unet_zoo_amd import data, metrics  # noqa: E402
from bench_volscore import timed  # noqa: E402
from bench_uncertainty import copy_rate  # noqa: E402

NATIVE, CH, ROWS = (240, 240, 155), 4, 17


def head(seed=1):
    """raw (240, 240, 155, 4) fp32 of integer intensities and mask (240, 240, 155) uint8"""
    rs = np.random.RandomState(seed)
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in NATIVE), indexing="ij")
    inside = ((x - 121) / 75) ** 2 + ((y - 118) / 90) ** 2 + ((z - 76) / 70) ** 2 <= 1
    raw = rs.randint(1, 1200, size=NATIVE + (CH,)).astype(np.float32)
    raw[rs.random_sample(raw.shape) < 0.05] = 0                             # holes
    raw[~inside] = 0
    mask = np.zeros(NATIVE, np.uint8)
    core = ((x - 140) / 20) ** 2 + ((y - 100) / 25) ** 2 + ((z - 80) / 18) ** 2
    mask[core <= 1] = 2
    mask[core <= 0.5] = 1
    mask[core <= 0.2] = 4
    return raw, mask


def one_size(size, raw_h, mask_h, raw, mask, args, dev, copy_gbs):
    from tests import _volprep as V
    Xt, Yt, Zt = size
    img = torch.empty(Xt, Yt, Zt, CH, device=dev)
    msk = torch.empty(Xt, Yt, Zt, dtype=torch.uint8, device=dev)
    sink = {}

    def call():
        sink["case"] = data.prepare_case(raw, mask, size=size, placement="centre", out=(img, msk))
    t = timed(call, args.warmup, args.repeats)
    first = [v.clone() for v in sink["case"]]
    call()
    bit_equal = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first, sink["case"]))
    info = sink["case"].info.cpu().tolist()
    P, Pt, Pb = int(np.prod(NATIVE)), Xt * Yt * Zt, info[12] * info[13] * info[14]
    floor = P * CH * 4 + 2 * Pb * CH * 4 + (Pb + Pt) * CH * 4 + Pb + Pt
    row = dict(size=list(size), box=info[0:6], extent=info[12:15], flags=info[15], call_ms=t, floor_mb=round(floor / 1e6, 1),
               gbs=round(floor / t["median"] / 1e6, 1), share=round(floor / t["median"] / 1e6 / copy_gbs, 3), floor_ms_at_copy_rate=round(floor / copy_gbs / 1e6, 3),
               repeat_bit_equal=bit_equal, stats=[[round(float(v), 6) for v in r] for r in sink["case"].stats.cpu()])
    if not args.no_host:
        t0 = time.perf_counter()
        want, want_mask, off = V.ref_pipeline(raw_h, mask_h, size, 0)
        dt = time.perf_counter() - t0
        got = img.cpu().numpy()
        row.update(host_s=round(dt, 3), speedup_vs_host=round(dt * 1e3 / t["median"], 1), image_bit_equal=bool(got.tobytes() == want.tobytes()),
                   image_max_abs_diff=float(np.abs(got - want).max()), mask_equal=bool(np.array_equal(msk.cpu().numpy(), want_mask)), offsets=off)
    if not args.no_restore:
        rows = torch.randint(0, 4, (ROWS, Xt, Yt, Zt), dtype=torch.uint8, device=dev)
        ent = torch.rand(1, Xt, Yt, Zt, device=dev)
        place = sink["case"].place.clone()
        tr = timed(lambda: sink.__setitem__("lab", data.restore_volume(rows, place, native_shape=NATIVE, lut=metrics.BRATS_LABELS)), args.warmup, args.repeats)
        te = timed(lambda: sink.__setitem__("ent", data.restore_volume(ent, place, native_shape=NATIVE)), args.warmup, args.repeats)
        br, be = ROWS * (Pb + P), 4 * (Pb + P)
        row.update(restore_ms=tr, restore_mb=round(br / 1e6, 1), restore_gbs=round(br / tr["median"] / 1e6, 1), restore_share=round(br / tr["median"] / 1e6 / copy_gbs, 3),
                   restore_f32_ms=te, restore_f32_mb=round(be / 1e6, 1), restore_f32_gbs=round(be / te["median"] / 1e6, 1),
                   restore_f32_share=round(be / te["median"] / 1e6 / copy_gbs, 3))
        if not args.no_host:
            rows_h, pl = rows.cpu().numpy(), place.cpu().numpy()
            t0 = time.perf_counter()
            want = V.restore(rows_h, pl, NATIVE, lut=metrics.BRATS_LABELS, fill=0)
            row.update(restore_host_s=round(time.perf_counter() - t0, 3), restore_equal=bool(np.array_equal(sink["lab"].cpu().numpy(), want)))
    return row


def kernel_rows(path):
    """this file's launches out of a rocprofv3 --stats CSV: [(name, calls, average us, min us, max us)]"""
    out = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            if "prep_" in r["Name"] or "restore_k" in r["Name"]:
                name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                out.append((name, int(r["Calls"]), round(float(r["AverageNs"]) / 1e3, 2), round(float(r["MinNs"]) / 1e3, 2), round(float(r["MaxNs"]) / 1e3, 2)))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", action="store_true", help="write profiles/NOTES_prepare.md")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", nargs="+", default=["160x192x160", "128x128x128"])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-restore", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats CSV of a separate run of this tool")
    ap.add_argument("--kernel-stats-what", default="into 160 x 192 x 160, with the restores", help="what that run timed")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_prepare needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    copy_gbs, t_copy = copy_rate(dev, args.warmup, args.repeats)
    raw_h, mask_h = head()
    t0 = time.perf_counter()
    raw, mask = torch.from_numpy(raw_h).to(dev), torch.from_numpy(mask_h).to(dev)
    torch.cuda.synchronize()
    upload_ms = round(1e3 * (time.perf_counter() - t0), 1)
    rows = [one_size(tuple(int(v) for v in s.split("x")), raw_h, mask_h, raw, mask, args, dev, copy_gbs) for s in args.sizes]
    kernels = kernel_rows(args.kernel_stats) if args.kernel_stats else []
    res = dict(bench="prepare", calls=rows, copy_gbs=round(copy_gbs, 1), copy_ms=t_copy, upload_ms=upload_ms, kernels=kernels, repeats=args.repeats, warmup=args.warmup,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    if args.notes:
        f = lambda t: f"{t['median']} ({t['min']} - {t['max']})"
        ext = lambda v: " x ".join(map(str, v))
        lines = ["# Raw BraTS cases onto the fixed extent, and maps back into native space", "",
                 f"`tools/bench_prepare.py --notes` on {res['device']}: a synthetic 240 x 240 x 155 x 4 head (an ellipsoid of integer intensities with 5 % holes, zero outside) with its mask,",
                 f"already on the device (the upload of the 143 MB case from pageable host memory took {upload_ms} ms once and is not in the figures).  Every device time is the median of",
                 f"{args.repeats} calls between two device events after {args.warmup} warm-up calls (min and max beside it).  A call is `data.prepare_case(..., out=...)`: seven launches.  The floor is",
                 "what the call must move: one read of raw for the bounds, two reads of the placed block for the statistics, one read of the block and one write of the target for the",
                 "store, the mask read and written.  The GB/s are those bytes over the WHOLE call's median, the share is that rate over the copy rate of the same run: a device-to-device",
                 f"copy of 1 GiB, read + written bytes over its median time, {res['copy_gbs']} GB/s ({f(t_copy)} ms).", "",
                 "| target | box | placed block | flags | call ms | floor MB | GB/s | of the copy rate | floor at the copy rate ms |", "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            b = r["box"]
            lines.append(f"| {ext(r['size'])} | {b[0]}:{b[3]}, {b[1]}:{b[4]}, {b[2]}:{b[5]} | {ext(r['extent'])} | {r['flags']} | {f(r['call_ms'])} | {r['floor_mb']} | {r['gbs']} | {r['share']} | "
                         f"{r['floor_ms_at_copy_rate']} |")
        if kernels:
            lines += ["", f"Every launch's own duration (`rocprofv3 --kernel-trace --stats`, a run of its own: {args.kernel_stats_what}):", "",
                      "| kernel | calls | average us | min us | max us |", "|---|---|---|---|---|"]
            lines += [f"| `{k[0]}` | {k[1]} | {k[2]} | {k[3]} | {k[4]} |" for k in kernels]
        if not args.no_host:
            lines += ["", "Against the restated reference functions in numpy on the host (`tests/_volprep.py`: argwhere crop, placement, fp64 nanmean / nanstd, fp32 store; one core):", "",
                      "| target | host s | device call ms | ratio | image bit for bit equal | max abs difference | mask equal | offsets |", "|---|---|---|---|---|---|---|---|"]
            for r in rows:
                lines.append(f"| {ext(r['size'])} | {r['host_s']} | {r['call_ms']['median']} | {r['speedup_vs_host']} | {r['image_bit_equal']} | {r['image_max_abs_diff']} | {r['mask_equal']} | {r['offsets']} |")
        if not args.no_restore:
            lines += ["", f"Restore (`data.restore_volume`, one launch): N = {ROWS} uint8 rows of target extent with the BraTS lut into {ROWS} x 240 x 240 x 155, and one fp32 row; bytes = the placed block",
                      "read + the native volumes written.", "",
                      "| target | uint8 x 17 ms | MB | GB/s | of the copy rate | fp32 x 1 ms | MB | GB/s | of the copy rate |" + (" numpy on the host s | equal |" if not args.no_host else ""),
                      "|---|---|---|---|---|---|---|---|---|" + ("---|---|" if not args.no_host else "")]
            for r in rows:
                lines.append(f"| {ext(r['size'])} | {f(r['restore_ms'])} | {r['restore_mb']} | {r['restore_gbs']} | {r['restore_share']} | {f(r['restore_f32_ms'])} | {r['restore_f32_mb']} | "
                             f"{r['restore_f32_gbs']} | {r['restore_f32_share']} |" + (f" {r['restore_host_s']} | {r['restore_equal']} |" if not args.no_host else ""))
        lines += ["", "A repeated call was bit-equal on every size: " + str(all(r["repeat_bit_equal"] for r in rows)) + ".",
                  "", "Unmeasured: the scalar form (C other than 4, or pointers off 16 bytes) at a large size; corner placement at this size; real BraTS cases (their box and their share of",
                  "zeros differ from the ellipsoid's); the upload from pinned memory; sizes near 2^31 elements."]
        with open(os.path.join(ROOT, "profiles", "NOTES_prepare.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
