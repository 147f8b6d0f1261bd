#!/usr/bin/env python3
"""Time uz_vol_keep_components and uz_vol_label_components (csrc/volcomp.hip) on BraTS-sized label volumes: N = 17 rows (16 samples and
the mean label), R = 3 nested regions (WT / TC / ET of the raw BraTS values), at 128^3 and 240 x 240 x 155, on two inputs: the
smooth-blob volumes of tools/bench_volscore.py, and the same volumes with 1 % of the voxels flipped to a random label - speckle is what
real samples have and what stresses the unions.

Per shape and input: the keep call (metrics.keep_largest_components) and one labelling alone (metrics.label_components of WT with
sizes), each with the bytes the built design must move per voxel as GB/s - keep, per set: runs 1 read + 4 written, merge 1, flatten 1,
select 4, apply 1 read + 1 written (the first set; later sets write only what they remove) = 13 bytes per voxel and set, the gathers at
foreground voxels and run heads not counted; labelling: runs 5, merge 1, flatten 1, the label pass 1 + 4 + 4 = 16 - and AGAINST them the
same work on the host: scipy.ndimage.label and a bincount per region on row 0, timed, the filtered row compared with the device's byte for
byte, and scaled by N.  BESIDE them metrics.score_volume with HD95 on the same rows in the same process: the call this one precedes.
--connectivity 1 2 3 times the keep call at each of them (2 and 3 go through uz_vol_keep_components_ex) beside scipy.ndimage.label with
the matching structure on row 0; --fill times metrics.fill_holes on the same regions (per set: runs 1 + 4, merge 1, flatten 1, border 1,
fill 1 read + 1 written on the first set = 10 bytes per voxel and set) beside scipy.ndimage.binary_fill_holes per region on row 0, the
filled row compared byte for byte.
Each device time is the median of `--repeats` calls between two device events after `--warmup` calls.  --notes writes
profiles/NOTES_components.md.  Without a GPU the tool exits.
usage: python tools/bench_components.py [--notes] [--repeats 10] [--warmup 2] [--shapes 128x128x128 240x240x155] [--connectivity 1 2 3] [--fill]
                                        [--no-oracle] [--no-score]"""
import argparse
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

N_ROWS, REGIONS = 17, metrics.BRATS_REGIONS
KEEP_BYTES_PER_VOXEL_AND_SET, LABEL_BYTES_PER_VOXEL, FILL_BYTES_PER_VOXEL_AND_SET = 13, 16, 10


def speckle(pred, share=0.01, seed=2):
    rs = np.random.RandomState(seed)
    out = pred.copy()
    flip = rs.random_sample(pred.shape) < share
    out[flip] = np.array([0, 1, 2, 4], np.uint8)[rs.randint(0, 4, int(flip.sum()))]
    return out


def host_keep(row, regions, connectivity=1):
    """the reference's method on one volume: scipy.ndimage.label per region, the largest blob kept (the first among equals), nested regions
    combined by the rule of uz_api.h -> (filtered row, components per region)"""
    from scipy import ndimage
    fails, listed, ncomp = np.zeros(row.shape, bool), np.zeros(row.shape, bool), []
    for reg in regions:
        fg = np.isin(row, reg)
        lab, n = ndimage.label(fg, structure=ndimage.generate_binary_structure(3, connectivity))
        ncomp.append(int(n))
        listed |= fg
        if n:
            fails |= fg & (lab != int(np.argmax(np.bincount(lab.ravel())[1:])) + 1)
    return np.where(listed & ~fails, row, 0).astype(np.uint8), ncomp


def host_fill(row, regions):
    """scipy.ndimage.binary_fill_holes per region on one volume, every region on the input, a later region over an earlier one"""
    from scipy import ndimage
    out = row.copy()
    for reg in regions:
        fg = np.isin(row, reg)
        out[ndimage.binary_fill_holes(fg) & ~fg] = reg[0]
    return out


def one_input(name, pred_h, ref_h, shape, args, dev):
    D, H, W = shape
    P = D * H * W
    pred, ref = torch.from_numpy(pred_h).to(dev), torch.from_numpy(ref_h).to(dev)
    route = (C.c_int * 2)()
    _ffi.lib().uz_vol_components_route(N_ROWS, D, H, W, route)
    sink = {}

    def keep():
        sink["keep"] = metrics.keep_largest_components(pred, REGIONS)

    def label():
        sink["label"] = metrics.label_components(pred, REGIONS[0], return_sizes=True)
    t_keep = timed(keep, args.warmup, args.repeats)
    first = sink["keep"].clone()
    keep()
    bit_equal = bool(torch.equal(first, sink["keep"]))
    t_label = timed(label, args.warmup, args.repeats)
    lab, sz = sink["label"]
    roots = lab.view(N_ROWS, -1) == torch.arange(1, P + 1, device=dev, dtype=torch.int32)[None]
    row = dict(input=name, shape=list(shape), rows=N_ROWS, regions=len(REGIONS), route=list(route), keep_ms=t_keep, label_ms=t_label,
               keep_gbs=round(KEEP_BYTES_PER_VOXEL_AND_SET * len(REGIONS) * N_ROWS * P / t_keep["median"] / 1e6, 1),
               label_gbs=round(LABEL_BYTES_PER_VOXEL * N_ROWS * P / t_label["median"] / 1e6, 1), repeat_bit_equal=bit_equal,
               wt_components_row0=int(roots[0].sum()), wt_components_all=int(roots.sum()), wt_largest_row0=int(sz[0].max()),
               wt_share=round(float((lab != 0).float().mean()), 4), workspace_mb=round(_ffi.lib().uz_vol_components_workspace(N_ROWS, D, H, W) / 1e6, 1))
    if not args.no_oracle:
        t0 = time.perf_counter()
        want, ncomp = host_keep(pred_h[0], REGIONS)
        dt = time.perf_counter() - t0
        row.update(host_row0_s=round(dt, 3), host_all_rows_s=round(dt * N_ROWS, 2), host_components_row0=ncomp,
                   row0_equal=bool(np.array_equal(want, sink["keep"][0].cpu().numpy())), speedup_vs_host=round(dt * N_ROWS * 1e3 / t_keep["median"], 1))
    for c in args.connectivity:
        if c == 1:
            continue
        def keep_c():
            sink["keep_c"] = metrics.keep_largest_components(pred, REGIONS, connectivity=c)
        t = timed(keep_c, args.warmup, args.repeats)
        ex = dict(keep_ms=t, over_c1=round(t["median"] / t_keep["median"], 3))
        if not args.no_oracle:
            t0 = time.perf_counter()
            want, ncomp = host_keep(pred_h[0], REGIONS, c)
            dt = time.perf_counter() - t0
            ex.update(host_row0_s=round(dt, 3), host_all_rows_s=round(dt * N_ROWS, 2), host_components_row0=ncomp,
                      row0_equal=bool(np.array_equal(want, sink["keep_c"][0].cpu().numpy())))
        row[f"connectivity_{c}"] = ex
    if args.fill:
        def fill():
            sink["fill"] = metrics.fill_holes(pred, REGIONS)
        t = timed(fill, args.warmup, args.repeats)
        first = sink["fill"].clone()
        fill()
        ex = dict(fill_ms=t, fill_gbs=round(FILL_BYTES_PER_VOXEL_AND_SET * len(REGIONS) * N_ROWS * P / t["median"] / 1e6, 1), over_keep=round(t["median"] / t_keep["median"], 3),
                  voxels_filled_all=int((sink["fill"] != pred).sum()), repeat_bit_equal=bool(torch.equal(first, sink["fill"])))
        if not args.no_oracle:
            t0 = time.perf_counter()
            want = host_fill(pred_h[0], REGIONS)
            dt = time.perf_counter() - t0
            ex.update(host_row0_s=round(dt, 3), host_all_rows_s=round(dt * N_ROWS, 2), row0_equal=bool(np.array_equal(want, sink["fill"][0].cpu().numpy())),
                      voxels_filled_row0=int((want != pred_h[0]).sum()))
        row["fill"] = ex
    if not args.no_score:
        def score():
            sink["score"] = metrics.score_volume(sink["keep"], ref, REGIONS)
        row["score_volume_ms"] = timed(score, args.warmup, args.repeats)
        row["keep_over_score"] = round(t_keep["median"] / row["score_volume_ms"]["median"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", action="store_true", help="write profiles/NOTES_components.md")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=["128x128x128", "240x240x155"])
    ap.add_argument("--connectivity", nargs="+", type=int, default=[1], choices=[1, 2, 3], help="also time the keep call at these connectivities")
    ap.add_argument("--fill", action="store_true", help="also time metrics.fill_holes")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--no-score", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_components needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    rows = []
    for s in args.shapes:
        shape = tuple(int(v) for v in s.split("x"))
        pred_h, ref_h = blobs(shape, N_ROWS)
        rows.append(one_input("smooth", pred_h, ref_h, shape, args, dev))
        rows.append(one_input("speckle", speckle(pred_h), ref_h, shape, args, dev))
    res = dict(bench="components", calls=rows, repeats=args.repeats, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    if args.notes:
        f = lambda t: f"{t['median']} ({t['min']} - {t['max']})"
        vol = lambda r: " x ".join(map(str, r["shape"]))
        lines = ["# Connected components of label volumes on the device", "",
                 f"`tools/bench_components.py --notes` on {res['device']}: N = {N_ROWS} label volumes, R = {len(REGIONS)} nested regions (WT / TC / ET), the smooth-blob volumes of",
                 "`tools/bench_volscore.py` and the same volumes with 1 % of the voxels flipped to a random label (speckle); every device time is the median of",
                 f"{args.repeats} calls between two device events after {args.warmup} warm-up calls (min and max beside it).  `keep` is `metrics.keep_largest_components` (three sets, five launches each),",
                 "`label` one `metrics.label_components` of WT with sizes (four launches).  The GB/s are the bytes the built design must move - keep 13 per voxel and set",
                 "(runs 1 + 4, merge 1, flatten 1, select 4, apply 1 + 1), label 16 per voxel (runs 5, merge 1, flatten 1, label pass 1 + 4 + 4), gathers at foreground voxels",
                 "and run heads not counted - over the median: a rate of the whole call.", "",
                 "| volume | input | keep ms | keep GB/s | label ms | label GB/s | WT components, row 0 / all rows | largest WT, row 0 | WT share | workspace MB | widest launch |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {vol(r)} | {r['input']} | {f(r['keep_ms'])} | {r['keep_gbs']} | {f(r['label_ms'])} | {r['label_gbs']} | {r['wt_components_row0']} / {r['wt_components_all']} | "
                         f"{r['wt_largest_row0']} | {r['wt_share']} | {r['workspace_mb']} | {r['route'][1]} |")
        if not args.no_oracle:
            lines += ["", "Against the same work on the host (`scipy.ndimage.label` and a bincount per region on row 0, timed, times N for a loop over the rows; one core):", "",
                      "| volume | input | host, 3 regions of one row, s | host, all rows (x N), s | device call, ms | ratio | row 0 byte for byte equal |", "|---|---|---|---|---|---|---|"]
            for r in rows:
                lines.append(f"| {vol(r)} | {r['input']} | {r['host_row0_s']} | {r['host_all_rows_s']} | {r['keep_ms']['median']} | {r['speedup_vs_host']} | {r['row0_equal']} |")
        if not args.no_score:
            lines += ["", "Beside `metrics.score_volume` with HD95 of the filtered rows against the reference volume, in the same process (the call this one precedes):", "",
                      "| volume | input | keep ms | score_volume ms | keep / score_volume |", "|---|---|---|---|---|"]
            for r in rows:
                lines.append(f"| {vol(r)} | {r['input']} | {r['keep_ms']['median']} | {f(r['score_volume_ms'])} | {r['keep_over_score']} |")
        if any(c != 1 for c in args.connectivity):
            lines += ["", "The keep call at 18- and 26-connectivity (`connectivity=2`, `3`: `uz_vol_keep_components_ex`, the same launches with the wider merge kernel), and",
                      "`scipy.ndimage.label` with the matching structure on row 0:", "",
                      "| volume | input | connectivity | keep ms | over connectivity 1 | components of the 3 regions, row 0 | host, one row, s | host, all rows (x N), s | row 0 byte for byte equal |",
                      "|---|---|---|---|---|---|---|---|---|"]
            for r in rows:
                for c in args.connectivity:
                    e = r.get(f"connectivity_{c}")
                    if e:
                        lines.append(f"| {vol(r)} | {r['input']} | {c} | {f(e['keep_ms'])} | {e['over_c1']} | {e.get('host_components_row0', '-')} | {e.get('host_row0_s', '-')} | "
                                     f"{e.get('host_all_rows_s', '-')} | {e.get('row0_equal', '-')} |")
        if args.fill:
            lines += ["", "`metrics.fill_holes` of the same three regions (background connectivity 1; per set runs, merge, flatten, border, fill: 10 bytes per voxel and set), and",
                      "`scipy.ndimage.binary_fill_holes` per region on row 0:", "",
                      "| volume | input | fill ms | fill GB/s | fill / keep | voxels filled, all rows | host, one row, s | host, all rows (x N), s | row 0 byte for byte equal |", "|---|---|---|---|---|---|---|---|---|"]
            for r in rows:
                e = r["fill"]
                lines.append(f"| {vol(r)} | {r['input']} | {f(e['fill_ms'])} | {e['fill_gbs']} | {e['over_keep']} | {e['voxels_filled_all']} | {e.get('host_row0_s', '-')} | "
                             f"{e.get('host_all_rows_s', '-')} | {e.get('row0_equal', '-')} |")
        lines += ["", "A repeated call was bit-equal on every shape and input: " + str(all(r["repeat_bit_equal"] and r.get("fill", r)["repeat_bit_equal"] for r in rows)) + "."]
        with open(os.path.join(ROOT, "profiles", "NOTES_components.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
