#!/usr/bin/env python3
"""Time uz_vol_lesion_scores (csrc/vollesion.hip) and uz_vol_morph (csrc/volmorph.hip) on BraTS-sized label volumes: N = 17 rows (16
samples and the mean label), R = 3 nested regions (WT / TC / ET of the raw BraTS values), at 128^3 and 240 x 240 x 155, on the two
inputs of tools/bench_components.py: smooth blobs, and the same rows with 1 % of the voxels flipped to a random label (speckle).

Per shape and input, in one process:
  score     one metrics.score_lesions call with its defaults (dilation 3, min_ref_voxels 50, 256 lesions, 4 links), AGAINST the two
            26-connectivity labelling sweeps it contains per region - metrics.label_components(connectivity=3) with sizes of the N rows
            and of the one reference volume, timed on their own for each region and summed;
  dilation  one metrics.binary_dilation of WT in the N rows, 3 iterations of the 18-neighbour structure, as GB/s over one byte read and one
            byte written per voxel, AGAINST a device copy of the same rows (one byte read, one written: the rate the design aims at);
  keep      metrics.keep_largest_components(connectivity=3) of the same rows: the clean-up call that precedes the score;
  host      the scipy route on row 0: per region binary_dilation of the reference (18-neighbour, 3 iterations), ndimage.label of the
            dilated mask and of the prediction (26-neighbour), the pairs by np.unique - timed, its lesion and component counts compared
            with the device's, and scaled by N for a loop over the rows (the reference side counted once).
Each device time is the median of `--repeats` calls between two device events after `--warmup` calls.  --notes writes
profiles/NOTES_lesions.md.  Without a GPU the tool exits.
usage: python tools/bench_lesions.py [--notes] [--repeats 10] [--warmup 2] [--shapes 128x128x128 240x240x155] [--no-oracle]"""
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
from bench_components import speckle  # noqa: E402
from bench_volscore import blobs, timed  # noqa: E402

N_ROWS, REGIONS = 17, metrics.BRATS_REGIONS
DILATION, MIN_REF = 3, 50


def host_row(row, ref):
    """the scipy route for one row -> (seconds of the reference side, seconds of the row's side, per region (n_ref, n_pred, pairs))"""
    from scipy import ndimage
    st18, st26 = ndimage.generate_binary_structure(3, 2), np.ones((3, 3, 3), bool)
    t_ref = t_row = 0.0
    out = []
    for reg in REGIONS:
        t0 = time.perf_counter()
        G = np.isin(ref, reg)
        Lg, n_ref = ndimage.label(ndimage.binary_dilation(G, structure=st18, iterations=DILATION), structure=st26)
        gt_vol = np.bincount(Lg[G], minlength=n_ref + 1)
        t1 = time.perf_counter()
        Lp, n_pred = ndimage.label(np.isin(row, reg), structure=st26)
        size = np.bincount(Lp.ravel(), minlength=n_pred + 1)
        both = (Lp > 0) & (Lg > 0)
        pairs = np.unique(Lp[both].astype(np.int64) * (n_ref + 1) + Lg[both]) if both.any() else np.zeros(0, np.int64)
        pred_vol = np.bincount(pairs % (n_ref + 1), weights=size[pairs // (n_ref + 1)], minlength=n_ref + 1)
        t2 = time.perf_counter()
        t_ref += t1 - t0
        t_row += t2 - t1
        out.append((int(n_ref), int(n_pred), int(len(pairs)), int((gt_vol[1:] >= MIN_REF).sum()), int(pred_vol.sum())))
    return t_ref, t_row, out


def one_input(name, pred_h, ref_h, shape, args, dev):
    D, H, W = shape
    P = D * H * W
    pred, ref = torch.from_numpy(pred_h).to(dev), torch.from_numpy(ref_h).to(dev)
    sink = {}

    def score():
        sink["score"] = metrics.score_lesions(pred, ref, REGIONS)
    t_score = timed(score, args.warmup, args.repeats)
    first = [t.clone() for t in (sink["score"].counts, sink["score"].lesion_dice)]
    score()
    bit_equal = bool(torch.equal(first[0], sink["score"].counts)) and bool(torch.equal(first[1].view(torch.int64), sink["score"].lesion_dice.view(torch.int64)))
    t_lab_rows = t_lab_ref = 0.0
    for reg in REGIONS:
        t_lab_rows += timed(lambda: sink.__setitem__("l", metrics.label_components(pred, reg, return_sizes=True, connectivity=3)), args.warmup, args.repeats)["median"]
        t_lab_ref += timed(lambda: sink.__setitem__("l", metrics.label_components(ref[None], reg, return_sizes=True, connectivity=3)), args.warmup, args.repeats)["median"]
    sink.pop("l")
    t_dil = timed(lambda: sink.__setitem__("d", metrics.binary_dilation(pred, REGIONS[0], iterations=3, connectivity=2)), args.warmup, args.repeats)
    dst = torch.empty_like(pred)
    t_copy = timed(lambda: dst.copy_(pred), args.warmup, args.repeats)
    t_keep = timed(lambda: sink.__setitem__("k", metrics.keep_largest_components(pred, REGIONS, connectivity=3)), args.warmup, args.repeats)
    counts = sink["score"].counts.cpu().numpy()
    r2 = (C.c_int * 2)()
    _ffi.lib().uz_vol_lesion_scores_route(N_ROWS, len(REGIONS), D, H, W, r2)
    row = dict(input=name, shape=list(shape), rows=N_ROWS, regions=len(REGIONS), route=list(r2), score_ms=t_score, label_rows_ms=round(t_lab_rows, 3),
               label_ref_ms=round(t_lab_ref, 3), score_over_labelling=round(t_score["median"] / (t_lab_rows + t_lab_ref), 3), dilation_ms=t_dil,
               dilation_gbs=round(2 * N_ROWS * P / t_dil["median"] / 1e6, 1), copy_ms=t_copy, copy_gbs=round(2 * N_ROWS * P / t_copy["median"] / 1e6, 1),
               dilation_over_copy=round(t_dil["median"] / t_copy["median"], 2), keep_c3_ms=t_keep, repeat_bit_equal=bit_equal,
               counts_row0=counts[0].tolist(), overflow_any=bool(counts[..., 6:].any()), lesion_dice_row0=[round(float(v), 4) for v in sink["score"].lesion_dice[0].cpu()],
               workspace_mb=round(_ffi.lib().uz_vol_lesion_scores_workspace(N_ROWS, len(REGIONS), D, H, W, 256) / 1e6, 1),
               morph_workspace_mb=round(_ffi.lib().uz_vol_morph_workspace(N_ROWS, D, H, W) / 1e6, 1))
    if not args.no_oracle:
        t_ref, t_row, host = host_row(pred_h[0], ref_h)
        row.update(host_ref_side_s=round(t_ref, 2), host_row0_s=round(t_row, 2), host_all_rows_s=round(t_ref + t_row * N_ROWS, 1),
                   host_counts_row0=[list(h) for h in host],
                   row0_counts_equal=all(int(counts[0, r, 0]) == h[0] and int(counts[0, r, 5]) == h[1] and int(counts[0, r, 1]) == h[3] for r, h in enumerate(host)),
                   speedup_vs_host=round((t_ref + t_row * N_ROWS) * 1e3 / t_score["median"], 1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", action="store_true", help="write profiles/NOTES_lesions.md")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=["128x128x128", "240x240x155"])
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lesions needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    rows = []
    for s in args.shapes:
        shape = tuple(int(v) for v in s.split("x"))
        pred_h, ref_h = blobs(shape, N_ROWS)
        rows.append(one_input("smooth", pred_h, ref_h, shape, args, dev))
        print(json.dumps(rows[-1]), flush=True)
        rows.append(one_input("speckle", speckle(pred_h), ref_h, shape, args, dev))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="lesions", calls=rows, repeats=args.repeats, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    if args.notes:
        f = lambda t: f"{t['median']} ({t['min']} - {t['max']})"
        vol = lambda r: " x ".join(map(str, r["shape"]))
        lines = ["# Lesion-wise scores and binary morphology on the device", "",
                 f"`tools/bench_lesions.py --notes` on {res['device']}: N = {N_ROWS} label volumes, R = {len(REGIONS)} nested regions (WT / TC / ET), the smooth-blob volumes of",
                 "`tools/bench_volscore.py` and the same rows with 1 % of the voxels flipped to a random label (speckle); every device time is the median of",
                 f"{args.repeats} calls between two device events after {args.warmup} warm-up calls (min and max beside it), all in one process.  There is no gate on these times.", "",
                 "`score` is one `metrics.score_lesions` call with its defaults (dilation 3, min_ref_voxels 50, 256 lesions, 4 links).  Per region it contains one",
                 "26-connectivity labelling of the N rows and one of the dilated reference; `labelling` is `metrics.label_components(connectivity=3)` with sizes of the N rows",
                 "plus of the one reference volume, timed on their own for each of the three regions and summed - the share of the call that is the two sweeps.", "",
                 "| volume | input | score ms | labelling of the rows ms | of the reference ms | score / labelling | lesions, kept, components of WT in row 0 | table overflow | workspace MB | widest launch |",
                 "|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            c = r["counts_row0"][0]
            lines.append(f"| {vol(r)} | {r['input']} | {f(r['score_ms'])} | {r['label_rows_ms']} | {r['label_ref_ms']} | {r['score_over_labelling']} | {c[0]}, {c[1]}, {c[5]} | "
                         f"{r['overflow_any']} | {r['workspace_mb']} | {r['route'][1]} |")
        lines += ["", "`dilation` is one `metrics.binary_dilation` of WT in the N rows, 3 iterations of the 18-neighbour structure (five launches: pack, three passes on bit planes,",
                  "unpack); its GB/s count one byte read and one byte written per voxel, and `copy` is `Tensor.copy_` of the same rows - the same two bytes per voxel.", "",
                  "| volume | input | dilation ms | dilation GB/s | copy ms | copy GB/s | dilation / copy | packed planes MB | keep_largest_components(connectivity=3) ms |", "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {vol(r)} | {r['input']} | {f(r['dilation_ms'])} | {r['dilation_gbs']} | {f(r['copy_ms'])} | {r['copy_gbs']} | {r['dilation_over_copy']} | "
                         f"{r['morph_workspace_mb']} | {f(r['keep_c3_ms'])} |")
        if not args.no_oracle:
            lines += ["", "Against the scipy route on the host (per region `binary_dilation` and `label` of the reference once, `label` of the row and the pairs by `np.unique`,",
                      "timed on row 0 and scaled by N for a loop over the rows; one core).  The lesion, kept-lesion and component counts of row 0 are compared with the device's:", "",
                      "| volume | input | host, reference side, s | host, one row, s | host, all rows, s | device call, ms | ratio | row 0 counts equal |", "|---|---|---|---|---|---|---|---|"]
            for r in rows:
                lines.append(f"| {vol(r)} | {r['input']} | {r['host_ref_side_s']} | {r['host_row0_s']} | {r['host_all_rows_s']} | {r['score_ms']['median']} | {r['speedup_vs_host']} | "
                             f"{r['row0_counts_equal']} |")
        lines += ["", "A repeated score call was bit-equal on every shape and input: " + str(all(r["repeat_bit_equal"] for r in rows)) + "."]
        with open(os.path.join(ROOT, "profiles", "NOTES_lesions.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
