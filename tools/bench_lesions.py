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
  --hd95    adds the lesion-wise HD95: score_lesions(hd95=True) beside the plain call, the pair kernel and the select on their own (the sums of
            their launches in one profiled call, torch.profiler), the border voxels and (border voxel, lesion) entries of row 0, the grown
            workspace, and as the host route _volscore.hd95 per matched lesion on row 0, both masks cropped to their common box, scaled by N.
Each device time is the median of `--repeats` calls between two device events after `--warmup` calls.  --notes writes
profiles/NOTES_lesions.md.  Without a GPU the tool exits.
usage: python tools/bench_lesions.py [--notes] [--hd95] [--repeats 10] [--warmup 2] [--shapes 128x128x128 240x240x155] [--no-oracle]"""
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


def host_hd95_row(row, ref):
    """the scipy route of the lesion-wise HD95 for one row -> (seconds, per region [hd95_g of the matched lesions], reference border voxels, entries)"""
    from scipy import ndimage
    from tests import _volscore as V
    st18, st26 = ndimage.generate_binary_structure(3, 2), np.ones((3, 3, 3), bool)
    t0 = time.perf_counter()
    out, n_border, n_entries = [], 0, 0
    for reg in REGIONS:
        G = np.isin(ref, reg)
        Dk = ndimage.binary_dilation(G, structure=st18, iterations=DILATION)
        Lg, n_ref = ndimage.label(Dk, structure=st26)
        Lp, _ = ndimage.label(np.isin(row, reg), structure=st26)
        vals, boxes_p = [], ndimage.find_objects(Lp)
        for g, box in enumerate(ndimage.find_objects(Lg)):
            ids = np.unique(Lp[box][Lg[box] == g + 1])
            ids = ids[ids > 0]
            if not len(ids):
                continue
            lo, hi = [b.start for b in box], [b.stop for b in box]
            for b in (boxes_p[i - 1] for i in ids):
                lo, hi = [min(a, c.start) for a, c in zip(lo, b)], [max(a, c.stop) for a, c in zip(hi, b)]
            # one voxel of margin, so that only the volume's own faces are faces of the crop
            crop = tuple(slice(max(a - 1, 0), min(c + 1, n)) for a, c, n in zip(lo, hi, row.shape))
            A, B = (G[crop] & (Lg[crop] == g + 1)), np.isin(Lp[crop], ids)
            pad = [(int(c.start > 0), int(c.stop < n)) for c, n in zip(crop, row.shape)]         # faces inside the volume are no border
            inner = tuple(slice(a, s - b) for (a, b), s in zip(pad, A.shape))
            bA, bB = np.zeros(A.shape, bool), np.zeros(B.shape, bool)
            bA[inner], bB[inner] = V.border(A)[inner], V.border(B)[inner]
            n_border += int(bA.sum()); n_entries += int(bB.sum())
            d = np.hstack([ndimage.distance_transform_edt(~bA)[bB], ndimage.distance_transform_edt(~bB)[bA]])
            vals.append(float(np.percentile(d, 95)))
        out.append(vals)
    return time.perf_counter() - t0, out, n_border, n_entries


def kernel_ms(fn, names):
    """device time of the kernels whose name contains one of `names`, summed over one call of fn; None where the profiler gives nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        tot = {k: 0.0 for k in names}
        for ev in prof.key_averages():
            for k in names:
                if k in ev.key:
                    tot[k] += getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
        return {k: round(v / 1e3, 3) for k, v in tot.items()} if any(tot.values()) else None
    except Exception as e:                                               # the numbers are optional, the run is not
        print("profiler:", repr(e), file=sys.stderr)
        return None


def hd95_part(pred, ref, pred_h, ref_h, shape, args):
    D, H, W = shape
    sink = {}

    def score():
        sink["s"] = metrics.score_lesions(pred, ref, REGIONS, hd95=True)
    t = timed(score, args.warmup, args.repeats)
    first = sink["s"].hd95.clone()
    score()
    mb = min(max(4096, D * H * W // 8), D * H * W)
    out = dict(hd95_score_ms=t, hd95_row0=[round(float(v), 4) for v in sink["s"].hd95[0].cpu()], hd95_overflow_any=bool(sink["s"].hd_counts.any()),
               hd95_nan_any=bool(torch.isnan(sink["s"].hd95).any()), hd95_repeat_bit_equal=bool(torch.equal(first.view(torch.int64), sink["s"].hd95.view(torch.int64))),
               max_border=mb, hd95_workspace_mb=round(_ffi.lib().uz_vol_lesion_scores_workspace_ex(N_ROWS, len(REGIONS), D, H, W, 256, 1, mb) / 1e6, 1),
               hd95_kernels_ms=kernel_ms(score, ("hd_pair_k", "hd_select_k", "hd_entries_k")))
    if not args.no_oracle:
        sec, vals, n_border, n_entries = host_hd95_row(pred_h[0], ref_h)
        kept_all = all(len(v) > 0 for v in vals)
        out.update(host_hd95_row0_s=round(sec, 2), host_hd95_all_rows_s=round(sec * N_ROWS, 1), border_voxels_row0=n_border, entries_row0=n_entries,
                   host_hd95_matched_row0=[len(v) for v in vals], hd95_speedup_vs_host=round(sec * N_ROWS * 1e3 / t["median"], 1), host_hd95_any=kept_all)
    return out


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
    if args.hd95:
        row.update(hd95_part(pred, ref, pred_h, ref_h, shape, args))
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
    ap.add_argument("--hd95", action="store_true", help="also time score_lesions(hd95=True), its pair kernel and select, and the host route per lesion")
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
        if args.hd95:
            k = lambda r, n: "-" if not r.get("hd95_kernels_ms") else r["hd95_kernels_ms"][n]
            lines += ["", "`--hd95`: `score_lesions(hd95=True)` with its defaults (penalty 374, max_border = D*H*W // 8) beside the plain call above; `pair` and `select` are the",
                      "sums of the launches of the pair kernel and of the radix select in one profiled call (three regions each); border voxels and entries are the sizes of the",
                      "two lists of row 0, summed over the regions; the host route is `distance_transform_edt` per matched lesion of row 0 on the common box of the lesion",
                      "and its components, scaled by N.", "",
                      "| volume | input | score ms | score with hd95 ms | pair ms | select ms | border voxels, entries of row 0 | list overflow | workspace MB | host, row 0, s | host, all rows, s | ratio |",
                      "|---|---|---|---|---|---|---|---|---|---|---|---|"]
            for r in rows:
                lines.append(f"| {vol(r)} | {r['input']} | {f(r['score_ms'])} | {f(r['hd95_score_ms'])} | {k(r, 'hd_pair_k')} | {k(r, 'hd_select_k')} | "
                             f"{r.get('border_voxels_row0', '-')}, {r.get('entries_row0', '-')} | {r['hd95_overflow_any']} | {r['hd95_workspace_mb']} | {r.get('host_hd95_row0_s', '-')} | "
                             f"{r.get('host_hd95_all_rows_s', '-')} | {r.get('hd95_speedup_vs_host', '-')} |")
            lines += ["", "A repeated call with hd95 was bit-equal on every shape and input: " + str(all(r["hd95_repeat_bit_equal"] for r in rows)) + "."]
        lines += ["", "A repeated score call was bit-equal on every shape and input: " + str(all(r["repeat_bit_equal"] for r in rows)) + "."]
        with open(os.path.join(ROOT, "profiles", "NOTES_lesions.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
