#!/usr/bin/env python3
"""Time PHISeg3D.predict_volume on a BraTS-sized volume, in one process on one GPU, with the model of
`tools/bench_predict.py --model phiseg3d` (filters 32/64/128/192/192, 4 channels, 3 classes, 5 latent levels).

  windows : net.predict_volume(volume, S, window, stride)         - per window: gather, trunk plan, S x (noise crop, draw plan,
            uz_vol_window_accum); one uz_vol_window_finish
  plain   : one net.predict(patch of the window's size, S) per window of the grid - the network's share of the call, without gather,
            blending or coherent noise (what a host loop would launch before it crops, pads and stitches)
  single  : net.predict_volume(volume, S, window=the padded volume) - the pad-to-divisible route: ONE window, a plan of the whole
            volume (skipped with --no-single, or when its plan cannot be built)
  With --flips (all | masks 0 .. 7) the windows call runs predict_volume(..., flips=...): per window and mask the mirrored gather, the
  trunk plan, S x (mirrored noise crop, draw plan, mirrored accum) - and the mirrored kernels are timed alone, per mask, beside the
  unmirrored ones (gather_ex, accum_ex, and the uz_vol_window_noise launches of one sample: one per latent level).
  and the three kernels of csrc/volwindow.hip alone on the buffers the windows call left: one gather, one accum (an interior
  window), the finish; with the bytes each must move and the GB/s that makes against the HBM figures of BASELINE.md.

Every time is the median of --repeats calls between two device events after --warmup calls (fastest and slowest beside it).  All
draw their noise on the device.  Prints one JSON line; --notes writes profiles/NOTES_volwindow.md.  Without a GPU the tool exits.
usage: python tools/bench_volwindow.py [--volume 240 240 155] [--window 128 128 128] [--stride 64 64 64] [--samples 16] [--repeats 3]
       [--warmup 1] [--graphs 1] [--no-single] [--flips all | --flips 0 7 ...] [--notes]
--notes writes the whole file without --flips and only its section on mirrored passes with it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_zoo_amd  # noqa: E402,F401
from unet_zoo_amd import _ffi  # noqa: E402
from unet_zoo_amd.models import phiseg3D as M  # noqa: E402

FILTERS3D = [32, 64, 128, 192, 192]                                 # bench.py --model phiseg3d
HBM_SPEC_GBS, HBM_COPY_GBS = 8000.0, 6290.0                         # HBM3E spec, measured copy


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def measure(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [timed(fn) for _ in range(repeats)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, nargs=3, default=[240, 240, 155])
    ap.add_argument("--window", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--stride", type=int, nargs=3, default=[64, 64, 64])
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--graphs", type=int, default=1, help="enable_graphs(), as the harness runs the nets")
    ap.add_argument("--no-single", action="store_true", help="skip the single-window route")
    ap.add_argument("--flips", nargs="+", default=None, help="mirrored passes: all, or masks in 0 .. 7")
    ap.add_argument("--notes", action="store_true", help="write profiles/NOTES_volwindow.md")
    args = ap.parse_args()
    flips = None if args.flips is None else "all" if args.flips == ["all"] else tuple(int(m) for m in args.flips)
    masks = None if flips is None else M.flip_masks(flips)
    if not torch.cuda.is_available():
        sys.exit("bench_volwindow needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    (D, H, W), window, stride, S = args.volume, tuple(args.window), tuple(args.stride), args.samples
    Cin, K, nl = 4, 3, 5
    n = D * H * W
    torch.manual_seed(1)
    net = M.PHISeg3D(Cin, K, FILTERS3D, latent_levels=nl, image_size=(Cin, *window))
    with torch.no_grad():                          # running statistics away from (0, 1): BatchNorm is then no identity
        net._ptab.bflat.uniform_(0.5, 1.5)
    net.eval()
    net.enable_graphs(bool(args.graphs))
    g = torch.Generator(device=dev).manual_seed(5)
    volume = (torch.randn(1, Cin, D, H, W, generator=g, device=dev) * 0.25).clamp_(-0.5, 0.5)
    padded, extent, origins = net.window_plan((D, H, W), window, stride)
    ed, eh, ew = extent
    patch = volume[:, :, :ed, :eh, :ew].contiguous() if min(D - ed, H - eh, W - ew) >= 0 else torch.zeros(1, Cin, *extent, device=dev)
    sink = {}

    def windows():
        sink["w"] = net.predict_volume(volume, n_samples=S, window=window, stride=stride, flips=flips)

    def plain():
        for _ in origins:
            sink["p"] = net.predict(patch, n_samples=S)

    def single():
        sink["s"] = net.predict_volume(volume, n_samples=S, window=padded, flips=flips)

    lib, st = _ffi.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(bench="volwindow", filters=FILTERS3D, volume=[D, H, W], window=list(extent), stride=list(stride), windows=len(origins), samples=S,
               graphs=args.graphs, repeats=args.repeats, flips=None if masks is None else list(masks), conv_math=lib.uz_get_conv_math(), device=torch.cuda.get_device_name(0))
    with torch.no_grad():
        tw = measure(windows, args.warmup, args.repeats)
        tp = measure(plain, args.warmup, args.repeats)
        res.update(windows_ms=stats(tw), plain_ms=stats(tp), windows_over_plain=round(statistics.median(tw) / statistics.median(tp), 3))
        # the three kernels alone, on the buffers the call left
        trunk, draw = net._plans[("trunk", *extent)], net._plans[("draw", *extent)]
        tb, state, wt = net._level_tables(draw, *extent), draw.host["vol_window"], draw.host["vol_blend"]["gaussian"]
        acc, wsum = state["acc"], state["wsum"]
        o = origins[0]
        pview = trunk.io["patch"]
        src = volume[0].contiguous()
        out = dict(labels=torch.empty(S, n, dtype=torch.uint8, device=dev), mean_soft=torch.empty(K, n, device=dev),
                   mean_label=torch.empty(n, dtype=torch.uint8, device=dev), entropy=torch.empty(n, device=dev))

        def gather():
            _ffi.check(lib.uz_vol_window_gather(src.data_ptr(), Cin, D, H, W, *o, trunk._resolve(pview), pview.Ctot, ed, eh, ew, st), "gather")

        def accum():
            _ffi.check(lib.uz_vol_window_accum(tb["ptrs"], tb["ctot"], tb["f"], tb["fz"], nl, K, ed, eh, ew, *o, D, H, W, wt[0].data_ptr(),
                                               wt[1].data_ptr(), wt[2].data_ptr(), acc[0].data_ptr(), wsum.data_ptr(), 0, st), "accum")

        def finish():
            _ffi.check(lib.uz_vol_window_finish(acc.data_ptr(), wsum.data_ptr(), K, S, D, H, W, out["labels"].data_ptr(), None,
                                                out["mean_soft"].data_ptr(), out["mean_label"].data_ptr(), out["entropy"].data_ptr(), st), "finish")
        tg, ta, tf = (measure(fn, max(args.warmup, 2), max(args.repeats, 10)) for fn in (gather, accum, finish))
        inside = min(ed, D - o[0]) * min(eh, H - o[1]) * min(ew, W - o[2])            # voxels of this window inside the volume
        nwin = ed * eh * ew
        bytes_ = dict(gather=4 * Cin * (inside + nwin), accum=sum(4 * K * (nwin >> (3 * l)) for l in range(nl)) + 2 * 8 * K * inside,
                      finish=8 * n * (S * K + 1) + n * (S + 4 * K + 1 + 4))
        med = dict(gather=statistics.median(tg), accum=statistics.median(ta), finish=statistics.median(tf))
        in_call = len(origins) * med["gather"] + len(origins) * S * med["accum"] + med["finish"]
        res.update(gather_ms=stats(tg), accum_ms=stats(ta), finish_ms=stats(tf), kernel_bytes=bytes_,
                   kernel_gbs={k: round(bytes_[k] / med[k] / 1e6, 1) for k in med}, kernels_in_call_ms=round(in_call, 3),
                   kernels_share_of_call=round(in_call / statistics.median(tw), 4),
                   accumulators_GB=round(8 * n * (S * K + 1) / 1e9, 3),
                   window_plans_GB=round(4 * (trunk.arena_floats + draw.arena_floats) / 1e9, 3))
        if masks is not None:                                                        # the mirrored kernels alone, per mask
            eps = [torch.randn(1, 2, *(p >> (nl - 1 - k) for p in padded), device=dev) for k in range(nl)]

            def kernels(m):
                def gather_ex():
                    _ffi.check(lib.uz_vol_window_gather_ex(src.data_ptr(), Cin, D, H, W, *o, trunk._resolve(pview), pview.Ctot, ed, eh, ew, m, st),
                               "gather_ex")

                def noise():
                    for k, (e, v) in enumerate(zip(eps, draw.io["eps"])):
                        sh = nl - 1 - k
                        _ffi.check(lib.uz_vol_window_noise(e.data_ptr(), 2, *e.shape[2:], o[0] >> sh, o[1] >> sh, o[2] >> sh, ed >> sh, eh >> sh,
                                                           ew >> sh, m, draw._resolve(v), v.Ctot, st), "noise")

                def accum_ex():
                    _ffi.check(lib.uz_vol_window_accum_ex(tb["ptrs"], tb["ctot"], tb["f"], tb["fz"], nl, K, ed, eh, ew, *o, D, H, W, wt[0].data_ptr(),
                                                          wt[1].data_ptr(), wt[2].data_ptr(), acc[0].data_ptr(), wsum.data_ptr(), 0, m, st), "accum_ex")
                return {fn.__name__: stats(measure(fn, max(args.warmup, 2), max(args.repeats, 10))) for fn in (gather_ex, noise, accum_ex)}
            res["flip_kernels_ms"] = {str(m): kernels(m) for m in masks}
            per_pass = {m: v["gather_ex"]["median"] + S * (v["noise"]["median"] + v["accum_ex"]["median"]) for m, v in res["flip_kernels_ms"].items()}
            res.update(flip_kernels_per_window_ms={m: round(v, 3) for m, v in per_pass.items()},
                       unmirrored_kernels_per_window_ms=round(med["gather"] + S * med["accum"], 3),
                       flip_kernels_in_call_ms=round(len(origins) * sum(per_pass.values()) + med["finish"], 3))
        windows()                                                                    # the timing launches added to acc: a fresh call, then compare
        net.set_rng_state(11)
        x = net.predict_volume(volume, n_samples=2, window=window, stride=stride, flips=flips)
        keep = (x.labels.clone(), x.mean_soft.clone())
        net.set_rng_state(11)
        y = net.predict_volume(volume, n_samples=2, window=window, stride=stride, flips=flips)
        res["repeat_bit_equal"] = bool(torch.equal(keep[0], y.labels) and torch.equal(keep[1], y.mean_soft))
        if not args.no_single:
            try:
                ts = measure(single, args.warmup, args.repeats)
                big = [net._plans[(part, *padded)] for part in ("trunk", "draw")]
                res.update(single_ms=stats(ts), single_window=list(padded), windows_over_single=round(statistics.median(tw) / statistics.median(ts), 3),
                           single_plans_GB=round(4 * sum(p.arena_floats for p in big) / 1e9, 3))
            except (RuntimeError, _ffi.UzError) as e:                               # the whole-volume plan does not fit
                res.update(single_ms=None, single_error=str(e).splitlines()[0][:200])
        res["bound_flags"] = net.check_bounds()
    print(json.dumps(res), flush=True)
    if args.notes:
        (write_flip_notes if masks is not None else write_notes)(res, args)


FLIP_HEAD = "## Mirrored passes"
KEPT_HEAD = "## Against the parent commit"          # written by hand behind the section on mirrored passes: kept as it is


def _flip_section():
    """The section on mirrored passes of the notes as they stand (write_flip_notes wrote it), or nothing."""
    path = os.path.join(ROOT, "profiles", "NOTES_volwindow.md")
    text = open(path).read() if os.path.exists(path) else ""
    return text[text.index(FLIP_HEAD):] if FLIP_HEAD in text else ""


def write_flip_notes(r, args):
    """Replace the section on mirrored passes; the rest of the notes - the run without --flips - stays."""
    f3 = lambda d: f"{d['median']} ({d['min']} - {d['max']})"                       # noqa: E731
    path = os.path.join(ROOT, "profiles", "NOTES_volwindow.md")
    text = open(path).read() if os.path.exists(path) else ""
    head = text[:text.index(FLIP_HEAD)] if FLIP_HEAD in text else text.rstrip("\n") + "\n\n"
    kept = text[text.index(KEPT_HEAD):] if KEPT_HEAD in text else ""
    n = len(r["flips"])
    lines = [
        FLIP_HEAD, "",
        f"`tools/bench_volwindow.py --flips {' '.join(map(str, args.flips))} --notes` on {r['device']}: the same volume, window, stride and S = "
        f"{r['samples']}, `predict_volume(..., flips={r['flips']})` = {n} passes per window, graphs {r['graphs']}, convolution mode {r['conv_math']}; "
        "times as above.", "",
        "| what | ms |", "|---|---|",
        f"| `predict_volume`, {r['windows']} windows x {n} masks | {f3(r['windows_ms'])} |",
        f"| {r['windows']} plain `predict()` calls (no mirror) | {f3(r['plain_ms'])} |", "",
        f"The call over the plain calls: {r['windows_over_plain']} for {n} passes.", "",
        "The mirrored kernels alone, on one interior window (`noise`: one sample's `uz_vol_window_noise` launches, one per latent level):", "",
        "| mask | `gather_ex` ms | `noise` ms | `accum_ex` ms | per window: gather + S (noise + accum) ms |", "|---|---|---|---|---|"]
    for m, v in r["flip_kernels_ms"].items():
        lines.append(f"| {m} | {f3(v['gather_ex'])} | {f3(v['noise'])} | {f3(v['accum_ex'])} | {r['flip_kernels_per_window_ms'][m]} |")
    lines += ["", f"Unmirrored in the same run: `uz_vol_window_gather` {f3(r['gather_ms'])}, `uz_vol_window_accum` {f3(r['accum_ms'])}, per window "
              f"gather + S accum = {r['unmirrored_kernels_per_window_ms']} ms (the unmirrored call crops its noise with ATen copies, which are not in that sum).",
              f"In one call: {r['flip_kernels_in_call_ms']} ms of window kernels, {100 * r['flip_kernels_in_call_ms'] / r['windows_ms']['median']:.2f} % of the call.  "
              f"A repeated call from the same generator state was bit-equal: {r['repeat_bit_equal']}.  Bound flags after the run: {r['bound_flags']}.", ""]
    with open(path, "w") as f:
        f.write(head + "\n".join(lines) + "\n" + kept)


def write_notes(r, args):
    flip_section = _flip_section()
    f3 = lambda d: f"{d['median']} ({d['min']} - {d['max']})"                       # noqa: E731
    vol, win = " x ".join(map(str, r["volume"])), " x ".join(map(str, r["window"]))
    lines = [
        "# Whole volumes from blended windows", "",
        f"`tools/bench_volwindow.py --notes` on {r['device']}: one `PHISeg3D.predict_volume` of a {vol} volume (4 channels, filters "
        f"{'/'.join(map(str, r['filters']))}, 3 classes, 5 latent levels), window {win}, stride {' x '.join(map(str, r['stride']))} = "
        f"{r['windows']} windows, S = {r['samples']} samples, gaussian blend, graphs {r['graphs']}, convolution mode {r['conv_math']}.",
        f"Every time is the median of {r['repeats']} calls (kernels alone: at least 10) between two device events after warm-up calls, "
        "fastest and slowest beside it.", "",
        "| what | ms |", "|---|---|",
        f"| `predict_volume`, {r['windows']} windows | {f3(r['windows_ms'])} |",
        f"| {r['windows']} plain `predict()` calls of {win} | {f3(r['plain_ms'])} |",
    ]
    if r.get("single_ms"):
        lines.append(f"| `predict_volume`, one window of {' x '.join(map(str, r['single_window']))} (pad-to-divisible route) | {f3(r['single_ms'])} |")
    elif "single_error" in r:
        lines.append(f"| one window of the padded volume | not measured: its plan could not be built ({r['single_error']}) |")
    else:
        lines.append("| one window of the padded volume | not measured (--no-single) |")
    lines += ["", f"`predict_volume` over the plain calls: {r['windows_over_plain']}." +
              (f"  Over the single window: {r['windows_over_single']}." if r.get("single_ms") else ""), "",
              "## The three kernels", "",
              "| kernel | ms | bytes it must move | GB/s | of the HBM copy rate (6.29 TB/s) | of the spec (8.0 TB/s) |", "|---|---|---|---|---|---|"]
    for k, what in (("gather", "`uz_vol_window_gather`, one window"), ("accum", "`uz_vol_window_accum`, one sample of an interior window"),
                    ("finish", f"`uz_vol_window_finish`, all {r['samples']} samples")):
        gbs = r["kernel_gbs"][k]
        lines.append(f"| {what} | {f3(r[k + '_ms'])} | {r['kernel_bytes'][k] / 1e6:.1f} MB | {gbs} | {gbs / HBM_COPY_GBS:.2f} | {gbs / HBM_SPEC_GBS:.2f} |")
    lines += ["", f"In one call: {r['windows']} gathers, {r['windows'] * r['samples']} accums and one finish = {r['kernels_in_call_ms']} ms, "
              f"{100 * r['kernels_share_of_call']:.2f} % of the call.  Accumulators: {r['accumulators_GB']} GB (8 (S K + 1) D H W bytes).", "",
              f"A repeated call from the same generator state was bit-equal: {r['repeat_bit_equal']}.  Bound flags after the run: {r['bound_flags']}.", "",
              "## Which route to prefer", "",
              "The windows run the net at the size it was trained at (`image_size`), and every voxel away from the volume's faces is seen by "
              "several windows, weighted towards their centres.  The single window runs a plan of the whole padded volume: a size no training "
              "step ever ran, whose deepest latent levels see a context they were never fitted on."]
    if r.get("single_ms"):
        lines += [f"Measured here the single window takes {1 / r['windows_over_single']:.2f} of the windows' time and its two plans hold "
                  f"{r['single_plans_GB']} GB against {r['window_plans_GB']} GB for the window's.  Prefer the windows - the default - for results; "
                  "the single window is the route for volumes that are at most a window large (there it is the only one: the window shrinks), "
                  "and a faster one for a net that was validated at the whole-volume size.", ""]
    else:
        lines += [f"The single window was not measured here; the window's two plans hold {r['window_plans_GB']} GB.  Prefer the windows - the "
                  "default; the single window is the route for volumes that are at most a window large.", ""]
    with open(os.path.join(ROOT, "profiles", "NOTES_volwindow.md"), "w") as f:
        f.write("\n".join(lines) + "\n" + (flip_section and "\n" + flip_section))


if __name__ == "__main__":
    main()
