#!/usr/bin/env python3
"""Time uz_augment_volume on one full-size BraTS volume: 240 x 240 x 155 x 4, every stage on (rotate 20 degrees, scale 1 / 1.1,
elastic sigma 10, intensity shift, three flips), cropped to 128^3, labels included - what BratsDataset.__getitem__ costs the device
per training item.  Also each geometric stage alone and the bare copy (flip + crop + planar store), so that the dear stage has a
name, and the bytes each call has to move (computed from shapes below), so that the times read as rates.

Each call sits between two device events on the current stream; `--warmup` calls first, then `--repeats` timed ones, median with
the fastest and the slowest beside it.  Successive calls take successive volumes of `--volumes` resident ones (default 4: 610 MB of
sources against 256 MiB of Infinity Cache), as successive items of a dataset do, so a call reads its source from HBM and not from what
the call before left in the memory-side cache.  The figure the time has to hide behind is PHISeg3D's training step: pass the ms/step that
`bench.py --model phiseg3d` printed IN THE SAME GPU VISIT as --step-ms; with it the ratio is printed and --notes writes
profiles/NOTES_augment3d.md.  Without a GPU the tool exits: a time taken anywhere else says nothing.
usage: python tools/bench_augment3d.py [--step-ms 29.7] [--notes] [--repeats 30] [--warmup 5] [--volumes 4]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_zoo_amd  # noqa: E402,F401
from unet_zoo_amd import _ffi  # noqa: E402

X, Y, Z, CH, CROP = 240, 240, 155, 4, (128, 128, 128)


def table(angle=None, scale=None, sigma=None, shift=False, flips=0, origin=(0, 0, 0)):
    rs = np.random.RandomState(1)
    p = np.zeros(34, np.float64)
    p[1] = 1.0
    if angle is not None:
        p[0], p[1], p[2] = 1.0, np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
    if scale is not None:
        p[3], p[4], p[5] = 1.0, round(X * scale), round(Y * scale)
    if sigma is not None:
        p[6], p[7:16], p[16:25] = 1.0, rs.normal(0, sigma, 9), rs.normal(0, sigma, 9)
    if shift:
        p[25], p[26:30] = 1.0, rs.uniform(-0.1, 0.1, 4)
    p[30] = flips
    p[31:34] = origin
    return p


def traffic(n_stages, crop):
    """bytes a call must move: every stage that is not the last reads and writes the whole volume (4 channels fp32 + 1 label byte per
    voxel; the four bilinear taps of a voxel are neighbours and count once), the last one reads what its crop needs - at most the
    volume - and writes image, three maps and the raw label of the crop"""
    vol, out = X * Y * Z * (4 * CH + 1), crop[0] * crop[1] * crop[2] * (4 * CH + 4 * 3 + 1)
    cropped_read = crop[0] * crop[1] * crop[2] * (4 * CH + 1)
    return max(n_stages - 1, 0) * 2 * vol + cropped_read + out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-ms", type=float, default=None, help="PHISeg3D ms/step from bench.py --model phiseg3d in the same GPU visit")
    ap.add_argument("--notes", action="store_true", help="write profiles/NOTES_augment3d.md (needs --step-ms)")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--volumes", type=int, default=4, help="resident volumes the calls cycle through")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_augment3d needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    L = _ffi.lib()
    g = torch.Generator(device=dev).manual_seed(3)
    img = torch.randn(args.volumes, X, Y, Z, CH, generator=g, device=dev)
    lbl = (torch.rand(args.volumes, X, Y, Z, generator=g, device=dev) * 4).to(torch.uint8)
    lbl[lbl == 3] = 4
    turn = [0]
    ws = torch.empty(L.uz_augment_volume_workspace(CH, X, Y, Z), dtype=torch.uint8, device=dev)
    route = (C.c_int * 2)()
    L.uz_augment_volume_route(CH, X, Y, Z, 16, route)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    origin = (56, 56, 13)
    rows = {}
    for name, prm, crop, n_stages in [
            ("all stages, crop 128^3", table(20.0, 1 / 1.1, 10.0, True, 7, origin), CROP, 3),
            ("rotate alone, crop 128^3", table(angle=20.0, origin=origin), CROP, 1),
            ("scale alone, crop 128^3", table(scale=1 / 1.1, origin=origin), CROP, 1),
            ("elastic alone, crop 128^3", table(sigma=10.0, origin=origin), CROP, 1),
            ("copy (flips + crop + planar store), crop 128^3", table(flips=7, origin=origin), CROP, 0),
            ("all stages, no crop", table(20.0, 1 / 1.1, 10.0, True, 7), (X, Y, Z), 3)]:
        x = torch.empty(CH, *crop, device=dev)
        ye = torch.empty(3, *crop, device=dev)
        yr = torch.empty(*crop, dtype=torch.uint8, device=dev)

        def call():
            v = turn[0] = (turn[0] + 1) % args.volumes
            _ffi.check(L.uz_augment_volume(img[v].data_ptr(), lbl[v].data_ptr(), CH, X, Y, Z, prm.ctypes.data, *crop, ws.data_ptr(), x.data_ptr(),
                                           ye.data_ptr(), yr.data_ptr(), st), "augment_volume")
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
        assert bool(torch.isfinite(x).all())
        nbytes = traffic(n_stages, crop)
        rows[name] = dict(ms=dict(median=round(statistics.median(t), 3), min=round(min(t), 3), max=round(max(t), 3)), bytes=nbytes,
                          gbs=round(nbytes / statistics.median(t) / 1e6, 1))
    full = rows["all stages, crop 128^3"]["ms"]["median"]
    res = dict(bench="augment3d", volume=[X, Y, Z, CH], volumes=args.volumes, crop=list(CROP), route=list(route), repeats=args.repeats, calls=rows,
               step_ms=args.step_ms, ratio_to_step=None if args.step_ms is None else round(full / args.step_ms, 4),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    if args.notes:
        if args.step_ms is None:
            sys.exit("--notes needs --step-ms: the ratio is the point of the note")
        ratio = full / args.step_ms
        stage = max(("rotate alone, crop 128^3", "scale alone, crop 128^3", "elastic alone, crop 128^3"), key=lambda k: rows[k]["ms"]["median"])
        lines = ["# Volume augmentation against the PHISeg3D step", "",
                 f"`tools/bench_augment3d.py --step-ms {args.step_ms:g} --notes` on {res['device']}: one 240 x 240 x 155 x 4 volume with its label per call,",
                 f"successive calls on successive volumes of {args.volumes} resident ones (a call reads its source from HBM, not from the memory-side cache),",
                 f"route {list(route)} (float4 path, workgroups of the widest launch), {args.repeats} timed calls between device events after "
                 f"{args.warmup} warm-up calls.", "`bytes` is what the call must move (tools/bench_augment3d.py:traffic), GB/s = bytes / median - a rate of the call, not of HBM: the two",
                 "ping-pong images are written and read back inside one call, and the 256 MiB memory-side cache serves part of that.", "",
                 "| call | median ms | min | max | bytes | GB/s |", "|---|---|---|---|---|---|"]
        for k, v in rows.items():
            lines.append(f"| {k} | {v['ms']['median']} | {v['ms']['min']} | {v['ms']['max']} | {v['bytes']} | {v['gbs']} |")
        lines += ["", f"PHISeg3D training step, `bench.py --gpus 1 --model phiseg3d` in the same GPU visit: {args.step_ms:g} ms.",
                  f"All stages on, cropped to 128^3: {full} ms = {ratio:.3f} of the step "
                  f"({'within' if ratio <= 0.1 else 'ABOVE'} the tenth the pipeline was expected to stay under; on one stream it adds to the step directly).",
                  f"The dearest single stage is `{stage}` at {rows[stage]['ms']['median']} ms."]
        with open(os.path.join(ROOT, "profiles", "NOTES_augment3d.md"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
