#!/usr/bin/env python3
"""Time predict() against the way samples were drawn before it existed, in one process on one GPU.

--model phiseg (default):
  predict : net.predict(patch, n_samples=S)                       - trunk plan at batch B, draw plan at batch B*S, uz_sample_stats
  parent  : net.forward(patch.repeat(S, 1, 1, 1), zeros, training=False) + accumulate_output(use_softmax=True) + argmax + mean
            (what train_model._evaluate_image does per image, without its metrics)
--model probunet (ProbabilisticUnet, latent_dim 6, no_convs_fcomb 3):
  predict : net.predict(patch, n_samples=S)                       - eval plan at batch B, uz_fcomb_sample_fwd, uz_sample_stats
  parent  : net.forward(patch, None) once, then S x net.sample(testing=True), then softmax, argmax and mean in torch
            (the harness loop gives S identical maps for this model, so it is no way to distinct samples)
  and `fcomb_ms`: uz_fcomb_sample_fwd alone on predict's buffers, the kernel's own share of predict

Both draw their noise on the device.  Per S the two are warmed up, then timed alternately `--repeats` times, each call between two
torch.cuda.Event records on the current stream; the figures are the medians, with the fastest and slowest call beside them.
Before timing, the two paths run once on the SAME noise and the largest difference of their level logits is printed.
Prints one JSON line per S.  usage: python tools/bench_predict.py [--model phiseg|probunet] [--samples 16 100] [--repeats 30] [--warmup 5] [--graphs 1]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_zoo_amd  # noqa: E402,F401
from unet_zoo_amd import _ffi  # noqa: E402
from unet_zoo_amd.models.phiseg import PHISeg  # noqa: E402
from unet_zoo_amd.models.probabilistic_unet import ProbabilisticUnet  # noqa: E402
from unet_zoo_amd.synthetic import synthetic_batch  # noqa: E402

FILTERS = [32, 64, 128, 192, 192, 192, 192]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def probunet(args, dev):
    B, hw, L = args.batch, args.size, 6
    torch.manual_seed(1)
    net = ProbabilisticUnet(1, 2, FILTERS, latent_dim=L, no_convs_fcomb=3, image_size=(1, hw, hw))
    with torch.no_grad():                          # running statistics away from (0, 1): BatchNorm is then no identity to either route
        net._ptab.bflat.uniform_(0.5, 1.5)
    net.eval()
    net.enable_graphs(bool(args.graphs))
    x, _, _ = synthetic_batch(B, hw, hw, seed=5)
    patch = torch.from_numpy(x).to(dev)
    lib = _ffi.lib()
    for S in args.samples:
        sink = {}

        def predict():
            sink["p"] = net.predict(patch, n_samples=S)

        def parent():
            net.forward(patch, None)
            lg = torch.cat([net.sample(testing=True) for _ in range(S)], dim=0)
            soft = torch.softmax(lg, dim=1)
            sink["q"] = (torch.argmax(soft, dim=1), soft.reshape(S, B, *soft.shape[1:]).mean(dim=0))

        with torch.no_grad():
            g = torch.Generator(device=dev).manual_seed(7)
            eps = torch.randn(S * B, L, generator=g, device=dev)
            lv = net.predict(patch, n_samples=S, eps=eps).levels[0].clone()
            z = net.z_prior_sample.reshape(S, B, L).clone()
            net.forward(patch, None)
            diff = float((torch.cat([net._decode(z[s]) for s in range(S)], dim=0) - lv).abs().max())
            for _ in range(args.warmup):
                predict(), parent()
            torch.cuda.synchronize()
            tp, tq, tk = [], [], []
            for _ in range(args.repeats):
                tp.append(timed(predict))
                tq.append(timed(parent))
            # the kernel alone: the launch predict() makes (ProbabilisticUnet._fcomb_sample), on the buffers its last call left
            plan = net._cur
            route = (C.c_int * 5)()
            lib.uz_fcomb_sample_route(net.latent_dim, net.num_classes, net.no_convs_fcomb - 1, B, S, hw, hw, route)

            def kernel():
                net._fcomb_sample(plan, S)
            for _ in range(args.warmup):
                kernel()
            for _ in range(args.repeats):
                tk.append(timed(kernel))
        flags = net.check_bounds()
        print(json.dumps(dict(bench="predict", model="probunet", filters=FILTERS, latent_dim=L, size=hw, batch=B, samples=S, graphs=args.graphs,
                              repeats=args.repeats, predict_ms=stats(tp), parent_ms=stats(tq), fcomb_ms=stats(tk), fcomb_route=list(route),
                              fcomb_px_env=os.environ.get("UZ_FCOMB_PX"), speedup=round(statistics.median(tq) / statistics.median(tp), 3),
                              max_logit_diff_same_noise=diff, bound_flags=flags, device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["phiseg", "probunet"], default="phiseg")
    ap.add_argument("--samples", type=int, nargs="+", default=[16, 100])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=1, help="enable_graphs(), as the harness runs the nets")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_predict needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    if args.model == "probunet":
        return probunet(args, dev)
    B, hw = args.batch, args.size
    torch.manual_seed(1)
    net = PHISeg(1, 2, FILTERS, latent_levels=5, image_size=(1, hw, hw))
    net.eval()
    net.enable_graphs(bool(args.graphs))
    x, _, _ = synthetic_batch(B, hw, hw, seed=5)
    patch = torch.from_numpy(x).to(dev)
    for S in args.samples:
        rep = patch.repeat(S, 1, 1, 1)
        zeros = torch.zeros(B * S, 1, hw, hw, device=dev)
        sink = {}

        def predict():
            sink["p"] = net.predict(patch, n_samples=S)

        def parent():
            out = net.forward(rep, zeros, training=False)
            soft = net.accumulate_output(out, use_softmax=True)
            sink["q"] = (torch.argmax(soft, dim=1), soft.reshape(S, B, *soft.shape[1:]).mean(dim=0))

        with torch.no_grad():
            g = torch.Generator(device=dev).manual_seed(7)
            eps = [torch.randn(B * S, 2, hw >> (6 - k), hw >> (6 - k), generator=g, device=dev) for k in range(5)]
            lv = [t.clone() for t in net.predict(patch, n_samples=S, eps=eps).levels]
            ref = net.forward(rep, zeros, training=False, eps=eps + eps)
            diff = max(float((a - b).abs().max()) for a, b in zip(lv, ref))
            for _ in range(args.warmup):
                predict(), parent()
            torch.cuda.synchronize()
            tp, tq = [], []
            for _ in range(args.repeats):
                tp.append(timed(predict))
                tq.append(timed(parent))
        flags = net.check_bounds()
        print(json.dumps(dict(bench="predict", filters=FILTERS, size=hw, batch=B, samples=S, graphs=args.graphs, repeats=args.repeats,
                              predict_ms=dict(median=round(statistics.median(tp), 3), min=round(min(tp), 3), max=round(max(tp), 3)),
                              parent_ms=dict(median=round(statistics.median(tq), 3), min=round(min(tq), 3), max=round(max(tq), 3)),
                              speedup=round(statistics.median(tq) / statistics.median(tp), 3), max_logit_diff_same_noise=diff, bound_flags=flags,
                              device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
