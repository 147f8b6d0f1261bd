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

--model phiseg3d (PHISeg3D at the volume setting of bench.py: filters 32/64/128/192/192, 4 channels, 3 classes, one 128 x 128 x 64 volume):
  predict : net.predict(patch, n_samples=S)                       - trunk plan once, S x (noise, draw plan, uz_vol_sample_accum), uz_vol_sample_finish
  parent  : S x (net.forward(patch, zeros, training=False) + accumulate_output(use_softmax=True) + argmax), then the mean in torch
  and `accum_ms` / `finish_ms`: the two kernels alone on predict's buffers, with the bytes they move and the GB/s that makes

--score (with --model phiseg | probunet): a pass over a 32-image test split, the way UNetModel.test walks it
  parent  : the loop over UNetModel._evaluate_image (forward on the repeated patch and mask, loss, argmax, then GED / NCC / Dice one
            label and one pair set at a time, each behind a .cpu())
  score   : UNetModel.score at --images-per-call 1 2 4 8 (predict + metrics.score_prediction, one host copy per call)
  Host clock around a pass that ends in a device synchronise (the parent's cost includes its syncs); both warmed, then --passes
  rounds of [parent, score at every images-per-call]; median, fastest, slowest.  Also per setting: uz_score_samples alone against
  the per-image sequence of the existing metric launches on the SAME Prediction (device events), and the arena of the plan that
  draws.  One JSON line per S.

All draw their noise on the device.  Per S the two are warmed up, then timed alternately `--repeats` times, each call between two
torch.cuda.Event records on the current stream; the figures are the medians, with the fastest and slowest call beside them.
Before timing, the two paths run once on the SAME noise and the largest difference of their level logits is printed.
Prints one JSON line per S.  usage: python tools/bench_predict.py [--model phiseg|probunet|phiseg3d] [--score [--samples 10 16 100] [--passes 10]] [--samples 16 100] [--repeats 30] [--warmup 5] [--graphs 1]"""
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
FILTERS3D, DHW3D = [32, 64, 128, 192, 192], (128, 128, 64)        # bench.py --model phiseg3d


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


def phiseg3d(args, dev):
    import torch.nn.functional as F
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    (D, H, W), Cin, K, nl = DHW3D, 4, 3, 5
    n = D * H * W
    torch.manual_seed(1)
    net = PHISeg3D(Cin, K, FILTERS3D, latent_levels=nl, image_size=(Cin, D, H, W))
    with torch.no_grad():                          # running statistics away from (0, 1): BatchNorm is then no identity to either route
        net._ptab.bflat.uniform_(0.5, 1.5)
    net.eval()
    net.enable_graphs(bool(args.graphs))
    g = torch.Generator(device=dev).manual_seed(5)
    patch = (torch.randn(1, Cin, D, H, W, generator=g, device=dev) * 0.25).clamp_(-0.5, 0.5)
    zeros = torch.zeros(1, K, D, H, W, device=dev)
    lib, st = _ffi.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.no_grad():
        eps = [torch.randn(1, 2, D >> (4 - k), H >> (4 - k), W >> (4 - k), generator=g, device=dev) for k in range(nl)]
        lv = net.predict(patch, n_samples=1, eps=eps, return_levels=True).levels
        ref = net.forward(patch, zeros, training=False, eps=eps + eps)
        diff = max(float((F.interpolate(a[0], size=[D, H, W], mode="nearest") - b).abs().max()) for a, b in zip(lv, ref))
        del lv, ref
    for S in args.samples:
        sink = {}

        def predict():
            sink["p"] = net.predict(patch, n_samples=S)

        def parent():
            labels, acc = [], None
            for _ in range(S):
                soft = net.accumulate_output(net.forward(patch, zeros, training=False), use_softmax=True)
                labels.append(torch.argmax(soft, dim=1))
                acc = soft if acc is None else acc + soft
            sink["q"] = (labels, acc / S)

        with torch.no_grad():
            for _ in range(args.warmup):
                predict(), parent()
            torch.cuda.synchronize()
            tp, tq, ta, tf = [], [], [], []
            for _ in range(args.repeats):
                tp.append(timed(predict))
                tq.append(timed(parent))
            # the two kernels alone: the launches predict() makes, on the buffers its last call left (first = 0: the sum is read and written)
            draw = net._plans[("draw", D, H, W)]
            host = net._predict_state(draw, D, H, W)
            labels = torch.empty(n, dtype=torch.uint8, device=dev)
            mean_soft, mean_label, entropy = torch.empty(K * n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, device=dev)

            def accum():
                _ffi.check(lib.uz_vol_sample_accum(host["ptrs"], host["ctot"], host["f"], host["fz"], nl, K, D, H, W, labels.data_ptr(), None,
                                                   host["acc"].data_ptr(), 0, st), "vol_sample_accum")

            def finish():
                _ffi.check(lib.uz_vol_sample_finish(host["acc"].data_ptr(), K, S, D, H, W, mean_soft.data_ptr(), mean_label.data_ptr(),
                                                    entropy.data_ptr(), st), "vol_sample_finish")
            for _ in range(args.warmup):
                accum(), finish()
            for _ in range(args.repeats):
                ta.append(timed(accum))
                tf.append(timed(finish))
        flags = net.check_bounds()
        accum_bytes = sum(4 * K * (n >> (3 * l)) for l in range(nl)) + 2 * 8 * K * n + n          # levels read, sum read + written, labels
        finish_bytes = 8 * K * n + 4 * K * n + n + 4 * n                                         # sum read; mean_soft, mean_label, entropy written
        print(json.dumps(dict(bench="predict", model="phiseg3d", filters=FILTERS3D, dhw=[D, H, W], samples=S, graphs=args.graphs, repeats=args.repeats,
                              conv_math=lib.uz_get_conv_math(), predict_ms=stats(tp), parent_ms=stats(tq),
                              speedup=round(statistics.median(tq) / statistics.median(tp), 3), accum_ms=stats(ta), finish_ms=stats(tf),
                              accum_bytes=accum_bytes, finish_bytes=finish_bytes,
                              accum_gbs=round(accum_bytes / statistics.median(ta) / 1e6, 1), finish_gbs=round(finish_bytes / statistics.median(tf) / 1e6, 1),
                              draw_ops=len(draw.fwd_ops), max_logit_diff_same_noise=diff, bound_flags=flags,
                              device=torch.cuda.get_device_name(0))), flush=True)


def score(args, dev):
    """--score: see the module docstring."""
    import tempfile
    import time
    import types

    import numpy as np

    from unet_zoo_amd import metrics as DM
    from unet_zoo_amd import train_model as TM
    hw, K, A, n_img = args.size, 2, 4, args.images
    model = PHISeg if args.model == "phiseg" else ProbabilisticUnet
    cfg = types.SimpleNamespace(experiment_name="bench", log_dir_name="bench", filter_channels=FILTERS, latent_levels=5, n_classes=K,
                                no_convs_fcomb=3, beta=10.0, use_reversible=False, input_channels=1, image_size=(1, hw, hw), batch_size=12,
                                num_labels_per_subject=A, model=model)
    torch.manual_seed(1)
    h = TM.UNetModel(cfg, log_root=tempfile.mkdtemp())            # enables lane replay, as the harness runs the nets
    with torch.no_grad():                                          # running statistics away from (0, 1)
        h.net._ptab.bflat.uniform_(0.5, 1.5)
    h.net.eval()
    data = TM.SyntheticData(None, cfg, n_train=4, n_val=n_img)
    images, labels = data.test.images, data.test.labels

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for S in args.samples:
        def parent():
            rng = np.random.default_rng(0)
            return [h._evaluate_image(images[i], labels[i], S, rng) for i in range(n_img)]

        def new(ipc):
            return h.score(images, labels, n_samples=S, images_per_call=ipc, rng=np.random.default_rng(0))

        for _ in range(args.warmup):
            parent()
            for ipc in args.images_per_call:
                new(ipc)
        tq, tn = [], {ipc: [] for ipc in args.images_per_call}
        for _ in range(args.passes):
            tq.append(wall(parent))
            for ipc in args.images_per_call:
                tn[ipc].append(wall(lambda: new(ipc)))
        rows = {}
        for ipc in args.images_per_call:
            # the scoring call alone against the per-image launches it replaces, on one Prediction of this shape
            patch = torch.as_tensor(images[:ipc], dtype=torch.float32).to(dev).unsqueeze(1).contiguous()
            ann = torch.from_numpy(np.ascontiguousarray(np.moveaxis(labels[:ipc], -1, 1)).astype(np.uint8)).to(dev)
            with torch.no_grad():
                pred = h.net.predict(patch, n_samples=S, return_soft=True)

                def one_call():
                    DM.score_prediction(pred, ann)

                def per_image():
                    for b in range(ipc):
                        yb = ann[b].long()
                        DM.generalised_energy_distance(pred.labels[:, b], yb, nlabels=K - 1, label_range=range(1, K))
                        DM.variance_ncc_dist(pred.soft[:, b], torch.stack([(yb == k) for k in range(K)], dim=1).long())
                        DM.per_label_dice(pred.mean_label[b], yb[0], K)
                for _ in range(args.warmup):
                    one_call(), per_image()
                tk, tp = [], []
                for _ in range(args.repeats):
                    tk.append(timed(one_call))
                    tp.append(timed(per_image))
            if args.model == "phiseg":
                arena = h.net._plans[("draw", ipc * S, hw, hw)].arena_floats * 4 / 2 ** 20
            else:                                                  # the eval plan at batch ipc + the logits of all samples behind it
                arena = h.net._cur.arena_floats * 4 / 2 ** 20 + ipc * S * K * hw * hw * 4 / 2 ** 20
            rows[str(ipc)] = dict(pass_ms=stats(tn[ipc]), speedup=round(statistics.median(tq) / statistics.median(tn[ipc]), 3),
                                  score_call_ms=stats(tk), per_image_metrics_ms=stats(tp), draw_arena_MB=round(arena, 1),
                                  score_workspace_MB=round(_ffi.lib().uz_score_workspace(ipc, S, A, K, hw * hw) / 2 ** 20, 2))
        print(json.dumps(dict(bench="score", model=args.model, filters=FILTERS, size=hw, classes=K, annotators=A, images=n_img, samples=S,
                              passes=args.passes, parent_pass_ms=stats(tq), score=rows, bound_flags=h.net.check_bounds(),
                              conv_math=_ffi.lib().uz_get_conv_math(), device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--score", action="store_true", help="time UNetModel.score against the per-image evaluation loop (phiseg | probunet)")
    ap.add_argument("--images", type=int, default=32, help="--score: images of the synthetic test split")
    ap.add_argument("--images-per-call", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--passes", type=int, default=10, help="--score: alternating timed passes over the split")
    ap.add_argument("--model", choices=["phiseg", "probunet", "phiseg3d"], default="phiseg")
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
    if args.score:
        if args.model == "phiseg3d":
            sys.exit("--score times the 2-D models")
        return score(args, dev)
    if args.model == "probunet":
        return probunet(args, dev)
    if args.model == "phiseg3d":
        return phiseg3d(args, dev)
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
