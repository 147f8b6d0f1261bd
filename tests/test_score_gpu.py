"""Scoring on the device: uz_score_samples (csrc/score.hip) on the op-level cases of tests/_score.py against oracle.metrics' values
and against the per-image kernels it batches (uz_label_pair_counts, uz_ncc_maps + uz_ncc, metrics.*), then
metrics.score_prediction on model-made and hand-made Predictions and UNetModel.score / test(mask_free=True).
Gates: counts integer for integer; GED and Dice 1e-12 (test_metrics.py's gate: fp64 sums of at most 49 terms in [0, 1] cannot differ
by more than about 1e-14 between summation orders); ncc_pairs bit for bit (the same device functions); ncc 1e-12 against the fp64
mean of ncc_pairs and 1e-5 against the golden values (test_metrics.py's gate)."""
import functools
import types

import numpy as np
import pytest
import torch

import oracle
from tests import _golden as G
from tests import _nets as N
from tests import _score as SC

pytestmark = pytest.mark.gpu



def _g():
    from tests import _gpu
    return _gpu


def _call(g, labels, ann, mean_label, soft, K, with_counts=True, sizes=None, check=True):
    """One uz_score_samples call with every output and the workspace between canaries.  sizes overrides (B, S, A, K, P) as the call
    states them (refusals).  -> (rc, outputs as guarded (raw, view) pairs)."""
    S, B, P = labels.shape
    A = ann.shape[1]
    L = g.L()
    nbytes = L.uz_score_workspace(B, S, A, K, P) if sizes is None else 4096
    np_ = SC.n_pairs(S, A)
    # 64 canary elements in front of and behind every output, 256 around the workspace
    out = dict(ws=g.guarded(nbytes, torch.uint8, 256), counts=g.guarded(B * K * np_ * 3, torch.int32), ged=g.guarded(B, torch.float64),
               ncc_pairs=g.guarded(B * A, torch.float32), ncc=g.guarded(B, torch.float64), dice=g.guarded(B * A * K, torch.float64))
    assert out["ws"][1].data_ptr() % 256 == 0
    b_, s_, a_, k_, p_ = sizes if sizes is not None else (B, S, A, K, P)
    rc = L.uz_score_samples(labels.data_ptr(), ann.data_ptr(), mean_label.data_ptr(), soft.data_ptr() if soft is not None else None,
                            b_, s_, a_, k_, p_, out["ws"][1].data_ptr(), out["counts"][1].data_ptr() if with_counts else None,
                            out["ged"][1].data_ptr(), out["ncc_pairs"][1].data_ptr(), out["ncc"][1].data_ptr(), out["dice"][1].data_ptr(), g.stream())
    torch.cuda.synchronize()
    if check:
        assert rc == 0, L.uz_last_error()
        for k, (raw, view) in out.items():
            assert g.intact(raw, view), k
    return rc, out


def _dev_case(g, c):
    v = SC.case(*c)
    T = lambda a: torch.from_numpy(a.copy()).to(g.dev())
    return v, T(v.labels), T(v.ann), T(v.mean_label), (T(v.soft) if v.soft is not None else None)


def _ncc_pairs_per_image(g, soft, ann, b, K):
    """uz_ncc_maps + uz_ncc on soft[:, b] and the materialised one-hot of ann[b]: what variance_ncc_dist launches."""
    S, A, P = soft.shape[0], ann.shape[1], ann.shape[2]
    s = soft[:, b].contiguous()
    onehot = torch.stack([(ann[b] == k) for k in range(K)], dim=1).float().contiguous()          # (A, K, P)
    ess, esy, out = torch.empty(P, device=g.dev()), torch.empty(A, P, device=g.dev()), torch.empty(A, device=g.dev())
    g.call("uz_ncc_maps", s, onehot, S, A, K, P, ess, esy)
    g.call("uz_ncc", ess, esy, A, P, out)
    return out


def _check_case(g, c):
    from unet_zoo_amd import metrics as DM
    P, K, B, S, A = c
    v, labels, ann, mean_label, soft = _dev_case(g, c)
    e = SC.expected(*c)
    _, out = _call(g, labels, ann, mean_label, soft, K)
    counts = out["counts"][1].view(B, K, SC.n_pairs(S, A), 3)
    ged, dice = out["ged"][1].cpu().numpy(), out["dice"][1].view(B, A, K).cpu().numpy()
    # ---- counts: numpy's integers, and uz_label_pair_counts on the same slices
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), e.counts), c
    for b in range(B):
        sb, yb = labels[:, b].contiguous(), ann[b].contiguous()
        for k in range(K):
            per_image = torch.cat([DM.pair_counts(x, y, k).reshape(-1, 3) for x, y in ((sb, yb), (sb, sb), (yb, yb))])
            assert torch.equal(counts[b, k], per_image), (c, b, k)
    # ---- GED and Dice: oracle.metrics' values and the per-image device functions
    eg = float(np.abs(ged - e.ged).max())
    ed = float(np.abs(dice - e.dice).max())
    assert eg <= 1e-12 and ed <= 1e-12, (c, eg, ed)
    for b in range(B):
        per_image = DM.generalised_energy_distance(labels[:, b], ann[b], nlabels=K - 1, label_range=range(1, K))
        assert abs(ged[b] - per_image) <= 1e-12, (c, b)
        for j in range(A):
            d = DM.per_label_dice(mean_label[b].reshape(1, P), ann[b, j].reshape(1, P), K)
            assert np.abs(dice[b, j] - np.asarray(d)).max() <= 1e-12, (c, b, j)
    # ---- NCC
    en = None
    if soft is not None:
        pairs = out["ncc_pairs"][1].view(B, A)
        for b in range(B):
            per_image = _ncc_pairs_per_image(g, soft, ann, b, K)
            assert torch.equal(torch.nan_to_num(pairs[b], nan=12345.0), torch.nan_to_num(per_image, nan=12345.0)), (c, b)      # bit-equal, NaNs included
        ncc = out["ncc"][1].cpu().numpy()
        mean = pairs.double().cpu().numpy().mean(axis=1)
        if c == SC.CONSTANT_SOFT:
            assert not np.isfinite(ncc).any() and not np.isfinite(mean).any()
        else:
            en = float(np.abs(ncc - e.ncc).max())
            assert np.isfinite(ncc).all() and np.abs(ncc - mean).max() <= 1e-12, c
            assert en <= 1e-5, (c, en)                                                 # against the oracle: test_metrics.py's device gate
    print(f"score {c}: ged {eg:.1e} dice {ed:.1e} ncc vs oracle {en if en is None else format(en, '.1e')}")
    # ---- a second call: bit-equal in every output; without `counts` and without `soft` the rest is what it was
    _, again = _call(g, labels, ann, mean_label, soft, K)
    keys = ("counts", "ged", "dice") + (("ncc_pairs", "ncc") if soft is not None else ())
    for k in keys:
        assert torch.equal(torch.nan_to_num(out[k][1], nan=12345.0), torch.nan_to_num(again[k][1], nan=12345.0)), (c, k)
    _, bare = _call(g, labels, ann, mean_label, None, K, with_counts=False)
    assert torch.equal(bare["ged"][1], out["ged"][1]) and torch.equal(bare["dice"][1], out["dice"][1]), c
    for k in ("counts", "ncc_pairs", "ncc"):                                            # null counts / null soft: untouched
        assert bool((bare[k][0] == g.CANARY[bare[k][0].dtype]).all()), (c, k)
    for t, a in ((labels, v.labels), (ann, v.ann), (mean_label, v.mean_label)):
        assert np.array_equal(t.cpu().numpy(), a), c                                   # the inputs are read only


@pytest.mark.parametrize("P", SC.PS)
def test_score_samples_vs_oracle_and_the_per_image_kernels(P):
    g = _g()
    for c in SC.CASES:
        if c[0] == P:
            _check_case(g, c)


def test_score_samples_on_the_golden_batch():
    """m0, m1 (stacked, B = 2) and m2 of tests/golden/metrics.*: the reference's own GED within 1e-12, its NCC within 1e-5."""
    g = _g()
    arrays, meta = G.load("metrics")
    for names, labels, ann, soft in SC.golden_batches(arrays):
        S, B, P = labels.shape
        A = ann.shape[1]
        T = lambda a: torch.from_numpy(a).to(g.dev())
        _, out = _call(g, T(labels), T(ann), T(np.ascontiguousarray(labels[0])), T(soft), 2)
        ged, ncc = out["ged"][1].cpu().numpy(), out["ncc"][1].cpu().numpy()
        for b, n in enumerate(names):
            print(f"golden {n}: ged {abs(ged[b] - meta[f'{n}_ged']):.1e} ncc {abs(ncc[b] - meta[f'{n}_ncc']):.1e}")
            assert abs(ged[b] - meta[f"{n}_ged"]) <= 1e-12, n
            assert abs(ncc[b] - meta[f"{n}_ncc"]) <= 1e-5, n


def test_score_samples_refusals_write_nothing():
    g = _g()
    c = (65, 3, 2, 6, 3)
    v, labels, ann, mean_label, soft = _dev_case(g, c)
    P, K, B, S, A = c
    L = g.L()
    for sizes in ((B, S, A, 1, P), (B, S, A, 9, P), (B, S, A, K, 0), (B, 0, A, K, P)):
        assert L.uz_score_workspace(*sizes) == 0, sizes
        rc, out = _call(g, labels, ann, mean_label, soft, K, sizes=sizes, check=False)
        assert rc != 0 and L.uz_last_error(), sizes
        for k, (raw, _) in out.items():
            assert bool((raw == g.CANARY[raw.dtype]).all()), (sizes, k)
    assert L.uz_score_workspace(B, S, A, K, P) > 0
    assert L.uz_score_workspace(1 << 12, 1 << 12, 4, 2, 1 << 12) == 0                   # S B P past int32


# ------------------------------------------------------------------------------------------ metrics.score_prediction
def _prediction(labels, mean_label, soft, K, shape):
    """A Prediction from tensors, without a model: labels (S, B, P) ... reshaped to (S, B) + shape."""
    from unet_zoo_amd.models.phiseg import Prediction
    S, B = labels.shape[:2]
    mean_soft = torch.zeros((B, K) + shape, device=labels.device)                       # score_prediction reads its class dimension only
    return Prediction(labels=labels.reshape((S, B) + shape), mean_soft=mean_soft, mean_label=mean_label.reshape((B,) + shape),
                      entropy=None, levels=[], soft=None if soft is None else soft.reshape((S, B, K) + shape))


def _same(a, b):
    for k in ("ged", "dice", "ncc", "ncc_pairs", "counts"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0)), k


def test_score_prediction_on_a_volume_shaped_prediction():
    """B = 1, (D, H, W) = (3, 5, 7): what the same maps flattened to P = 105 give, and the oracle's values."""
    from unet_zoo_amd import metrics as DM
    g = _g()
    K, S, A, shape = 3, 4, 3, (3, 5, 7)
    rng = np.random.Generator(np.random.PCG64(105))
    labels = rng.integers(0, K, size=(S, 1, 105)).astype(np.uint8)
    ann = rng.integers(0, K, size=(1, A, 105)).astype(np.uint8)
    mean_label = rng.integers(0, K, size=(1, 105)).astype(np.uint8)
    z = rng.standard_normal((S, 1, K, 105))
    soft = (np.exp(z) / np.exp(z).sum(axis=2, keepdims=True)).astype(np.float32)
    T = lambda a: torch.from_numpy(a).to(g.dev())
    vol = DM.score_prediction(_prediction(T(labels), T(mean_label), T(soft), K, shape), T(ann).reshape(1, A, *shape), return_counts=True)
    flat = DM.score_prediction(_prediction(T(labels), T(mean_label), T(soft), K, (105,)), T(ann), return_counts=True)
    _same(vol, flat)
    assert vol.ged.shape == (1,) and vol.dice.shape == (1, A, K) and vol.ncc.shape == (1,) and vol.ncc_pairs.shape == (1, A)
    assert vol.ged.dtype == vol.dice.dtype == vol.ncc.dtype == torch.float64 and vol.ncc_pairs.dtype == torch.float32
    assert vol.counts.shape == (1, K, SC.n_pairs(S, A), 3) and vol.counts.dtype == torch.int32
    e = SC.expected_from(labels, ann, mean_label, soft, K)
    assert np.array_equal(vol.counts.cpu().numpy(), e.counts)
    assert np.abs(vol.ged.cpu().numpy() - e.ged).max() <= 1e-12 and np.abs(vol.dice.cpu().numpy() - e.dice).max() <= 1e-12
    assert np.abs(vol.ncc.cpu().numpy() - e.ncc).max() <= 1e-5
    # int64 annotations are converted; no soft -> no NCC, no counts unless asked for
    bare = DM.score_prediction(_prediction(T(labels), T(mean_label), None, K, shape), T(ann).reshape(1, A, *shape).long())
    assert bare.ncc is None and bare.ncc_pairs is None and bare.counts is None
    assert torch.equal(bare.ged, vol.ged) and torch.equal(bare.dice, vol.dice)
    with pytest.raises(ValueError):
        DM.score_prediction(_prediction(T(labels), T(mean_label), None, K, shape), T(ann))      # annotations of another shape


PHISEG_FILTERS = [4, 8, 8, 8, 8, 8, 8]
PROBUNET_FILTERS = [32, 8, 8, 8, 8, 8, 8]
MODEL_BS = (3, 2)


def _annotators(B, H, W, A=4, seed=23):
    _, m, _ = oracle.synthetic_batch(B, H, W, seed=seed)
    m = m[:, 0].astype(np.uint8)
    return np.stack([np.roll(m, shift=(a, -a), axis=(1, 2)) for a in range(A)], axis=1)          # (B, A, H, W), as SyntheticData's


def _model_prediction(model):
    dev = torch.device("cuda", 0)
    B, S = MODEL_BS
    H = W = 64
    if model == "phiseg":
        from unet_zoo_amd.models.phiseg import PHISeg, phiseg_spec
        net = PHISeg(1, 2, PHISEG_FILTERS, image_size=(1, H, W))
        sd = N.off_identity_state(phiseg_spec(1, 2, PHISEG_FILTERS), seed=91)
        shapes = oracle.phiseg_eps_shapes(B * S, H, W)
        x, _, eps = oracle.synthetic_batch(B * S, H, W, seed=45, eps_shapes=shapes)
        eps = [torch.from_numpy(a).to(dev) for a in eps]
    else:
        from unet_zoo_amd.models.probabilistic_unet import ProbabilisticUnet, probunet_spec
        net = ProbabilisticUnet(1, 2, PROBUNET_FILTERS, latent_dim=6, no_convs_fcomb=3, image_size=(1, H, W))
        sd = N.off_identity_state(probunet_spec(1, 2, PROBUNET_FILTERS, 6, 3), seed=1239)
        x, _, eps = oracle.synthetic_batch(B * S, H, W, seed=85, eps_shapes=[(S * B, 6)])
        eps = torch.from_numpy(eps[0]).to(dev)
    res = net.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    net.eval()
    with torch.no_grad():
        pred = net.predict(torch.from_numpy(x[:B]).to(dev), n_samples=S, eps=eps, return_soft=True)
    assert net.check_bounds() == 0
    return pred


@pytest.mark.parametrize("model", ["phiseg", "probunet"])
def test_score_prediction_model_vs_the_per_image_metrics(model):
    """score_prediction(net.predict(...), ann) against metrics.generalised_energy_distance / variance_ncc_dist / per_label_dice on
    pred.labels[:, b], pred.soft[:, b] and pred.mean_label[b]."""
    from unet_zoo_amd import metrics as DM
    g = _g()
    B, S = MODEL_BS
    K, A, H, W = 2, 4, 64, 64
    pred = _model_prediction(model)
    ann = torch.from_numpy(_annotators(B, H, W, A)).to(g.dev())
    sc = DM.score_prediction(pred, ann, return_counts=True)
    _same(sc, DM.score_prediction(pred, ann, return_counts=True))
    assert sc.ged.shape == (B,) and sc.dice.shape == (B, A, K) and sc.ncc.shape == (B,) and sc.ncc_pairs.shape == (B, A)
    assert torch.equal(sc.packed[:B], sc.ged) and torch.equal(sc.packed[2 * B:].view(B, A, K), sc.dice)
    counts = sc.counts.cpu()
    for b in range(B):
        lb, yb = pred.labels[:, b].contiguous(), ann[b].contiguous()
        for k in range(K):
            per_image = torch.cat([DM.pair_counts(x, y, k).reshape(-1, 3) for x, y in ((lb, yb), (lb, lb), (yb, yb))]).cpu()
            assert torch.equal(counts[b, k], per_image), (b, k)
        ged = DM.generalised_energy_distance(lb, yb.long(), nlabels=K - 1, label_range=range(1, K))
        onehot = torch.stack([(yb == k) for k in range(K)], dim=1).long()
        ncc = DM.variance_ncc_dist(pred.soft[:, b], onehot)
        pairs = _ncc_pairs_per_image(g, pred.soft.reshape(S, B, K, H * W), ann.reshape(B, A, H * W), b, K)
        print(f"{model} image {b}: ged {float(sc.ged[b]):.6f} (per image {ged:.6f}) ncc {float(sc.ncc[b]):.6f} (per image {ncc:.6f})")
        assert abs(float(sc.ged[b]) - ged) <= 1e-12, b
        assert torch.equal(torch.nan_to_num(sc.ncc_pairs[b], nan=12345.0), torch.nan_to_num(pairs, nan=12345.0)), b
        assert np.isfinite(ncc) and abs(float(sc.ncc[b]) - ncc) <= 1e-12, b
        assert abs(float(sc.ncc[b]) - float(sc.ncc_pairs[b].double().mean())) <= 1e-12
        for j in range(A):
            d = DM.per_label_dice(pred.mean_label[b], ann[b, j], K)
            assert np.abs(sc.dice[b, j].cpu().numpy() - np.asarray(d)).max() <= 1e-12, (b, j)


# ------------------------------------------------------------------------------------------ harness
def _cfg(model, filters):
    return types.SimpleNamespace(experiment_name="t", log_dir_name="t", filter_channels=filters, latent_levels=5, n_classes=2, no_convs_fcomb=3,
                                 beta=1.0, use_reversible=False, input_channels=1, image_size=(1, 64, 64), batch_size=2, iterations=2,
                                 logging_frequency=2, model=model)


def test_harness_score_is_predict_plus_score_prediction_chunk_by_chunk(tmp_path):
    from unet_zoo_amd import metrics as DM
    from unet_zoo_amd import train_model as TM
    from unet_zoo_amd.models import PHISeg
    cfg = _cfg(PHISeg, PHISEG_FILTERS)
    h = TM.UNetModel(cfg, log_root=str(tmp_path))
    data = TM.SyntheticData(None, cfg, n_train=4, n_val=3)
    images, labels = data.test.images, data.test.labels                                 # (3, 64, 64), (3, 64, 64, 4)
    assert images.shape == (3, 64, 64) and labels.shape == (3, 64, 64, 4)
    h.net.train()
    h.net.set_rng_state(4321)
    h.net.snapshot_step()
    got = h.score(images, labels, n_samples=2, images_per_call=2, rng=np.random.default_rng(5))
    assert not h.net.training
    assert got["ged"].shape == (3,) and got["ncc"].shape == (3,) and got["dice"].shape == (3, 2)
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in got.values())
    h.net.restore_step()
    rng = np.random.default_rng(5)
    pick = [rng.choice(list(cfg.annotator_range)) for _ in range(3)]
    want = dict(ged=[], ncc=[], dice=[])
    for idx, keep in (([0, 1], 2), ([2, 2], 1)):                                        # the padded last chunk, by hand
        patch = torch.as_tensor(images[idx], dtype=torch.float32).to(h.device).unsqueeze(1)
        ann = torch.from_numpy(np.ascontiguousarray(np.moveaxis(labels[idx], -1, 1)).astype(np.uint8)).to(h.device)
        with torch.no_grad():
            sc = DM.score_prediction(h.net.predict(patch, n_samples=2, return_soft=True), ann)
        for q in range(keep):
            want["ged"].append(float(sc.ged[q])); want["ncc"].append(float(sc.ncc[q]))
            want["dice"].append(sc.dice[q, pick[idx[q]]].cpu().numpy())
    assert np.array_equal(got["ged"], np.asarray(want["ged"])) and np.array_equal(got["ncc"], np.asarray(want["ncc"]), equal_nan=True)
    assert np.array_equal(got["dice"], np.stack(want["dice"]))
    assert sorted(k[0] for k in h.net._plans) == ["draw", "trunk"]                      # one plan pair for the call shape


def test_harness_test_mask_free_writes_the_reference_files(tmp_path):
    from unet_zoo_amd import train_model as TM
    from unet_zoo_amd.models import PHISeg, Unet
    cfg = _cfg(PHISeg, PHISEG_FILTERS)
    h = TM.UNetModel(cfg, log_root=str(tmp_path))
    data = TM.SyntheticData(None, cfg, n_train=4, n_val=3)
    assert h.test(data, mask_free=True) is None                                         # no checkpoint yet: as the default route
    h.save_model("best_loss")
    out = h.test(data, rounds=2, n_samples=2, mask_free=True, images_per_call=2)
    assert sorted(out) == ["dice", "ged", "ncc"] and all(isinstance(v, float) for v in out.values())
    d = tmp_path / "t" / "t"
    ged = np.load(d / "ged2_t_best_loss.pth_2.npz")["arr_0"]
    ncc = np.load(d / "ncc2_t_best_loss.pth_2.npz")["arr_0"]
    assert ged.shape == (6,) and ncc.shape == (6,) and np.isfinite(ged).all()
    assert abs(h.avg_ged - float(ged.mean())) <= 1e-12
    cfg_u = types.SimpleNamespace(**{**vars(cfg), "model": Unet, "filter_channels": [8, 16, 16, 16]})
    hu = TM.UNetModel(cfg_u, log_root=str(tmp_path))
    with pytest.raises(NotImplementedError):
        hu.score(data.test.images, data.test.labels, n_samples=2)
