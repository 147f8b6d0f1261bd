"""Harness / config-surface tests: experiment modules (ours and, when present, the reference's own file)
load against the native package; the train-step contract runs on the GPU."""
import os
import types

import pytest
import torch

import unet_zoo_amd  # noqa: F401
from unet_zoo_amd import train_model as TM

EXP_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unet-zoo_amd", "models", "experiments")
REQUIRED = ["experiment_name", "log_dir_name", "filter_channels", "latent_levels", "n_classes", "no_convs_fcomb", "beta",
            "use_reversible", "input_channels", "model"]


@pytest.mark.parametrize("name", ["phiseg_7_5_12", "phiseg_7_5_32", "prob_unet", "unet"])
def test_experiment_modules_load(name):
    m = TM.load_experiment(os.path.join(EXP_DIR, name + ".py"))
    for attr in REQUIRED:
        assert hasattr(m, attr), attr
    assert m.model.__module__.startswith("unet_zoo_amd.models")


def test_reference_experiment_file_loads_unchanged(tmp_path):
    """An experiment file in the reference's own layout - top-level torch imports, then the reference's module paths
    (models.phiseg, data.lidc_data, utils) - loads as it is: load_experiment maps those paths onto the native package.
    The file is our phiseg_7_5_12.py (same attribute surface as the reference's) under the reference's import header."""
    with open(os.path.join(EXP_DIR, "phiseg_7_5_12.py")) as f:
        body = f.read()
    assert "from models.phiseg import PHISeg" in body and "from data.lidc_data import lidc_data" in body
    path = tmp_path / "phiseg_7_5_12.py"
    path.write_text("import torch\nimport torch.nn as nn\n" + body)
    m = TM.load_experiment(str(path))
    assert m.model.__name__ == "PHISeg" and m.model.__module__ == "unet_zoo_amd.models.phiseg"
    assert m.filter_channels == [32, 64, 128, 192, 192, 192, 192] and m.batch_size == 12


def _small_cfg(model, filters):
    cfg = types.SimpleNamespace(experiment_name="t", log_dir_name="t", filter_channels=filters, latent_levels=5, n_classes=2,
                                no_convs_fcomb=3, beta=1.0, use_reversible=False, input_channels=1, image_size=(1, 128, 128),
                                batch_size=4, iterations=4, logging_frequency=2, model=model)
    return cfg


def test_harness_builds_on_cpu_structure_only():
    from unet_zoo_amd.models.phiseg import PHISeg
    if torch.cuda.is_available():
        pytest.skip("CPU-tier check")
    h = TM.UNetModel(_small_cfg(PHISeg, [4, 8, 8, 8, 8, 8, 8]))
    assert h.optimizer.param_groups[0]["lr"] == 1e-3 and h.optimizer.param_groups[0]["weight_decay"] == 1e-5
    assert h.scheduler.patience == 50000 and h.scheduler.min_lrs == [1e-4]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["phiseg", "probunet", "unet"])
def test_train_step_contract_runs(which, tmp_path):
    from unet_zoo_amd.models import PHISeg, ProbabilisticUnet, Unet
    model, filters = {"phiseg": (PHISeg, [8, 16, 16, 16, 16, 16, 16]), "probunet": (ProbabilisticUnet, [32, 8, 8, 8, 8, 8, 8]),
                      "unet": (Unet, [8, 16, 16, 16])}[which]
    h = TM.UNetModel(_small_cfg(model, filters), log_root=str(tmp_path))
    data = TM.SyntheticData(None, h.exp_config, n_train=16, n_val=4)
    before = {k: v.detach().clone() for k, v in h.net.state_dict().items() if v.dtype.is_floating_point}
    h.train(data)                                   # 3 iterations (range(1, iterations))
    assert torch.isfinite(h.loss)
    after = h.net.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
    path = h.save_model("last")
    sd = torch.load(path)
    assert list(sd.keys()) == list(after.keys())
    h.net.load_state_dict(sd)
    if which in ("phiseg", "probunet"):
        h.exp_config.validation_samples, h.exp_config.num_validation_images = 4, 2
        m = h.validate(data)
        assert 0.0 <= m["dice"] <= 1.0 and -1.0 <= m["ncc"] <= 1.0 and m["ged"] >= -1e-9
        assert os.path.exists(os.path.join(str(tmp_path), "t", "t", "t_best_ged.pth"))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["phiseg", "probunet"])
def test_validate_and_test_loops_match_oracle_metrics(which, tmp_path):
    """UNetModel.validate / .test (train_model.py:138-275,333-475): the per-image evaluation returns the samples it
    drew; the CPU oracle's GED / NCC / Dice (oracle/metrics.py, pinned to the reference's own utils functions) on those
    SAME samples must reproduce the device metrics, and validate()'s means must be the means of the per-image values."""
    import numpy as np
    from oracle import metrics as OM
    from unet_zoo_amd.models import PHISeg, ProbabilisticUnet
    model, filters = {"phiseg": (PHISeg, [8, 16, 16, 16, 16, 16, 16]), "probunet": (ProbabilisticUnet, [32, 8, 8, 8, 8, 8, 8])}[which]
    cfg = _small_cfg(model, filters)
    cfg.validation_samples, cfg.num_validation_images = 6, 3
    h = TM.UNetModel(cfg, log_root=str(tmp_path))
    data = TM.SyntheticData(None, cfg, n_train=16, n_val=3)
    h.train(data, iterations=3)
    h.net.eval()
    rng = np.random.default_rng(h.iteration)
    per_image = []
    for ii in range(3):
        r = h._evaluate_image(data.validation.images[ii], data.validation.labels[ii], 6, rng, keep=True)
        pred, gts, soft = r["pred"].cpu().numpy(), r["gts"].cpu().numpy().astype(np.int64), r["soft"].cpu().numpy()
        ged = OM.generalised_energy_distance(pred, gts, nlabels=1, label_range=range(1, 2))
        assert abs(ged - r["ged"]) <= 1e-12, (ged, r["ged"])                     # integer pair counts: exact
        ncc = float(np.asarray(OM.variance_ncc_dist(soft, r["onehot"].cpu().numpy())).reshape(-1)[0])
        assert abs(ncc - r["ncc"]) <= 2e-5, (ncc, r["ncc"])
        s_mean = np.argmax(soft.mean(axis=0), axis=0)
        dice = OM.per_label_dice(s_mean, r["mask"].cpu().numpy().astype(np.int64), 2)
        assert np.allclose(dice, r["dice"], atol=1e-12)
        assert np.array_equal(pred, np.argmax(soft, axis=1))
        per_image.append(r)
    h.net.train()
    # validate() with the same iteration counter draws the same annotators; eps differs (device RNG), so compare structure:
    m = h.validate(data)
    assert set(m) == {"dice", "foreground_dice", "elbo", "ged", "ncc"} and 0.0 <= m["dice"] <= 1.0
    for name in ("validation_ckpt", "best_dice", "best_loss", "best_ged", "best_ncc"):
        assert os.path.exists(os.path.join(str(tmp_path), "t", "t", f"t_{name}.pth")), name
    # test(): loads <experiment>_best_loss.pth, dumps ged/ncc arrays next to it (train_model.py:446-447)
    out = h.test(data, rounds=2, n_samples=4)
    assert set(out) == {"dice", "ged", "ncc"} and out["ged"] >= -1e-9
    ged_file = os.path.join(str(tmp_path), "t", "t", "ged4_t_best_loss.pth_2.npz")
    assert os.path.exists(ged_file) and np.load(ged_file)["arr_0"].shape == (2 * data.test.images.shape[0],)
    os.remove(os.path.join(str(tmp_path), "t", "t", "t_best_loss.pth"))
    assert h.test(data, rounds=1) is None                                         # missing checkpoint: abort like the reference (:349-352)


def test_cli_resolves_sys_config_from_local_and_flags(tmp_path, caplog):
    """`train_model EXP LOCAL` ignored LOCAL and always trained on synthetic data.  LOCAL may now be a sys_config file
    (or 'local' with an importable config package); flags override single attributes; the synthetic fallback is logged loudly."""
    import logging
    from unet_zoo_amd import train_model as TM
    cfg_file = tmp_path / "my_sys.py"
    cfg_file.write_text("data_root = '/nonexistent/data_lidc.pickle'\nlog_root = '%s'\npreproc_folder = '/x/pre'\n" % (tmp_path / "logs"))
    c = TM.resolve_sys_config(str(cfg_file))
    assert c.data_root == "/nonexistent/data_lidc.pickle" and c.log_root == str(tmp_path / "logs") and c.preproc_folder == "/x/pre"
    c = TM.resolve_sys_config(str(cfg_file), data_root="/d/p.pickle", log_root="/l")
    assert c.data_root == "/d/p.pickle" and c.log_root == "/l"
    c = TM.resolve_sys_config("local", data_root="/d/p.pickle")                  # no config package here: flags only, preproc next to the data
    assert c.preproc_folder == "/d/preproc" and c.log_root == "./logs"
    exp = TM.load_experiment(os.path.join(os.path.dirname(TM.__file__), "models", "experiments", "unet.py"))
    with caplog.at_level(logging.WARNING, logger="unet_zoo_amd"):
        data = TM.lidc_data(TM.resolve_sys_config(str(cfg_file)), exp)
    assert isinstance(data, TM.SyntheticData) and "SYNTHETIC" in caplog.text
