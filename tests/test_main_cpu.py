"""CPU: the training command's host side (`mobi_amd.main`, the `main.py` shim) -- its parser against the reference's command line
(tests/golden/train_cli.json), the run folder and `-r` rules, the saved configs, the learning-rate and checkpoint wiring and
`DataModuleFromConfig` over the mini database.  Nothing here touches a device."""
import importlib
import json
import os
import sys

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "configs", "mobi_nusc_256.yaml")


@pytest.fixture(scope="module")
def m():
    from mobi_amd import main
    return main


def test_parser_equals_the_reference_command_line(m):
    with open(os.path.join(ROOT, "tests", "golden", "train_cli.json")) as f:
        ref = json.load(f)["arguments"]
    assert len(ref) == 14
    mine = {s: a for a in m.get_parser()._actions for s in a.option_strings}
    types = {"int": int, "str": str, "str2bool": m.str2bool}
    for arg in ref:
        acts = {id(mine[flag]) for flag in arg["flags"]}
        assert len(acts) == 1, arg["flags"]                                     # -n and --name are one argument
        a = mine[arg["flags"][0]]
        assert sorted(a.option_strings) == sorted(arg["flags"])
        assert a.default == arg.get("default") and a.nargs == arg.get("nargs") and a.const == arg.get("const"), arg["flags"]
        assert a.type is (types[arg["type"]] if "type" in arg else None), arg["flags"]
    for flag in ("--gpus", "--max_epochs", "--max_steps", "--accumulate_grad_batches", "--gradient_clip_val", "--resume_from_checkpoint"):
        assert mine[flag].default is None
    assert mine["--dtype"].default == "fp16" and mine["--dtype"].choices == ("fp16", "bf16") and mine["--no-refresh"].default is False
    assert m.str2bool("Yes") is True and m.str2bool("f") is False and m.str2bool(True) is True
    with pytest.raises(Exception):
        m.str2bool("maybe")


def test_name_with_resume_unknown_flags_and_the_dot_list(m, capsys):
    with pytest.raises(ValueError, match="cannot be specified both"):
        m.parse_args(["-n", "x", "-r", "somewhere"])
    with pytest.raises(SystemExit):
        m.parse_args(["--base", "c.yaml", "--no_such_flag", "1"])
    assert "no_such_flag" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        m.parse_args(["--base", "c.yaml", "--gpus", "0", "stray"])
    opt, dots = m.parse_args(["--base", "a.yaml", "b.yaml", "--scale_lr", "False", "--save_top_k", "5", "--gpus", "0,", "x.y=3", "z=q"])
    assert dots == ["x.y=3", "z=q"] and opt.base == ["a.yaml", "b.yaml"] and opt.scale_lr is False and opt.save_top_k == 5
    assert opt.train is True and opt.no_test is False and opt.seed == 23 and opt.logdir == "logs" and opt.no_refresh is False
    assert m.parse_args(["--no-refresh", "--no-test", "-t", "false"])[0].no_refresh is True


def test_run_folder_names(m):
    now = "2031-02-03T04-05-06"
    opt, _ = m.parse_args(["-b", "configs/mobi_nusc_512.yaml", "x.yaml", "-l", "runs"])
    assert m.run_folder(opt, now) == (os.path.join("runs", now + "_mobi_nusc_512"), None, ["configs/mobi_nusc_512.yaml", "x.yaml"])
    opt, _ = m.parse_args(["-b", "configs/mobi_nusc_512.yaml", "-n", "trial", "-f", "_b", "--resume_from_checkpoint", "old.ckpt"])
    assert m.run_folder(opt, now) == (os.path.join("logs", now + "_trial_b"), "old.ckpt", ["configs/mobi_nusc_512.yaml"])
    opt, _ = m.parse_args(["-b", "-f", "_p"])
    assert m.run_folder(opt, now)[0] == os.path.join("logs", now + "_p")


def test_resume_resolves_folder_checkpoint_and_config_order(m, tmp_path):
    run = tmp_path / "runs" / "2031-02-03T04-05-06_trial"
    (run / "checkpoints").mkdir(parents=True)
    (run / "configs").mkdir()
    for name in ("2031-02-03T04-05-06-project.yaml", "2031-02-03T04-05-06-lightning.yaml", "2031-03-01T00-00-00-project.yaml"):
        (run / "configs" / name).write_text("a: 1\n")
    ckpt = run / "checkpoints" / "epoch=000003.ckpt"
    ckpt.write_bytes(b"x")
    saved = [str(run / "configs" / n) for n in ("2031-02-03T04-05-06-lightning.yaml", "2031-02-03T04-05-06-project.yaml",
                                                "2031-03-01T00-00-00-project.yaml")]
    opt, _ = m.parse_args(["-r", str(ckpt), "-b", "more.yaml"])
    assert m.run_folder(opt, "now") == (str(run), str(ckpt), saved + ["more.yaml"])
    opt, _ = m.parse_args(["-r", str(run) + "/"])                               # a folder; the default base nobody named is dropped
    assert m.run_folder(opt, "now") == (str(run), str(run / "checkpoints" / "last.ckpt"), saved)
    with pytest.raises(ValueError, match="Cannot find"):
        m.run_folder(m.parse_args(["-r", str(tmp_path / "nothing")])[0], "now")


def test_saved_configs_reload_and_keep_their_references(m, tmp_path):
    from mobi_amd.ldm.util import load_config, load_configs
    overrides = ["latent_size=16", "lightning.callbacks.image_logger.params.disabled=True"]
    opt, dots = m.parse_args(["-b", CONFIG, "--max_epochs", "2", "--max_steps", "3", "--gradient_clip_val", "0.5", "--gpus", "0,", *overrides])
    resolved, raw = load_configs([CONFIG], dots)
    assert resolved == load_config(CONFIG, overrides)                           # (load_config keeps its behaviour)
    project, lightning = m.split_lightning(raw, opt)
    cfgdir = str(tmp_path / "configs")
    m.save_configs(cfgdir, "NOW", project, lightning)
    assert sorted(os.listdir(cfgdir)) == ["NOW-lightning.yaml", "NOW-project.yaml"]
    files = sorted(os.path.join(cfgdir, f) for f in os.listdir(cfgdir))
    with open(files[1]) as f:
        on_disk = yaml.safe_load(f)
    assert "lightning" not in on_disk and on_disk["model"]["params"]["image_size"] == "${latent_size}"       # unresolved
    again, _ = load_configs(files)
    want = {k: v for k, v in resolved.items() if k != "lightning"}
    assert {k: v for k, v in again.items() if k != "lightning"} == want and again["model"]["params"]["image_size"] == 16
    eight, _ = load_configs(files, ["latent_size=8"])
    assert eight["model"]["params"]["image_size"] == 8
    tr = again["lightning"]["trainer"]
    assert tr["max_epochs"] == 2 and tr["gradient_clip_val"] == 0.5 and tr["gpus"] == "0," and "max_steps" not in tr
    assert again["lightning"]["callbacks"]["image_logger"]["params"]["disabled"] is True
    # several bases merge left to right, dict by dict
    (tmp_path / "late.yaml").write_text("model:\n  base_learning_rate: 0.5\nextra: {a: 1}\n")
    merged, _ = load_configs([CONFIG, str(tmp_path / "late.yaml")])
    assert merged["model"]["base_learning_rate"] == 0.5 and merged["extra"] == {"a": 1}
    assert merged["model"]["params"] == load_config(CONFIG)["model"]["params"]


def test_learning_rate_wiring(m, capsys):
    opt, _ = m.parse_args(["--scale_lr", "False"])
    assert m.learning_rate(opt, 1e-5, 4, 1, 2) == 1e-5
    assert "NOT USING LR SCALING" in capsys.readouterr().out
    opt, _ = m.parse_args([])
    assert m.learning_rate(opt, 1e-5, 4, 1, 2) == 4 * 1 * 1 * 2 * 1e-5
    assert "8.00e-05 = 4 (accumulate_grad_batches) * 1 (num_nodes) * 1 (num_gpus) * 2 (batchsize) * 1.00e-05 (base_lr)" in capsys.readouterr().out


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.model = torch.nn.Linear(2, 2)
        self.first_stage_model = torch.nn.Linear(2, 2)
        self.modelish = torch.nn.Linear(2, 2)          # `modelish.*` does not begin with `model.`


def test_train_from_scratch_drops_exactly_the_model_keys(m, tmp_path, monkeypatch):
    from mobi_amd.ldm import util
    torch.manual_seed(0)
    src = _Tiny()
    path = str(tmp_path / "pre.ckpt")
    torch.save({"state_dict": src.state_dict()}, path)
    monkeypatch.setattr(util, "instantiate_from_config", lambda cfg: _Tiny())
    for scratch in (False, True):
        torch.manual_seed(1)
        dst = util.instantiate_from_config({"target": "anything"})
        before = {k: v.clone() for k, v in dst.state_dict().items()}
        loaded = m.load_pretrained(dst, path, scratch)
        for k, v in dst.state_dict().items():
            kept = scratch and k.startswith("model.")
            assert torch.equal(v, before[k] if kept else src.state_dict()[k]), k
        assert loaded == sorted(k for k in before if not (scratch and k.startswith("model.")))


def test_the_config_target_resolves_and_imports_run_nothing(m, capsys):
    from mobi_amd.ldm.util import get_obj_from_str
    assert get_obj_from_str("main.DataModuleFromConfig") is m.DataModuleFromConfig
    sys.path.insert(0, ROOT)
    try:
        for name in ("main", "mobi_amd.main"):
            sys.modules.pop(name, None)
            mod = importlib.import_module(name)
            assert mod.DataModuleFromConfig.__name__ == "DataModuleFromConfig" and callable(mod.main)
    finally:
        sys.path.remove(ROOT)
        sys.modules["mobi_amd.main"] = m
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""
    assert not torch.cuda.is_initialized()


def test_data_module_over_the_mini_database(m, tmp_path, capsys):
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    from tests import mini_db
    csv, pkl = mini_db.build(str(tmp_path / "db"))
    overrides = ["batch_size=2", "num_workers_per_gpu=0", "use_lidar=True", "data.params.test=null"]
    for split in ("train", "validation"):
        d = f"data.params.{split}.params."
        overrides += [f"{d}object_database_path={csv}", f"{d}scene_database_path={pkl}", f"{d}num_samples_per_class=2",
                      f"{d}min_lidar_points=8", f"{d}range_int_norm=True"]
    cfg = load_config(CONFIG, overrides)
    assert cfg["data"]["target"] == "main.DataModuleFromConfig"
    dm = instantiate_from_config(cfg["data"])
    assert isinstance(dm, m.DataModuleFromConfig) and dm.batch_size == 2 and dm.num_workers == 0
    # two classes in the mini database (car, pedestrian), num_samples_per_class = 2
    assert {k: len(v) for k, v in dm.datasets.items()} == {"train": 4, "validation": 4}
    assert capsys.readouterr().out.splitlines()[-3:] == ["#### Data #####", "train, NuScenesDataset, 4", "validation, NuScenesDataset, 4"]
    order = lambda seed, epoch, start=0: (setattr(dm, "seed", seed), list(dm.train_batches(epoch, start).inner.batch_sampler))[1]
    full = order(23, 0)
    assert sorted(i for b in full for i in b) == [0, 1, 2, 3] and all(len(b) == 2 for b in full)
    torch.manual_seed(99)                                                      # (the global stream has no say)
    assert order(23, 0) == full and order(23, 0, 1) == full[1:]
    assert {tuple(map(tuple, order(23, e))) for e in range(6)} != {tuple(map(tuple, full))}          # the epoch moves it
    assert {tuple(map(tuple, order(s, 0))) for s in range(6)} != {tuple(map(tuple, full))}           # the seed moves it
    assert not torch.cuda.is_initialized()


def test_more_than_one_gpu_exits_before_a_device_is_touched(m, tmp_path):
    with pytest.raises(SystemExit, match="one process on one GPU"):
        m.main(["-b", CONFIG, "--gpus", "0,1", "-l", str(tmp_path)])
    with pytest.raises(SystemExit, match="one process on one GPU"):
        m.main(["-b", CONFIG, "-l", str(tmp_path), "lightning.trainer.gpus='0,1,2'"])      # (after another flag: -b takes words)
    assert os.listdir(tmp_path) == [] and not torch.cuda.is_initialized()
