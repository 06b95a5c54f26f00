"""The training command: `python -m mobi_amd.main --base configs/mobi_nusc_512.yaml --pretrained_model model.ckpt --logdir runs
[--scale_lr False] [--save_top_k 5] [--gpus 0,] [key=value ...]` -- the reference's `scripts/train.sh` -> main.py, for ONE process
on ONE GPU, written from its behaviour and none of its text.  It wires the library together: `instantiate_from_config(config.model)`,
`DataModuleFromConfig` (`train.epoch_loader` / `NuScenesDataset.device_loader`), `train.Trainer.fit` (`training_step`,
`AdamW.step_scaled`, `GradScaler`, `GradAccumulator`, EMA, `checkpoint.Checkpointer`) and `train.ImageLogger`.

    <logdir>/<now>_<name or first base's stem><postfix>/
        checkpoints/last.ckpt, epoch=NNNNNN.ckpt          `python -m mobi_amd.checkpoint verify` accepts them
        configs/<now>-project.yaml, <now>-lightning.yaml    the merged values BEFORE `${}` resolution (the reference's SetupCallback)
        metrics.jsonl                                       train / val / images rows
        images/<split>/...png                               the image logger's collages

`-r <run folder>` continues `<run folder>/checkpoints/last.ckpt`, `-r <checkpoint file>` that file in the folder two levels up;
the folder's `configs/*.yaml`, sorted, are merged in front of `--base`.  Every optimizer step ends with ONE launch that rebuilds
the 16-bit copies of the trained weights (`train.WeightRefresher`; `--no-refresh`: the lazy per-tensor path, the same numbers).
SIGUSR1 asks for a `last.ckpt` after the optimizer step in progress; SIGUSR2 is ignored.  Unlike the reference an exception does
NOT trigger a save: it may be a device fault, after which nothing more is started on the GPU.  No test stage runs (the model
defines no `test_step`); `--no-test`, `--debug` and `--project` are accepted.  `--max_steps` ends this invocation with a `last.ckpt`
at that step and is not written to the run's configs, so that `-r` continues.  More than one GPU id exits: launching ranks is not this command's job."""
import argparse
import datetime
import glob
import os

ONE_GPU = ("this command runs one process on one GPU: --gpus / lightning.trainer.gpus names {n} devices ({gpus!r}); start one process "
           "per rank with torch.distributed initialised and drive `train.Trainer` from there")
TRAINER_FLAGS = ("gpus", "max_epochs", "max_steps", "accumulate_grad_batches", "gradient_clip_val", "resume_from_checkpoint")
IMAGE_LOGGER_DEFAULTS = {"batch_frequency": 400, "max_images": 8, "clamp": False, "log_on_batch_idx": True, "log_first_step": True}


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def get_parser():
    """The reference's flags with its defaults (tests/golden/train_cli.json), the Lightning trainer flags its scripts and configs
    use, and `--dtype` / `--no-refresh`."""
    ap = argparse.ArgumentParser(prog="python -m mobi_amd.main")
    ap.add_argument("-n", "--name", type=str, const=True, default="", nargs="?", help="postfix of the run folder")
    ap.add_argument("-r", "--resume", type=str, const=True, default="", nargs="?", help="a run folder, or a checkpoint inside one")
    ap.add_argument("-b", "--base", nargs="*", metavar="base_config.yaml", default=["configs/stable-diffusion/v1-inference-inpaint.yaml"],
                    help="configs, merged left to right; key=value words override them")
    ap.add_argument("-t", "--train", type=str2bool, const=True, default=True, nargs="?", help="train")
    ap.add_argument("--no-test", type=str2bool, const=True, default=False, nargs="?", help="accepted: no test stage exists")
    ap.add_argument("-p", "--project", help="accepted, not used")
    ap.add_argument("-d", "--debug", type=str2bool, nargs="?", const=True, default=False, help="accepted, not used")
    ap.add_argument("-s", "--seed", type=int, default=23, help="seed of the run and of the epoch orders")
    ap.add_argument("-f", "--postfix", type=str, default="", help="appended to the run folder's name")
    ap.add_argument("-l", "--logdir", type=str, default="logs", help="where run folders are made")
    ap.add_argument("--pretrained_model", type=str, default="", help="a checkpoint holding `state_dict`, loaded with strict=False")
    ap.add_argument("--scale_lr", type=str2bool, nargs="?", const=True, default=True,
                    help="learning rate = accumulate * gpus * batch size * base rate")
    ap.add_argument("--train_from_scratch", type=str2bool, nargs="?", const=True, default=False,
                    help="drop every `model.*` key of the pretrained checkpoint")
    ap.add_argument("--save_top_k", type=int, default=1)
    ap.add_argument("--gpus", type=str, default=None, help="device ids, comma separated (one id)")
    ap.add_argument("--max_epochs", type=int, default=None)
    ap.add_argument("--max_steps", type=int, default=None, help="end this invocation after that many optimizer steps")
    ap.add_argument("--accumulate_grad_batches", type=int, default=None)
    ap.add_argument("--gradient_clip_val", type=float, default=None)
    ap.add_argument("--resume_from_checkpoint", type=str, default=None, help="continue a checkpoint in a NEW run folder")
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16", help="engine storage type (fp16 trains with a GradScaler)")
    ap.add_argument("--no-refresh", dest="no_refresh", action="store_true",
                    help="rebuild the trained weights' 16-bit copies lazily, tensor by tensor, instead of by one launch per step")
    return ap


def parse_args(argv=None):
    """-> (options, dot-list overrides).  Words the parser does not know are overrides when they read `key=value`; an unknown
    `--flag` is an error."""
    ap = get_parser()
    opt, rest = ap.parse_known_args(argv)
    bad = [w for w in rest if w.startswith("-") or "=" not in w]
    if bad:
        ap.error(f"unrecognized arguments: {' '.join(bad)}")
    if opt.name and opt.resume:
        raise ValueError("-n/--name and -r/--resume cannot be specified both. If you want to resume training in a new log folder, "
                         "use -n/--name in combination with --resume_from_checkpoint")
    return opt, rest


def run_folder(opt, now):
    """-> (logdir, checkpoint to continue or None, the configs to merge in order)."""
    default_base = get_parser().get_default("base")
    if opt.resume:
        if not os.path.exists(opt.resume):
            raise ValueError(f"Cannot find {opt.resume}")
        if os.path.isfile(opt.resume):
            logdir = os.path.dirname(os.path.dirname(opt.resume))
            ckpt = opt.resume
        else:
            logdir = opt.resume.rstrip("/")
            ckpt = os.path.join(logdir, "checkpoints", "last.ckpt")
        base = [b for b in opt.base if not (opt.base == default_base and not os.path.exists(b))]    # (a default nobody named)
        return logdir, ckpt, sorted(glob.glob(os.path.join(logdir, "configs", "*.yaml"))) + base
    if opt.name:
        name = "_" + opt.name
    elif opt.base:
        name = "_" + os.path.splitext(os.path.basename(opt.base[0]))[0]
    else:
        name = ""
    return os.path.join(opt.logdir, now + name + opt.postfix), opt.resume_from_checkpoint, list(opt.base)


def split_lightning(raw, opt):
    """The unresolved merged tree -> (project tree, lightning tree) as the reference saves them; the trainer flags given on the
    command line go into `lightning.trainer` (not `max_steps` and `resume_from_checkpoint`: they belong to one invocation)."""
    project = {k: v for k, v in raw.items() if k != "lightning"}
    lightning = dict(raw.get("lightning") or {})
    trainer = dict(lightning.get("trainer") or {})
    for k in TRAINER_FLAGS:
        if getattr(opt, k) is not None and k not in ("max_steps", "resume_from_checkpoint"):
            trainer[k] = getattr(opt, k)
    lightning["trainer"] = trainer
    return project, lightning


def save_configs(cfgdir, now, project, lightning):
    import yaml
    os.makedirs(cfgdir, exist_ok=True)
    for name, tree in (("project", project), ("lightning", {"lightning": lightning})):
        with open(os.path.join(cfgdir, f"{now}-{name}.yaml"), "w") as f:
            yaml.safe_dump(tree, f, sort_keys=False)


def gpu_ids(gpus):
    return [g for g in str(gpus).strip(",").split(",")] if gpus is not None else ["0"]


def learning_rate(opt, base_lr, accumulate, ngpu, batch_size):
    """`train.scaled_lr` with `--scale_lr` (the default), else the base rate; prints what the reference prints."""
    from . import train
    if opt.scale_lr:
        lr = train.scaled_lr(base_lr, accumulate, 1, ngpu, batch_size)
        print("Setting learning rate to {:.2e} = {} (accumulate_grad_batches) * {} (num_nodes) * {} (num_gpus) * {} (batchsize) * "
              "{:.2e} (base_lr)".format(lr, accumulate, 1, ngpu, batch_size, base_lr))
        return lr
    print("++++ NOT USING LR SCALING ++++")
    print(f"Setting learning rate to {base_lr:.2e}")
    return base_lr


def load_pretrained(model, path, from_scratch=False):
    """`state_dict` of the checkpoint at `path` into `model` with strict=False; from_scratch: without its `model.*` keys (the
    UNet keeps its initialisation, the autoencoders and the conditioning stage are loaded)."""
    import torch
    sd = torch.load(path, map_location="cpu")["state_dict"]
    if from_scratch:
        sd = {k: v for k, v in sd.items() if not k.startswith("model.")}
        print("Train from scratch!")
    else:
        print(f"Load {path}!")
    model.load_state_dict(sd, strict=False)
    return sorted(sd)


class DataModuleFromConfig:
    """`data.target: main.DataModuleFromConfig` of the configs: the splits (`datasets`: train / validation / test, whichever are
    given) and their loaders for `train.Trainer.fit`.  `train_batches(epoch, start_batch)` is `train.epoch_loader`'s: the order
    depends on (`seed`, epoch) only; `val_batches()` walks the validation split in order.  Both are `device_loader`s: worker
    processes build raw items, collation runs in the iterating process (README, the worker-process rule)."""

    def __init__(self, batch_size, train=None, validation=None, test=None, wrap=False, num_workers_per_gpu=None, **ignored):
        from .ldm.util import instantiate_from_config
        self.batch_size, self.num_workers, self.wrap, self.seed = int(batch_size), int(num_workers_per_gpu or 0), wrap, 0
        self.dataset_configs = {k: v for k, v in (("train", train), ("validation", validation), ("test", test)) if v is not None}
        self.datasets = {k: instantiate_from_config(v) for k, v in self.dataset_configs.items()}
        print("#### Data #####")
        for k, d in self.datasets.items():
            print(f"{k}, {d.__class__.__name__}, {len(d)}")

    def train_batches(self, epoch, start_batch=0):
        from . import train
        return train.epoch_loader(self.datasets["train"], self.batch_size, self.seed, self.num_workers)(epoch, start_batch)

    def val_batches(self):
        return self.datasets["validation"].device_loader(self.batch_size, self.num_workers)


def main(argv=None):
    opt, overrides = parse_args(argv)
    now = datetime.datetime.now().strftime("%Y-%m-%dT%H-%M-%S")
    logdir, ckpt, bases = run_folder(opt, now)
    from .ldm.util import instantiate_from_config, load_configs, resolve_config
    config, raw = load_configs(bases, overrides)
    project, lightning_raw = split_lightning(raw, opt)
    lightning = resolve_config({**raw, "lightning": lightning_raw})["lightning"]
    trainer_cfg = lightning["trainer"]
    gpus = gpu_ids(trainer_cfg.get("gpus"))
    if len(gpus) > 1:
        raise SystemExit(ONE_GPU.format(n=len(gpus), gpus=trainer_cfg.get("gpus")))
    print(f"Running on GPUs {trainer_cfg.get('gpus', '0')}")

    import signal
    import torch
    import mobi_amd
    from . import dist as mdist, train
    from .test_bench import seed_everything
    mobi_amd.set_engine_dtype({"fp16": torch.float16, "bf16": torch.bfloat16}[opt.dtype])
    torch.cuda.set_device(int(gpus[0] or 0))
    seed_everything(opt.seed)

    model = instantiate_from_config(config["model"])
    if not ckpt:
        if not opt.pretrained_model:
            raise SystemExit("--pretrained_model is needed where nothing is resumed")
        load_pretrained(model, opt.pretrained_model, opt.train_from_scratch)
    model = model.cuda()
    if getattr(model, "monitor", None) is not None:
        print(f"Monitoring {model.monitor} as checkpoint metric.")

    if mdist.world()[0] == 0:
        save_configs(os.path.join(logdir, "configs"), now, project, lightning_raw)
    logger_params = {**IMAGE_LOGGER_DEFAULTS, **((((lightning.get("callbacks") or {}).get("image_logger") or {}).get("params")) or {})}
    image_logger = train.ImageLogger(logdir, **logger_params)

    data = instantiate_from_config(config["data"])
    data.seed = opt.seed
    accumulate = int(trainer_cfg.get("accumulate_grad_batches") or 1)
    print(f"accumulate_grad_batches = {accumulate}")
    model.learning_rate = learning_rate(opt, config["model"]["base_learning_rate"], accumulate, len(gpus), data.batch_size)

    trainer = train.Trainer(model, max_epochs=int(trainer_cfg.get("max_epochs") or 1000), accumulate_grad_batches=accumulate,
                            max_norm=trainer_cfg.get("gradient_clip_val"), scaler=train.GradScaler() if opt.dtype == "fp16" else None,
                            ckpt_dir=os.path.join(logdir, "checkpoints"), save_top_k=opt.save_top_k, seed=opt.seed,
                            every_n_steps=opt.max_steps,          # (the step `--max_steps` ends at leaves a `last.ckpt` for `-r`)
                            max_steps=opt.max_steps, image_logger=image_logger, log_dir=logdir, refresh_weights=not opt.no_refresh)
    try:
        signal.signal(signal.SIGUSR1, lambda *a: trainer.request_save())
        signal.signal(signal.SIGUSR2, signal.SIG_IGN)
    except ValueError:                                 # (not the main thread: no handlers)
        pass
    if opt.train:
        trainer.fit(data.train_batches, data.val_batches if "validation" in data.datasets else None, resume=ckpt or None)
    print(f"The run is in {logdir}")
    return trainer


if __name__ == "__main__":
    main()
