"""Checkpoints of a training run: written while training goes on, in the reference's layout, with an exact resume.

The file is a `torch.save` dict that the reference's readers (`torch.load(path)["state_dict"]`, scripts/inference_test_bench.py)
and `init_from_ckpt` load:

    "state_dict"        the model's state_dict(), the reference's keys, CPU tensors
    "optimizer_states"  [train.AdamW.state_dict()]        "lr_schedulers"  [train.LambdaLR.state_dict()]
    "global_step", "epoch"                                (the position the run continues at)
    "mobi_amd"          {"format": 1, "scaler", "batch_in_epoch", "monitor", "extra",
                         "rng": {"python", "numpy", "torch", "device"},
                         "digests": {name: [digest, numel]}}    every fp32 tensor of state_dict and of both moments

A moment's name in "digests" is `optimizer.<index>.exp_avg` / `optimizer.<index>.exp_avg_sq`, <index> its key in the optimizer's
"state".  The digest of a tensor is sum_i uint64(u_i ^ 0x9E3779B9) * uint64((2 i + 1) mod 2^32) mod 2^64 over its 32-bit words
(`digest_host`; on the device `mobi_snapshot_multi` computes it inside the launch that takes the snapshot).

    python -m mobi_amd.checkpoint verify FILE

checks a file's digests on the host (numpy): a tool over a file, no engine, no device."""
import copy
import os
import random
import sys
import threading

import numpy as np
import torch

FORMAT = 1
DIGEST_XOR = 0x9E3779B9


class NonFiniteState(RuntimeError):
    """`Checkpointer.save`: a tensor of the training state holds inf or nan; nothing was written."""


class DigestMismatch(RuntimeError):
    """`Checkpointer.load`: a tensor on the device does not have the digest the file recorded for it."""


def digest_host(tensor):
    """The digest of an fp32 tensor (torch, CPU; or a numpy array) on the host: an int in [0, 2^64)."""
    a = tensor.detach().contiguous().numpy() if isinstance(tensor, torch.Tensor) else np.ascontiguousarray(tensor)
    assert a.dtype == np.float32, a.dtype
    u = a.reshape(-1).view(np.uint32)
    n = u.size
    with np.errstate(over="ignore"):
        return int(((u ^ np.uint32(DIGEST_XOR)).astype(np.uint64)
                    * ((np.uint64(2) * np.arange(n, dtype=np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF))).sum(dtype=np.uint64))


def _numpy_rng_get():
    """numpy's global generator state in plain types and one tensor: the file stays loadable with `torch.load`'s default
    (weights-only) unpickler, which `init_from_ckpt` uses."""
    name, keys, pos, has_gauss, cached = np.random.get_state()
    return {"name": str(name), "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos), "has_gauss": int(has_gauss),
            "cached_gaussian": float(cached)}


def _numpy_rng_set(st):
    np.random.set_state((st["name"], st["keys"].numpy().astype(np.uint32), st["pos"], st["has_gauss"], st["cached_gaussian"]))


def rng_get(device=None):
    """The four generator states a run depends on: Python `random`, numpy, torch CPU and (device given) the torch device generator."""
    return {"python": random.getstate(), "numpy": _numpy_rng_get(), "torch": torch.get_rng_state(),
            "device": None if device is None else torch.cuda.get_rng_state(device)}


def rng_set(rng, device=None):
    random.setstate(rng["python"])
    _numpy_rng_set(rng["numpy"])
    torch.set_rng_state(rng["torch"])
    if device is not None and rng.get("device") is not None:
        torch.cuda.set_rng_state(rng["device"], device)


def _plain(x):
    """numpy scalars (a schedule's rate, a mean) as python numbers, through dicts, lists and tuples: see `_numpy_rng_get`."""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_plain(v) for v in x)
    return x.item() if isinstance(x, np.generic) else x


def _digested(t):
    return isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.numel() > 0


def file_tensors(ckpt):
    """{name: tensor} of everything a checkpoint dict's "digests" may speak of: the state_dict and both moments."""
    out = dict(ckpt["state_dict"])
    for opt in ckpt.get("optimizer_states", [])[:1]:
        for index, entry in opt["state"].items():
            out[f"optimizer.{index}.exp_avg"] = entry["exp_avg"]
            out[f"optimizer.{index}.exp_avg_sq"] = entry["exp_avg_sq"]
    return out


def verify_file(path):
    """-> (names checked, [(name, why)] that failed) of the file's recorded digests against `digest_host` of its tensors."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if "mobi_amd" not in ckpt:
        raise ValueError(f"{path} has no \"mobi_amd\" entry: a reference or Lightning checkpoint, which records no digests")
    tensors, bad = file_tensors(ckpt), []
    digests = ckpt["mobi_amd"]["digests"]
    for name, (digest, numel) in digests.items():
        t = tensors.get(name)
        if t is None:
            bad.append((name, "recorded, but not in the file"))
        elif t.numel() != numel:
            bad.append((name, f"{t.numel()} elements, {numel} recorded"))
        elif digest_host(t) != digest:
            bad.append((name, f"digest {digest_host(t):#018x}, {digest:#018x} recorded"))
    for name, t in tensors.items():
        if _digested(t) and name not in digests:
            bad.append((name, "an fp32 tensor without a recorded digest"))
    return len(digests), bad


class AtomicWriter:
    """One background write at a time: `submit(make, path)` starts a thread that calls `make()` for the object, `torch.save`s it to
    `path + ".tmp"` and renames that onto `path`; a failure removes the tmp file, leaves `path` as it was and is re-raised by
    `wait()`.  `submit` waits for the write before it."""

    def __init__(self):
        self._thread, self._error = None, None

    def _run(self, make, path):
        tmp = path + ".tmp"
        try:
            obj = make()
            torch.save(obj, tmp)
            os.replace(tmp, path)
        except BaseException as e:                     # (kept for wait(); the thread must not die silently)
            self._error = e
            try:
                os.remove(tmp)
            except OSError:
                pass

    def submit(self, make, path):
        self.wait()
        self._thread = threading.Thread(target=self._run, args=(make, path), name="mobi-checkpoint-writer")
        self._thread.start()

    def wait(self):
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self._error is not None:
            e, self._error = self._error, None
            raise e


class _Plan:
    """What a save of one set of tensors needs, built once: the pair table (every fp32 tensor; a destination in the staging buffer
    for the mutable ones, none for the frozen), the staging buffer and the pinned host memory."""


class Checkpointer:
    """save / wait / load for (model, optimizer, scheduler, scaler, accumulator) -- see the module's docstring for the file.

    `save` takes a consistent copy of everything a step mutates (trained parameters, both moments, every EMA shadow) in ONE launch
    on the current stream, `mobi_snapshot_multi`, into a flat staging buffer (sorted names, 16-byte aligned starts: the rule of
    `dist.gradient_bucket_layout`); the same launch digests every other fp32 tensor of the state_dict in place.  One read-back
    (16 bytes per tensor) is the host sync of a save; then the staging buffer and the frozen tensors go to pinned host memory on
    a side stream and a background thread writes the file.  `save` returns once those copies are enqueued: the next step may
    start at once and the file does not see its writes."""

    def __init__(self, model, optimizer, scheduler=None, scaler=None, accumulator=None):
        self.model, self.optimizer, self.scheduler, self.scaler, self.accumulator = model, optimizer, scheduler, scaler, accumulator
        self._writer = AtomicWriter()
        self._plan = None
        self._side = None

    # ------------------------------------------------------------------------------------------------------------------
    def _named_tensors(self):
        """-> ([(name, tensor)] in the file's naming: the model's state_dict, then both moments of every optimizer entry; copies).
        Every fp32 tensor listed is dense: one that is not (a channels_last weight) is listed as a dense copy made here, on the
        current stream, and named in `copies` -- it is digested and checked for inf / nan like every other, in the element
        order the file holds it in."""
        named = [(k, v.detach()) for k, v in self.model.state_dict().items()]
        for index, n in enumerate(self.optimizer.params):
            if n in self.optimizer.state:
                m, v = self.optimizer.state[n]
                named += [(f"optimizer.{index}.exp_avg", m), (f"optimizer.{index}.exp_avg_sq", v)]
        copies = {k for k, t in named if _digested(t) and not t.is_contiguous()}
        return [(k, t.contiguous() if k in copies else t) for k, t in named], copies

    def _mutable_ptrs(self):
        ptrs = {p.data_ptr() for p in self.optimizer.params.values()}
        ema = getattr(self.model, "model_ema", None)
        if ema is not None:
            ptrs |= {b.data_ptr() for b in ema.buffers()}
        return ptrs

    def _build_plan(self, named, copies, key):
        from . import dist as mdist, ops
        plan = _Plan()
        plan.key = key
        mutable = self._mutable_ptrs()
        fp32 = [(k, t) for k, t in named if _digested(t)]
        plan.names = [k for k, _ in fp32]
        plan.other = [k for k, t in named if not _digested(t)]                  # integer buffers, empty tensors
        # (a dense copy is staged like a mutable tensor: the launch, on this stream, is then the last to read the temporary)
        plan.staged = sorted(k for k, t in fp32 if t.data_ptr() in mutable or k.startswith("optimizer.") or k in copies)
        staged = set(plan.staged)
        plan.frozen = sorted(k for k, t in fp32 if k not in staged)
        by_name = dict(fp32)
        device = fp32[0][1].device
        one_bucket = 1 << 62
        plan.stage_layout, lengths = mdist.gradient_bucket_layout({k: by_name[k].numel() for k in plan.staged}, one_bucket)
        plan.frozen_layout, flen = mdist.gradient_bucket_layout({k: by_name[k].numel() for k in plan.frozen}, one_bucket)
        n_stage, n_frozen = (lengths or [0])[0], (flen or [0])[0]
        plan.staging = torch.empty(max(n_stage, 4), dtype=torch.float32, device=device)
        plan.pinned_stage = torch.empty(max(n_stage, 4), dtype=torch.float32).pin_memory()
        plan.pinned_frozen = torch.empty(max(n_frozen, 4), dtype=torch.float32).pin_memory()
        dst = []
        for k, t in fp32:
            if k in plan.stage_layout:
                _, off, n = plan.stage_layout[k]
                dst.append(plan.staging[off:off + n])
            else:
                dst.append(None)
        plan.table = ops.MultiTensorTable([[t.reshape(-1) for _, t in fp32], dst])
        return plan

    def _check_records(self, names, records, what):
        bad = [k for k, (_, nonfinite) in zip(names, records) if nonfinite]
        if bad:
            raise NonFiniteState(f"{what}: {len(bad)} tensors hold inf or nan (first: {bad[:4]}); nothing was written")

    def save(self, path, global_step, epoch, batch_in_epoch=0, extra=None, monitor=None):
        """-> None, after the copies to the host are enqueued; `wait()` joins the writer.  Raises `NonFiniteState` (and writes
        nothing: the file at `path` stays as it was) where a tensor holds inf or nan, and RuntimeError inside `ema_scope()`
        (weights and shadows have traded places there) or inside an accumulation window."""
        from . import ops
        ema = getattr(self.model, "model_ema", None)
        if ema is not None and getattr(ema, "swapped", False):
            raise RuntimeError("save() inside ema_scope(): the weights and their shadows have traded places")
        if self.accumulator is not None:
            self.accumulator.state_dict()              # raises inside a window
        self.wait()                                    # the staging buffer and the pinned memory are the previous save's until then
        named, copies = self._named_tensors()
        key = tuple((k, t.data_ptr(), t.numel()) for k, t in named)             # (never equal where there are dense copies)
        if self._plan is None or self._plan.key != key:
            self._plan = self._build_plan(named, copies, key)
        plan, by_name = self._plan, dict(named)
        records = ops.read_snapshot_records(ops.snapshot_multi(plan.table))     # the launch; the one host sync of a save
        self._check_records(plan.names, records, "save")
        digests = {k: [d, by_name[k].numel()] for k, (d, _) in zip(plan.names, records)}
        others = {k: by_name[k].clone() for k in plan.other}                    # (`num_updates` and its like: a few words)
        # everything the writer needs from the host side, as it is NOW
        head = {"optimizer": self.optimizer.state_dict(), "global_step": int(global_step), "epoch": int(epoch),
                "scheduler": None if self.scheduler is None else _plain(copy.deepcopy(self.scheduler.state_dict())),
                "mobi_amd": {"format": FORMAT, "scaler": None if self.scaler is None else _plain(copy.deepcopy(self.scaler.state_dict())),
                             "batch_in_epoch": int(batch_in_epoch), "monitor": _plain(copy.deepcopy(monitor)), "extra": _plain(copy.deepcopy(extra)),
                             "rng": rng_get(plan.staging.device),
                             "digests": digests}}
        head["optimizer"] = {"state": {i: {"step": e["step"].clone()} for i, e in head["optimizer"]["state"].items()},
                             "param_groups": _plain(copy.deepcopy(head["optimizer"]["param_groups"]))}
        if self._side is None:
            self._side = torch.cuda.Stream(plan.staging.device)
        taken = torch.cuda.Event()
        taken.record()
        with torch.cuda.stream(self._side):
            self._side.wait_event(taken)
            plan.pinned_stage.copy_(plan.staging, non_blocking=True)
            for k, (_, off, n) in plan.frozen_layout.items():
                plan.pinned_frozen[off:off + n].copy_(by_name[k].reshape(-1), non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
        for t in others.values():
            t.record_stream(self._side)
        shapes = {k: tuple(by_name[k].shape) for k in plan.names}
        order = [k for k, _ in named]
        side = self._side

        def make():
            torch.cuda.set_device(side.device)
            copied.synchronize()
            host = {}
            for k, (_, off, n) in plan.stage_layout.items():
                host[k] = plan.pinned_stage[off:off + n].clone().view(shapes[k])
            for k, (_, off, n) in plan.frozen_layout.items():
                host[k] = plan.pinned_frozen[off:off + n].clone().view(shapes[k])
            with torch.cuda.stream(side):
                for k, t in others.items():
                    host[k] = t.cpu()
            opt = head["optimizer"]
            for i, e in opt["state"].items():
                e["exp_avg"], e["exp_avg_sq"] = host[f"optimizer.{i}.exp_avg"], host[f"optimizer.{i}.exp_avg_sq"]
            out = {"state_dict": {k: host[k] for k in order if not k.startswith("optimizer.")}, "optimizer_states": [opt],
                   "lr_schedulers": [] if head["scheduler"] is None else [head["scheduler"]],
                   "global_step": head["global_step"], "epoch": head["epoch"], "mobi_amd": head["mobi_amd"]}
            return out
        self._writer.submit(make, path)

    def wait(self):
        """Joins the writer; re-raises what it failed with (the file at `path` is then as it was before the save)."""
        self._writer.wait()

    # ------------------------------------------------------------------------------------------------------------------
    def load(self, path, strict_digests=True):
        """Everything `save` wrote, back into the objects of this Checkpointer, then ONE `mobi_snapshot_multi` without destinations
        over what now lies on the device against the file's digests (file, host copy and upload in one check): `DigestMismatch`
        names the first tensors that differ (strict_digests=False: printed instead).  A file without a "mobi_amd" entry is a
        reference / Lightning checkpoint: weights, and optimizer / scheduler states where present; no digests to check.
        -> {"global_step", "epoch", "batch_in_epoch", "extra", "monitor"}."""
        from . import ops
        self.wait()
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        self.model.load_state_dict(ckpt["state_dict"], strict=True)
        if ckpt.get("optimizer_states"):
            self.optimizer.load_state_dict(ckpt["optimizer_states"][0])
        if self.scheduler is not None and ckpt.get("lr_schedulers"):
            self.scheduler.load_state_dict(ckpt["lr_schedulers"][0])
        if self.accumulator is not None:
            self.accumulator.load_state_dict({})
        own = ckpt.get("mobi_amd")
        at = {"global_step": int(ckpt.get("global_step", 0)), "epoch": int(ckpt.get("epoch", 0)), "batch_in_epoch": 0, "extra": None,
              "monitor": None}
        if own is None:
            print(f"{path}: no \"mobi_amd\" entry (a reference / Lightning checkpoint): weights and optimizer state loaded, "
                  "no digests to check, RNG and loss scale left as they are")
            return at
        if own["format"] != FORMAT:
            raise ValueError(f"{path}: checkpoint format {own['format']!r}, this reader knows {FORMAT}")
        if self.scaler is not None and own.get("scaler") is not None:
            self.scaler.load_state_dict(own["scaler"])
        named = [(k, t) for k, t in self._named_tensors()[0] if _digested(t)]
        rng_set(own["rng"], named[0][1].device)
        table = ops.MultiTensorTable([[t.reshape(-1) for _, t in named], [None] * len(named)])
        records = ops.read_snapshot_records(ops.snapshot_multi(table))
        digests, bad = own["digests"], []
        for (k, t), (d, _) in zip(named, records):
            if k not in digests:
                bad.append(f"{k}: no digest in the file")
            elif digests[k][1] != t.numel() or digests[k][0] != d:
                bad.append(f"{k}: digest {d:#018x} on the device, {digests[k][0]:#018x} recorded")
        missing = sorted(set(digests) - {k for k, _ in named})
        bad += [f"{k}: recorded, but not loaded" for k in missing]
        if bad:
            text = f"{path}: {len(bad)} tensors do not match their recorded digests (first: {bad[:3]})"
            if strict_digests:
                raise DigestMismatch(text)
            print(text)
        at.update(batch_in_epoch=int(own["batch_in_epoch"]), extra=own.get("extra"), monitor=own.get("monitor"))
        return at


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2 or argv[0] != "verify":
        print("usage: python -m mobi_amd.checkpoint verify FILE", file=sys.stderr)
        return 2
    count, bad = verify_file(argv[1])
    for name, why in bad:
        print(f"MISMATCH {name}: {why}")
    print(f"{argv[1]}: {count} digests, {len(bad)} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
