"""GPU: `train.WeightRefresher` -- one `mobi_repack_multi` launch after an optimizer update instead of the lazy per-tensor re-pack
-- changes no number anywhere: every comparison here is `torch.equal` between a run with `refresh=` and the same run without.

Two networks, both fp16: the reduced LatentDiffusion of tests/test_gpu_grad_accum.py (model_channels 64, latent 16 x 16, two camera /
lidar pairs: 432 block tensors + the box embedder + `bbox_uncond_vector`) for the optimizer paths, and the reduced full model of
tests/test_gpu_image_logger.py (VAEs, CLIP tower, EMA shadows) where sampling, `ema_scope` and the Trainer are involved."""
import pytest
import torch

from oracle import weights as W
from tests.test_gpu_grad_accum import _latent_diffusion
from tests.test_gpu_image_logger import _Case, _assert_same_final, _assert_same_log, _batch, _clone, _final, _log, _model, _seed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    """(ld, start state, step inputs) of the reduced network, shared: every run begins with `load_state_dict(start)`."""
    import mobi_amd
    mobi_amd.set_engine_dtype(torch.float16)
    n, side = 4, 16
    ld = _latent_diffusion(n, side)
    x = W.synth_input("tl.x", (n, 9, side, side)).cuda()
    bbox = (W.synth_input("gs.bbox", (n, 8, 3), kind="uniform") * 0.5 + 0.5).cuda()
    ld.get_input = lambda batch, k, **kw: {"z": x, "cond": {"ref_image": None, "ref_bbox": bbox.clone()}}
    ld.u_cond_percent = 0.0
    start = {k: v.detach().clone() for k, v in ld.state_dict().items()}
    noise = [W.synth_input(f"wr.noise{i}", (n, 4, side, side)).cuda() for i in range(8)]
    ts = [torch.tensor(v, dtype=torch.long).cuda() for v in ([741, 741, 21, 21], [5, 5, 999, 999], [400, 400, 87, 87])]
    yield ld, start, noise, ts
    mobi_amd.set_engine_dtype(torch.float16)


def _snapshot(ld, opt, losses):
    out = {"param/" + k: p.detach().clone() for k, p in opt.params.items()}
    for k, (m, v) in opt.state.items():
        out["exp_avg/" + k], out["exp_avg_sq/" + k] = m.clone(), v.clone()
    out.update({"grad/" + k: g.detach().clone() for k, g in ld.adapter_grads.items()})
    for i, d in enumerate(losses):
        out.update({f"loss{i}/" + k: v.detach().clone() for k, v in d.items()})
    return out


def _assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def _run(net, refresh, script, micro=1):
    """`script`: a list of "step", "load" (load_state_dict of the start values), "move" (one trained weight gets new storage),
    "skip" (a step on a non-finite gradient), "bf16" / "fp16" (the engine dtype) -> (snapshot, refresher, optimizer)."""
    import mobi_amd
    from mobi_amd import train
    ld, start, noise, ts = net
    mobi_amd.set_engine_dtype(torch.float16)
    ld.load_state_dict(start)
    opt = ld.configure_optimizers()
    s = train.GradScaler(init_scale=None)
    r = train.WeightRefresher(ld, list(opt.params)) if refresh else None
    acc = train.GradAccumulator(opt, micro) if micro > 1 else None
    losses, it = [], 0
    for what in script:
        if what == "step":
            if acc is None:
                ld.training_step({}, 0, t=ts[it % 3], noise=noise[it], scaler=s)
                losses.append(dict(ld.loss_dict))
                res = opt.step_scaled(ld.adapter_grads, scaler=s, refresh=r)
            else:
                for j in range(micro):
                    ld.training_step({}, 0, t=ts[(it + j) % 3], noise=noise[micro * it + j], scaler=s, allreduce=False)
                    losses.append(dict(ld.loss_dict))
                    acc.add(ld.adapter_grads, scale=ld.adapter_grads_scale)
                res = acc.step(scaler=s, refresh=r)
            assert res.found_inf is False
            it += 1
        elif what == "skip":
            bad = {k: g.clone() for k, g in ld.adapter_grads.items()}
            next(iter(bad.values())).view(-1)[0] = float("inf")
            launches = r.launches if r else 0
            caches = [dict(m.__dict__.get("_pack_cache", {})) for m, _ in r.layers] if r else []
            assert opt.step_scaled(bad, scaler=s, refresh=r).found_inf is True
            if r:
                assert r.launches == launches
                assert all(sorted(m._pack_cache) == sorted(c) and all(m._pack_cache[t] is c[t] for t in c)
                           for (m, _), c in zip(r.layers, caches))
        elif what == "load":
            ld.load_state_dict(start)
        elif what == "move":
            p = ld.model.diffusion_model.get_parameter(next(n for n in train.trainable_names(ld.model.diffusion_model)
                                                            if n.endswith("to_q.weight")))
            p.data = p.data.clone()
            opt._multi = train._TableCache()           # (the optimizer's own tables hold addresses: `AdamW.load_state_dict` does this)
        else:
            mobi_amd.set_engine_dtype({"bf16": torch.bfloat16, "fp16": torch.float16}[what])
    return _snapshot(ld, opt, losses), r, opt


@pytest.fixture(scope="module")
def plain3(net):
    """Three unrefreshed steps: the reference of the parity tests, computed once."""
    return _run(net, False, ["step"] * 3)[0]


def test_three_steps_are_bit_equal_with_refresh(net, plain3):
    got, r, opt = _run(net, True, ["step"] * 3)
    kinds = [kind for _, kind in r.layers]
    assert r.launches == 3 and (kinds.count("mfma"), kinds.count("forward"), kinds.count("skinny")) == (240 - 32, 32, 4)
    _assert_same(got, plain3)
    assert any(not torch.equal(got["param/" + k], net[1][k].cuda()) for k in opt.params)


def test_three_windows_of_two_micro_batches_are_bit_equal(net):
    want = _run(net, False, ["step"] * 3, micro=2)[0]
    got, r, _ = _run(net, True, ["step"] * 3, micro=2)
    assert r.launches == 3
    _assert_same(got, want)


def test_the_next_step_hits_the_installed_copies(net, monkeypatch):
    """`mobi_tile_weights` is counted by wrapping the library attribute.  `ops.linear_wgrad` tiles an ACTIVATION operand (x^T) with
    the same function once per weight gradient, step after step, refreshed or not: those calls are counted apart (made while
    `linear_wgrad` runs) and must be equal in number in both runs.  Of the others -- the weight images -- the refreshed step makes
    none, the unrefreshed step one per tiled image the refresher's table holds."""
    from mobi_amd import _lib, ops, train
    ld, _, noise, ts = net
    lib = _lib.load()
    calls, inside = [], [False]
    real, real_wgrad = lib.mobi_tile_weights, ops.linear_wgrad
    monkeypatch.setattr(lib, "mobi_tile_weights", lambda *a: calls.append(inside[0]) or real(*a), raising=False)

    def wgrad(*a, **k):
        inside[0] = True
        try:
            return real_wgrad(*a, **k)
        finally:
            inside[0] = False
    monkeypatch.setattr(ops, "linear_wgrad", wgrad)
    activation_side = None
    for refresh in (False, True):
        _, r, opt = _run(net, refresh, ["step"])
        del calls[:]
        ld.training_step({}, 0, t=ts[1], noise=noise[1], scaler=train.GradScaler(init_scale=None))
        weight_side = sum(not c for c in calls)
        if not refresh:
            activation_side = sum(calls)
            probe = train.WeightRefresher(ld, list(opt.params))
            probe.refresh()
            tiled = sum(im[name] is not None for im in probe.table.images for name in ("wt", "wt_t"))
            assert weight_side == tiled > 0
            continue
        assert weight_side == 0 and sum(calls) == activation_side
        lo = r.table.buffer.data_ptr()
        hi = lo + r.table.buffer.numel() * 2
        for (m, kind), im in zip(r.layers, r.table.images):
            if kind == "skinny":
                w, b = m.skinny()
                assert w is im["w"] and b.data_ptr() == m.bias.data_ptr() and b.dtype == torch.float32
                continue
            pw = m.packed()
            assert pw is m._pack_cache["mfma"][1] and pw.w is im["w"] and pw.wt is im["wt"]
            pt = train._packed_t(m) if kind == "mfma" else None
            assert (pt.w is im["w_t"] and pt.wt is im["wt_t"]) if pt else (im["w_t"] is None and im["wt_t"] is None)
            assert (pw.bias is None) == (m.bias is None) and (pw.bias is None or pw.bias.data_ptr() == m.bias.data_ptr())
            want = ops.pack_linear(m.weight, m.bias, torch.float16, m.weight.device)
            assert (pw.kh, pw.kw, pw.cin, pw.cout, pw.n_packed, pw.geglu) == \
                   (want.kh, want.kw, want.cin, want.cout, want.n_packed, want.geglu)
            assert (pw.wt is None) == (want.wt is None) and torch.equal(pw.w, want.w)
            for t in (pw.w, pw.wt) + ((pt.w, pt.wt) if pt else ()):
                assert t is None or lo <= t.data_ptr() < hi


def test_a_skipped_step_launches_nothing_and_keeps_the_caches(net):
    want = _run(net, False, ["step", "skip", "step"])[0]
    got, r, _ = _run(net, True, ["step", "skip", "step"])
    assert r.launches == 2
    _assert_same(got, want)


def test_load_state_dict_and_a_moved_parameter_rebuild_the_table(net):
    script = ["step", "load", "step", "move", "step"]
    want = _run(net, False, script)[0]
    tables = []
    import mobi_amd.train as train
    real = train.ops.RepackTable
    try:
        train.ops.RepackTable = lambda *a, **k: tables.append(real(*a, **k)) or tables[-1]
        got, r, _ = _run(net, True, script)
    finally:
        train.ops.RepackTable = real
    assert len(tables) == 2 and r.table is tables[1] and tables[0].ptrs != tables[1].ptrs
    _assert_same(got, want)


def test_an_engine_dtype_change_rebuilds_the_table(net):
    script = ["step", "bf16", "step", "step", "fp16", "step"]
    want = _run(net, False, script)[0]
    got, r, _ = _run(net, True, script)
    assert r.table.dtype == torch.float16 and r.launches == 4
    _assert_same(got, want)
    _, r, _ = _run(net, True, ["step", "bf16", "step"])
    assert r.table.dtype == torch.bfloat16 and r.table.buffer.dtype == torch.bfloat16


# ----------------------------------------------------------------------------------------------------------------------
# the full reduced model: EMA swaps, sampling, the Trainer
def _steps_with_ema(refresh):
    from mobi_amd import train
    model, batches = _model(19, use_ema=True), [_batch("a"), _batch("t0"), _batch("t1")]
    opt = model.configure_optimizers()
    opt = opt[0][0] if isinstance(opt, tuple) else opt
    s = train.GradScaler(init_scale=None)
    r = train.WeightRefresher(model, list(opt.params)) if refresh else None
    model.train()
    _seed(3)
    losses = []

    def step(i):
        model.training_step(_clone(batches[i]), i, scaler=s)
        losses.append(dict(model.loss_dict))
        assert not opt.step_scaled(model.adapter_grads, scaler=s, refresh=r).found_inf
        model.on_train_batch_end()
    step(0)
    with model.ema_scope():                        # the shadows are live: every installed copy is stale and is rebuilt lazily
        step(1)
    step(2)                                        # the weights are back: stale again, and re-installed by this step's refresh
    out = _snapshot(model, opt, losses)
    out.update({"ema/" + k: b.clone() for k, b in model.model_ema.named_buffers()})
    return out, model, r


def test_steps_inside_and_after_ema_scope_and_sampling_after_them():
    want, _, _ = _steps_with_ema(False)
    got, model, r = _steps_with_ema(True)
    assert r.launches == 3
    _assert_same(got, want)
    # sampling after refreshed steps reads the stepped weights (tests/test_gpu_image_logger.py's check, with refresh on)
    batch = _batch("a")
    model.eval()
    after = _log(model, batch, 7, ddim_steps=2)
    fresh = _model(23, use_ema=True)
    fresh.load_state_dict(model.state_dict())
    _assert_same_log(after, _log(fresh, batch, 7, ddim_steps=2))


@pytest.mark.parametrize("k", [1, 2], ids=["k1", "k2"])
def test_the_trainer_ends_bit_equal_with_refresh_weights(k):
    from mobi_amd import train
    case = _Case(k)

    def fit(refresh):
        tr = train.Trainer(_model(21, use_ema=True), max_epochs=2, accumulate_grad_batches=k, scaler=train.GradScaler(init_scale=None),
                           seed=3, log_every=2, refresh_weights=refresh)
        return tr.fit(case.train_batches, case.val_batches)
    plain, fast = fit(False), fit(True)
    assert plain.refresher is None and fast.refresher.launches == 4 == fast.global_step
    assert fast.history == plain.history and fast.val_history == plain.val_history
    _assert_same_final(_final(fast), _final(plain))
