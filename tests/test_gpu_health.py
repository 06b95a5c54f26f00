"""GPU: numeric health -- `mobi_tensor_health` against the numpy definition (exact), its independence of order and company, the
probe (it changes nothing; its rows are what torch computes on kept clones; it names the launch that overflowed), the weight
audit, the heavy-tailed stand-in and the probed test-bench run.  Every comparison is exact: counts and bit patterns are integers."""
import os

import numpy as np
import pytest
import torch

from oracle import sampler as osampler, unet as ounet, vae as ovae, weights as W
from tests import health_cases as hc
from tests.test_gpu_models import _unet, _vae

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 7, 8, 63, 64, 65, 4095, 4096, 4097, 100003]
OFFSETS = {"fp16": [0, 1, 3, 5, 7], "bf16": [0, 1, 3, 5, 7], "fp32": [0, 1, 3]}
NAMES = ["fp16", "bf16", "fp32"]
BLOCK = 8192          # elements per block of a launch this small (csrc/health.hip: kHealthGrain)


def _case_list():
    """70 tensors as host bit patterns: (name, offset, bits).  Even entries are scaled to 0.3 of the dtype maximum (some elements
    near the ceiling, a few past it), odd entries are N(0, 1) (none)."""
    rng = np.random.default_rng(20)
    cases = []
    for k in range(70):
        name = NAMES[k % 3]
        n = LENGTHS[k % 10]
        off = OFFSETS[name][(k // 3) % len(OFFSETS[name])]
        with np.errstate(over="ignore"):                           # (fp32 at 0.3 of its maximum: a few products are inf, on purpose)
            v = rng.standard_normal(n).astype(np.float32) * np.float32(0.3 * hc.MAX[name] if k % 2 == 0 else 1.0)
        t = torch.from_numpy(v).to(hc.TORCH[name])
        bits = t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().view(hc.LAYOUT[name][2]).copy()
        cases.append((name, off, bits))
    return cases


def _upload(cases):
    """-> device tensors that start `offset` elements into a larger buffer."""
    out = []
    for name, off, bits in cases:
        buf = torch.zeros(len(bits) + 8, dtype=hc.TORCH[name], device="cuda")
        t = buf[off:off + len(bits)]
        t.copy_(hc.torch_from_bits(name, bits))
        assert t.is_contiguous() and t.data_ptr() == buf.data_ptr() + off * buf.element_size()
        out.append(t)
    return out


def _want(cases, near=0.5):
    from mobi_amd import health
    return [health.tensor_health_ref(bits, name, np.float32(near * hc.MAX[name])) for name, _, bits in cases]


def _measure(tensors, near=0.5):
    from mobi_amd import ops
    return ops.read_tensor_health(ops.tensor_health(tensors, near))


def test_kernel_against_the_numpy_definition():
    cases = _case_list()
    assert len(cases) == 70                                        # the Python layer splits 64 + 6
    want = _want(cases)
    got = _measure(_upload(cases))
    assert got == want
    nears = [w["near"] for w in want]
    assert any(n > 0 for n in nears) and any(n == 0 for n in nears) and any(w["inf"] > 0 for w in want)
    # every special value in turn at the first and last element and on both sides of a block boundary, in every tensor at once
    for name in NAMES:
        p = hc.patterns(name)
        near_pattern = p["max"] - (1 << hc.LAYOUT[name][1])       # exactly half the maximum = near_abs
        assert hc.value_of(name, near_pattern) == np.float32(0.5 * hc.MAX[name])
    checked = 0
    for s in range(12):
        for where in ("first", "last", "before", "after"):
            planted = []
            for name, off, bits in cases:
                p = hc.patterns(name)
                label, pattern = hc.specials(name, p["max"] - (1 << hc.LAYOUT[name][1]))[s]
                pos = {"first": 0, "last": len(bits) - 1, "before": BLOCK - 1, "after": BLOCK}[where]
                b = bits
                if pos < len(bits):
                    b = bits.copy()
                    b[pos] = pattern
                planted.append((name, off, b))
            got, want = _measure(_upload(planted)), _want(planted)
            assert got == want, (s, where, [i for i in range(70) if got[i] != want[i]])
            checked += 1
    assert checked == 48


def test_records_do_not_depend_on_order_or_company():
    from mobi_amd import ops
    cases = _case_list()
    tensors = _upload(cases)
    a = ops.tensor_health(tensors).cpu()
    b = ops.tensor_health(tensors).cpu()
    assert torch.equal(a, b)
    perm = np.random.default_rng(3).permutation(len(tensors))
    c = ops.tensor_health([tensors[i] for i in perm]).cpu()
    assert torch.equal(c, a[torch.from_numpy(perm)])
    alone = torch.cat([ops.tensor_health([t]) for t in tensors]).cpu()     # each alone: another grid, the same record
    assert torch.equal(alone, a)
    assert _measure(tensors) == _want(cases)


# --------------------------------------------------------------------------------------
# the probe
# --------------------------------------------------------------------------------------
def _setup(dtype, seed=9):
    """The reduced UNet (model_channels 64, latent 16 x 16, batch 4 = 2 objects) behind a sampler's model, and its inputs."""
    import mobi_amd
    mobi_amd.set_engine_dtype(dtype)
    side, b = 16, 4
    cfg = ounet.UNetConfig(model_channels=64)
    net = _unet(cfg, side)
    net.load_state_dict(W.synth_state_dict(ounet.unet_param_shapes(cfg), seed))
    net = net.cuda().eval()
    sch = osampler.Schedule(2)

    class Model(torch.nn.Module):
        num_timesteps = 1000

        def __init__(self):
            super().__init__()
            self.net = net
            for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev"):
                self.register_buffer(k, torch.from_numpy(sch.buffers[k]))

        @property
        def device(self):
            return self.betas.device

        def apply_model(self, x, t, c):
            return self.net(x, t, context=c)

    i = dict(x=W.synth_input("h.x", (b, 4, side, side)).cuda(), inp=W.synth_input("h.inp", (b, 4, side, side)).cuda(),
             msk=(W.synth_input("h.mask", (b, 1, side, side)) > 0).float().cuda(), cond=W.synth_input("h.cond", (b, 2, 768)).cuda(),
             t=torch.full((b,), 500, dtype=torch.long, device="cuda"))
    return Model().cuda(), net, i


def _forward(net, i):
    with torch.no_grad():
        return net([i["x"], i["inp"], i["msk"]], i["t"], context=i["cond"])


def _ddim2(model, i):
    from mobi_amd.ldm.models.diffusion.ddim import DDIMSampler
    with torch.no_grad():
        out, _ = DDIMSampler(model).sample(S=2, batch_size=4, shape=[4, 16, 16], conditioning=i["cond"], verbose=False, x_T=i["x"],
                                           test_model_kwargs={"inpaint_image": i["inp"], "inpaint_mask": i["msk"]})
    return out


def _unet_paths(net):
    from mobi_amd.ldm.modules.attention import BasicTransformerBlock, SpatialTransformer
    from mobi_amd.ldm.modules.diffusionmodules.openaimodel import Downsample, ResBlock, Upsample
    kinds = (ResBlock, SpatialTransformer, BasicTransformerBlock, Upsample, Downsample)
    return ["UNetModel." + n for n, m in net.named_modules() if isinstance(m, kinds)] + ["UNetModel.out"]


def _assert_unet_rows(rep, net):
    paths = _unet_paths(net)
    have = {r.module for r in rep.rows}
    covered = lambda p: any(h == p or h.startswith(p + ".") for h in have)
    assert [p for p in paths if not covered(p)] == []
    assert len(rep.rows) >= len(paths) > 40


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_probe_changes_nothing(dtype):
    from mobi_amd import graph, health, ops
    model, net, i = _setup(dtype)
    ref = _forward(net, i)
    before = _ddim2(model, i)
    with health.probe() as hp:
        assert not graph.usable(i["x"])
        got = _forward(net, i)
    assert torch.equal(got, ref)
    assert ops._HEALTH is None and graph.usable(i["x"])
    assert len(hp.report().rows) > 40
    assert torch.equal(_ddim2(model, i), before)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_rows_are_true(dtype):
    from mobi_amd import health
    model, net, i = _setup(dtype)
    with health.probe(keep=True) as hp:
        _forward(net, i)
    rep = hp.report()
    hc.assert_rows_match_torch(rep)
    _assert_unet_rows(rep, net)
    assert [r.seq for r in rep.rows] == list(range(len(rep.rows)))
    name = health.DTYPE_NAMES[dtype]
    assert {r.dtype for r in rep.rows} == {name, "fp32"} and sum(r.dtype == name for r in rep.rows) > 40


def test_a_sampling_run_has_one_sampler_row_per_step():
    from mobi_amd import health
    model, net, i = _setup(torch.float16)
    with health.probe(keep=True) as hp:
        _ddim2(model, i)
    rep = hp.report()
    hc.assert_rows_match_torch(rep)
    sampler = [r for r in rep.rows if r.kind == "sampler"]
    assert len(sampler) == 2 and all(r.dtype == "fp32" and len(r.kept) == 2 for r in sampler)
    assert len(rep.rows) >= 2 * len(_unet_paths(net)) + 2


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_autoencoders_rows_are_true(dtype):
    """Encode and decode of the two reduced autoencoders (ch 32, 64 x 64): every row is what torch computes on its clone, and
    every ResnetBlock, mid.attn_1, conv_in and conv_out (the lidar adapter's: conv_in_lidar, conv_out_lidar) has a row with its
    path -- also where the decoder calls a block's stream / trunk body directly (ops.health_labelled, ops.health_scope)."""
    import mobi_amd
    from mobi_amd import health
    from mobi_amd.ldm.modules.diffusionmodules import model as vm
    mobi_amd.set_engine_dtype(dtype)
    for lidar in (False, True):
        cfg = ovae.VAEConfig(ch=32, lidar_adapter=lidar)
        vae = _vae(cfg, 64)
        W.fill_module_(vae, seed=31)
        vae = vae.cuda().eval()
        x = W.synth_input("h.vae", (2, cfg.in_channels, 64, 64)).cuda()
        with torch.no_grad(), health.probe(keep=True) as hp:
            z = vae.encode(x).mode()
            vae.decode(z)
        rep = hp.report()
        hc.assert_rows_match_torch(rep)
        assert len(rep.rows) > 60 and any(r.dtype == "fp32" for r in rep.rows)
        have = {r.module for r in rep.rows}
        want = []
        for root, net in (("Encoder", vae.encoder), ("Decoder", vae.decoder)):
            want += [f"{root}.{n}" for n, m in net.named_modules() if isinstance(m, vm.ResnetBlock)]
            want += [f"{root}.mid.attn_1"]
            want += [f"{root}.{n}" for n in ("conv_in", "conv_in_lidar", "conv_out", "conv_out_lidar") if hasattr(net, n)]
        covered = lambda p: any(h == p or h.startswith(p + ".") for h in have)
        assert [p for p in want if not covered(p)] == [], lidar
        assert len(want) > 25 and len(rep.rows) >= len(want)


def test_localisation():
    """The last output block's SpatialTransformer.proj_out, scaled until its output leaves fp16's range but not bf16's: the first
    non-finite row is that module's; only the closing GroupNorm and the out convolution read the result."""
    from mobi_amd import health
    from mobi_amd.ldm.modules.attention import SpatialTransformer
    from mobi_amd.ldm.modules.diffusionmodules.util import weights_changed
    reports = {}
    model, net, i = _setup(torch.bfloat16)
    st_name, st = [(n, m) for n, m in net.named_modules() if isinstance(m, SpatialTransformer)][-1]
    assert st_name.startswith("output_blocks.11")
    path = "UNetModel." + st_name

    def last_row(rep):
        return [r for r in rep.rows if r.module == path or r.module.startswith(path + ".")][-1]

    with health.probe() as hp:
        _forward(net, i)
    base = last_row(hp.report())
    assert 0 < base.absmax < 65504.0
    factor = 4.0 * 65504.0 / base.absmax
    with torch.no_grad():
        st.proj_out.weight.mul_(factor)
        st.proj_out.bias.mul_(factor)
    weights_changed([st.proj_out.weight, st.proj_out.bias])
    import mobi_amd
    for dtype in (torch.bfloat16, torch.float16):
        mobi_amd.set_engine_dtype(dtype)
        with health.probe() as hp:
            out = _forward(net, i)
        torch.cuda.synchronize()                                    # overflow in data is no fault: the run ends normally
        reports[dtype] = hp.report()
        assert out.shape == (4, 4, 16, 16)
    bf, fp = reports[torch.bfloat16], reports[torch.float16]
    assert bf.first_nonfinite() is None
    assert last_row(bf).absmax > 65504.0
    bad = fp.first_nonfinite()
    assert bad is not None and (bad.module == path or bad.module.startswith(path + ".")) and bad.seq == last_row(fp).seq
    assert all(r.inf == r.nan == 0 for r in fp.rows[:bad.seq])


def test_audit_weights():
    from mobi_amd import health
    model, net, i = _setup(torch.float16)
    _forward(net, i)                                               # packs the 16-bit images
    rep = health.audit_weights(net, torch.float16)
    n_params = sum(1 for _ in net.parameters())
    assert sum(r.kind == "param" for r in rep.rows) == n_params and sum(r.kind == "image" for r in rep.rows) > 20
    assert all(r.inf == r.nan == r.overflow == 0 for r in rep.rows)
    conv = net.output_blocks[5][0].in_layers[2]
    with torch.no_grad():
        conv.weight[3, 2, 1, 1] = 1e5
    _forward(net, i)                                               # repacks that weight
    rep = health.audit_weights(net, torch.float16)
    hot = [r for r in rep.rows if r.kind == "param" and (r.near or r.overflow)]
    assert [r.module for r in hot] == ["output_blocks.5.0.in_layers.2.weight"] and hot[0].near >= 1 and hot[0].overflow == 1
    inf_rows = [r for r in rep.rows if r.inf]
    assert len(inf_rows) >= 1 and all(r.kind == "image" and r.inf == 1 and r.dtype == "fp16" and
                                      r.module.startswith("output_blocks.5.0.in_layers.2[") for r in inf_rows)
    assert all(r.nan == 0 for r in rep.rows)
    bf = health.audit_weights(net, torch.bfloat16)
    assert all(r.near == r.overflow == 0 for r in bf.rows if r.kind == "param")


def test_heavy_tailed_forward_is_reported_consistently():
    """Whether anything overflows with the stand-in weights is a finding (README, "Numeric health"), not a condition."""
    from mobi_amd import health
    model, net, i = _setup(torch.float16)
    health.heavy_tailed_(net, 4)
    with health.probe(keep=True) as hp:
        _forward(net, i)
    torch.cuda.synchronize()
    rep = hp.report()
    hc.assert_rows_match_torch(rep)
    _assert_unet_rows(rep, net)
    print(rep.summary())


# --------------------------------------------------------------------------------------
# the commands
# --------------------------------------------------------------------------------------
REDUCED = ["latent_size=16", "image_height=128", "image_width=128", "range_height=128", "range_width=128", "use_lidar=True",
           "model.params.lidar_stage_config.params.ckpt_path=null",
           "model.params.unet_config.params.model_channels=64",
           "model.params.first_stage_config.params.ddconfig.ch=32",
           "model.params.lidar_stage_config.params.ddconfig.ch=32",
           "model.params.cond_stage_config.params.clip_config.hidden_size=1024",
           "model.params.cond_stage_config.params.clip_config.intermediate_size=256",
           "model.params.cond_stage_config.params.clip_config.num_hidden_layers=1",
           "model.params.cond_stage_config.params.clip_config.num_attention_heads=16"]


def test_the_command_probes_the_whole_model(tmp_path):
    """`python -m mobi_amd.health --synthetic gauss --dtype both` on the reduced model: the audit lists every parameter of the
    whole model, the run has rows of the conditioning producer, both autoencoders in encode and decode, the UNet and the sampler;
    a checkpoint that matches nothing is refused instead of being reported on."""
    import json
    from mobi_amd import health
    config = os.path.join(ROOT, "configs", "mobi_nusc_256.yaml")
    out = str(tmp_path / "health.json")
    rc = health.main(["--config", config, "--synthetic", "gauss", "--dtype", "both", "--objects", "2", "--json", out, *REDUCED])
    assert rc in (0, 3)
    got = json.load(open(out))
    assert set(got) == {"audit_fp16", "audit_bf16", "run_fp16", "run_bf16"}
    names = [r["module"] for r in got["audit_fp16"]["rows"] if r["kind"] == "param"]
    for part in ("model.diffusion_model.", "first_stage_model.encoder.", "first_stage_model.decoder.", "lidar_stage_model.decoder.",
                 "cond_stage_model."):
        assert any(n.startswith(part) for n in names), part
    rows = got["run_fp16"]["rows"]
    assert len(rows) > 300 and len(got["run_bf16"]["rows"]) > 300     # (not the same count: fp16 decodes on its fp32-stream paths)
    roots = {r["module"].split(".")[0] for r in rows}
    assert {"DiffusionWrapper", "Encoder", "Decoder"} <= roots and len(roots) >= 4, roots
    assert sum(r["kind"] == "sampler" for r in rows) == 2
    assert (rc == 3) == any(r["inf"] + r["nan"] for k in ("run_fp16", "run_bf16") for r in got[k]["rows"])
    bad = str(tmp_path / "other.ckpt")
    torch.save({"state_dict": {"nothing.of.this.model": torch.zeros(3)}}, bad)
    with pytest.raises(SystemExit):
        health.main(["--config", config, "--ckpt", bad, *REDUCED])


def _files(d):
    return sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)


def test_test_bench_health_adds_one_file(tmp_path):
    """The recipe of tests/test_gpu_test_bench.py: the miniature database and a reduced model; `python -m mobi_amd.health
    test_bench ...` adds health.json to what `python -m mobi_amd.test_bench ...` writes and changes no other byte."""
    import mobi_amd
    from mobi_amd import health, ops, test_bench as tb
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    from tests import mini_db
    csv, pkl = mini_db.build(str(tmp_path / "db"))
    data = "data.params.test.params."
    overrides = ["latent_size=16", "image_height=128", "image_width=128", "range_height=128", "range_width=128", "use_lidar=True",
                 "ref_mode=id-ref",
                 "model.params.lidar_stage_config.params.ckpt_path=null",
                 "model.params.unet_config.params.model_channels=64",
                 "model.params.first_stage_config.params.ddconfig.ch=32",
                 "model.params.lidar_stage_config.params.ddconfig.ch=32",
                 "model.params.cond_stage_config.params.clip_config.hidden_size=1024",
                 "model.params.cond_stage_config.params.clip_config.intermediate_size=256",
                 "model.params.cond_stage_config.params.clip_config.num_hidden_layers=1",
                 "model.params.cond_stage_config.params.clip_config.num_attention_heads=16",
                 f"{data}object_database_path={csv}", f"{data}scene_database_path={pkl}", f"{data}num_samples_per_class=2",
                 f"{data}min_lidar_points=8", f"{data}range_int_norm=True"]
    config = os.path.join(ROOT, "configs", "mobi_nusc_256.yaml")
    mobi_amd.set_engine_dtype(torch.float16)
    model = instantiate_from_config(load_config(config, overrides)["model"])
    W.fill_module_(model, seed=29)
    ckpt = str(tmp_path / "model.ckpt")
    torch.save({"state_dict": model.state_dict()}, ckpt)
    del model
    common = ["--config", config, "--ckpt", ckpt, "--scale", "5", "--n_samples", "2", "--n_workers", "0", "--ddim_steps", "2",
              "--save_samples"]
    plain, probed = str(tmp_path / "plain"), str(tmp_path / "probed")
    tb.main(common + ["--outdir", plain, *overrides])
    assert health.main(["test_bench"] + common + ["--outdir", probed, *overrides]) == 0
    assert tb.load_model.__module__ == "mobi_amd.test_bench" and ops._HEALTH is None
    a, b = _files(plain), _files(probed)
    assert "health.json" not in a and b == sorted(a + ["health.json"]) and len(a) > 10
    for f in a:
        with open(os.path.join(plain, f), "rb") as fa, open(os.path.join(probed, f), "rb") as fb:
            assert fa.read() == fb.read(), f
    rep = health.Report.from_json(open(os.path.join(probed, "health.json")).read())
    kinds = {r.kind for r in rep.rows}
    assert len(rep.rows) > 200 and "sampler" in kinds and sum(r.kind == "sampler" for r in rep.rows) == 2
    roots = {r.module.split(".")[0] for r in rep.rows}
    assert {"DiffusionWrapper", "Encoder", "Decoder"} <= roots
