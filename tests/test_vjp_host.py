"""CPU: what the differentiable ``Denoiser.forward`` and ``sampler.sample_with_loss_guidance`` decide without a device -- the limits of
the row-tile path in one pure function (``denoiser.vjp_refusal``), the refusals of the differentiable forward (raised before any device
work: on a CPU module, which has no engine), the refusals between run kinds of the loss-guided loop -- and the pin of the float64
restatement ``tests/vjp_ref.py`` against float32 torch autograd through ``oracle.denoiser_torch``."""
import re

import numpy as np
import pytest
import torch

from convofusion_amd import _lib, denoiser, edit, run_kind, sampler, scheduler
from oracle import denoiser_torch, inputs
from tests import vjp_ref
from tests.helpers import rel_l2, state_dict

YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
S_PRODUCT = (24, 161, 24, 8, 1)            # 32 + 192 + 32 + 32 + 32 = 320 padded keys


def test_float64_restatement_matches_float32_torch_autograd():
    """B = 2, L = 4, ragged masks, timestep 613: out and d_out^T d(out)/d(sample) of tests/vjp_ref.py at float64 against torch
    autograd through oracle.denoiser_torch at float32 (1e-5: float32 autograd's own distance from float64 on this network is ~1e-6);
    the restatement at float32 lands as close."""
    sd = state_dict(1234, 1.0)
    inp = inputs.make_plain_batch(seed=611, Be=2, L=4, S=(3, 5, 6, 2, 1), pad_tail=(1, 0, 2, 0, 0))
    c = vjp_ref.cotangent(612, inp["sample"].shape)
    x = torch.from_numpy(inp["sample"]).clone().requires_grad_(True)
    masks = {k: (torch.from_numpy(v) if v is not None else None) for k, v in inp["masks"].items()}
    with torch.enable_grad():
        out, _ = denoiser_torch.denoiser_forward.__wrapped__(denoiser_torch.to_torch(sd), x, 613, [torch.from_numpy(m) for m in inp["memories"]], masks)
        (grad,) = torch.autograd.grad(out, x, torch.from_numpy(c))
    o64, g64, g_emb = vjp_ref.out_and_vjp(sd, inp["sample"], 613, inp["memories"], inp["masks"], c)
    o32, g32, _ = vjp_ref.out_and_vjp(sd, inp["sample"], 613, inp["memories"], inp["masks"], c, dtype=np.float32)
    e = (rel_l2(out.detach().numpy(), o64), rel_l2(grad.numpy(), g64), rel_l2(o32, o64), rel_l2(g32, g64))
    print("torch float32 vs float64: out %.2e grad %.2e; numpy float32 vs float64: out %.2e grad %.2e" % e)
    assert max(e) < 1e-5
    assert g_emb.shape == (2 * 4, 512) and rel_l2(g_emb @ sd["latent_embd.weight"].astype(np.float64), g64.reshape(8, 128)) < 1e-12


def test_vjp_refusal_at_and_one_past_each_limit():
    ok = denoiser.vjp_refusal
    assert denoiser.VJP_MAX_ROWS == 700 and denoiser.VJP_MAX_L == 32 and denoiser.VJP_MAX_KEYS == 1024
    # token rows: 700 at the default (25 x 28), 701 = 1 x ... is not a shape, so 702 (27 x 26) and 701 through max_rows
    assert ok(25, 28, S_PRODUCT, max_rows=700) is None
    assert "Be * L = 702 token rows exceed the row-tile path's 700" in ok(27, 26, S_PRODUCT, max_rows=700)
    assert ok(701, 1, (1, 1, 1, 1, 1), max_rows=701) is None and "701 token rows exceed the row-tile path's 700" in ok(701, 1, (1, 1, 1, 1, 1), max_rows=700)
    assert ok(43, 16, S_PRODUCT) is None and ok(44, 16, S_PRODUCT) is not None          # the 7-chunk batch of 6 utterances: 42 rows x 16
    # tokens per row
    assert ok(1, 32, S_PRODUCT) is None
    assert "L = 34 tokens per batch row exceed the row-tile path's 32" in ok(1, 34, S_PRODUCT)
    # padded keys: 32 + 896 + 32 + 32 + 32 = 1024 at the limit, 32 more one past it
    assert ok(1, 16, (24, 896, 24, 8, 1)) is None and ok(1, 16, (32, 865, 1, 1, 1)) is None
    assert "1056 padded keys of the five memories together" in ok(1, 16, (24, 897, 24, 8, 1))
    assert "exceed the row-tile path's 1024" in ok(1, 16, (24, 897, 24, 8, 1))


def test_vjp_limits_are_the_library_s():
    text = open(_lib.HERE + "/csrc/rowtile.hpp").read()
    assert int(re.search(r"#define RT_MAX_L (\d+)", text).group(1)) == denoiser.VJP_MAX_L
    assert int(re.search(r"#define RT_MAX_KEYS (\d+)", text).group(1)) == denoiser.VJP_MAX_KEYS
    assert int(re.search(r"long long rt_max_rows = (\d+);", open(_lib.HERE + "/csrc/cfd_internal.hpp").read()).group(1)) == denoiser.VJP_MAX_ROWS
    header = open(_lib.HERE + "/../include/cfdenoise.h").read()
    assert "cfd_denoise_vjp" in _lib.SYMBOLS
    assert re.search(r"\bint cfd_denoise_vjp\(cfd_handle h, const cfd_vjp_args\* args, const float\* d_out, float\* out, float\* grad, void\* stream\);", header)
    assert [f[0] for f in _lib.VjpArgs._fields_] == ["Be", "L", "timestep", "sample", "mem"]


def _cpu_denoiser():
    from tests.gpu_helpers import ABL, DENOISER_KW
    return denoiser.Denoiser(ablation=ABL, **DENOISER_KW)


def test_differentiable_forward_refuses_before_any_device_work():
    """On a CPU module (no engine: reaching the library raises RuntimeError) every refusal of the differentiable forward is the
    NotImplementedError that names its reason."""
    m = _cpu_denoiser()
    mems = [torch.zeros(2, s, 512) for s in (3, 5, 6, 2, 1)]
    x = torch.zeros(2, 4, 128, requires_grad=True)
    with pytest.raises(NotImplementedError, match=r"no gradient with respect to its memories \(tlsn requires grad\)"):
        m(x, 5, [mm.clone().requires_grad_(j == 2) for j, mm in enumerate(mems)])
    with pytest.raises(NotImplementedError, match="one timestep for all rows"):
        m(x, torch.tensor([5, 6]), mems)
    with pytest.raises(NotImplementedError, match="L = 34 tokens per batch row exceed the row-tile path's 32"):
        m(torch.zeros(2, 34, 128, requires_grad=True), 5, mems)
    with pytest.raises(NotImplementedError, match="token rows exceed the row-tile path's 700"):
        m(torch.zeros(44, 16, 128, requires_grad=True), 5, [torch.zeros(44, s, 512) for s in (3, 5, 6, 2, 1)])
    with pytest.raises(NotImplementedError, match="1056 padded keys"):
        m(x, 5, [torch.zeros(2, s, 512) for s in (24, 897, 24, 8, 1)])
    with pytest.raises(NotImplementedError, match="1056 padded keys"):
        m.vjp(x, 5, [torch.zeros(2, s, 512) for s in (24, 897, 24, 8, 1)], {}, torch.zeros(2, 4, 128))
    # an eligible call gets as far as the engine, and so does the same call under no_grad (the inference path is as it was)
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        m(x, 5, mems)
    with torch.no_grad(), pytest.raises(RuntimeError, match="runs on an MI355X only"):
        m(x, 5, mems)


def _sched(kind, **kw):
    cls = dict(ddpm=scheduler.DDPMScheduler, ddim=scheduler.DDIMScheduler, inverse=scheduler.DDIMInverseScheduler,
               dpmpp=scheduler.DPMSolverMultistepScheduler)[kind]
    return cls(**YAML, **kw)


LOSS_GUIDANCE_REFUSALS = {
    "dpm-solver++": ("with DDPMScheduler / DDIMScheduler; with DPMSolverMultistepScheduler it has no reference trajectory", "dpmpp", {}, {}),
    "sample prediction": ("with prediction_type='epsilon' only", "ddim", dict(prediction_type="sample"), {}),
    "inversion": ("a DDIM inversion (DDIMInverseScheduler) takes no loss guidance", "inverse", {}, {}),
    "replay": ("the replay of a noise space (noise_space) takes no loss guidance", "ddpm", {}, dict(noise_space=(torch.zeros(1), torch.zeros(1)))),
    "anchored": ("an anchored run (anchor_trajectory) takes no loss guidance", "ddim", {}, dict(anchor_trajectory=torch.zeros(1))),
    "tied": ("a tied run (tie) takes no loss guidance", "ddpm", {}, dict(tie=torch.zeros(1, 16, dtype=torch.int64))),
}


@pytest.mark.parametrize("name", list(LOSS_GUIDANCE_REFUSALS))
def test_loss_guided_loop_refuses_run_kinds_before_any_device_work(name):
    text, kind, sched_kw, kw = LOSS_GUIDANCE_REFUSALS[name]
    sch = _sched(kind, **sched_kw)
    with pytest.raises(NotImplementedError, match=re.escape(text)):
        run_kind.check_loss_guidance(sch, **kw)
    # the loop itself: no denoiser, CPU memories -- the refusal comes first
    with pytest.raises(NotImplementedError, match=re.escape(text)):
        sampler.sample_with_loss_guidance(None, sch, [torch.zeros(7, s, 512) for s in (3, 5, 6, 2, 1)], None, lambda x0: x0.sum(), 0.1,
                                          B=1, L=16, num_inference_steps=5, **kw)


def test_loss_guided_loop_accepts_ddpm_and_ddim_and_checks_its_shape_first():
    for kind in ("ddpm", "ddim"):
        run_kind.check_loss_guidance(_sched(kind))
    enc = [torch.zeros(7 * 8, s, 512) for s in (3, 5, 6, 2, 1)]
    # 6 evaluated chunks (the full-conditioning chunk has weight 0) x 8 utterances x 16 tokens = 768 rows
    with pytest.raises(NotImplementedError, match=re.escape("the gradient of the 6 evaluated guidance chunks runs on the row-tile path only: Be * L = 768")):
        sampler.sample_with_loss_guidance(None, _sched("ddim"), enc, None, lambda x0: x0.sum(), 0.1, B=8, L=16, num_inference_steps=5)
    with pytest.raises(NotImplementedError, match="operands='auto'"):
        sampler.sample_with_loss_guidance(None, _sched("ddim"), enc, None, lambda x0: x0.sum(), 0.1, B=1, L=16, num_inference_steps=5, operands="auto")
    assert sampler.guided_chunks(sampler.default_guidance_weights(7, 7.5)) == [0, 1, 2, 3, 4, 5]
    assert sampler.guided_chunks(sampler.default_guidance_weights(2, 7.5)) == [0, 1]
    tab = sampler.modality_weight_table(dict(text=0.0, audio=2.0, spk=0.0, apb=0.0, lsnid=0.0, all=1.0), 7.5, 5, 2)
    assert sampler.guided_chunks(tab) == [0, 2, 6]


def test_keyframe_loss_is_the_masked_mean_square_error():
    target = torch.arange(2 * 4 * 128, dtype=torch.float32).reshape(2, 4, 128) / 100.0
    mask = torch.zeros(2, 4, dtype=torch.bool)
    mask[0, 1] = mask[1, 3] = True
    x0 = (target + 0.5).requires_grad_(True)
    loss = edit.keyframe_loss(target, mask)(x0)
    assert abs(float(loss.detach()) - 0.25) < 1e-6
    (g,) = torch.autograd.grad(loss, x0)
    assert torch.equal(g != 0, mask[..., None].expand_as(g)) and torch.allclose(g[mask], torch.full((2, 128), 2 * 0.5 / 256))
    with pytest.raises(ValueError):
        edit.keyframe_loss(target, torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        edit.keyframe_loss(target, torch.ones(2, 5, dtype=torch.bool))
