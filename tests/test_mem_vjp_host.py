"""CPU: the pin of the float64 restatement ``tests/mem_vjp_ref.py`` (the gradient of one denoiser forward at its five memories) against
float32 torch autograd through ``oracle.denoiser_torch``; every refusal of ``Denoiser.forward(..., memory_grad=True)``,
``Denoiser.vjp_memories`` and ``fit.fit_conditioning`` before any device work (on a CPU module, which has no engine); the C
declaration of ``cfd_denoise_vjp_mem``."""
import re

import numpy as np
import pytest
import torch

from convofusion_amd import _lib, denoiser, fit, scheduler
from oracle import denoiser_torch, inputs
from tests import mem_vjp_ref, vjp_ref
from tests.helpers import rel_l2, state_dict

MEM_NAMES = inputs.MEM_NAMES
S_TINY = (3, 5, 6, 2, 1)
YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def test_float64_restatement_matches_float32_torch_autograd_at_all_five_memories():
    """B = 2, L = 4, S = (3, 5, 6, 2, 1), pad_tail (1, 0, 2, 0, 0), timestep 613: tests/mem_vjp_ref.py at float64 against torch autograd
    through oracle.denoiser_torch at float32, gate 1e-5 (the pin of tests/vjp_ref.py; 6e-7 - 8e-7 measured on these weights); the
    sample's gradient and the output are ``vjp_ref``'s; masked keys are exactly 0 on both sides."""
    sd = state_dict(1234, 1.0)
    inp = inputs.make_plain_batch(seed=611, Be=2, L=4, S=S_TINY, pad_tail=(1, 0, 2, 0, 0))
    c = vjp_ref.cotangent(612, inp["sample"].shape)
    mems = [torch.from_numpy(m).clone().requires_grad_(True) for m in inp["memories"]]
    masks = {k: (torch.from_numpy(v) if v is not None else None) for k, v in inp["masks"].items()}
    with torch.enable_grad():
        out, _ = denoiser_torch.denoiser_forward.__wrapped__(denoiser_torch.to_torch(sd), torch.from_numpy(inp["sample"]), 613, mems, masks)
        grads = torch.autograd.grad(out, mems, torch.from_numpy(c))
    o64, g64, d64 = mem_vjp_ref.out_and_vjp_mem(sd, inp["sample"], 613, inp["memories"], inp["masks"], c)
    d32 = mem_vjp_ref.out_and_vjp_mem(sd, inp["sample"], 613, inp["memories"], inp["masks"], c, dtype=np.float32)[2]
    o_ref, g_ref, _ = vjp_ref.out_and_vjp(sd, inp["sample"], 613, inp["memories"], inp["masks"], c)
    assert np.array_equal(o64, o_ref) and np.array_equal(g64, g_ref)
    masked = 0
    for j, k in enumerate(MEM_NAMES):
        e, f = rel_l2(grads[j].numpy(), d64[j]), rel_l2(d32[j], d64[j])
        print(f"{k}: torch float32 vs float64 {e:.2e}; numpy float32 vs float64 {f:.2e}; |d_mem| {np.abs(d64[j]).max():.2e}")
        assert d64[j].shape == inp["memories"][j].shape and d32[j].dtype == np.float32
        assert e < 1e-5 and f < 1e-5, k
        if inp["masks"][k] is not None:
            mk = np.asarray(inp["masks"][k]).astype(bool)
            masked += int(mk.sum())
            assert not d64[j][mk].any() and not grads[j].numpy()[mk].any() and d64[j][~mk].any(), k
    assert masked >= 1 + 2                    # the padded tails of spkemb and tlsn (at least pad_tail keys in some row)
    # the single key of lsnemb (p = 1, dS = 0) receives its gradient through the value path alone: of order 1
    assert 0.05 < np.abs(d64[4]).max() < 20.0


def test_sum_instances_sums_rows_in_order_and_leaves_orphans_zero():
    d = np.arange(3 * 2 * 4, dtype=np.float64).reshape(3, 2, 4)
    got = mem_vjp_ref.sum_instances(d, [2, 0, 2], 4)
    assert got.shape == (4, 2, 4) and np.array_equal(got[2], d[0] + d[2]) and np.array_equal(got[0], d[1]) and not got[1].any() and not got[3].any()


def _cpu_denoiser():
    from tests.gpu_helpers import ABL, DENOISER_KW
    return denoiser.Denoiser(ablation=ABL, **DENOISER_KW)


def _mems(B=2, S=S_TINY, grad=()):
    return [torch.zeros(B, s, 512, requires_grad=(j in grad)) for j, s in enumerate(S)]


def test_memory_grad_forward_refuses_before_any_device_work():
    m = _cpu_denoiser()
    x = torch.zeros(2, 4, 128)
    with pytest.raises(NotImplementedError, match=r"key-padding mask \(tlsn requires grad\)"):
        m(x, 5, _mems(grad=(2,)), mem_mask_dict={"tlsn": torch.zeros(2, 6, requires_grad=True)}, memory_grad=True)
    with pytest.raises(NotImplementedError, match="one timestep for all rows"):
        m(x, torch.tensor([5, 6]), _mems(grad=(4,)), memory_grad=True)
    with pytest.raises(NotImplementedError, match="L = 34 tokens per batch row exceed the row-tile path's 32"):
        m(torch.zeros(2, 34, 128), 5, _mems(grad=(4,)), memory_grad=True)
    with pytest.raises(NotImplementedError, match="token rows exceed the row-tile path's 700"):
        m(torch.zeros(44, 16, 128), 5, _mems(B=44, grad=(0,)), memory_grad=True)
    with pytest.raises(NotImplementedError, match="1056 padded keys"):
        m(x, 5, _mems(S=(24, 897, 24, 8, 1), grad=(1,)), memory_grad=True)
    with pytest.raises(ValueError, match="one memory per batch row: alsn"):
        m(x, 5, [torch.zeros(1 if j == 1 else 2, s, 512, requires_grad=True) for j, s in enumerate(S_TINY)], memory_grad=True)
    with pytest.raises(ValueError, match="5-tuple"):
        m(x, 5, _mems(grad=(0,))[:4], memory_grad=True)
    # an eligible call gets as far as the engine -- with a memory or with the sample requiring grad -- and so does the inference path
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        m(x, 5, _mems(grad=(4,)), memory_grad=True)
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        m(x.clone().requires_grad_(True), 5, _mems(), memory_grad=True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="runs on an MI355X only"):
        m(x, 5, _mems(grad=(4,)), memory_grad=True)
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        m(x, 5, _mems(), memory_grad=True)


def test_without_the_keyword_the_old_refusal_is_unchanged():
    m = _cpu_denoiser()
    x = torch.zeros(2, 4, 128, requires_grad=True)
    with pytest.raises(NotImplementedError) as e:
        m(x, 5, _mems(grad=(2,)))
    assert str(e.value) == "the HIP denoiser has no gradient with respect to its memories (tlsn requires grad): detach it"
    with pytest.raises(NotImplementedError) as e:
        m(x, 5, _mems(grad=(4,)), memory_grad=False)
    assert str(e.value) == "the HIP denoiser has no gradient with respect to its memories (lsnemb requires grad): detach it"
    # a sample that does not require grad still takes the inference path, whatever the memories ask for
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        m(torch.zeros(2, 4, 128), 5, _mems(grad=(2,)))


def test_vjp_memories_refuses_before_any_device_work():
    m = _cpu_denoiser()
    x, d = torch.zeros(2, 4, 128), torch.zeros(2, 4, 128)
    with pytest.raises(ValueError, match="wrt names a memory that does not exist: 'audio'"):
        m.vjp_memories(x, 5, _mems(), {}, d, wrt=("audio",))
    with pytest.raises(ValueError, match="nothing is wanted"):
        m.vjp_memories(x, 5, _mems(), {}, d, wrt=(), want_grad=False)
    with pytest.raises(ValueError, match="5-tuple"):
        m.vjp_memories(x, 5, _mems()[:3], {}, d)
    with pytest.raises(NotImplementedError, match="with respect to its memories runs on the row-tile path only: L = 34"):
        m.vjp_memories(torch.zeros(2, 34, 128), 5, _mems(), {}, torch.zeros(2, 34, 128))
    with pytest.raises(NotImplementedError, match="Be \\* L = 704 token rows"):
        m.vjp_memories(torch.zeros(44, 16, 128), 5, _mems(B=44), {}, torch.zeros(44, 16, 128))
    with pytest.raises(NotImplementedError, match="1056 padded keys"):
        m.vjp_memories(x, 5, _mems(S=(24, 897, 24, 8, 1)), {}, d)
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        m.vjp_memories(x, 5, _mems(), {}, d, wrt=("lsnemb",))


def test_fit_conditioning_refuses_before_any_device_work():
    m = _cpu_denoiser()
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **YAML)
    lat = torch.zeros(2, 4, 128)
    kw = dict(steps=3, lr=0.1)
    with pytest.raises(ValueError, match="fit names a memory that does not exist: 'identity'"):
        fit.fit_conditioning(m, sch, lat, _mems(), fit=("identity",), **kw)
    with pytest.raises(ValueError, match="fit names no memory"):
        fit.fit_conditioning(m, sch, lat, _mems(), fit=(), **kw)
    with pytest.raises(ValueError, match="fit names a memory twice"):
        fit.fit_conditioning(m, sch, lat, _mems(), fit=("apb", "apb"), **kw)
    with pytest.raises(ValueError, match=r"memory tlsn: expected the examples' own conditional memory \[2, S, 512\]"):
        fit.fit_conditioning(m, sch, lat, [torch.zeros(1 if j == 2 else 2, s, 512) for j, s in enumerate(S_TINY)], **kw)
    with pytest.raises(ValueError, match=r"init\['lsnemb'\] must be \[1, 1, 512\]"):
        fit.fit_conditioning(m, sch, lat, _mems(), init={"lsnemb": torch.zeros(2, 1, 512)}, **kw)
    with pytest.raises(ValueError, match="init has a tensor for 'apb', which is not fitted"):
        fit.fit_conditioning(m, sch, lat, _mems(), init={"apb": torch.zeros(1, 2, 512)}, **kw)
    with pytest.raises(ValueError, match="timesteps has 2 entries for 3 steps"):
        fit.fit_conditioning(m, sch, lat, _mems(), timesteps=[1, 2], **kw)
    with pytest.raises(ValueError, match=r"timestep 1000 outside \[0, 1000\)"):
        fit.fit_conditioning(m, sch, lat, _mems(), timesteps=[1, 2, 1000], **kw)
    with pytest.raises(ValueError, match="steps = 0 must be at least 1"):
        fit.fit_conditioning(m, sch, lat, _mems(), steps=0, lr=0.1)
    with pytest.raises(NotImplementedError, match="memory gradient of the row-tile path only: Be \\* L = 704 token rows"):
        fit.fit_conditioning(m, sch, torch.zeros(44, 16, 128), _mems(B=44), **kw)
    with pytest.raises(NotImplementedError, match="memory gradient of the row-tile path only: L = 34"):
        fit.fit_identity(m, sch, torch.zeros(2, 34, 128), _mems(), **kw)
    # an eligible fit gets as far as the device (the schedulers take device tensors only)
    with pytest.raises(RuntimeError, match="no CPU fallback|runs on an MI355X only"):
        fit.fit_identity(m, sch, lat, _mems(), **kw)


def test_denoising_loss_cotangent_is_the_mean_squared_error_and_its_gradient():
    out = torch.arange(2 * 4 * 128, dtype=torch.float32).reshape(2, 4, 128) / 100.0
    target = (out - 0.5).clone()
    x = out.clone().requires_grad_(True)
    loss = ((x - target) ** 2).mean()
    (g,) = torch.autograd.grad(loss, x)
    got_loss, got = fit.denoising_loss_cotangent(out, target)
    assert abs(float(got_loss) - 0.25) < 1e-6 and torch.allclose(got, g, rtol=1e-6, atol=0) and torch.allclose(got, torch.full_like(got, 2 * 0.5 / 1024))


def test_the_header_declares_the_entry_and_the_binding_loads_it():
    header = open(_lib.HERE + "/../include/cfdenoise.h").read()
    assert "cfd_denoise_vjp_mem" in _lib.SYMBOLS
    assert re.search(r"\bint cfd_denoise_vjp_mem\(cfd_handle h, const cfd_vjp_args\* args, const float\* d_out, float\* out, float\* grad, "
                     r"float\* const d_mem\[CFD_NUM_MEM\],\s+void\* stream\);", header)
    # cfd_vjp_args and cfd_denoise_vjp keep their layout and signature (tests/test_vjp_host.py pins them too)
    assert re.search(r"\bint cfd_denoise_vjp\(cfd_handle h, const cfd_vjp_args\* args, const float\* d_out, float\* out, float\* grad, void\* stream\);", header)
    assert [f[0] for f in _lib.VjpArgs._fields_] == ["Be", "L", "timestep", "sample", "mem"]
