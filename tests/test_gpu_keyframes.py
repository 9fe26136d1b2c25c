"""GPU: ``sampler.sample_with_keyframes`` -- the key-pose guided loop whose update is one ``cfd_denoise_guide`` call -- and long-form
synthesis with key poses (``longform.synthesize_latents(keyframes=)``).

Against the existing torch loop (``sample_with_loss_guidance`` with ``edit.keyframe_loss``) and against the same loop on the CPU: torch
autograd through oracle.denoiser_torch for the gradient, oracle.sampler_ref's combine and oracle.scheduler_ref's step for the iteration
(the construction of tests/test_gpu_denoise_vjp.py's three-iteration loop), a tie applied by indexing inside the graph and re-applied
after each update and after the last iteration as tests/longform_ref.py states it.  Gate: 1e-3 relative, the project's loop gate; the
guidance moves every result by more than 100 times that (asserted on the reference, so no comparison passes vacuously).  Errors are printed.
"""
import functools

import numpy as np
import pytest

from oracle import inputs, philox_ref
from tests.helpers import rel_l2, state_dict

pytestmark = pytest.mark.gpu

GATE = 1e-3
S = (6, 20, 6, 8, 1)
PAD = (2, 0, 1, 0, 0)
SCALE = 7.5
STEP = 8.0           # large on purpose: the mean over kept tokens x 128 elements makes the raw gradient small (reference: the results move by 0.17 - 0.73)


def _sched(kind):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    return scheduler.DDIMScheduler(**SCHED_KW) if kind == "ddim" else scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)


def _sched_ref(kind):
    from oracle import scheduler_ref
    from tests.gpu_helpers import SCHED_KW
    return scheduler_ref.DDIMSchedulerRef(**SCHED_KW) if kind == "ddim" else scheduler_ref.DDPMSchedulerRef(variance_type="fixed_small", **SCHED_KW)


def _targets(seed, B, L, tokens):
    target = (np.random.Generator(np.random.PCG64(seed)).standard_normal((B, L, 128), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    mask = np.zeros((B, L), dtype=bool)
    for b, l in tokens:
        mask[b, l] = True
    return target, mask


def reference_loop(kind, N, mems, masks, init, step_noise, target, mask, step, guided=None, tie=None, source=None, keep=None):
    """The guided loop on the CPU.  mems / masks: the 7 B-row guidance batch (numpy); init [B, L, 128]; step_noise [N, B, L, 128] or
    None; tie int [B, L] or None; source / keep: kept tokens re-noised from the initial draw at the start of every iteration."""
    import torch
    from convofusion_amd import edit
    from oracle import denoiser_torch, sampler_ref
    from tests.edit_ref import add_noise
    from tests.longform_ref import tie_copy
    B, L, _ = init.shape
    sd = denoiser_torch.to_torch(state_dict(1234, 1.0))
    tm = [torch.from_numpy(np.ascontiguousarray(v)) for v in mems]
    tk = {k: (torch.from_numpy(np.ascontiguousarray(v)) if v is not None else None) for k, v in masks.items()}
    fwd = denoiser_torch.denoiser_forward.__wrapped__
    loss_fn = edit.keyframe_loss(torch.from_numpy(target), torch.from_numpy(mask))
    ref = _sched_ref(kind)
    ref.set_timesteps(N)
    eps0 = (init * np.float32(ref.init_noise_sigma)).astype(np.float32)
    lat = eps0.copy()
    idx = None if tie is None else torch.from_numpy(np.where(tie.reshape(-1) >= 0, tie.reshape(-1), np.arange(B * L)).astype(np.int64))
    for i, t in enumerate(ref.timesteps):
        if tie is not None:
            lat = tie_copy(lat, tie)
        if keep is not None:
            lat[keep] = add_noise(ref, source, eps0, int(t))[keep]
        if step and (guided is None or i in guided):
            x = torch.from_numpy(lat).clone().requires_grad_(True)
            with torch.enable_grad():
                xt = x if idx is None else x.reshape(B * L, 128)[idx].reshape(B, L, 128)      # the tie, inside the graph
                e = fwd(sd, xt.repeat(7, 1, 1), int(t), tm, tk)[0].view(7, B, L, 128)
                eps = e[0]
                for k in range(1, 6):
                    eps = eps + SCALE * (e[k] - e[0])
                a = float(ref.alphas_cumprod[int(t)])
                (g,) = torch.autograd.grad(loss_fn((xt - (1.0 - a) ** 0.5 * eps) / a ** 0.5), x)
            lat = (lat - np.float32(step) * g.numpy()).astype(np.float32)
            if tie is not None:
                lat = tie_copy(lat, tie)
        with torch.no_grad():
            pred = fwd(sd, torch.from_numpy(np.concatenate([lat] * 7)), int(t), tm, tk)[0].numpy()
        if kind == "ddim":
            lat = ref.step(sampler_ref.cfg_combine(pred, SCALE), t, lat, eta=0.0)
        else:
            lat = ref.step(sampler_ref.cfg_combine(pred, SCALE), t, lat, noise=step_noise[i] if int(t) > 0 else None)
    return lat if tie is None else tie_copy(lat, tie)


LOOPS = {"ddim3": ("ddim", 3, None), "ddpm4": ("ddpm", 4, (1, 2))}


@functools.lru_cache(maxsize=None)
def plain_case(name):
    kind, N, guided = LOOPS[name]
    B, L = 1, 16
    cb = inputs.make_cfg_batch(seed=81, B=B, L=L, S=S, pad_tail=PAD)
    target, mask = _targets(82, B, L, [(0, 3), (0, 4), (0, 9), (0, 14)])
    noise = np.random.Generator(np.random.PCG64(83)).standard_normal((N, B, L, 128), dtype=np.float32)
    args = (kind, N, cb["memories"], cb["masks"], cb["init"], noise, target, mask)
    return cb, target, mask, noise, reference_loop(*args, STEP, guided), reference_loop(*args, 0.0, guided)


@pytest.mark.parametrize("name", list(LOOPS))
def test_keyframe_loop_matches_the_torch_loop_and_the_cpu_loop(name):
    """Fails on a tree without the feature: ``sampler.sample_with_keyframes`` does not exist there."""
    import torch
    from convofusion_amd import edit, sampler
    from tests.gpu_helpers import hip_denoiser, to_dev
    kind, N, guided = LOOPS[name]
    B, L = 1, 16
    cb, target, mask, noise, want, unguided = plain_case(name)
    moved = rel_l2(want, unguided)
    assert moved > 100 * GATE, moved          # (of the reference: the guidance moves the result far beyond the gate)
    m = hip_denoiser(1234, 1.0)
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=SCALE, eta=0.0, init_latents=to_dev(cb["init"]), guided_iterations=guided)
    if kind == "ddpm":
        kw["step_noise"] = to_dev(noise)
    got = sampler.sample_with_keyframes(m, _sched(kind), mems, masks, to_dev(target), to_dev(mask), STEP, **kw)
    torch_loop = sampler.sample_with_loss_guidance(m, _sched(kind), mems, masks, edit.keyframe_loss(to_dev(target), to_dev(mask)), STEP, **kw)
    e_torch, e_cpu = rel_l2(got.cpu().numpy(), torch_loop.cpu().numpy()), rel_l2(got.cpu().numpy(), want)
    print(f"{name}: sample_with_keyframes vs the torch loop {e_torch:.2e}, vs the CPU loop {e_cpu:.2e} (the torch loop vs the CPU loop "
          f"{rel_l2(torch_loop.cpu().numpy(), want):.2e}); guided vs unguided (reference) {moved:.2e}")
    assert e_torch < GATE and e_cpu < GATE
    assert not got.is_inference() and not got.requires_grad
    # step size 0, and no guided iteration: ``sample``, bit for bit; called under inference mode: the same bits
    del kw["guided_iterations"]
    plain = sampler.sample(m, _sched(kind), mems, masks, **kw)
    assert torch.equal(sampler.sample_with_keyframes(m, _sched(kind), mems, masks, to_dev(target), to_dev(mask), 0.0, **kw), plain)
    assert torch.equal(sampler.sample_with_keyframes(m, _sched(kind), mems, masks, to_dev(target), to_dev(mask), STEP, guided_iterations=(), **kw), plain)
    with torch.inference_mode():
        again = sampler.sample_with_keyframes(m, _sched(kind), mems, masks, to_dev(target), to_dev(mask), STEP, guided_iterations=guided, **kw)
    assert torch.equal(again, got)


@functools.lru_cache(maxsize=None)
def tied_case():
    """One utterance, three windows, DDIM-3; key tokens on a tied token (window 1, token 2), on a source and on a free token."""
    from convofusion_amd import longform
    B, L, N = 3, 16, 3
    cb = inputs.make_cfg_batch(seed=91, B=B, L=L, S=S, pad_tail=PAD)
    target, mask = _targets(92, B, L, [(1, 2), (0, 12), (2, 13)])
    tie = longform.window_ties(1, 3, L).numpy()
    assert tie[1, 2] == 0 * L + 10
    args = ("ddim", N, cb["memories"], cb["masks"], cb["init"], None, target, mask)
    return cb, target, mask, tie, reference_loop(*args, STEP, tie=tie), reference_loop(*args, 0.0, tie=tie)


def test_tied_run_takes_key_poses_and_keeps_its_tie():
    import torch
    from convofusion_amd import sampler
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, N = 3, 16, 3
    cb, target, mask, tie, want, unguided = tied_case()
    moved = rel_l2(want, unguided)
    assert moved > 100 * GATE, moved
    m = hip_denoiser(1234, 1.0)
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=SCALE, eta=0.0, init_latents=to_dev(cb["init"]), tie=to_dev(tie))
    got = sampler.sample_with_keyframes(m, _sched("ddim"), mems, masks, to_dev(target), to_dev(mask), STEP, **kw)
    e = rel_l2(got.cpu().numpy(), want)
    print(f"tied DDIM-3, three windows: vs the CPU loop {e:.2e}; guided vs unguided (reference) {moved:.2e}")
    assert e < GATE
    flat, t = got.reshape(-1, 128), torch.from_numpy(tie.reshape(-1).astype(np.int64)).cuda()
    assert torch.equal(flat[t >= 0], flat[t[t >= 0]])                                   # the returned windows satisfy the tie bit for bit
    # step size 0 on the tied run: ``sample``'s bits; the torch loop still refuses the run
    assert torch.equal(sampler.sample_with_keyframes(m, _sched("ddim"), mems, masks, to_dev(target), to_dev(mask), 0.0, **kw),
                       sampler.sample(m, _sched("ddim"), mems, masks, **kw))
    with pytest.raises(NotImplementedError, match="sample_with_keyframes"):
        sampler.sample_with_loss_guidance(m, _sched("ddim"), mems, masks, lambda x0: x0.sum(), STEP, **kw)


def test_long_form_synthesis_with_key_poses_group_by_group():
    """3 windows with max_rows = 2: one tied group of two windows, then the third window on its own, keeping its first half from the
    second window's finished second half.  The reference is the CPU loop driven group by group on the global rows' Philox draws."""
    import torch
    from convofusion_amd.longform import group_ties, synthesize_latents, window_groups
    from tests.gpu_helpers import hip_denoiser, to_dev
    U, W, L, N, seed = 1, 3, 16, 3, 17
    B = U * W
    cb = inputs.make_cfg_batch(seed=95, B=B, L=L, S=S, pad_tail=PAD)
    target, mask = _targets(96, B, L, [(1, 2), (0, 12), (2, 13), (2, 1)])      # (2, 1): a kept (carried) token of the second run

    def reference(step):
        out = np.zeros((B, L, 128), dtype=np.float32)
        for a, b in window_groups(U, W, 2):
            tie, carried = group_ties(a, b, W, L)
            src = keep = None
            if bool(carried.any()):
                src, keep = np.zeros((b - a, L, 128), dtype=np.float32), carried.numpy()
                src[0, :L // 2] = out[a - 1, L // 2:]
            rows = lambda v: v.reshape((7, B) + v.shape[1:])[:, a:b].reshape((7 * (b - a),) + v.shape[1:])
            out[a:b] = reference_loop("ddim", N, [rows(v) for v in cb["memories"]], {k: (None if v is None else rows(v)) for k, v in cb["masks"].items()},
                                      philox_ref.normal_tensor(seed, 0, range(a, b), 1, L), None, target[a:b], mask[a:b], step,
                                      tie=tie.numpy() if bool((tie >= 0).any()) else None, source=src, keep=keep)
        return out

    want, unguided = reference(STEP), reference(0.0)
    moved = rel_l2(want, unguided)
    assert moved > 100 * GATE, moved
    m = hip_denoiser(1234, 1.0)
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    kw = dict(n_utterances=U, n_windows=W, L=L, num_inference_steps=N, guidance_scale=SCALE, seed=seed, max_rows=2)
    win, seq = synthesize_latents(m, _sched("ddim"), mems, masks, keyframes=(to_dev(target), to_dev(mask), STEP, None), **kw)
    e = rel_l2(win.reshape(B, L, 128).cpu().numpy(), want)
    print(f"long-form, 3 windows in runs of 2 + 1, DDIM-3: vs the CPU loop {e:.2e}; guided vs unguided (reference) {moved:.2e}")
    assert e < GATE and tuple(seq.shape) == (U, (W + 1) * L // 2, 128)
    assert torch.equal(win[0, 1, :L // 2], win[0, 0, L // 2:])                          # the tie of the first run
    # without key poses: the bits of the call without the argument; a zero step size: those bits too
    none, _ = synthesize_latents(m, _sched("ddim"), mems, masks, keyframes=None, **kw)
    plain, _ = synthesize_latents(m, _sched("ddim"), mems, masks, **kw)
    assert torch.equal(none, plain)
    zero, _ = synthesize_latents(m, _sched("ddim"), mems, masks, keyframes=(to_dev(target), to_dev(mask), 0.0, None), **kw)
    assert torch.equal(zero, plain)
    assert rel_l2(plain.reshape(B, L, 128).cpu().numpy(), unguided) < GATE
