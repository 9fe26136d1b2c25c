"""GPU: ``sampler.sample_with_pose_keyframes`` -- the loop with frame-accurate key poses whose update is one ``cfd_denoise_guide_pose``
call -- and long-form synthesis with them (``longform.synthesize_latents(pose_keyframes=)``).

Against the torch loop (``sample_with_loss_guidance`` with ``edit.pose_keyframe_loss(fused=True)``) and against a loop on the CPU whose
guided update is the float64 restatement tests/pose_guide_ref.py, rounded to float32 at the write, with oracle.denoiser_torch's forward,
oracle.sampler_ref's combine and oracle.scheduler_ref's step for the iteration (the construction of tests/test_gpu_keyframes.py); a tie
is re-applied after each update and after the last iteration as tests/longform_ref.py states it.  Gate: 1e-3 relative, the project's
loop gate; the guidance moves every reference result by more than 100 times that (asserted, so no comparison passes vacuously).
Errors are printed.

Measured on an MI355X:
    ddim3 (all iterations guided)  vs the torch loop 1.8e-5, vs the CPU loop 4.8e-5; the guidance moves the reference by 0.56
    ddpm4 (iterations 1, 2 guided) vs the torch loop 7.2e-6, vs the CPU loop 1.3e-5; guidance 0.25
    tied DDIM-3, three windows     vs the CPU loop 2.7e-5; guidance 0.18
    long-form, runs of 2 + 1       vs the CPU loop 3.3e-5; guidance 0.27
"""
import functools

import numpy as np
import pytest

from oracle import inputs, philox_ref, vae_weights
from tests import pose_guide_ref
from tests.helpers import rel_l2, state_dict
from tests.test_gpu_keyframes import GATE, PAD, S, SCALE, _sched, _sched_ref

pytestmark = pytest.mark.gpu

NF = 189
HANDS = slice(69, NF)
STEP = 25.0          # large on purpose: the mean over frames x features and the decoder's small Jacobian make the raw gradient small
CHUNKS = 6           # the chunks of non-zero weight of the default combine: 0 .. 5 of 7


def _pose_targets(seed, B, F, frames):
    target = (np.random.Generator(np.random.PCG64(seed)).standard_normal((B, F, NF), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    fm = np.zeros((B, F), dtype=bool)
    for b, f in frames:
        fm[b, f] = True
    cm = np.zeros(NF, dtype=bool)
    cm[HANDS] = True
    return target, fm, cm


def reference_loop(kind, N, mems, masks, init, step_noise, target, fm, cm, step, guided=None, tie=None, source=None, keep=None):
    """The guided loop on the CPU.  mems / masks: the 7 B-row guidance batch (numpy); init [B, L, 128]; step_noise [N, B, L, 128] or
    None; tie int [B, L] or None; source / keep: kept tokens re-noised from the initial draw at the start of every iteration."""
    import torch
    from oracle import denoiser_torch, sampler_ref
    from tests.edit_ref import add_noise
    from tests.longform_ref import tie_copy
    B, L, _ = init.shape
    F = target.shape[1]
    sd_np, vsd = state_dict(1234, 1.0), vae_weights.make_state_dict()
    sd = denoiser_torch.to_torch(sd_np)
    tm = [torch.from_numpy(np.ascontiguousarray(v)) for v in mems]
    tk = {k: (torch.from_numpy(np.ascontiguousarray(v)) if v is not None else None) for k, v in masks.items()}
    fwd = denoiser_torch.denoiser_forward.__wrapped__
    rows6 = [np.ascontiguousarray(v[:CHUNKS * B]) for v in mems]
    masks6 = {k: (None if v is None else np.ascontiguousarray(v[:CHUNKS * B])) for k, v in masks.items()}
    w = np.zeros((B, CHUNKS))
    w[:, 1:] = SCALE
    inv_n = 1.0 / (float(fm.sum()) * float(cm.sum()))
    ref = _sched_ref(kind)
    ref.set_timesteps(N)
    eps0 = (init * np.float32(ref.init_noise_sigma)).astype(np.float32)
    lat = eps0.copy()
    for i, t in enumerate(ref.timesteps):
        if tie is not None:
            lat = tie_copy(lat, tie)
        if keep is not None:
            lat[keep] = add_noise(ref, source, eps0, int(t))[keep]
        if step and (guided is None or i in guided):
            a = float(ref.alphas_cumprod[int(t)])
            new = pose_guide_ref.guide_pose(sd_np, vsd, lat, int(t), rows6, masks6, w, [F] * B, target, fm.astype(np.float64), cm.astype(np.float64),
                                            a ** 0.5, (1.0 - a) ** 0.5, inv_n, step, tie=tie)["x_new"]
            lat = np.asarray(new, dtype=np.float32)          # rounded to float32 at the write
        with torch.no_grad():
            pred = fwd(sd, torch.from_numpy(np.concatenate([lat] * 7)), int(t), tm, tk)[0].numpy()
        if kind == "ddim":
            lat = ref.step(sampler_ref.cfg_combine(pred, SCALE), t, lat, eta=0.0)
        else:
            lat = ref.step(sampler_ref.cfg_combine(pred, SCALE), t, lat, noise=step_noise[i] if int(t) > 0 else None)
    return lat if tie is None else tie_copy(lat, tie)


def _vae():
    from tests.test_gpu_vae_vjp import _model
    return _model()


LOOPS = {"ddim3": ("ddim", 3, None), "ddpm4": ("ddpm", 4, (1, 2))}


@functools.lru_cache(maxsize=None)
def plain_case(name):
    kind, N, guided = LOOPS[name]
    B, L = 1, 4
    cb = inputs.make_cfg_batch(seed=181, B=B, L=L, S=S, pad_tail=PAD)
    target, fm, cm = _pose_targets(182, B, 8 * L, [(0, 5), (0, 22)])
    noise = np.random.Generator(np.random.PCG64(183)).standard_normal((N, B, L, 128), dtype=np.float32)
    args = (kind, N, cb["memories"], cb["masks"], cb["init"], noise, target, fm, cm)
    return cb, target, fm, cm, noise, reference_loop(*args, STEP, guided), reference_loop(*args, 0.0, guided)


@pytest.mark.parametrize("name", list(LOOPS))
def test_pose_keyframe_loop_matches_the_torch_loop_and_the_cpu_loop(name):
    """Fails on a tree without the feature: ``sampler.sample_with_pose_keyframes`` does not exist there."""
    import torch
    from convofusion_amd import edit, sampler
    from tests.gpu_helpers import hip_denoiser, to_dev
    kind, N, guided = LOOPS[name]
    B, L = 1, 4
    cb, target, fm, cm, noise, want, unguided = plain_case(name)
    moved = rel_l2(want, unguided)
    assert moved > 100 * GATE, moved          # (of the reference: the guidance moves the result far beyond the gate)
    m, vae = hip_denoiser(1234, 1.0), _vae()
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=SCALE, eta=0.0, init_latents=to_dev(cb["init"]), guided_iterations=guided)
    if kind == "ddpm":
        kw["step_noise"] = to_dev(noise)
    pose = lambda step, **k: sampler.sample_with_pose_keyframes(m, _sched(kind), mems, masks, vae, to_dev(target), to_dev(fm), step,
                                                                feature_mask=to_dev(cm), **k)
    got = pose(STEP, **kw)
    torch_loop = sampler.sample_with_loss_guidance(m, _sched(kind), mems, masks,
                                                   edit.pose_keyframe_loss(vae, to_dev(target), to_dev(fm), to_dev(cm), fused=True), STEP, **kw)
    e_torch, e_cpu = rel_l2(got.cpu().numpy(), torch_loop.cpu().numpy()), rel_l2(got.cpu().numpy(), want)
    print(f"{name}: sample_with_pose_keyframes vs the torch loop {e_torch:.2e}, vs the CPU loop {e_cpu:.2e} (the torch loop vs the CPU loop "
          f"{rel_l2(torch_loop.cpu().numpy(), want):.2e}); guided vs unguided (reference) {moved:.2e}")
    assert e_torch < GATE and e_cpu < GATE
    assert not got.is_inference() and not got.requires_grad
    # step size 0, and no guided iteration: ``sample``, bit for bit; called under inference mode: the same bits
    del kw["guided_iterations"]
    plain = sampler.sample(m, _sched(kind), mems, masks, **kw)
    assert torch.equal(pose(0.0, **kw), plain)
    assert torch.equal(pose(STEP, guided_iterations=(), **kw), plain)
    with torch.inference_mode():
        again = pose(STEP, guided_iterations=guided, **kw)
    assert torch.equal(again, got)


@functools.lru_cache(maxsize=None)
def tied_case():
    """One utterance, three windows, DDIM-3; key frames in window 1's tied first half, in window 0's second half (their sources) and in
    window 2's free second half."""
    from convofusion_amd import longform
    B, L, N = 3, 16, 3
    cb = inputs.make_cfg_batch(seed=191, B=B, L=L, S=S, pad_tail=PAD)
    target, fm, cm = _pose_targets(192, B, 8 * L, [(1, 20), (0, 100), (2, 110)])
    tie = longform.window_ties(1, 3, L).numpy()
    args = ("ddim", N, cb["memories"], cb["masks"], cb["init"], None, target, fm, cm)
    return cb, target, fm, cm, tie, reference_loop(*args, STEP, tie=tie), reference_loop(*args, 0.0, tie=tie)


def test_tied_run_takes_pose_key_frames_and_keeps_its_tie():
    import torch
    from convofusion_amd import sampler
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, N = 3, 16, 3
    cb, target, fm, cm, tie, want, unguided = tied_case()
    moved = rel_l2(want, unguided)
    assert moved > 100 * GATE, moved
    m, vae = hip_denoiser(1234, 1.0), _vae()
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=SCALE, eta=0.0, init_latents=to_dev(cb["init"]), tie=to_dev(tie))
    pose = lambda step: sampler.sample_with_pose_keyframes(m, _sched("ddim"), mems, masks, vae, to_dev(target), to_dev(fm), step,
                                                           feature_mask=to_dev(cm), **kw)
    got = pose(STEP)
    e = rel_l2(got.cpu().numpy(), want)
    print(f"tied DDIM-3, three windows: vs the CPU loop {e:.2e}; guided vs unguided (reference) {moved:.2e}")
    assert e < GATE
    flat, t = got.reshape(-1, 128), torch.from_numpy(tie.reshape(-1).astype(np.int64)).cuda()
    assert torch.equal(flat[t >= 0], flat[t[t >= 0]])                                   # the returned windows satisfy the tie bit for bit
    # step size 0 on the tied run: ``sample``'s bits; the torch loop still refuses the run
    assert torch.equal(pose(0.0), sampler.sample(m, _sched("ddim"), mems, masks, **kw))
    with pytest.raises(NotImplementedError, match="a tied run"):
        sampler.sample_with_loss_guidance(m, _sched("ddim"), mems, masks, lambda x0: x0.sum(), STEP, **kw)


def test_long_form_synthesis_with_pose_key_frames_group_by_group():
    """3 windows with max_rows = 2: one tied group of two windows, then the third window on its own, keeping its first half from the
    second window's finished second half.  The reference is the CPU loop driven group by group on the global rows' Philox draws."""
    import torch
    from convofusion_amd.longform import group_ties, synthesize_latents, window_groups
    from tests.gpu_helpers import hip_denoiser, to_dev
    U, W, L, N, seed = 1, 3, 16, 3, 17
    B = U * W
    cb = inputs.make_cfg_batch(seed=195, B=B, L=L, S=S, pad_tail=PAD)
    target, fm, cm = _pose_targets(196, B, 8 * L, [(1, 20), (0, 100), (2, 110), (2, 9)])     # (2, 9): a frame of the second run's kept half

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
                                      philox_ref.normal_tensor(seed, 0, range(a, b), 1, L), None, target[a:b], fm[a:b], cm, step,
                                      tie=tie.numpy() if bool((tie >= 0).any()) else None, source=src, keep=keep)
        return out

    want, unguided = reference(STEP), reference(0.0)
    moved = rel_l2(want, unguided)
    assert moved > 100 * GATE, moved
    m, vae = hip_denoiser(1234, 1.0), _vae()
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    kw = dict(n_utterances=U, n_windows=W, L=L, num_inference_steps=N, guidance_scale=SCALE, seed=seed, max_rows=2)
    win, seq = synthesize_latents(m, _sched("ddim"), mems, masks, pose_keyframes=(to_dev(target), to_dev(fm), to_dev(cm), STEP, None), vae=vae, **kw)
    e = rel_l2(win.reshape(B, L, 128).cpu().numpy(), want)
    print(f"long-form, 3 windows in runs of 2 + 1, DDIM-3: vs the CPU loop {e:.2e}; guided vs unguided (reference) {moved:.2e}")
    assert e < GATE and tuple(seq.shape) == (U, (W + 1) * L // 2, 128)
    assert torch.equal(win[0, 1, :L // 2], win[0, 0, L // 2:])                          # the tie of the first run
    # without key poses: the bits of the call without the argument
    none, _ = synthesize_latents(m, _sched("ddim"), mems, masks, pose_keyframes=None, **kw)
    plain, _ = synthesize_latents(m, _sched("ddim"), mems, masks, **kw)
    assert torch.equal(none, plain)


def test_guide_pose_between_two_steps_leaves_an_open_run_s_bits():
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    m, vae = hip_denoiser(1234, 1.0), _vae()
    cb, target, fm, cm, _, _, _ = plain_case("ddim3")
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    six = [v[:CHUNKS].contiguous() for v in mems]
    six_masks = {k: (None if v is None else v[:CHUNKS].contiguous()) for k, v in masks.items()}
    w = torch.tensor([[0.0] + [SCALE] * (CHUNKS - 1)], device="cuda")
    x = to_dev(cb["init"])

    def go(interleave):
        new = []
        with SamplingRun(m, _sched("ddim"), mems, masks, 1, 4, 4, guidance_scale=SCALE, eta=0.0, seed=3) as run:
            for _ in range(4):
                run.steps(1)
                if interleave:
                    new.append(m.guide_pose(x, 500, six, six_masks, w, vae, to_dev(target), to_dev(fm), feature_mask=to_dev(cm), sqrt_acp=0.8,
                                            sqrt_1m_acp=0.6, step=STEP, side_engine=True, want=("x_new",))[2])
            return run.read(), new

    plain, _ = go(False)
    mixed, new = go(True)
    assert torch.equal(plain, mixed)
    assert all(torch.equal(v, new[0]) for v in new) and not torch.equal(new[0], x)
