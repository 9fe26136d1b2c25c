"""-m gpu: ``run.inpaint()`` before every ``steps(1)`` changes nothing.

The start-of-iteration overwrite is written in begin_step_kernel (inside the captured iteration) and again in inpaint_now_kernel
(``cfd_sample_inpaint``, after which the captured iteration skips its own).  For each of the four begin instances -- default with a preseq,
edit, anchored, tied -- a run that calls ``inpaint()`` before every iteration is compared bit for bit with a run that never calls it: the
kept / tied / preseq tokens after every iteration, and the whole final latents.  tools/run_digests.py's small shape."""
import pytest

from oracle import inputs

pytestmark = pytest.mark.gpu
B, L, S, PAD, N_IT, SEED = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), 4, 7
LEGS = ("preseq", "edit", "anchored", "tied")


@pytest.fixture(scope="module")
def setup():
    import torch
    from tests.gpu_helpers import to_dev
    cb = inputs.make_cfg_batch(seed=1, B=B, L=L, S=S, pad_tail=PAD)
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    source = torch.randn((B, L, 128), generator=torch.Generator().manual_seed(11)).cuda()
    keep = torch.zeros((B, L), dtype=torch.bool)
    keep[:, :L // 2] = True
    return mems, masks, source, keep.cuda()


def _leg(leg, setup):
    """(scheduler, SamplingRun keywords, [B][L] mask of the tokens the overwrite sets) of a leg"""
    import torch
    from convofusion_amd import sampler, scheduler
    from convofusion_amd.longform import window_ties
    from tests.gpu_helpers import SCHED_KW, hip_denoiser
    mems, masks, source, keep = setup
    ddpm = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    if leg == "preseq":      # the default instance: the first 5 of 16 tokens
        first = torch.zeros((B, L), dtype=torch.bool, device="cuda")
        first[:, :5] = True
        return ddpm, dict(preseq=source[:, :5].contiguous()), first
    if leg == "edit":
        return ddpm, dict(source_latents=source, keep_mask=keep), keep
    if leg == "anchored":    # a DDIM run over the trajectory of the source's inversion
        _, traj = sampler.invert(hip_denoiser(1234, 1.0), scheduler.DDIMInverseScheduler(**SCHED_KW), mems, masks, source_latents=source,
                                 num_inference_steps=N_IT, return_trajectory=True)
        return scheduler.DDIMScheduler(**dict(SCHED_KW, clip_sample=False)), dict(anchor_trajectory=traj, keep_mask=keep), keep
    tie = window_ties(1, B, L).cuda()
    return ddpm, dict(tie=tie), tie >= 0


def _run(sch, kw, setup, inpaint):
    """The latents after every iteration and the closed run's final latents"""
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    mems, masks = setup[:2]
    run = SamplingRun(hip_denoiser(1234, 1.0), sch, mems, masks, B, L, N_IT, seed=SEED, **kw)
    snaps = []
    try:
        assert run.N == N_IT
        for _ in range(run.N):
            if inpaint:
                run.inpaint()
            run.steps(1)
            snaps.append(run.read().clone())
        return snaps, run.read(close=True).clone()
    finally:
        run.close()


@pytest.mark.parametrize("leg", LEGS)
def test_inpaint_before_every_step_is_bit_identical(leg, setup):
    import torch
    sch, kw, fixed = _leg(leg, setup)
    assert 0 < int(fixed.sum()) < B * L
    snaps_a, final_a = _run(sch, kw, setup, inpaint=True)
    snaps_b, final_b = _run(sch, kw, setup, inpaint=False)
    assert torch.isfinite(final_b).all()
    for i, (a, b) in enumerate(zip(snaps_a, snaps_b)):
        assert torch.equal(a[fixed], b[fixed]), (leg, i)
    assert torch.equal(final_a, final_b), leg
