"""-m gpu: a handle gives back every device buffer it took.  ``cfd_debug_live_buffers`` counts the library's live device buffers and their
bytes over the whole process; a ``Denoiser`` of this test's own goes through one call of every kind that allocates on a handle, is dropped
(``cfd_destroy``), and both counters must be back at their first reading exactly.

Shape: tools/run_digests.py's small one -- B = 2, L = 16, memories S = (6, 20, 6, 8, 1) with pad tails (2, 0, 1, 0, 0), 4 iterations, the
seeded test weights.  Before buffers freed themselves the first case failed by one buffer of 128 bytes: the [B][L] int32 tie table of the
tied run, which cfd_destroy's hand-kept list did not name."""
import ctypes as C
import gc

import pytest

from oracle import inputs

pytestmark = pytest.mark.gpu
B, L, S, PAD, N_IT, SEED = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), 4, 7


def _live():
    from convofusion_amd import _lib
    n, nbytes = C.c_longlong(-1), C.c_longlong(-1)
    _lib.check(_lib.load().cfd_debug_live_buffers(C.byref(n), C.byref(nbytes)))
    return int(n.value), int(nbytes.value)


def _use_every_allocating_call(m, leave_tied_run_open):
    """One forward, a weighted edit run with ties and an attention ring, a DPM-Solver++ run, invert_ddpm, sample_parallel and one
    weg.loss_and_grad on ``m``; returns how many buffers the handle(s) hold afterwards."""
    import torch
    from convofusion_amd import sampler, scheduler, weg
    from convofusion_amd.longform import window_ties
    from tests.gpu_helpers import SCHED_KW, dev_inputs, to_dev
    cb = inputs.make_cfg_batch(seed=1, B=B, L=L, S=S, pad_tail=PAD)
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    ddpm = lambda: scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)  # noqa: E731
    g = torch.Generator().manual_seed(11)
    source = torch.randn((B, L, 128), generator=g).cuda()
    x = torch.randn((7 * B, L, 128), generator=g).cuda()
    with torch.no_grad():
        out, _ = m(x, torch.tensor(500), mems, mem_mask_dict=masks)
    assert torch.isfinite(out).all()

    tie = window_ties(1, B, L).cuda()
    keep = torch.zeros((B, L), dtype=torch.bool)
    keep[0, :4] = keep[1, 12:] = True

    def tied_run():
        return sampler.SamplingRun(m, ddpm(), mems, masks, B, L, N_IT, seed=SEED, tie=tie, source_latents=source, keep_mask=keep.cuda(),
                                   modality_weights=dict(apb=0.0, lsnid=0.0), attention_ring=True)
    run = tied_run()
    run.steps(run.N)
    assert torch.isfinite(run.read(close=True)).all() and all(torch.isfinite(r).all() for r in run.att_ring)

    yaml = {k: v for k, v in SCHED_KW.items() if k != "clip_sample"}
    with sampler.SamplingRun(m, scheduler.DPMSolverMultistepScheduler(**yaml), mems, masks, B, L, 6, seed=SEED) as run:
        run.steps(run.N)
        assert torch.isfinite(run.read()).all()

    traj, noise = sampler.invert_ddpm(m, ddpm(), mems, masks, source_latents=source, num_inference_steps=N_IT, seed=SEED)
    assert torch.isfinite(traj).all() and torch.isfinite(noise).all()
    lat, _ = sampler.sample_parallel(m, ddpm(), mems, masks, B=B, L=L, num_inference_steps=N_IT, tolerance=0, levels_per_batch=2, seed=SEED)
    assert torch.isfinite(lat).all()

    inp = inputs.make_plain_batch(seed=23, Be=B, L=L, S=S, pad_tail=PAD)
    wmems, wmasks = dev_inputs(inp)
    _, _, _, grad = weg.loss_and_grad(m, to_dev(inp["sample"]), 500, wmems, wmasks, [[1, 2], [2]], False)   # (two rows: no end-of-text normalisation)
    assert torch.isfinite(grad).all()

    if leave_tied_run_open:   # the library's run stays open: the wrapper must not close it on its way out
        run = tied_run()
        run.steps(2)
        torch.cuda.synchronize()
        run.open = False
    return _live()[0]


@pytest.mark.parametrize("leave_tied_run_open", [False, True], ids=["runs_closed", "tied_run_left_open"])
def test_destroyed_handle_returns_every_buffer(leave_tied_run_open):
    from tests.gpu_helpers import hip_denoiser
    gc.collect()   # (handles other tests dropped go now, not between the two readings)
    first = _live()
    m = hip_denoiser.__wrapped__(1234, 1.0)   # a Denoiser of this test's own: the cached one outlives the test
    held = _use_every_allocating_call(m, leave_tied_run_open)
    del m
    gc.collect()
    last = _live()
    print("live device buffers (count, bytes): before", first, "after", last, "; held by the handle before the drop:", held - first[0])
    assert held > first[0], "the counters do not see the handle's buffers"
    assert last == first, f"{last[0] - first[0]} buffers / {last[1] - first[1]} bytes were not freed by cfd_destroy"
