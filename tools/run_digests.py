"""Developer tool (GPU box): does a change of the host code that opens sampling runs leave every run kind as it was?  Opens each kind at the
small test shape (B = 2, L = 16, memories S = (6, 20, 6, 8, 1) with pad tails (2, 0, 1, 0, 0), 4 iterations, 6 for DPM-Solver++, fixed
seeds, the seeded test weights) and prints one line per run: the SHA-256 of the final latents' bytes, of ``read()`` after every iteration
(``steps``), of the trajectory, the noise and the attention ring where the run has them (``refused=`` with the library's message for a run it does not open), and N, first_iteration, chunks_evaluated and the
non-pointer fields of the run's cfd_sample_args; then the launches of one iteration per class and the SHA-256 of three single forwards
(``Denoiser.forward``: output and att_mats), the word-excitation-guidance lines of ``weg_lines``, the Python loops' lines of ``loop_lines``
and the lines of the row-tile gradient engine's other callers, ``grad_lines``.  The runs are deterministic: the outputs of two trees are compared with ``diff``, and a
line that differs is a change of behaviour.

Usage (once in each tree):  python tools/run_digests.py > digests.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from convofusion_amd import _lib, sampler, scheduler  # noqa: E402
from convofusion_amd.longform import window_ties  # noqa: E402
from oracle import inputs  # noqa: E402
from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev  # noqa: E402

B, L, S, PAD, N_IT, SEED = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), 4, 7
ARG_FIELDS = ("B", "L", "G", "guidance_weight", "scheduler", "num_train_timesteps", "num_inference_steps", "clip_sample", "eta",
              "set_alpha_to_one", "steps_offset", "preseq_len", "seed", "first_utterance", "skip_zero_weight_chunks", "dynamic_memory_mask",
              "operand_policy", "census_tau", "num_timesteps")
YAML = {k: v for k, v in SCHED_KW.items() if k != "clip_sample"}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def args_text(a):
    vals = {f: getattr(a, f) for f in ARG_FIELDS}
    vals["guidance_weight"] = [float(v) for v in vals["guidance_weight"]]
    return " ".join(f"{k}={v!r}" for k, v in vals.items())


def line(name, **parts):
    print(name + ": " + " ".join(f"{k}={v}" for k, v in parts.items()), flush=True)


def run_line(name, sch, mems, masks, n=N_IT, **kw):
    """One SamplingRun, stepped one iteration at a time; returns the closed run and its final latents."""
    try:
        run = sampler.SamplingRun(hip_denoiser(1234, 1.0), sch, mems, masks, B, L, n, seed=SEED, **kw)
    except _lib.CfdError as e:   # (a kind the developer knobs in force rule out: the attention ring on the three-launch cross-attention)
        line(name, refused=e)
        return None, None
    parts = {}
    try:
        h = hashlib.sha256()
        for _ in range(run.N):
            run.steps(1)
            h.update(run.read().cpu().numpy().tobytes())
        lat = run.read(close=True)
        parts["final"], parts["steps"] = sha(lat), h.hexdigest()
    except sampler.CensusTripped as e:
        lat = None
        parts["census_tripped"] = e.census["iterations"]
    finally:
        run.close()
    if run.trajectory is not None:
        parts["trajectory"] = sha(run.trajectory)
    if run.att_ring is not None:
        parts["att_ring"] = sha(*run.att_ring)
    line(name, **parts, N=run.N, first_iteration=run.first_iteration, chunks_evaluated=run.chunks_evaluated, timesteps=run.timesteps,
         guard=run._guard, args=args_text(run._args))
    return run, lat


def main():
    cb = inputs.make_cfg_batch(seed=1, B=B, L=L, S=S, pad_tail=PAD)
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    m = hip_denoiser(1234, 1.0)
    g = torch.Generator().manual_seed(11)
    source = torch.randn((B, L, 128), generator=g).cuda()
    keep = torch.zeros((B, L), dtype=torch.bool)
    keep[:, :L // 2] = True
    keep = keep.cuda()
    ddpm = lambda: scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)  # noqa: E731
    ddim = lambda **k: scheduler.DDIMScheduler(**dict(SCHED_KW, **k))  # noqa: E731

    run_line("ddpm", ddpm(), mems, masks)
    run_line("ddpm skip_zero_weight_chunks", ddpm(), mems, masks, skip_zero_weight_chunks=True)
    for prune in (True, False):
        run_line(f"ddpm modality_weights apb=0 lsnid=0 prune={prune}", ddpm(), mems, masks, modality_weights=dict(apb=0.0, lsnid=0.0),
                 prune_zero_weight_chunks=prune)
    run_line("ddim", ddim(), mems, masks)
    run_line("dpm-solver++", scheduler.DPMSolverMultistepScheduler(**YAML), mems, masks, n=6)
    run_line("ddpm preseq 4", ddpm(), mems, masks, preseq=source[:, :4].contiguous())
    run_line("edit keep_mask strength=0.5", ddpm(), mems, masks, source_latents=source, keep_mask=keep, strength=0.5)
    tie = window_ties(1, B, L).cuda()
    run_line("tied", ddpm(), mems, masks, tie=tie)
    tkeep = torch.zeros((B, L), dtype=torch.bool)
    tkeep[0, :4] = tkeep[1, 12:] = True
    run_line("tied with edit", ddpm(), mems, masks, tie=tie, source_latents=source, keep_mask=tkeep.cuda())

    inv = scheduler.DDIMInverseScheduler(**SCHED_KW)
    lat, traj = sampler.invert(m, inv, mems, masks, source_latents=source, num_inference_steps=N_IT, return_trajectory=True)
    line("invert return_trajectory", final=sha(lat), trajectory=sha(traj))
    run_line("ddim inverse run trajectory=True", inv, mems, masks, init_latents=source, trajectory=True,
             modality_weights=sampler.INVERSION_WEIGHTS, guidance_scale=1.0)
    run_line("anchored over the inversion's trajectory", ddim(clip_sample=False), mems, masks, anchor_trajectory=traj, keep_mask=keep)

    traj, noise = sampler.invert_ddpm(m, ddpm(), mems, masks, source_latents=source, num_inference_steps=N_IT, seed=SEED)
    line("invert_ddpm", trajectory=sha(traj), noise=sha(noise), last=sampler.invert_ddpm.last)
    run_line("replay strength=0.5", ddpm(), mems, masks, noise_space=(traj, noise), keep_mask=keep, strength=0.5)

    lat, ptraj, stats = sampler.sample_parallel(m, ddpm(), mems, masks, B=B, L=L, num_inference_steps=N_IT, tolerance=0, levels_per_batch=2,
                                                seed=SEED, trajectory=True)
    line("sample_parallel tolerance=0 levels_per_batch=2", final=sha(lat), trajectory=sha(ptraj), sweeps=stats.sweeps, strides=stats.strides,
         levels_per_batch=stats.levels_per_batch, chunks_evaluated=stats.chunks_evaluated)

    run_line("attention_ring", ddpm(), mems, masks, attention_ring=True)
    uq = [to_dev(u) for u in cb["unique"]]
    cm = {k: (v[6 * B:] if v is not None else None) for k, v in masks.items()}      # chunk 6 = full conditioning
    um = {k: (v[:1] if v is not None else None) for k, v in masks.items()}          # chunk 0 = all dropped
    u_mems, maps, u_masks = sampler.build_guidance_batch([u[1:] for u in uq], [u[:1] for u in uq], cm, um)
    run_line("build_guidance_batch row_maps", ddpm(), u_mems, u_masks, dedup=False, row_maps=maps)
    run_line("dedup=False dynamic_memories=(0,)", ddpm(), [x.clone() for x in mems], masks, dedup=False, dynamic_memories=(0,))
    run_line("operands=0", ddpm(), mems, masks, operands=0)
    run_line("operands=auto", ddpm(), mems, masks, operands="auto")
    # prediction_type="sample" (new lines only: ARG_FIELDS stays, so that every line above compares with older trees)
    for name, sch in (("ddpm", scheduler.DDPMScheduler(variance_type="fixed_small", prediction_type="sample", **SCHED_KW)),
                      ("ddim", scheduler.DDIMScheduler(prediction_type="sample", **SCHED_KW)),
                      ("dpm-solver++", scheduler.DPMSolverMultistepScheduler(prediction_type="sample", **YAML))):
        run, _ = run_line(f"{name} prediction_type=sample", sch, mems, masks, n=6 if sch.KIND == 2 else N_IT)
        assert run._args.prediction_type == 1
    # the launches of one iteration, per class, and single forwards (new lines only, as above)
    with sampler.SamplingRun(hip_denoiser(1234, 1.0), ddpm(), mems, masks, B, L, N_IT, seed=SEED) as run:
        run.steps(1)
        line("ddpm launches per iteration", **{k: n for k, (_, n) in run.profile().items()})
    Be = 7 * B
    for name, Lf, t in (("one timestep, att_mats", L, torch.tensor(500)), ("per-row timesteps", L, (torch.arange(Be) * 71 + 3) % 1000),
                        ("L=24", 24, torch.tensor(500))):
        x = torch.randn((Be, Lf, 128), generator=torch.Generator().manual_seed(12)).cuda()
        with torch.no_grad():
            out, att = m(x, t, mems, mem_mask_dict=masks)
        line(f"forward {name}", out=sha(out), att_mats=sha(*att))
    loop_lines(m, mems, masks, *weg_lines(m))
    grad_lines(m, cb, mems, masks)


def weg_lines(m):
    """Word-excitation guidance (new lines only, as above): the state-machine walk of tests/test_gpu_weg.py, one line per cfd_weg_eval
    -- results, loss and "weg.info" -- and the latents of a five-iteration guided loop at the same shape."""
    from convofusion_amd import weg
    from oracle import philox_ref
    from tests.gpu_helpers import read_debug
    from tests.test_gpu_weg import STATE_WALK, STATE_WALK_FOCUS, state_walk_inputs
    data = state_walk_inputs()
    for n, (name, t, fk, same) in enumerate(STATE_WALK, 1):
        inp, wmems, wmasks, eot = data[name]
        loss, losses, mx, grad = weg.loss_and_grad(m, to_dev(inp["sample"]), t, wmems, wmasks, STATE_WALK_FOCUS[fk], True, to_dev(eot),
                                                   same_conditioning=same)
        line(f"weg walk {n} {name} t={t} {fk} same_conditioning={same}", results=sha(losses, torch.stack([v for r in mx for v in r]), grad),
             loss=repr(float(loss)), info=[float(v) for v in read_debug(m, "weg.info", (5,))])
    cb = inputs.make_cfg_batch(seed=23, B=1, L=16, S=(6, 20, 12, 8, 1), pad_tail=(2, 0, 3, 0, 0))
    params = dict(scale_factor=1000, scale_range=[1.0, 0.5], max_iter_to_alter=3, thresholds={1: 0.16}, max_refinement_steps=3)
    lat = sampler.sample_with_weg(m, scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW), [to_dev(x) for x in cb["memories"]],
                                  {k: to_dev(v) for k, v in cb["masks"].items()}, [[2, 5]], params, B=1, L=16, num_inference_steps=5,
                                  guidance_scale=7.5, init_latents=to_dev(philox_ref.normal_tensor(23, 0, range(1), 1, 16)), seed=2)
    line("sample_with_weg 5 iterations", final=sha(lat))
    return cb, params


def att_sha(att):
    """The maps of one iteration (5 tensors) or a dict {timestep: maps}: the timesteps and the SHA-256 of every tensor in order."""
    if isinstance(att, dict):
        return f"{list(att)}:{sha(*[a for maps in att.values() for a in maps])}"
    return sha(*att)


def loop_lines(m, mems, masks, cb1, params):
    """The Python drivers of an open run (new lines only, as above): ``sample`` with its attention modes at the small shape, and the two
    guided loops at the B = 1 shape of ``weg_lines``."""
    from oracle import philox_ref
    ddpm = lambda: scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)  # noqa: E731
    for mode in (True, "all", "auto"):
        lat, att = sampler.sample(m, ddpm(), mems, masks, B=B, L=L, num_inference_steps=N_IT, seed=SEED, return_attention=mode)
        line(f"sample return_attention={mode!r}", final=sha(lat), maps=att_sha(att))
    mems1, masks1 = [to_dev(x) for x in cb1["memories"]], {k: to_dev(v) for k, v in cb1["masks"].items()}
    init = to_dev(philox_ref.normal_tensor(23, 0, range(1), 1, 16))
    for mode in (True, "all"):
        lat, att = sampler.sample_with_weg(m, ddpm(), mems1, masks1, [[2, 5]], params, B=1, L=16, num_inference_steps=5, guidance_scale=7.5,
                                           init_latents=init, seed=2, return_attention=mode)
        line(f"sample_with_weg return_attention={mode!r}", final=sha(lat), maps=att_sha(att))
    target = torch.randn((1, 16, 128), generator=torch.Generator().manual_seed(13)).cuda()
    for guided in ((1, 3), None):
        lat = sampler.sample_with_loss_guidance(m, ddpm(), mems1, masks1, lambda x0: ((x0 - target) ** 2).sum(), 0.05, B=1, L=16,
                                                num_inference_steps=N_IT, guidance_scale=7.5, init_latents=init, seed=2,
                                                guided_iterations=guided)
        line(f"sample_with_loss_guidance guided_iterations={guided}", final=sha(lat))


def grad_lines(m, cb, mems, masks):
    """``Denoiser.vjp``, ``vjp_memories`` and ``guide`` and the key-pose loop (new lines only, as above) at the small shape with three
    guidance chunks: every result and "weg.info" as the call left it."""
    import ctypes as C

    def info(side=False):      # of the engine the calls ran on: the key-pose loop's guide calls run on the denoiser's second engine
        out = torch.empty(5, dtype=torch.float32, device="cuda")
        h = m._side["handle"] if side else m._handle
        _lib.check(_lib.load().cfd_debug_read(h, b"weg.info", C.c_void_p(out.data_ptr()), 5))
        return [float(v) for v in out.cpu()]

    chunks, t = [0, 1, 2], 500
    n = len(chunks)
    states, cmasks = sampler.guidance_chunk_rows(mems, masks, chunks, 7, B)
    states = [e.contiguous() for e in states]
    g = torch.Generator().manual_seed(21)
    x = torch.randn((B, L, 128), generator=g).cuda()
    xin, d_out = x.repeat(n, 1, 1), torch.randn((n * B, L, 128), generator=g).cuda()
    out, grad = m.vjp(xin, t, states, cmasks, d_out)
    line("Denoiser.vjp", out=sha(out), grad=sha(grad), info=info())
    rows = np.concatenate([np.arange(c * B, (c + 1) * B) for c in chunks])
    maps = [to_dev(np.ascontiguousarray(cb["row_map"][j][rows])) for j in range(5)]
    umasks = {}
    for j, k in enumerate(inputs.MEM_NAMES):
        mk = cb["masks"][k]
        umasks[k] = None if mk is None else to_dev(np.stack([mk[list(cb["row_map"][j]).index(u)] for u in range(B + 1)]))
    out, grad, d_mem = m.vjp_memories(xin, t, [to_dev(u) for u in cb["unique"]], umasks, d_out, row_maps=maps)
    line("Denoiser.vjp_memories row_maps", out=sha(out), grad=sha(grad), info=info(), **{k: sha(v) for k, v in d_mem.items()})
    w = torch.tensor([[0.0, 0.4, 0.25], [0.0, 1.5, 2.0]]).cuda()
    target = (torch.randn((B, L, 128), generator=g) * 0.5).cuda()
    mask = torch.zeros((B, L))
    mask[:, 1::3] = 1
    mask = mask.cuda()
    acp = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW).alphas_cumprod.detach().to("cpu", torch.float64)
    tie = window_ties(1, B, L).cuda()

    def guide(name, tt, reuse, tie=None):
        a = float(acp[tt])
        r = m.guide(x, tt, states, cmasks, w, target, mask, sqrt_acp=a ** 0.5, sqrt_1m_acp=(1.0 - a) ** 0.5, step=0.5, tie=tie,
                    reuse_memory_side=reuse, want=("loss", "grad", "x_new", "d_out"))
        line(f"Denoiser.guide {name} t={tt} reuse_memory_side={reuse}", loss=sha(r[0]), grad=sha(r[1]), x_new=sha(r[2]), d_out=sha(r[3]), info=info())

    guide("fresh", t, 0)
    guide("tables over every timestep", t, 2)
    guide("another timestep", t - 1, 2)
    guide("tied", t, 0, tie)
    ddpm = lambda: scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)  # noqa: E731
    for name, kw in (("plain", {}), ("tied", dict(tie=tie))):
        lat = sampler.sample_with_keyframes(m, ddpm(), mems, masks, target, mask, 0.05, B=B, L=L, num_inference_steps=N_IT, seed=SEED,
                                            modality_weights=dict(text=0.0, apb=0.0, lsnid=0.0), **kw)
        line(f"sample_with_keyframes {name} 4 iterations 3 chunks", final=sha(lat), info=info(side=True))


if __name__ == "__main__":
    main()
