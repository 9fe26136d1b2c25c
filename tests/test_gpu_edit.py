"""-m gpu: motion editing in the captured loop (cfd_sample_begin_edit, ``SamplingRun(source_latents=, keep_mask=, strength=)``,
``convofusion_amd.edit``).

The edit loop against trajectories made with the REFERENCE denoiser and the restated edit loop (tests/golden/traj_edit_*.npz,
make_golden_edit.py), the no-op edit against the plain loop (bit for bit), the masked overwrite's exact values, composition with weight
tables, pruning, WEG and per-utterance rows, ``edit_motion`` against its steps done by hand, and the ABI's refusals.  Errors are printed."""
import ctypes as C

import numpy as np
import pytest

from oracle import inputs, philox_ref, vae_weights
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-3          # as tests/test_gpu_modality_weights.py
DPM_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _sched(kind):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    if kind == "dpmpp":
        return scheduler.DPMSolverMultistepScheduler(**DPM_KW)
    return scheduler.DDIMScheduler(**SCHED_KW) if kind == "ddim" else scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)


def _inputs(B, L, S, pad, seed):
    from tests.gpu_helpers import to_dev
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    return [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}


def _small(B=2, seed=2026):
    return _inputs(B, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), seed)


def _source(B, seed, L=16):
    from tests.gpu_helpers import to_dev
    return to_dev((0.8 * philox_ref.normal_tensor(seed, 0, range(B), 2, L)).astype(np.float32))


def _keep(B, seed, L=16):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, L), generator=g) < 0.5).cuda()


@pytest.mark.parametrize("operands", [None, 0])
@pytest.mark.parametrize("name", ["hands_ddpm20", "between_ddpm20", "dpmpp10"])
def test_edit_loop_matches_reference_trajectory(name, operands):
    """Per-utterance keep masks and a start iteration k0 from the strength, against the restated edit loop on the reference denoiser: every
    snapshot and the final latents within TRAJ_TOL relative L2."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g = load_golden("traj_edit_" + name)
    meta = [int(x) for x in g["meta"]]
    B, L, S, pad, n, seed = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13]
    mems, masks = _inputs(B, L, S, pad, seed)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    kind = "dpmpp" if "dpmpp" in name else "ddpm"
    noise = None if kind == "dpmpp" else to_dev(np.stack([philox_ref.normal_tensor(seed, i, range(B), 0, L) for i in range(n)]))
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched(kind), mems, masks, B, L, n, guidance_scale=7.5, init_latents=to_dev(init),
                      step_noise=noise, operands=operands, source_latents=to_dev(g["source"]),
                      keep_mask=torch.from_numpy(g["keep"]).bool().cuda(), strength=float(g["strength"]))
    assert run.first_iteration == int(g["k0"]) and run.N == n - int(g["k0"])
    errs = {}
    for k in sorted(int(f[4:]) for f in g.files if f.startswith("step")):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"step{k}"])
    run.steps(run.N - run.position)
    lat = run.read(close=True).cpu().numpy()
    errs["final"] = rel_l2(lat, g["latents"])
    print("edit", name, "k0", int(g["k0"]), "operands", operands, {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs


@pytest.mark.parametrize("kind", ["ddpm", "dpmpp"])
def test_no_op_edit_is_bit_identical_to_sample(kind):
    """strength 1 and an all-zero mask (and a source without a mask): the latents of sample() bit for bit -- the edit instance of the begin
    kernel overwrites nothing and the run starts at iteration 0 from the same draw."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    B, L, n, seed = 2, 16, 10, 5
    mems, masks = _small(B, seed)
    src = _source(B, seed)
    kw = dict(B=B, L=L, num_inference_steps=n, seed=seed, skip_zero_weight_chunks=True)
    plain = sample(m, _sched(kind), mems, masks, **kw)
    zero = sample(m, _sched(kind), mems, masks, source_latents=src, keep_mask=torch.zeros((B, L), dtype=torch.bool, device="cuda"), **kw)
    nomask = sample(m, _sched(kind), mems, masks, source_latents=src, **kw)
    assert torch.isfinite(plain).all()
    assert torch.equal(plain, zero) and torch.equal(plain, nomask)


def test_inpaint_sets_the_kept_tokens_exactly():
    """run.inpaint() at several iterations: the kept tokens equal sa_i * src + sb_i * eps in float32 (each product and the sum rounded on
    their own; sa_i / sb_i = sqrt(abar), sqrt(1 - abar) of iteration i's timestep), the others are untouched.  With strength 0.75 the run
    starts at k0 = 5 with every token at sa_k0 * src + sb_k0 * eps."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, n, seed = 2, 16, 20, 8
    mems, masks = _small(B, seed)
    src = _source(B, seed)
    keep = _keep(B, seed)
    eps = to_dev(philox_ref.normal_tensor(seed, 0, range(B), 1, L))
    sch = _sched("ddpm")
    run = SamplingRun(hip_denoiser(1234, 1.0), sch, mems, masks, B, L, n, guidance_scale=7.5, init_latents=eps, seed=seed,
                      source_latents=src, keep_mask=keep, strength=0.75)
    ac = sch.alphas_cumprod.to("cuda", torch.float32)

    def mix(i):
        t = run.timesteps[i - run.first_iteration]
        sa, sb = ac[t].sqrt(), (1.0 - ac[t]).sqrt()
        return sa * src + sb * eps

    assert run.first_iteration == 5 and run.N == 15
    assert torch.equal(run.read(), mix(5))
    checked = 0
    for pos in (0, 3, 9, 14):
        run.steps(pos - run.position)
        before = run.read()
        run.inpaint()
        after = run.read()
        want = mix(run.first_iteration + pos)
        assert torch.equal(after[keep], want[keep]), pos
        assert torch.equal(after[~keep], before[~keep]), pos
        checked += 1
        run.steps(1)            # (the captured iteration skips the overwrite it has had)
        assert torch.isfinite(run.read()).all()
    run.close()
    assert checked == 4 and int(keep.sum()) > 0 and int((~keep).sum()) > 0


def test_edit_composes_with_a_weight_table_and_pruning():
    """An [N, B, 6] weight table whose apb / lsnid / all columns are 0 throughout: the pruned edit run (4 chunks) within 1e-6 of the
    unpruned one (7 chunks), and different from the run without the table."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    B, L, n, seed = 3, 16, 20, 31
    mems, masks = _small(B, seed)
    src = _source(B, seed)
    keep = _keep(B, seed)
    rng = np.random.default_rng(7)
    w = rng.uniform(0.0, 2.0, size=(n, B, 6))
    w[:, :, 3:] = 0.0
    outs = {}
    for prune in (True, False):
        with SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, modality_weights=torch.from_numpy(w),
                         prune_zero_weight_chunks=prune, source_latents=src, keep_mask=keep, strength=0.6) as run:
            assert run.chunks_evaluated == (4 if prune else 7) and run.first_iteration == 8
            run.steps(run.N)
            outs[prune] = run.read(close=True)
    e = float((outs[True] - outs[False]).norm() / outs[False].norm())
    with SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, source_latents=src, keep_mask=keep,
                     strength=0.6) as run:
        assert run.chunks_evaluated == 7
        run.steps(run.N)
        plain = run.read(close=True)
    d = float((outs[False] - plain).norm() / plain.norm())
    print(f"edit: pruned (4 chunks) vs unpruned (7): {e:.2e}; weighted vs reference weights {d:.2e}")
    assert torch.isfinite(outs[True]).all() and e < 1e-6 and d > 1e-3


def test_weg_runs_with_a_keep_mask_on_ddpm():
    """sample_with_weg with an edit (DDPM): the masked overwrite goes in before the WEG update.  An all-zero mask gives the WEG run's
    latents bit for bit; a body mask changes them."""
    import torch
    from convofusion_amd.edit import token_mask
    from convofusion_amd.sampler import sample_with_weg
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    B, L, n, seed = 1, 16, 10, 21
    mems, masks = _inputs(B, L, (6, 20, 12, 8, 1), (2, 0, 3, 0, 0), 4)
    src = _source(B, seed)
    wp = dict(scale_factor=1000, scale_range=[1.0, 0.5], max_iter_to_alter=4, thresholds={0: 0.05}, max_refinement_steps=1)
    kw = dict(B=B, L=L, num_inference_steps=n, seed=seed, guidance_scale=7.5, skip_zero_weight_chunks=True)
    plain = sample_with_weg(m, _sched("ddpm"), mems, masks, [[2, 4]], wp, **kw)
    zero = sample_with_weg(m, _sched("ddpm"), mems, masks, [[2, 4]], wp, source_latents=src,
                           keep_mask=torch.zeros((B, L), dtype=torch.bool, device="cuda"), **kw)
    keep = token_mask(B, keep_parts=("body",)).cuda()
    body = sample_with_weg(m, _sched("ddpm"), mems, masks, [[2, 4]], wp, source_latents=src, keep_mask=keep, **kw)
    assert torch.isfinite(plain).all() and torch.isfinite(body).all()
    assert torch.equal(plain, zero)
    assert (body - plain).norm() / plain.norm() > 1e-3
    with pytest.raises(NotImplementedError):
        sample_with_weg(m, _sched("dpmpp"), mems, masks, [[2, 4]], wp, source_latents=src, keep_mask=keep, **kw)


def test_per_utterance_masks_match_one_utterance_runs():
    """Row b of a three-utterance edit run (a different mask per utterance, strength 0.6) equals a B = 1 run of utterance b's inputs, source
    and mask with first_utterance = b within 1e-5 (Philox streams are keyed by global utterance id; the shapes may take other kernels)."""
    from convofusion_amd.distributed import shard_cfg_batch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    B, L, n, seed = 3, 16, 20, 12
    mems, masks = _small(B, seed)
    src = _source(B, seed)
    keep = _keep(B, seed)
    full = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, source_latents=src, keep_mask=keep,
                  strength=0.6)
    for b in range(B):
        enc = [shard_cfg_batch(x, b, b + 1, B) for x in mems]
        mk = {k: shard_cfg_batch(v, b, b + 1, B) for k, v in masks.items()}
        one = sample(m, _sched("ddpm"), enc, mk, B=1, L=L, num_inference_steps=n, seed=seed, first_utterance=b,
                     source_latents=src[b:b + 1], keep_mask=keep[b:b + 1], strength=0.6)
        e = float((one[0] - full[b]).norm() / full[b].norm())
        print(f"utterance {b}: {e:.2e}")
        assert e < 1e-5


def test_attention_ring_of_an_edit_run_holds_the_executed_iterations():
    """return_attention="all" with strength 0.6: one entry per executed iteration (ring slot j = iteration k0 + j), the latents those of
    the run without maps within 1e-6 (the ring evaluates the full-conditioning chunk too)."""
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    B, L, n, seed = 2, 16, 20, 3
    mems, masks = _small(B, seed)
    src = _source(B, seed)
    keep = _keep(B, seed)
    kw = dict(B=B, L=L, num_inference_steps=n, seed=seed, source_latents=src, keep_mask=keep, strength=0.6)
    lat, atts = sample(m, _sched("ddpm"), mems, masks, return_attention="all", **kw)
    want = sample(m, _sched("ddpm"), mems, masks, **kw)
    e = float((lat - want).norm() / want.norm())
    assert sorted(atts, reverse=True) == list(range(550, -1, -50))      # DDPM-20's table 950, 900, ... 0 from k0 = 8 on
    assert all(len(v) == 5 and all(np.isfinite(a.cpu().numpy()).all() for a in v) for v in atts.values())
    assert e < 1e-6, e


def _vae():
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    from tests.test_vae_encode_host import ABL, KW
    v = ConvoFusionVae(ablation=ABL, **KW)
    v.load_state_dict({k: torch.from_numpy(a) for k, a in vae_weights.make_state_dict().items()}, strict=True)
    return v.cuda().eval()


def test_latent_parts_follow_the_encoder_stacks():
    """LATENT_PARTS is read off encode: changing only the hands features moves only stack part_index("hands") of the posterior mean."""
    import torch
    from convofusion_amd.edit import part_index
    vae = _vae()
    g = torch.Generator().manual_seed(3)
    f = torch.randn((2, 64, 189), generator=g).cuda()
    f2 = f.clone()
    f2[..., 69:] += 0.5                    # the hands' 40 x 3 feature columns (vae.py:53-54)
    mu1 = vae.encode(f)[1].mean.reshape(2, 2, 4, 128)
    mu2 = vae.encode(f2)[1].mean.reshape(2, 2, 4, 128)
    h, b = part_index("hands"), part_index("body")
    assert torch.equal(mu1[b], mu2[b]) and not torch.equal(mu1[h], mu2[h])


def test_edit_motion_equals_its_steps_by_hand():
    """edit_motion = HIP encode (posterior mean) -> vae_to_loop -> sample(edit) -> loop_to_vae -> HIP decode, bit for bit, on seeded VAE
    and denoiser weights."""
    import torch
    from types import SimpleNamespace
    from convofusion_amd.edit import edit_motion, loop_to_vae, token_mask, vae_to_loop
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    B, n, seed = 2, 10, 17
    mems, masks = _inputs(B, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), seed)
    model = SimpleNamespace(vae=_vae(), denoiser=hip_denoiser(1234, 1.0), scheduler=_sched("ddpm"), guidance_scale=7.5, clf_guidance_drops=6,
                            do_classifier_free_guidance=True,
                            cfg=SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=n, eta=0.0))))
    g = torch.Generator().manual_seed(seed)
    feats = (0.5 * torch.randn((B, 128, 189), generator=g)).cuda()
    lengths = [128, 128]
    keep = token_mask(B, keep_frames=[(0, 32), (96, 128)]).cuda()
    out, lat = edit_motion(model, feats, lengths, mems, masks, keep_mask=keep, strength=0.8, seed=seed)
    _, dist, _ = model.vae.encode(feats, lengths)
    src = vae_to_loop(dist.mean.reshape(2, B, 8, 128))
    want_lat = sample(model.denoiser, _sched("ddpm"), mems, masks, B=B, L=16, num_inference_steps=n, guidance_scale=7.5, seed=seed,
                      skip_zero_weight_chunks=True, source_latents=src, keep_mask=keep, strength=0.8)
    want = model.vae.decode(loop_to_vae(want_lat), lengths)
    assert tuple(out.shape) == (B, 128, 189) and tuple(lat.shape) == (B, 16, 128)
    assert torch.equal(lat, want_lat) and torch.equal(out, want)
    assert torch.isfinite(out).all()


def test_abi_refusals():
    """cfd_sample_begin_edit refuses a NULL edit, a NULL source, a first iteration outside [0, N), a keep value of 2 and preseq with an edit
    (CFD_E_ARG); a good call afterwards opens a run on the same handle."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    B, L, n = 1, 16, 10
    mems, masks = _small(B, 4)
    src = _source(B, 4)
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=1)
    run.close()
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad_keep = torch.zeros((B, L), dtype=torch.uint8, device="cuda")
    bad_keep[0, 3] = 2
    good_keep = torch.ones((B, L), dtype=torch.uint8, device="cuda")
    preseq = torch.zeros((B, 4, 128), device="cuda")
    g_eval = C.c_int(-7)

    def call(source, keep, k0, with_preseq=False, null_edit=False):
        a = _lib.SampleArgs.from_buffer_copy(run._args)
        if with_preseq:
            a.preseq, a.preseq_len = preseq.data_ptr(), 4
        e = _lib.EditArgs()
        e.source = source.data_ptr() if source is not None else None
        e.keep = keep.data_ptr() if keep is not None else None
        e.first_iteration = k0
        return lib.cfd_sample_begin_edit(run.handle, C.byref(a), None if null_edit else C.byref(e), None, 1, C.byref(g_eval), stream)

    for what, args in (("NULL edit", (src, None, 0, False, True)), ("NULL source", (None, good_keep, 0)), ("k0 = -1", (src, good_keep, -1)),
                       ("k0 = N", (src, good_keep, n)), ("keep 2", (src, bad_keep, 0)), ("preseq", (src, good_keep, 0, True))):
        rc = call(*args)
        print(what, "->", rc, lib.cfd_last_error().decode())
        assert rc == -1, what
    assert call(src, good_keep, 4) == 0 and g_eval.value == 7
    assert lib.cfd_sample_position(run.handle) == 0
    out = torch.empty((B, L, 128), device="cuda")
    assert lib.cfd_sample_steps(run.handle, n - 4 + 1) == -1          # the run has n - k0 iterations
    assert lib.cfd_sample_steps(run.handle, n - 4) == 0 and lib.cfd_sample_position(run.handle) == n - 4
    assert lib.cfd_sample_read(run.handle, C.c_void_p(out.data_ptr()), 1) == 0
    assert torch.isfinite(out).all()
