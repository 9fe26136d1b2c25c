"""-m gpu: the hipGraph-captured sampling loop against trajectories produced with the REFERENCE denoiser
(tests/golden/traj_*.npz), against the oracle, and size-independent properties at the full benchmark shape.

Tolerance on latents: 1e-3 relative L2 (BASELINE.json north_star); intermediate snapshots likewise.
"""
import numpy as np
import pytest

from oracle import denoiser_ref, inputs, philox_ref, sampler_ref, scheduler_ref
from tests.helpers import load_golden, max_abs, rel_l2, state_dict

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-3


def _sched(kind):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    return scheduler.DDIMScheduler(**SCHED_KW) if kind == "ddim" else scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)


@pytest.mark.parametrize("name", ["ddpm20_b2", "ddim50", "inpaint25", "ddpm1000"])
def test_sampler_matches_reference_trajectory(name):
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    g = load_golden("traj_" + name)
    meta = [int(x) for x in g["meta"]]
    B, L, S, pad, n_steps, seed = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    noise = np.stack([philox_ref.normal_tensor(seed, i, range(B), 0, L) for i in range(n_steps)])
    m = hip_denoiser(1234, 1.0)
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    kind = "ddim" if "ddim" in name else "ddpm"
    run = SamplingRun(m, _sched(kind), mems, masks, B, L, n_steps, guidance_scale=7.5, init_latents=to_dev(init),
                      step_noise=to_dev(noise), preseq=to_dev(g["preseq"]) if "inpaint" in name else None)
    keep = sorted(int(k[4:]) for k in g.files if k.startswith("step"))
    errs = {}
    for k in keep:
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"step{k}"])
    run.steps(n_steps - run.position)
    lat = run.read(close=True).permute(1, 0, 2).cpu().numpy()
    errs["final"] = rel_l2(lat, g["latents"])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all()
    assert all(v < TRAJ_TOL for v in errs.values()), errs
    if kind == "ddpm":      # (the operand policy's adoption gate; these small goldens mostly take the row-tile path, which has no policy)
        assert all(v < 3e-4 for v in errs.values()), errs


@pytest.mark.parametrize("B", [1, 3])
def test_dedup_is_exact(B):
    """Sharing the memory-side projections between guidance replicas must not change the result: bit-for-bit
    when every row takes the per-row attention path (B=1: no shared-memory run reaches 4 rows), to rounding
    when a run of rows attends to the shared audio memory through one un-batched product (B=3: the P.V sum of
    those rows is then split in two accumulation passes)."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    L, S = 16, (24, 161, 24, 8, 1)
    cb = inputs.make_cfg_batch(seed=5, B=B, L=L, S=S, pad_tail=(4, 0, 6, 0, 0))
    m = hip_denoiser(1234, 1.0)
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    a = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=4, seed=11, dedup=True)
    b = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=4, seed=11, dedup=False)
    assert torch.isfinite(a).all()
    if B == 1:
        assert torch.equal(a, b)
    else:
        # a 4-step schedule takes huge steps: rounding-order differences (~1e-6 per forward) are amplified
        # ~50x by the guidance and 1/sqrt(abar) factors; hold the pair to well under the 1e-3 budget
        d = float(((a - b).norm() / b.norm()))
        print("dedup (run path) vs per-row path: rel L2", d)
        assert d < 2e-4


def test_skipping_the_zero_weight_chunk_is_exact():
    """The full-conditioning chunk has guidance weight 7.5 * 0: not evaluating it must not change a bit."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S = 3, 16, (24, 161, 24, 8, 1)
    cb = inputs.make_cfg_batch(seed=6, B=B, L=L, S=S, pad_tail=(4, 0, 6, 0, 0))
    m = hip_denoiser(1234, 1.0)
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    a = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=4, seed=11)
    b = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=4, seed=11, skip_zero_weight_chunks=True)
    assert torch.equal(a, b)


@pytest.mark.parametrize("knob", ["CFD_SHARE0", "CFD_PERMUTE"])
def test_structural_shortcuts_of_the_loop_are_exact(knob):
    """CFD_SHARE0: the embedding, layer 0's self-attention and its first time block see the same latents and the
    same timestep in all 7 guidance chunks; evaluating them once per utterance (default) must not change a bit
    against evaluating them for every replica.  CFD_PERMUTE: the engine reorders the guidance chunks internally so
    that the chunks sharing the unconditional audio memory are adjacent (one un-batched attention product instead
    of one per run); rows are independent, so this must not change a bit either.  (Knobs are read at cfd_create.)
    Both are checked with layer 0's cross-attention as ONE launch (CFD_L0_DEDUP=0): the default splits it into the audio
    memory once per distinct (utterance, instance) plus the other memories per row, which sums the five memories'
    contributions in another order -- equal to rounding (third leg), not to the bit."""
    import torch
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S = 3, 64, (24, 288, 24, 8, 1)   # long enough for the shared-memory run path (L >= 64, >= 256 keys)
    cb = inputs.make_cfg_batch(seed=8, B=B, L=L, S=S, pad_tail=(4, 0, 6, 0, 0))
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    ma = _handle_with_env({"CFD_L0_DEDUP": "0"})
    mb = _handle_with_env({"CFD_L0_DEDUP": "0", knob: "0"})
    a = sample(ma, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=4, seed=11)
    b = sample(mb, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=4, seed=11)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    if knob == "CFD_SHARE0":
        launches = []
        for m in (hip_denoiser(1234, 1.0), ma):
            run = SamplingRun(m, _sched("ddpm"), mems, masks, B, L, 4, guidance_scale=7.5, seed=11)
            run.steps(2)
            launches.append(run.profile()["xattn"][1])
            run.steps(2)
            out = run.read(close=True)
            if m is not ma:
                d = float((out - a).norm() / a.norm())
                print("layer-0 de-duplication vs one launch, 4 guided steps: rel L2", d)
                assert torch.isfinite(out).all() and d < 2e-4   # (a 4-step schedule amplifies rounding ~50x, see test_dedup_is_exact)
        assert launches == [10, 9], launches                   # 9 layers, layer 0 as two launches by default


def test_structured_guidance_batch_equals_replicated_batch():
    """build_guidance_batch (distinct memories + maps, no 7x materialisation) == the reference's replicated batch."""
    import torch
    from convofusion_amd.sampler import build_guidance_batch, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S = 3, 64, (24, 288, 24, 8, 1)   # long enough for the shared-memory run path (L >= 64, >= 256 keys)
    cb = inputs.make_cfg_batch(seed=8, B=B, L=L, S=S, pad_tail=(4, 0, 6, 0, 0))
    m = hip_denoiser(1234, 1.0)
    rep = sample(m, _sched("ddpm"), [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()},
                 B=B, L=L, num_inference_steps=4, seed=4)
    uq = [to_dev(u) for u in cb["unique"]]
    cond, unc = [u[1:] for u in uq], [u[:1] for u in uq]
    cm = {k: (to_dev(v)[6 * B:] if v is not None else None) for k, v in cb["masks"].items()}    # chunk 6 = full conditioning
    um = {k: (to_dev(v)[:1] if v is not None else None) for k, v in cb["masks"].items()}         # chunk 0 = all dropped
    mems, maps, masks = build_guidance_batch(cond, unc, cm, um)
    for j in range(5):
        assert torch.equal(maps[j].cpu(), torch.from_numpy(cb["row_map"][j]))
    st = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=4, seed=4, row_maps=maps)
    assert torch.equal(rep, st)


def test_device_rng_stream_matches_oracle():
    """No injected noise: the on-device Philox stream (init latents + per-step noise) is reproduced by the
    oracle's restatement, so the whole loop can be checked end-to-end against the oracle."""
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n = 2, 16, (6, 20, 6, 8, 1), 5
    seed, first = 77, 5
    cb = inputs.make_cfg_batch(seed=9, B=B, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
    sd = state_dict()
    want, _, _ = sampler_ref.diffusion_reverse(
        lambda x, t, e, mk: denoiser_ref.denoiser_forward(sd, x, t, e, mk), scheduler_ref.DDPMSchedulerRef(),
        cb["memories"], cb["masks"], philox_ref.normal_tensor(seed, 0, range(first, first + B), 1, L),
        lambda i, t: philox_ref.normal_tensor(seed, i, range(first, first + B), 0, L), num_inference_steps=n)
    m = hip_denoiser(1234, 1.0)
    got = sample(m, _sched("ddpm"), [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()},
                 B=B, L=L, num_inference_steps=n, seed=seed, first_utterance=first)
    e = rel_l2(got.permute(1, 0, 2).cpu().numpy(), want)
    print("device-rng loop vs oracle", e)
    assert e < TRAJ_TOL


@pytest.mark.parametrize("S_audio,audio_pad", [(256, 0), (300, 37)])
def test_shared_memory_run_path_matches_oracle(S_audio, audio_pad):
    """Long latents + a long audio memory switch on the un-batched attention products for rows that share the
    unconditional memory in the three-launch path (cfd_forward.hip 'runs'; CFD_FUSED_XATTN=0 leg of
    test_developer_knobs_keep_parity) and give the fused cross-attention kernel a multi-tile online softmax with row-straddling
    workgroups; check the loop end-to-end against the oracle -- also with a key count that is
    not a multiple of the tile (300 = 2 x 128 + 44, padded to 320) and a key-padding mask on the shared memory that
    blanks the whole last tile's valid keys."""
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n = 2, 64, (8, S_audio, 8, 8, 1), 2
    seed = 31
    cb = inputs.make_cfg_batch(seed=12, B=B, L=L, S=S, pad_tail=(2, audio_pad, 1, 0, 0),
                               uncond_pad_tail=(3, 44 if audio_pad else 0, 2, 0, 0))
    sd = state_dict()
    want, _, _ = sampler_ref.diffusion_reverse(
        lambda x, t, e, mk: denoiser_ref.denoiser_forward(sd, x, t, e, mk), scheduler_ref.DDPMSchedulerRef(),
        cb["memories"], cb["masks"], philox_ref.normal_tensor(seed, 0, range(B), 1, L),
        lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), num_inference_steps=n)
    m = hip_denoiser(1234, 1.0)
    got = sample(m, _sched("ddpm"), [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()},
                 B=B, L=L, num_inference_steps=n, seed=seed)
    e = rel_l2(got.permute(1, 0, 2).cpu().numpy(), want)
    print("run path vs oracle", e)
    assert e < TRAJ_TOL


def test_model_level_drop_in():
    """diffusion_reverse(model, ...) reads the same attributes the reference method reads from ``self``."""
    from types import SimpleNamespace
    import torch
    from convofusion_amd.sampler import diffusion_reverse
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S = 2, 16, (6, 20, 6, 8, 1)
    cb = inputs.make_cfg_batch(seed=3, B=B, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
    model = SimpleNamespace(
        denoiser=hip_denoiser(1234, 1.0), scheduler=_sched("ddpm"), guidance_scale=7.5, clf_guidance_drops=6,
        latent_dim=[1, 128], do_classifier_free_guidance=True,
        cfg=SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=5, eta=0.0))))
    init0 = philox_ref.normal_tensor(21, 0, range(B), 1, L)
    lat, atts = diffusion_reverse(model, [to_dev(x) for x in cb["memories"]], None, {k: to_dev(v) for k, v in cb["masks"].items()},
                                  init_latents=to_dev(init0), seed=21)
    assert tuple(lat.shape) == (L, B, 128) and torch.isfinite(lat).all()
    # the attention dict: the reference keeps the full-conditioning chunk's maps of every iteration (convofusion.py:517-523);
    # the fused loop returns the last iteration's entry -- checked against the oracle loop's maps at that timestep
    sd = state_dict()
    want, _, ref_att = sampler_ref.diffusion_reverse(
        lambda x, t, e, mk: denoiser_ref.denoiser_forward(sd, x, t, e, mk), scheduler_ref.DDPMSchedulerRef(), cb["memories"], cb["masks"],
        init0, lambda i, t: philox_ref.normal_tensor(21, i, range(B), 0, L), num_inference_steps=5, return_att=True)
    assert rel_l2(lat.cpu().numpy(), want) < TRAJ_TOL
    t_last = int(model.scheduler.timesteps[-1])
    assert list(atts.keys()) == [t_last] and len(atts[t_last]) == 5
    for j in range(5):
        a = atts[t_last][j].cpu().numpy()
        assert a.shape == (B, 9, L, S[j]) and np.abs(a - ref_att[t_last][j]).max() < 5e-5
    # every iteration's maps on request, like the reference's dict
    lat_all, atts_all = diffusion_reverse(model, [to_dev(x) for x in cb["memories"]], None, {k: to_dev(v) for k, v in cb["masks"].items()},
                                          init_latents=to_dev(init0), seed=21, attention_steps="all")
    assert torch.equal(lat_all, lat) and sorted(atts_all.keys()) == sorted(ref_att.keys())
    for t, maps in atts_all.items():
        assert max(float(np.abs(maps[j].cpu().numpy() - ref_att[t][j]).max()) for j in range(5)) < 5e-5
    # the WEG branch (focus_indices) through the same entry point: batch size 1 as the reference requires
    # (word_excitation_guidance.py:25); it must change the result and stay finite
    from convofusion_amd.sampler import diffusion_reverse_forecast
    cb1 = inputs.make_cfg_batch(seed=4, B=1, L=L, S=(6, 20, 12, 8, 1), pad_tail=(2, 0, 3, 0, 0))
    enc1, masks1 = [to_dev(x) for x in cb1["memories"]], {k: to_dev(v) for k, v in cb1["masks"].items()}
    model.weg_parameters = dict(scale_factor=1000, scale_range=[1.0, 0.5], max_iter_to_alter=2, thresholds={0: 0.05}, max_refinement_steps=1)
    init = torch.randn((1, L, 128), device="cuda")
    plain, _ = diffusion_reverse(model, enc1, None, masks1, init_latents=init, seed=5)
    steered, _ = diffusion_reverse(model, enc1, None, masks1, focus_indices=[[2, 4]], init_latents=init, seed=5)
    again, _ = diffusion_reverse(model, enc1, None, masks1, focus_indices=[[2, 4]], init_latents=init, seed=5)
    assert torch.isfinite(steered).all() and torch.equal(steered, again)
    assert (steered - plain).norm() / plain.norm() > 1e-3
    # the rollout entry point with its hard-coded WEG constants (unbounded_synthesis.py:80-84)
    pre = 0.3 * torch.randn((1, 8, 128), device="cuda")
    f_plain, a_plain = diffusion_reverse_forecast(model, enc1, None, pre, masks1, init_latents=init, seed=5)
    f_weg, a_weg = diffusion_reverse_forecast(model, enc1, None, pre, masks1, focus_indices=[[2]], init_latents=init, seed=5)
    assert torch.isfinite(f_weg).all() and (f_weg - f_plain).norm() / f_plain.norm() > 1e-4
    # the rollout returns the last iteration's att_mats list itself (unbounded_synthesis.py:159,187)
    for att in (a_plain, a_weg):
        assert len(att) == 5 and all(tuple(a.shape) == (1, 9, L, s) for a, s in zip(att, (6, 20, 12, 8, 1)))
        assert all(torch.allclose(a.sum(-1), torch.ones_like(a.sum(-1)), atol=1e-4) for a in att)


@pytest.mark.parametrize("shape", ["C2"])
def test_full_size_properties(shape):
    """BASELINE config 2 (B=32, L=196, 1500 audio tokens): too big for the oracle, so check properties the
    domain guarantees: finiteness, replay determinism, utterance independence (a 16-utterance shard with the
    right global ids reproduces the first half bit-for-bit) and the guidance identity (all conditions equal to
    the unconditional one => the guided prediction equals the 1-chunk prediction: to rounding with layer 0's audio attention de-duplicated,
    to 1e-6 absolute in the one-launch form)."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n = 32, 196, (32, 1500, 32, 8, 1), 4
    cb = inputs.make_cfg_batch(seed=1234, B=B, L=L, S=S, pad_tail=(8, 0, 8, 0, 0), uncond_pad_tail=(8, 0, 8, 0, 0))
    m = hip_denoiser(1234, 1.0)
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    a = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=1)
    b = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=1)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    from convofusion_amd.distributed import shard_cfg_batch
    half = [shard_cfg_batch(x, 16, 32, B) for x in mems]
    hmask = {k: shard_cfg_batch(v, 16, 32, B) for k, v in masks.items()}
    c = sample(m, _sched("ddpm"), half, hmask, B=16, L=L, num_inference_steps=n, seed=1, first_utterance=16)
    assert torch.equal(c, a[16:])
    # guidance identity
    unc = [x[:B].repeat(7, 1, 1) for x in mems]
    umask = {k: (v[:B].repeat(7, 1) if v is not None else None) for k, v in masks.items()}
    g7 = sample(m, _sched("ddpm"), unc, umask, B=B, L=L, num_inference_steps=2, seed=2)
    g1 = sample(m, _sched("ddpm"), [x[:B] for x in mems], {k: (v[:B] if v is not None else None) for k, v in masks.items()},
                B=B, L=L, num_inference_steps=2, seed=2, guidance_chunks=1)
    # (layer 0's cross-attention of the 7-chunk run is the two-launch de-duplicated form, the 1-chunk run's is one launch: the five
    #  memories' contributions are summed in another order; the 2-step schedule amplifies that rounding ~50x)
    d = float((g7 - g1).norm() / g1.norm())
    print("guidance identity, layer-0 de-duplication on: rel L2", d, "max abs", float((g7 - g1).abs().max()))
    assert d < 5e-6
    m1 = _handle_with_env({"CFD_L0_DEDUP": "0"})      # one launch in both runs: equal to the last bit or two
    g7 = sample(m1, _sched("ddpm"), unc, umask, B=B, L=L, num_inference_steps=2, seed=2)
    assert torch.allclose(g7, g1, rtol=0, atol=1e-6)


def test_ddim_with_eta_matches_oracle():
    """DDIM with eta > 0 draws per-step noise from the device Philox stream (diffusers 0.14.0 DDIMScheduler.step)."""
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n, eta, seed = 2, 16, (6, 20, 6, 8, 1), 5, 0.5, 123
    cb = inputs.make_cfg_batch(seed=21, B=B, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
    sd = state_dict()
    want, _, _ = sampler_ref.diffusion_reverse(
        lambda x, t, e, mk: denoiser_ref.denoiser_forward(sd, x, t, e, mk), scheduler_ref.DDIMSchedulerRef(),
        cb["memories"], cb["masks"], philox_ref.normal_tensor(seed, 0, range(B), 1, L),
        lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), num_inference_steps=n, eta=eta)
    got = sample(hip_denoiser(1234, 1.0), _sched("ddim"), [to_dev(x) for x in cb["memories"]],
                 {k: to_dev(v) for k, v in cb["masks"].items()}, B=B, L=L, num_inference_steps=n, eta=eta, seed=seed)
    e = rel_l2(got.permute(1, 0, 2).cpu().numpy(), want)
    print("ddim eta=0.5 vs oracle", e)
    assert e < TRAJ_TOL


# (each leg keeps the id it had when the list also held the legs of retired knobs, so a leg's results stay comparable across commits)
@pytest.mark.parametrize("env", [pytest.param({"CFD_FUSED_XATTN": "0"}, id="env2"), pytest.param({"CFD_ROWTILE": "0"}, id="env4"),
                                 pytest.param({"CFD_ROWTILE": "0", "CFD_FUSED_XATTN": "0"}, id="env7"),
                                 pytest.param({"CFD_L0_DEDUP": "0"}, id="env9"),
                                 pytest.param({"CFD_ROWTILE": "0", "CFD_LN_FOLD": "1"}, id="env10")])
def test_developer_knobs_keep_parity(env):
    """The developer knobs that force another code path for the same arithmetic (read once at cfd_create) must not change
    results: CFD_FUSED_XATTN=0 (three-launch cross-attention everywhere, with its shared-memory runs), CFD_ROWTILE=0 (small problems
    on the tile kernels instead of the row-tile kernels of rowtile.hpp; at 16 tokens per batch row those make q | k and v^T in one
    grouped launch whose epilogue stores the value projection transposed, and the row-tile path's attention core behind it), the same
    with CFD_FUSED_XATTN=0 (on the tile kernels, forwards that return att_mats take the three-launch cross-attention instead of the
    fused kernel's attention-map instance), CFD_L0_DEDUP=0 (layer 0's cross-attention as one launch over all rows), CFD_ROWTILE=0
    with CFD_LN_FOLD=1 (the small goldens on the tile kernels with the algebraic LayerNorm fold of mid-size problems forced on:
    gemm_sp.hpp EpiResidStat / EpiLn).  Each leg runs the golden forward, the 20-step trajectory, the run-path test and the
    headline-shape loop rows in a child process.  (The fused cross-attention fed by per-call memory-side projections and the one-key
    memory as a 32-key tile step are reached through public arguments: test_forward_matches_oracle_per_row_timesteps and
    test_static_and_dynamic_memory_declarations_agree_and_mean_what_they_say.)"""
    import os
    import subprocess
    import sys
    e = dict(os.environ, **env)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tests = ["tests/test_gpu_forward.py::test_forward_matches_reference_golden",
             "tests/test_gpu_sampler.py::test_sampler_matches_reference_trajectory[ddpm20_b2]",
             "tests/test_gpu_sampler.py::test_shared_memory_run_path_matches_oracle",
             "tests/test_gpu_sampler.py::test_headline_shape_loop_row_matches_reference[b32-ddpm5]"]
    if env.get("CFD_LN_FOLD") == "1":   # the fold on the heavy-tailed weights (outlier LayerNorm gains, outlier rows) and their 1000-step trajectory
        tests += ["tests/test_gpu_forward.py::test_heavy_tailed_weights_stress_case",
                  "tests/test_gpu_sampler.py::test_heavy_tailed_weights_ddpm1000_trajectory"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", *tests], cwd=root, env=e, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]


@pytest.mark.parametrize("kind", ["ddpm5", "ddim5", "ddim50", "ddpm1000"])
@pytest.mark.parametrize("variant", ["b32", "b32_skip_zero_weight_chunk", "b1_shard"])
def test_headline_shape_loop_row_matches_reference(kind, variant):
    """The captured loop at BASELINE configs[1]'s full size (B = 32, L = 196, 1500 audio tokens): utterance
    17's latents against the trajectory the restated loop produced driving the REFERENCE denoiser for that utterance alone
    (tests/golden/traj_c2_*.npz) -- 5 guided steps of either scheduler, and the FULL LENGTH runs north_star's acceptance sentence
    names: 1000 DDPM steps (snapshots after 1 / 10 / 100 / 500 steps and the final latents) and 50 DDIM steps
    (tests/golden/make_golden_c2full.py; ~14 s per 1000-step B = 32 run on the GPU).  Utterances are independent and the Philox streams are keyed by global utterance id, so
    the B = 32 run's row 17 (default path: shared-memory runs, chunk permutation, shared layer-0 head), the same with the
    zero-weight chunk skipped, and a one-utterance shard with first_utterance = 17 must all reproduce it."""
    from convofusion_amd.distributed import shard_cfg_batch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g = load_golden("traj_c2_" + kind)
    meta = [int(v) for v in g["meta"]]
    B, L, S, pad, n, seed, u = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13], meta[14]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, uncond_pad_tail=pad)
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    m = hip_denoiser(1234, 1.0)
    sched = _sched("ddim" if "ddim" in kind else "ddpm")
    if variant == "b1_shard":
        mems = [shard_cfg_batch(x, u, u + 1, B) for x in mems]
        masks = {k: shard_cfg_batch(v, u, u + 1, B) for k, v in masks.items()}
        run = SamplingRun(m, sched, mems, masks, 1, L, n, guidance_scale=7.5, seed=seed, first_utterance=u)
        row = 0
    else:
        run = SamplingRun(m, sched, mems, masks, B, L, n, guidance_scale=7.5, seed=seed,
                          skip_zero_weight_chunks=variant.endswith("chunk"))
        row = u
    errs = {}
    for k in sorted(int(f[4:]) for f in g.files if f.startswith("step")):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy()[row], g[f"step{k}"][0])
    run.steps(n - run.position)
    lat = run.read(close=True).cpu().numpy()
    errs["final"] = rel_l2(lat[row], g["latents"][:, 0])
    print(kind, variant, {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs
    if "ddpm" in kind:
        # the adoption gate of the DDPM runs' operand policy (sampler.OPERAND_POLICY): every DDPM golden within 3e-4
        # (measured 2.3e-5 - 6.1e-5 here with single-fp16 attention against the audio memory; 0.8e-5 - 2.0e-5 with split pairs)
        assert all(v < 3e-4 for v in errs.values()), errs


def test_small_goldens_on_the_default_attention_path():
    """tests/conftest.py lifts CFD_FUSED_XATTN_MIN_WGS to 0 so that the small goldens exercise the fused cross-attention kernel; in
    production a problem of fewer than 6 workgroups (one utterance at L = 16 is 3) takes the three-launch path.  The long small-shape
    trajectories -- 1000 DDPM steps, 50 DDIM steps, the 25-step in-painting rollout -- once more with the library's own default."""
    import os
    import subprocess
    import sys
    e = dict(os.environ, CFD_FUSED_XATTN_MIN_WGS="6")   # = the library default (cfd_internal.hpp: fused_xattn_min_wgs)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tests = [f"tests/test_gpu_sampler.py::test_sampler_matches_reference_trajectory[{n}]" for n in ("ddpm1000", "ddim50", "inpaint25")]
    tests.append("tests/test_gpu_conditioning.py::test_dyadic_loop_matches_oracle")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", *tests], cwd=root, env=e, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]


def test_attention_of_every_iteration_leaves_the_latents_alone():
    """sample(return_attention="all"): one extra forward of the full-conditioning rows on the denoiser's second engine before every
    replay, the host waiting in between (the two engines must not run side by side: DESIGN.md sections 6 and 7.2).  The latents must
    equal the attention-free run's bit for bit over a longer run and every entry must equal a plain forward of the iteration's input."""
    import torch
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n, seed = 3, 16, (24, 161, 24, 8, 1), 40, 17
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=(4, 0, 6, 0, 0))
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    m = hip_denoiser(1234, 1.0)
    plain = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed)
    lat, atts = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, return_attention="all")
    assert torch.equal(lat, plain)
    assert sorted(atts) == sorted(range(0, 1000, 1000 // n)) and all(len(v) == 5 for v in atts.values())
    # entry t = att_mats of Denoiser.forward on the full-conditioning chunk with the latents that enter iteration t
    with SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=seed) as run:
        run.steps(7)
        x7, t7 = run.read(), run.timesteps[7]
    keep = m.return_attention
    m.return_attention = True
    try:
        with torch.no_grad():
            _, want = m(sample=x7, timestep=t7, encoder_hidden_states=[e.chunk(7)[-1] for e in mems],
                        mem_mask_dict={k: (v.chunk(7)[-1] if v is not None else None) for k, v in masks.items()})
    finally:
        m.return_attention = keep
    assert all(torch.equal(a, b) for a, b in zip(atts[t7], want))


def test_every_iterations_attention_maps_match_the_oracle():
    """The reference fills ``attention_matrices[t]`` with the full-conditioning chunk's att_mats of EVERY iteration (convofusion.py:517-523;
    base.py:243-259 writes them out).  The captured iteration keeps them itself (cfd_sample_args.att_ring: the row-tile path's second
    cross-attention launch stores the last chunk's probabilities into slot *d_step): every entry of a 10-step run against the restated
    loop driving the numpy oracle, the latents untouched by the extra chunk -- and the same through the tile kernels."""
    import torch
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n, seed = 2, 16, (6, 20, 6, 8, 1), 10, 5
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
    sd = state_dict()
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    want_lat, _, want = sampler_ref.diffusion_reverse(
        lambda x, t, e, mk: denoiser_ref.denoiser_forward(sd, x, t, e, mk), scheduler_ref.DDPMSchedulerRef(), cb["memories"], cb["masks"],
        init, lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), num_inference_steps=n, return_att=True)
    m = hip_denoiser(1234, 1.0)
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    with SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, seed=seed, attention_ring=True) as run:     # (this shape is served by the ring)
        assert run.att_ring is not None and tuple(run.att_ring[1].shape) == (n, B, 9, L, S[1])
    lat, atts = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, return_attention="all")
    plain = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed)
    assert torch.equal(lat, plain)
    assert rel_l2(lat.permute(1, 0, 2).cpu().numpy(), want_lat) < TRAJ_TOL
    assert sorted(atts) == sorted(want)
    worst = 0.0
    for t in want:
        for j in range(5):
            got = atts[t][j].cpu().numpy()
            assert got.shape == want[t][j].shape
            worst = max(worst, max_abs(got, want[t][j]))
    print("worst attention-map difference over", n, "iterations x 5 memories:", worst)
    assert worst < 1e-4
    # The same run on the TILE kernels (CFD_ROWTILE=0): there the fused cross-attention kernel keeps the maps (its ATT instance stores each
    # key tile's probabilities relative to the tile's exponent reference, att_fixup_kernel normalises them once per step).
    m_tile = _handle_with_env({"CFD_ROWTILE": "0"})
    lat_t, atts_t = sample(m_tile, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, return_attention="all")
    assert torch.equal(lat_t, sample(m_tile, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed))
    worst_t = max(max_abs(atts_t[t][j].cpu().numpy(), want[t][j]) for t in want for j in range(5))
    print("tile kernels, the same run: worst attention-map difference", worst_t)
    assert sorted(atts_t) == sorted(want) and worst_t < 1e-4


def test_attention_maps_of_every_iteration_beyond_the_row_tile_path():
    """Eight utterances (896 token rows: the tile kernels, with layer 0's de-duplicated cross-attention lists): the ring is filled by the fused
    cross-attention kernel.  Every entry against the restated loop driving the numpy oracle (masked keys exactly 0, rows summing to 1), the
    latents bit-identical to a run that keeps no maps, and the fall-back that an over-budget ring takes (one forward per iteration through the
    three-launch attention) giving the same dict."""
    import torch
    from convofusion_amd import sampler
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n, seed = 8, 16, (6, 40, 6, 8, 1), 4, 6
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=(2, 5, 1, 0, 0))
    sd = state_dict()
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    want_lat, _, want = sampler_ref.diffusion_reverse(
        lambda x, t, e, mk: denoiser_ref.denoiser_forward(sd, x, t, e, mk), scheduler_ref.DDPMSchedulerRef(), cb["memories"], cb["masks"],
        init, lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), num_inference_steps=n, return_att=True)
    m = hip_denoiser(1234, 1.0)
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    with SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, seed=seed, attention_ring=True) as run:
        assert run.att_ring is not None and tuple(run.att_ring[1].shape) == (n, B, 9, L, S[1])
    lat, atts = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, return_attention="all")
    assert torch.equal(lat, sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed))
    assert rel_l2(lat.permute(1, 0, 2).cpu().numpy(), want_lat) < TRAJ_TOL
    assert sorted(atts) == sorted(want)
    worst = 0.0
    for t in want:
        for j in range(5):
            got = atts[t][j].cpu().numpy()
            assert got.shape == want[t][j].shape
            worst = max(worst, max_abs(got, want[t][j]))
            assert np.all(got[want[t][j] == 0] == 0)                       # masked keys: exactly 0
            assert np.abs(got.sum(-1) - 1).max() < 1e-5
    print("8 utterances, fused kernel's maps: worst difference over", n, "iterations x 5 memories:", worst)
    assert worst < 1e-4
    keep = sampler.ATT_RING_MAX_BYTES
    try:
        sampler.ATT_RING_MAX_BYTES = 0     # the ring "does not fit": one forward per iteration
        lat2, atts2 = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, return_attention="all")
    finally:
        sampler.ATT_RING_MAX_BYTES = keep
    assert torch.equal(lat2, lat)
    assert max(max_abs(atts2[t][j].cpu().numpy(), want[t][j]) for t in want for j in range(5)) < 1e-4


def test_ddpm_step_count_that_does_not_divide_the_schedule():
    """DDPM with N = 300 of 1000 (opt-in, unpinned: scheduler.DDPMScheduler(allow_unpinned_timesteps=True)): the loop runs over the
    334 entries of diffusers 0.14.0's table arange(0, 1000, 3)[::-1] with prev_t = t - 3, like the oracle's restated loop; the
    default scheduler refuses the count."""
    import torch
    from convofusion_amd import scheduler
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    B, L, S, n, seed = 2, 16, (6, 20, 6, 8, 1), 300, 21
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    m = hip_denoiser(1234, 1.0)
    with pytest.raises(ValueError):
        SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, seed=seed)
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", allow_unpinned_timesteps=True, **SCHED_KW)
    run = SamplingRun(m, sch, mems, masks, B, L, n, guidance_scale=7.5, seed=seed)
    assert run.N == 334 and run.timesteps[:3] == [999, 996, 993] and run.timesteps[-1] == 0
    sd = state_dict(1234, 1.0)
    ref = scheduler_ref.DDPMSchedulerRef(allow_unpinned_timesteps=True)
    keep = (1, 8)
    want, snaps, _ = sampler_ref.diffusion_reverse(
        lambda x, t, enc, mk: denoiser_ref.denoiser_forward(sd, x, t, enc, mk), ref, cb["memories"], cb["masks"],
        philox_ref.normal_tensor(seed, 0, range(B), 1, L), lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L),
        guidance_scale=7.5, num_inference_steps=n, keep_steps=keep, stop_after=max(keep))
    for k in keep:
        run.steps(k - run.position)
        assert rel_l2(run.read().cpu().numpy(), snaps[k]) < TRAJ_TOL
    with pytest.raises(Exception):
        run.steps(run.N)          # more than the table holds
    run.steps(run.N - run.position)
    assert run.position == 334 and torch.isfinite(run.read(close=True)).all()


def test_no_edit_installer_runs_the_fused_loop():
    """convofusion_amd.install(model) + patch_rollout(module): the reference call sites (`self._diffusion_reverse(cond_emb, lengths,
    cond_masks=..., focus_indices=...)`, convofusion.py:1023; `diffusion_reverse_forecast(model, cond_emb, lengths, preseq, cond_masks=...)`,
    unbounded_synthesis.py:438) reach the fused loop through the bindings, with the reference's keyword usage."""
    import types
    from types import SimpleNamespace
    import torch
    import convofusion_amd
    from convofusion_amd.sampler import diffusion_reverse, diffusion_reverse_forecast
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S = 2, 16, (6, 20, 6, 8, 1)
    cb = inputs.make_cfg_batch(seed=3, B=B, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))

    class RefLike:
        def _diffusion_reverse(self, encoder_hidden_states, lengths=None, cond_masks=dict(), focus_indices=[]):
            raise AssertionError("the class method must be shadowed by the installed binding")
    model = RefLike()
    model.denoiser, model.scheduler, model.guidance_scale, model.clf_guidance_drops = hip_denoiser(1234, 1.0), _sched("ddpm"), 7.5, 6
    model.latent_dim, model.do_classifier_free_guidance = [1, 128], True
    model.cfg = SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=4, eta=0.0)))
    convofusion_amd.install(model, attention_steps="last")
    enc = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    torch.manual_seed(7)
    z, att = model._diffusion_reverse(enc, None, cond_masks=masks, focus_indices=[])
    torch.manual_seed(7)
    z2, _ = diffusion_reverse(model, enc, None, masks, [])
    assert tuple(z.shape) == (L, B, 128) and torch.equal(z, z2) and len(att) == 1
    # the DEFAULT binding ("auto"): at this size the captured iteration keeps every iteration's maps itself, so the dict is the reference's
    convofusion_amd.install(model)
    torch.manual_seed(7)
    z_auto, att_auto = model._diffusion_reverse(enc, None, cond_masks=masks, focus_indices=[])
    assert torch.equal(z_auto, z) and sorted(att_auto) == [0, 250, 500, 750]
    # the reference's dict holds the full-conditioning chunk's maps of EVERY iteration (convofusion.py:517-523; base.py:252-259 dumps
    # one file per entry): install(model, attention_steps="all") reproduces it -- same latents, one entry per timestep, and the last
    # entry equals the "last" binding's only entry
    convofusion_amd.install(model, attention_steps="all")
    torch.manual_seed(7)
    z3, att_all = model._diffusion_reverse(enc, None, cond_masks=masks, focus_indices=[])
    assert torch.equal(z3, z) and sorted(att_all) == [0, 250, 500, 750]
    (t_last, last), = att.items()
    assert t_last == 0 and all(torch.equal(a, b) for a, b in zip(att_all[0], last))
    assert all(tuple(a.shape) == (B, 9, L, s) for a, s in zip(att_all[750], S))
    convofusion_amd.install(model)
    script = types.ModuleType("unbounded_synthesis")
    script.diffusion_reverse_forecast = lambda *a, **k: (_ for _ in ()).throw(AssertionError("not replaced"))
    convofusion_amd.patch_rollout(script)
    pre = 0.3 * torch.randn((B, 8, 128), device="cuda")
    torch.manual_seed(9)
    r, ratt = script.diffusion_reverse_forecast(model, enc, None, pre, cond_masks=masks, focus_indices=[])
    torch.manual_seed(9)
    r2, _ = diffusion_reverse_forecast(model, enc, None, pre, masks, [])
    assert tuple(r.shape) == (L, B, 128) and torch.equal(r, r2) and len(ratt) == 5


def _handle_with_env(env):
    """A Denoiser with the session's test weights whose library handle is created under `env` (the knobs are read at cfd_create)."""
    import os
    import torch
    from convofusion_amd.denoiser import Denoiser
    from tests.gpu_helpers import ABL, DENOISER_KW, hip_denoiser
    keep = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        m = Denoiser(ablation=ABL, **DENOISER_KW)
        m.load_state_dict(hip_denoiser(1234, 1.0).state_dict(), strict=True)
        m = m.cuda().eval()
        m.engine(torch.device("cuda"))
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return m


def test_small_problems_take_the_row_tile_path_and_the_three_paths_agree():
    """Path selection by SHAPE.  A 2-utterance run at the product shape (224 token rows of 16) takes the row-tile path (rowtile.hpp: two
    cross-attention launches per layer, no row kernels); with CFD_ROWTILE=0 the same run goes through the tile kernels -- the
    three-launch cross-attention at the default threshold (4 workgroups < 6), the fused kernel with the threshold lifted.  All three
    must agree to rounding (different summation orders, hoisted / per-step memory LayerNorm) and the profile must show which ran."""
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S = 2, 16, (24, 161, 24, 8, 1)
    cb = inputs.make_cfg_batch(seed=5, B=B, L=L, S=S, pad_tail=(4, 0, 6, 0, 0))
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    models = (hip_denoiser(1234, 1.0),                                                       # row-tile (default)
              _handle_with_env({"CFD_ROWTILE": "0"}),                                        # tile kernels, fused cross-attention (conftest lifts the threshold)
              _handle_with_env({"CFD_ROWTILE": "0", "CFD_FUSED_XATTN_MIN_WGS": None}))       # tile kernels, default threshold: three-launch
    outs, prof = [], []
    for m in models:
        run = SamplingRun(m, _sched("ddpm"), mems, masks, B, L, 4, guidance_scale=7.5, seed=11)
        run.steps(2)
        pf = run.profile()
        prof.append((pf["xattn"][1], pf["rows"][1], sum(v[1] for v in pf.values())))
        run.steps(2)
        outs.append(run.read(close=True))
    print("launches (xattn class, row kernels, all) per path:", prof)
    assert prof[0][:2] == (18, 0) and prof[0][2] == 84          # this step's table rows + embedding + 9 layers x 9 launches + final projection
    assert prof[1][0] == 9 and prof[2][0] == 0
    for k in (1, 2):
        d = float((outs[0] - outs[k]).norm() / outs[k].norm())
        print("row-tile vs", ("fused", "three-launch")[k - 1], "tile-kernel path, 4 guided steps: rel L2", d)
        assert d < 2e-4


def test_row_tile_path_is_race_free_and_shape_general():
    """The row-tile kernels hand data from launch to launch only (no workgroup reads what another workgroup of the same launch writes):
    repeated forwards are bit-identical -- the time blocks' in-place update was a race before the residual stream alternated between two
    buffers -- for one to five utterances, ragged last tiles (L = 20: a 4-token tile) and L = 32 (two full tiles, 32 keys)."""
    import torch
    from oracle import denoiser_ref
    from tests.gpu_helpers import hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    sd = state_dict(1234, 1.0)
    # ... and the edges of the path's eligibility: 700 token rows exactly, 1024 padded keys exactly (the 1024-key instantiation of
    # the second cross-attention launch), both with padded tails in the key masks
    shapes = ((7, 16, (24, 161, 24, 8, 1), None), (35, 16, (6, 20, 6, 8, 1), None), (3, 20, (5, 40, 3, 8, 1), None),
              (2, 32, (33, 70, 12, 8, 1), None), (1, 2, (1, 1, 1, 1, 1), None),
              (25, 28, (32, 700, 32, 8, 1), (3, 100, 5, 0, 0)), (2, 16, (32, 890, 32, 8, 1), (0, 37, 31, 0, 0)))
    for Be, L, S, pad in shapes:
        inp = inputs.make_plain_batch(seed=50 + Be, Be=Be, L=L, S=S, pad_tail=pad or (0, 0, 0, 0, 0), scale=1.0)
        mems = [to_dev(x) for x in inp["memories"]]
        x = to_dev(inp["sample"])
        with torch.no_grad():
            masks = {k: to_dev(v) for k, v in inp["masks"].items()}
            first, att0 = m(x, torch.tensor(321), mems, mem_mask_dict=masks)
            for _ in range(6):
                again, att = m(x, torch.tensor(321), mems, mem_mask_dict=masks)
                assert torch.equal(first, again) and all(torch.equal(p, q) for p, q in zip(att0, att))
        want, watt = denoiser_ref.denoiser_forward(sd, inp["sample"], 321, inp["memories"], inp["masks"])
        e = rel_l2(first.cpu().numpy(), want)
        print(f"Be={Be} L={L} S={S}: forward vs oracle {e:.2e}")
        assert e < 1e-4
        for j in range(5):
            assert max_abs(att0[j].cpu().numpy(), watt[j]) < 1e-4


@pytest.mark.parametrize("case", ["b10", "b32", "b10_rows_far_from_zero_mean", "b10_half_rows_apart"])
def test_layernorm_fold_of_mid_size_problems(case):
    """Between 1 024 and 3 840 token rows at the product shape (L = 16: `test.py`'s batches) norm3, the norm1 of layers 1.. and the decoder's
    final norm are not launched: the residual product in front of each stores the raw rows' split pairs and per-row slot statistics, the consumer
    runs on W diag(gamma) and rescales its accumulators (gemm_sp.hpp EpiResidStat / EpiLn; cross_attention.py:568-570, :659-661, :238-239).  The
    forward with the fold (default) against the numpy oracle and against the same forward with the LayerNorms launched (CFD_LN_FOLD=0): 10 and 32
    utterances of 7 guidance chunks (1 120 / 3 584 rows), and rows whose mean is 25 deviations away from zero / whose two halves sit 24 apart --
    where W' x - mu c cancels most of its digits."""
    import os
    import torch
    from convofusion_amd.denoiser import Denoiser
    from oracle import denoiser_ref
    from tests.gpu_helpers import ABL, DENOISER_KW, to_dev
    Be, L, S = (224 if case == "b32" else 70), 16, (24, 161, 24, 8, 1)
    inp = inputs.make_plain_batch(seed=77 + Be, Be=Be, L=L, S=S, pad_tail=(3, 17, 0, 0, 0))
    sd = {k: v.copy() for k, v in state_dict().items()}
    if case.endswith("zero_mean"):
        sd["latent_embd.bias"] = (sd["latent_embd.bias"] + 25.0).astype(np.float32)
    elif case.endswith("apart"):
        sd["latent_embd.bias"] = (sd["latent_embd.bias"] + np.where(np.arange(512) < 256, 12.0, -12.0)).astype(np.float32)
    want, _ = denoiser_ref.denoiser_forward(sd, inp["sample"], 577, inp["memories"], inp["masks"])
    outs = {}
    for fold in ("-1", "0"):
        keep = os.environ.get("CFD_LN_FOLD")
        os.environ["CFD_LN_FOLD"] = fold
        try:
            m = Denoiser(ablation=ABL, **DENOISER_KW)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            m = m.cuda().eval()
            m.engine(torch.device("cuda"))          # (the knobs are read when the handle is created)
        finally:
            if keep is None:
                os.environ.pop("CFD_LN_FOLD", None)
            else:
                os.environ["CFD_LN_FOLD"] = keep
        with torch.no_grad():
            out, _ = m(to_dev(inp["sample"]), torch.tensor(577), [to_dev(x) for x in inp["memories"]],
                       mem_mask_dict={k: to_dev(v) for k, v in inp["masks"].items()})
            again, _ = m(to_dev(inp["sample"]), torch.tensor(577), [to_dev(x) for x in inp["memories"]],
                         mem_mask_dict={k: to_dev(v) for k, v in inp["masks"].items()})
        assert torch.equal(out, again)
        outs[fold] = out.cpu().numpy()
    e_fold, e_ln, e_pair = rel_l2(outs["-1"], want), rel_l2(outs["0"], want), rel_l2(outs["-1"], outs["0"])
    print(f"{case}: fold vs oracle {e_fold:.2e}, launched LayerNorms vs oracle {e_ln:.2e}, fold vs launched {e_pair:.2e}")
    assert e_fold < 1e-4 and e_ln < 1e-4
    assert e_pair > 0.0, "the two legs ran the same launches"
    assert e_pair < 5e-5


def test_layernorm_fold_in_a_sampling_run():
    """Eight guided DDPM steps of 10 utterances at the product shape (1 120 rows: the fold's range) with the fold and with the LayerNorms launched:
    the captured iteration holds the fold's launches like the eager forward does."""
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import to_dev
    B, L, S = 10, 16, (24, 161, 24, 8, 1)
    cb = inputs.make_cfg_batch(seed=31, B=B, L=L, S=S, pad_tail=(4, 9, 6, 0, 0))
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    lat = {}
    for fold in ("-1", "0"):
        m = _handle_with_env({"CFD_LN_FOLD": fold})
        lat[fold] = sample(m, _sched("ddpm"), mems, masks, B=B, L=L, num_inference_steps=8, seed=5).cpu().numpy()
        assert np.isfinite(lat[fold]).all()
    d = rel_l2(lat["-1"], lat["0"])
    print("8 DDPM steps, fold vs launched LayerNorms: rel L2", d)
    assert 0.0 < d < 2e-4        # (an 8-step schedule amplifies a 1e-6 rounding difference per forward ~50x)


def test_row_tile_path_agrees_with_the_tile_kernels_on_random_shapes():
    """Random shapes inside the row-tile path's eligibility (batch rows, even L <= 32, memory lengths, padded tails, timestep) through both
    implementations of the forward -- the row-tile kernels (default) and the tile kernels (CFD_ROWTILE=0): latents to 1e-4 relative,
    attention maps to 1e-4 absolute, including rows whose key masks leave a single live key."""
    import torch
    from tests.gpu_helpers import hip_denoiser, to_dev
    rng = np.random.Generator(np.random.PCG64(2024))
    m_rt = hip_denoiser(1234, 1.0)
    m_tile = _handle_with_env({"CFD_ROWTILE": "0"})
    worst = 0.0
    for case in range(12):
        L = int(rng.choice([2, 4, 6, 10, 16, 18, 24, 32]))
        Be = int(rng.integers(1, max(2, min(20, 800 // L))))
        S = (int(rng.integers(1, 40)), int(rng.integers(1, 600)), int(rng.integers(1, 40)), int(rng.integers(1, 12)), int(rng.integers(1, 3)))
        pad = tuple(int(rng.integers(0, max(1, s // 2))) if rng.random() < 0.5 else 0 for s in S)
        t = int(rng.integers(0, 1000))
        inp = inputs.make_plain_batch(seed=900 + case, Be=Be, L=L, S=S, pad_tail=pad, scale=float(rng.choice([0.5, 1.0, 2.0])))
        mems = [to_dev(x) for x in inp["memories"]]
        masks = {k: to_dev(v) for k, v in inp["masks"].items()}
        x = to_dev(inp["sample"])
        with torch.no_grad():
            a, att_a = m_rt(x, torch.tensor(t), mems, mem_mask_dict=masks)
            b, att_b = m_tile(x, torch.tensor(t), mems, mem_mask_dict=masks)
        e = float((a - b).norm() / b.norm())
        ea = max(float((p - q).abs().max()) for p, q in zip(att_a, att_b))
        worst = max(worst, e)
        print(f"case {case}: Be={Be} L={L} S={S} pad={pad} t={t}: latents {e:.2e}, attention {ea:.2e}")
        assert torch.isfinite(a).all() and e < 1e-4 and ea < 1e-4
    print("worst", worst)


def test_tile_kernel_forms_agree_on_random_shapes():
    """Random shapes beyond the row-tile path (more than 700 token rows or L > 32) through the two forms of the tile-kernel forward --
    fused cross-attention (with layer-0 de-duplication off: a plain forward has no guidance structure; the one-key memory as a vector)
    and the three-launch cross-attention (CFD_FUSED_XATTN=0) -- including odd tile counts, ragged last tiles, memories of 1 .. 1600 keys
    with padded tails and batches whose rows share memory instances through a row map."""
    import torch
    from tests.gpu_helpers import hip_denoiser, to_dev
    rng = np.random.Generator(np.random.PCG64(4242))
    m_fused = _handle_with_env({})                       # (handles of their own: return_attention is switched off below --
    m_three = _handle_with_env({"CFD_FUSED_XATTN": "0"})  #  with attention maps wanted every forward takes the three-launch form)
    m_fused.return_attention = m_three.return_attention = False
    for case in range(8):
        L = int(rng.choice([34, 48, 64, 100, 130, 196]))
        lo = max(1, 820 // L + 1)                         # (past the row-tile path's 700 token rows, or L > 32 anyway)
        Be = int(rng.integers(lo, lo + 10))
        S = (int(rng.integers(1, 40)), int(rng.integers(33, 1600)), int(rng.integers(1, 40)), int(rng.integers(1, 12)), 1)
        pad = tuple(int(rng.integers(0, max(1, s // 3))) if rng.random() < 0.5 else 0 for s in S[:4]) + (0,)
        t = int(rng.integers(0, 1000))
        inp = inputs.make_plain_batch(seed=300 + case, Be=Be, L=L, S=S, pad_tail=pad, scale=float(rng.choice([0.5, 1.0, 2.0])))
        mems = [to_dev(x) for x in inp["memories"]]
        masks = {k: to_dev(v) for k, v in inp["masks"].items()}
        x = to_dev(inp["sample"])
        with torch.no_grad():
            a, _ = m_fused(x, torch.tensor(t), mems, mem_mask_dict=masks)
            b, _ = m_three(x, torch.tensor(t), mems, mem_mask_dict=masks)
        e = float((a - b).norm() / b.norm())
        print(f"case {case}: Be={Be} L={L} S={S} pad={pad} t={t}: fused vs three-launch {e:.2e}")
        assert torch.isfinite(a).all() and e < 1e-4


def test_operand_policies_of_the_fused_cross_attention():
    """cfd_sample_args.operand_policy (xattn_fused.hpp, F16): the folded values (bit 0) / keys (bit 1) of the LONG memories (>= 128 padded
    keys) as single fp16 tiles.  Policy 0 is the split-pair kernel of every other test.  The single-fp16 instances read tiles that
    xa_pack16_kernel re-lays once per run (tile-major, pre-swizzled), run the long memories' segments in a loop of their own (other piece
    counts behind the counted waits; both formats: a double-buffered tile pipeline) and drain the pipeline before the short memories' pair
    loop -- so this test is about the PLUMBING: random shapes with ragged tails, masks, partial last query tiles, one or two long memories
    (the accumulator flush), a second online memory that is NOT long, idle tiles; every policy must be deterministic, finite, and within the
    rounding of its format of policy 0, and policy 0 given explicitly must equal the default pairs bit for bit.  Where no memory is long, or
    the fused kernel does not run on once-per-run projections (row-tile path, a dynamic memory, an attention ring), the policy is ignored:
    bit-identical results.  The accuracy of the policies on the DDPM goldens is tools/xa_operands_table.py's table."""
    import torch
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    rng = np.random.Generator(np.random.PCG64(778))
    m = hip_denoiser(1234, 1.0)
    for case in range(7):
        L = int(rng.choice([34, 48, 66, 100, 130, 196]))
        B = int(rng.integers(max(1, 120 // L + 1), 6))
        spk = int(rng.integers(1, 33)) if case % 3 else (int(rng.integers(33, 90)) if case else int(rng.integers(130, 200)))   # case 0: two LONG memories
        S = (spk, int(rng.integers(97, 700)) if case != 6 else int(rng.integers(33, 96)), int(rng.integers(1, 33)), int(rng.integers(1, 12)), 1)
        pad = tuple(int(rng.integers(0, max(1, s // 3))) if rng.random() < 0.5 else 0 for s in S[:4]) + (0,)
        cb = inputs.make_cfg_batch(seed=40 + case, B=B, L=L, S=S, pad_tail=pad)
        mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
        kw = dict(B=B, L=L, num_inference_steps=4, seed=3 + case)
        base = sample(m, _sched("ddpm"), mems, masks, operands=0, **kw)
        assert torch.isfinite(base).all() and torch.equal(sample(m, _sched("ddpm"), mems, masks, operands=0, **kw), base)
        errs = {}
        for pol in (15, 1):      # (the shipped library implements the four bits together: any non-zero value means 15)
            got = sample(m, _sched("ddpm"), mems, masks, operands=pol, **kw)
            assert torch.isfinite(got).all() and torch.equal(sample(m, _sched("ddpm"), mems, masks, operands=pol, **kw), got), (case, pol)
            errs[pol] = float((got - base).norm() / base.norm())
        print(f"case {case}: B={B} L={L} S={S} pad={pad}: single-fp16 tiles of the long memories vs pairs after 4 guided steps: {errs}")
        if case == 6:       # no memory of 128 padded keys: nothing has single-fp16 tiles
            assert errs == {15: 0.0, 1: 0.0}, errs
        else:               # (a 4-step schedule amplifies a per-forward perturbation ~50x: test_dedup_is_exact)
            assert 0 < errs[15] < 1e-3 and errs[1] == errs[15], errs
    # ignored where it cannot apply: the row-tile path (small problem), a dynamic memory, an attention ring
    cb = inputs.make_cfg_batch(seed=31, B=2, L=16, S=(20, 100, 24, 8, 1), pad_tail=(3, 17, 2, 0, 0))
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    assert torch.equal(sample(m, _sched("ddpm"), mems, masks, B=2, L=16, num_inference_steps=4, seed=3, operands=15),
                       sample(m, _sched("ddpm"), mems, masks, B=2, L=16, num_inference_steps=4, seed=3, operands=0))
    cb = inputs.make_cfg_batch(seed=32, B=5, L=50, S=(20, 300, 24, 8, 1), pad_tail=(3, 17, 2, 0, 0))
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}

    def dyn(pol):
        with SamplingRun(m, _sched("ddpm"), mems, masks, 5, 50, 4, seed=3, dynamic_memories=(0,), operands=pol) as r:
            r.steps(4)
            return r.read()
    assert torch.equal(dyn(15), dyn(0))
    a, _ = sample(m, _sched("ddpm"), mems, masks, B=5, L=50, num_inference_steps=4, seed=3, operands=15, return_attention="all")
    b, _ = sample(m, _sched("ddpm"), mems, masks, B=5, L=50, num_inference_steps=4, seed=3, operands=0, return_attention="all")
    assert torch.equal(a, b)


def test_static_and_dynamic_memory_declarations_agree_and_mean_what_they_say():
    """cfd_sample_args.dynamic_memory_mask.  Memories are constants of a reference sampling run (convofusion.py:391-549), so by
    default the library projects the timestep-independent part of every memory once at cfd_sample_begin and never reads the
    memory again; a memory declared dynamic (the dyadic rollout's partner projection) is projected in every iteration.
    (1) With unchanged memories every declaration gives the same latents (the two forms of the same arithmetic; tolerance =
    rounding of the re-associated LayerNorm), also when mixed per memory.  (2) Overwriting a memory between iterations changes
    the result exactly when it was declared dynamic."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n, seed = 2, 16, (24, 161, 24, 8, 1), 4, 9
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=(2, 3, 0, 0, 0))
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    m = hip_denoiser(1234, 1.0)

    def go(dynamic, overwrite=None):
        mems = [to_dev(x).clone() for x in cb["memories"]]
        run = SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, dedup=False, dynamic_memories=dynamic)
        try:
            run.steps(2)
            if overwrite is not None:
                run.read()                                   # (syncs the run's stream)
                mems[overwrite].mul_(-0.5)
                torch.cuda.synchronize()
            run.steps(n - 2)
            return run.read(close=True).cpu().numpy()
        finally:
            run.close()

    base = go(())
    for dyn in [(0, 1, 2, 3, 4), (1,), (0, 2, 4)]:
        e = rel_l2(go(dyn), base)
        print("dynamic", dyn, "vs static: rel L2", e)
        assert e < 2e-5
    assert np.array_equal(go((), overwrite=1), base)                      # static: the memory is not read again
    changed = go((1,), overwrite=1)
    assert rel_l2(changed, base) > 1e-3                                   # dynamic: the new contents are used
    assert np.array_equal(go((1,), overwrite=1), changed)                 # ... deterministically


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_utterance_shards_equal_the_single_run(kind):
    """The batch as two utterance shards (distributed.shard_cfg_batch, an odd 3 + 2 split), run ONE AFTER THE OTHER on the denoiser's
    two library handles, gives the single run's latents bit for bit -- device-drawn noise (Philox keyed by global utterance id),
    caller-supplied initial latents and per-step noise, an in-painting prefix.  (Replaying the two shards' graphs at the same time
    is not a product path: tools/experiments/concurrent_runs.py)"""
    import torch
    from convofusion_amd.distributed import shard_cfg_batch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n, seed = 5, 16, (24, 161, 24, 8, 1), 4, 11
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=(2, 3, 0, 0, 0))
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    m = hip_denoiser(1234, 1.0)
    g = torch.Generator().manual_seed(3)
    cases = [dict(seed=seed, first_utterance=7),
             dict(seed=seed, init_latents=to_dev(torch.randn(B, L, 128, generator=g).numpy()),
                  step_noise=to_dev(torch.randn(n, B, L, 128, generator=g).numpy())),
             dict(seed=seed, preseq=to_dev(torch.randn(B, 6, 128, generator=g).numpy()))]
    for kw in cases:
        with SamplingRun(m, _sched(kind), mems, masks, B, L, n, guidance_scale=7.5, **kw) as one:
            one.steps(n)
            want = one.read(close=True)
        got = []
        for k, (a, b) in enumerate(((0, 3), (3, 5))):
            skw = dict(kw, first_utterance=kw.get("first_utterance", 0) + a)
            for name in ("init_latents", "preseq"):
                if name in skw:
                    skw[name] = skw[name][a:b]
            if "step_noise" in skw:
                skw["step_noise"] = skw["step_noise"][:, a:b]
            sm = [shard_cfg_batch(x, a, b, B) for x in mems]
            sk = {name: shard_cfg_batch(v, a, b, B) for name, v in masks.items()}
            with SamplingRun(m, _sched(kind), sm, sk, b - a, L, n, guidance_scale=7.5, side_engine=bool(k), **skw) as part:
                part.steps(n)
                got.append(part.read(close=True))
        assert torch.equal(torch.cat(got), want), sorted(kw)


def test_heavy_tailed_weights_ddim50_trajectory():
    """50 guided DDIM steps (eta = 0: nothing damps a perturbation, the hardest case for the split-pair arithmetic) on the heavy-tailed
    stress weights with outlier-token memories, against the trajectory the restated loop produced driving the REFERENCE denoiser
    (tests/golden/heavy.npz, make_golden_heavy.py): the 1e-3 budget must hold with outliers in weights and conditioning too."""
    import torch
    from convofusion_amd.denoiser import Denoiser
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import ABL, DENOISER_KW, to_dev
    from tests.helpers import heavy_state_dict, heavy_traj_case
    cb, B, L, n, seed, g = heavy_traj_case()
    m = Denoiser(ablation=ABL, **DENOISER_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in heavy_state_dict(8.0).items()}, strict=True)   # (outlier factor 8: at 20 the loop is chaotic, oracle/weights.py)
    m = m.cuda().eval()
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    run = SamplingRun(m, _sched("ddim"), [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}, B, L, n,
                      guidance_scale=7.5, init_latents=to_dev(init), eta=0.0)
    errs = {}
    for k in (1, 10, 50):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"traj_step{k}"])
    lat = run.read(close=True).permute(1, 0, 2).cpu().numpy()
    errs["final"] = rel_l2(lat, g["traj"])
    print("heavy-tailed ddim50:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs


def test_heavy_tailed_weights_ddpm1000_trajectory():
    """The full-length loop -- 1000 guided DDPM steps, one utterance, the row-tile path -- on the heavy-tailed stress weights (outlier factor 8)
    with outlier-token memories, against the restated loop driving the REFERENCE denoiser (tests/golden/heavy.npz).  This loop is well
    conditioned (the clipped x0 estimate contracts it: the numpy oracle ends 1.4e-6 from the reference), so it holds the whole budget."""
    import torch
    from convofusion_amd.denoiser import Denoiser
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import ABL, DENOISER_KW, to_dev
    from tests.helpers import heavy_state_dict, heavy_traj_case
    cb, B, L, n, seed, g = heavy_traj_case("ddpm1000")
    m = Denoiser(ablation=ABL, **DENOISER_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in heavy_state_dict(8.0).items()}, strict=True)
    m = m.cuda().eval()
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    noise = np.stack([philox_ref.normal_tensor(seed, i, range(B), 0, L) for i in range(n)])
    run = SamplingRun(m, _sched("ddpm"), [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}, B, L, n,
                      guidance_scale=7.5, init_latents=to_dev(init), step_noise=to_dev(noise))
    errs = {}
    for k in (1, 10, 100, 500, 1000):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"ddpm1000_step{k}"])
    lat = run.read(close=True).permute(1, 0, 2).cpu().numpy()
    errs["final"] = rel_l2(lat, g["ddpm1000"])
    print("heavy-tailed ddpm1000:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs


def test_heavy_tailed_weights_at_the_headline_shape():
    """BASELINE configs[1] at full size (B = 32, L = 196, 1500 audio tokens) on the heavy-tailed stress weights with outlier-token memories
    (tests/golden/heavy_c2.npz, make_golden_heavy_c2.py: the imported reference on the 7 guidance rows of utterance 5): one forward of the
    224-row batch at outlier factor 20, and 5 guided DDIM steps of the captured B = 32 loop at factor 8 (row 5 against the restated loop
    driving the reference denoiser for that utterance alone).  The forward is judged per guidance chunk against the reference run in float64
    (below): at this size and factor the numpy oracle and the torch reference, both float32, are already 1.4e-4 apart; the loop keeps the
    1e-3 budget."""
    import torch
    from convofusion_amd.denoiser import Denoiser
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import ABL, DENOISER_KW, read_debug, to_dev
    from tests.helpers import heavy_state_dict
    g = load_golden("heavy_c2")
    meta = [int(v) for v in g["meta"]]
    B, L, S, pad, t, seed, u = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13], meta[14]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, uncond_pad_tail=pad)
    mems = [to_dev(inputs.add_outlier_tokens(uq, seed + j)[rm]) for j, (uq, rm) in enumerate(zip(cb["unique"], cb["row_map"]))]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}

    def model(gain):
        m = Denoiser(ablation=ABL, **DENOISER_KW)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in heavy_state_dict(gain).items()}, strict=True)
        m = m.cuda().eval()
        m.return_attention = False
        return m
    m20 = model(20.0)
    with torch.no_grad():
        out, _ = m20(to_dev(np.concatenate([cb["init"]] * 7)), torch.tensor(t), mems, mem_mask_dict=masks)
    idx = np.array([c * B + u for c in range(7)])
    got = out.cpu().numpy()[idx]
    # Per guidance chunk, against the reference module run in FLOAT64 (out5_f64): what the float32 reference itself is worth on this input,
    # and what the split-pair path is.  Six chunks are well conditioned (float32 1e-5 from the exact result); in the listener-id chunk one
    # query token meets a softmax with very large logits at layer 4 (tools/heavy_c2_debug.py: all of the error sits there) and float32 itself
    # is 3e-4 off.  The engine's operands carry 22 significant bits against float32's 24, so it may be a small multiple of float32's own
    # error further out.
    e32 = [rel_l2(g["out5"][c], g["out5_f64"][c]) for c in range(7)]
    ehip = [rel_l2(got[c], g["out5_f64"][c]) for c in range(7)]
    e = rel_l2(got, g["out5"])
    print(f"heavy-tailed weights, headline shape: utterance {u} rows vs the float32 reference {e:.2e}; per chunk vs float64: reference "
          f"{[f'{v:.1e}' for v in e32]}, HIP {[f'{v:.1e}' for v in ehip]}, census {float(read_debug(m20, 'sat', (1,))[0])}")
    assert torch.isfinite(out).all() and float(read_debug(m20, "sat", (1,))[0]) == 0
    assert all(h < max(2e-4, 10 * r) for h, r in zip(ehip, e32)), (ehip, e32)
    assert e < 1e-3            # the forward as a whole stays inside the budget even here
    del m20, out
    run = SamplingRun(model(8.0), _sched("ddim"), mems, masks, B, L, 50, guidance_scale=7.5, seed=seed, eta=0.0)
    errs = {}
    for k in (1, 3, 5):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy()[u], g[f"traj_step{k}"][0])
    run.close()
    print("heavy-tailed weights, headline shape, guided DDIM steps:", {k: f"{v:.2e}" for k, v in errs.items()})
    # (at this shape the guided loop is ill-conditioned even at factor 8: the numpy oracle and the torch reference, both float32, are
    #  9e-6 / 8e-5 / 8.5e-4 apart after 1 / 3 / 5 steps -- make_golden_heavy_c2.py prints it -- so the later steps say less and less)
    assert errs[1] < 1e-4 and errs[3] < 5e-4 and errs[5] < 3e-3, errs


def test_cached_time_tables_never_serve_another_timestep_list():
    """cfd_sample_begin keeps the timestep-only tables (temb, AdaLN rows, A b_t / VV b_t of every memory) on the handle, keyed by the
    timestep list and the weights' generation, and skips their 31 launches when the key matches (the rollout opens eleven runs per sample
    with the same list).  Runs with list A, list B of the same length, a longer list, A again, a plain forward in between and new weights
    must each equal the result of a handle that has never seen another list -- bit for bit -- and the skip must really happen."""
    import torch
    from convofusion_amd.denoiser import Denoiser
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import ABL, DENOISER_KW, hip_denoiser, read_debug, to_dev
    B, L, S = 2, 16, (6, 20, 6, 8, 1)
    cb = inputs.make_cfg_batch(seed=9, B=B, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}

    def fresh_model(src):
        m = Denoiser(ablation=ABL, **DENOISER_KW)
        m.load_state_dict(src.state_dict(), strict=True)
        return m.cuda().eval()

    def run(m, kind, n):
        return sample(m, _sched(kind), mems, masks, B=B, L=L, num_inference_steps=n, seed=4)
    base = hip_denoiser(1234, 1.0)
    m = fresh_model(base)
    plan = [("ddpm", 10), ("ddim", 10), ("ddpm", 20), ("ddpm", 10), ("ddim", 50), ("ddpm", 10)]
    got = []
    for k, (kind, n) in enumerate(plan):
        if k == 3:       # a plain forward rebuilds the tables for its single timestep
            with torch.no_grad():
                m(to_dev(np.concatenate([cb["init"]] * 7)), torch.tensor(77), mems, mem_mask_dict=masks)
        got.append(run(m, kind, n))
    for (kind, n), g_ in zip(plan, got):
        assert torch.equal(g_, run(fresh_model(base), kind, n)), (kind, n)
    # the skip happens: same list twice in a row (DDPM-10 and DDIM-10 walk the same timesteps) -> no table launches the second time
    SamplingRun(m, _sched("ddpm"), mems, masks, B, L, 10, seed=4).close()
    r = SamplingRun(m, _sched("ddim"), mems, masks, B, L, 10, seed=4)
    assert float(read_debug(m, "setup_launches", (1,))[0]) == 0
    r.close()
    r = SamplingRun(m, _sched("ddpm"), mems, masks, B, L, 20, seed=4)
    assert float(read_debug(m, "setup_launches", (1,))[0]) > 0
    r.close()
    # new weights on the same module: the tables are rebuilt (the engine re-uploads and the generation changes)
    sharp = hip_denoiser(4321, 4.0)
    m.load_state_dict(sharp.state_dict(), strict=True)
    assert torch.equal(run(m, "ddpm", 20), run(fresh_model(sharp), "ddpm", 20))


def test_attention_maps_of_every_iteration_at_the_headline_row_shape():
    """The fused kernel's maps where its online softmax really runs: one utterance of the headline shape (196 tokens: a last query tile of 4
    rows; 1500 audio keys: 47 key tiles whose running maximum moves, with a masked tail; layer 0 through the de-duplicated lists), two
    iterations against the restated loop driving the numpy oracle."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n, seed = 1, 196, (32, 1500, 32, 8, 1), 2, 11
    pad = (5, 37, 7, 0, 0)
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, uncond_pad_tail=pad)
    sd = state_dict(1234, 1.0, 1500)     # (the memory PE buffer extended to 1500 rows, as the HIP Denoiser extends its own)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    want_lat, _, want = sampler_ref.diffusion_reverse(
        lambda x, t, e, mk: denoiser_ref.denoiser_forward(sd, x, t, e, mk), scheduler_ref.DDIMSchedulerRef(), cb["memories"], cb["masks"],
        init, lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L), num_inference_steps=n, return_att=True)
    m = hip_denoiser(1234, 1.0)
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    lat, atts = sample(m, _sched("ddim"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed, return_attention="all")
    assert torch.equal(lat, sample(m, _sched("ddim"), mems, masks, B=B, L=L, num_inference_steps=n, seed=seed))
    assert rel_l2(lat.permute(1, 0, 2).cpu().numpy(), want_lat) < TRAJ_TOL
    assert sorted(atts) == sorted(want)
    worst = 0.0
    for t in want:
        for j in range(5):
            got = atts[t][j].cpu().numpy()
            assert got.shape == want[t][j].shape == (B, 9, L, S[j])
            worst = max(worst, max_abs(got, want[t][j]))
            assert np.all(got[want[t][j] == 0] == 0)
            assert np.abs(got.sum(-1) - 1).max() < 1e-5
    print("headline row shape, fused kernel's maps: worst difference", worst)
    assert worst < 1e-4
