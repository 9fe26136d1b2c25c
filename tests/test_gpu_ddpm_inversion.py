"""-m gpu: edit-friendly DDPM inversion in level batches (cfd_ddpm_invert, ``sampler.invert_ddpm``) and the replay of its noise space
(cfd_sample_begin_replay, ``sample(..., noise_space=, keep_mask=, strength=)``), against the noise space and the replays made with the
REFERENCE denoiser (tests/golden/traj_ddpm_inversion.npz, make_golden_ddpm_inversion.py).  The fixture keeps the trajectory at three
slots and the noise at four iterations (with every row's norm) to stay within the size of the other inversion fixtures; the trajectory
is a float32 expression of the source and the level noise alone and is recomputed here in numpy for every slot.  Errors are printed.

Measured on an MI355X with the seeded weights (budget 1e-3 each): noise against the golden rows 8.1e-7; levels_per_batch 1 / 7 against N
4.3e-7 / 4.3e-7; closure 1.4e-6 (closure_ref of the float32 reference: 3.8e-7; with Philox step noise the replay lands 1.48 away);
re-conditioned replays 6.2e-6 - 8.8e-6."""
import numpy as np
import pytest

from oracle import inputs, philox_ref
from tests import ddpm_inversion_ref as ref
from tests import modality_ref
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-3          # the project's trajectory budget (tests/test_gpu_edit.py)


def _sched(oracle_table=True):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    s = scheduler.DDPMScheduler(**dict(SCHED_KW, clip_sample=True))
    if not oracle_table:      # the table users get (test_closure_on_the_schedulers_own_table)
        return s
    # the golden was made on the oracle's float32 table, which differs from the mirror's (a torch cumprod) in the last bit of most
    # entries: the runs here take the oracle's, so that "the same float32 expression" is the same bits
    import torch
    from oracle.scheduler_ref import DDPMSchedulerRef
    s.alphas_cumprod = torch.from_numpy(DDPMSchedulerRef(clip_sample=True).alphas_cumprod.copy())
    return s


def _case():
    from tests.gpu_helpers import to_dev
    g = load_golden("traj_ddpm_inversion")
    m = [int(v) for v in g["meta"]]
    B, L, S, pad, seed, N = m[0], m[1], tuple(m[2:7]), tuple(m[7:12]), m[12], int(g["n"])

    def cb(sd):
        c = inputs.make_cfg_batch(seed=sd, B=B, L=L, S=S, pad_tail=pad)
        return [to_dev(x) for x in c["memories"]], {k: to_dev(v) for k, v in c["masks"].items()}

    source = (0.8 * philox_ref.normal_tensor(seed, 0, range(B), 2, L)).astype(np.float32)
    eps = np.stack([philox_ref.normal_tensor(seed, i, range(B), 3, L) for i in range(N)]).astype(np.float32)
    return dict(g=g, B=B, L=L, N=N, seed=seed, src=cb(seed), tgt=cb(seed + 1), source=source, eps=eps, k0=int(g["k0"]))


@pytest.fixture(scope="module")
def case():
    return _case()


@pytest.fixture(scope="module")
def space(case):
    """The GPU noise space of the golden's source and level noise (default guidance, J from the budget)."""
    from convofusion_amd.sampler import invert_ddpm
    from tests.gpu_helpers import hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    traj, noise = invert_ddpm(m, _sched(), *case["src"], source_latents=to_dev(case["source"]), num_inference_steps=case["N"],
                              level_noise=to_dev(case["eps"]))
    return m, traj, noise


def _expected_trajectory(case):
    from oracle.scheduler_ref import DDPMSchedulerRef
    s = DDPMSchedulerRef(clip_sample=True)
    s.set_timesteps(case["N"])
    N = case["N"]
    t = np.empty((N + 1,) + case["source"].shape, np.float32)
    t[0] = case["source"]
    for i, ts in enumerate(s.timesteps):
        t[N - i] = ref.level(s, int(ts), case["source"], case["eps"][i])
    return t


def test_level_construction_is_exact(case, space):
    """With the golden's level noise the trajectory is the golden's, bit for bit (every slot against the float32 expression, the stored
    slots against the file).  Without: one seed twice agrees bit for bit, two seeds differ, and a level's draw depends neither on the
    table's other levels nor on levels_per_batch."""
    import torch
    from convofusion_amd.sampler import invert_ddpm
    from tests.gpu_helpers import to_dev
    m, traj, noise = space
    g, N = case["g"], case["N"]
    want = _expected_trajectory(case)
    for k in g.files:
        if k.startswith("traj"):
            assert np.array_equal(want[int(k[4:])], g[k]), k
    assert np.array_equal(traj.cpu().numpy(), want)
    assert invert_ddpm.last["chunks_evaluated"] == 2
    src = to_dev(case["source"])
    kw = dict(source_latents=src, num_inference_steps=N)
    a, _ = invert_ddpm(m, _sched(), *case["src"], seed=7, **kw)
    b, _ = invert_ddpm(m, _sched(), *case["src"], seed=7, levels_per_batch=3, **kw)
    c, _ = invert_ddpm(m, _sched(), *case["src"], seed=8, **kw)
    assert torch.equal(a, b) and not torch.equal(a[1:], c[1:]) and torch.equal(a[0], src)
    # the draw of level j is keyed by (seed, step j) alone: from a zero source slot = sb_j * eps_j, so the N- and the N / 2-level tables
    # give the same eps_j, each scaled by its own sb_j
    z, _ = invert_ddpm(m, _sched(), *case["src"], seed=7, source_latents=torch.zeros_like(src), num_inference_steps=N)
    h, _ = invert_ddpm(m, _sched(), *case["src"], seed=7, source_latents=torch.zeros_like(src), num_inference_steps=N // 2)
    s = _sched()
    s.set_timesteps(N)
    acp = s.alphas_cumprod.numpy()
    tN, tH = [int(t) for t in s.timestep_table(N)[1]], [int(t) for t in s.timestep_table(N // 2)[1]]
    for j in (0, 3, N // 2 - 1):   # eps_j = slot / sb: the same draw (seed, step j) at both tables, scaled by each table's sb_j
        eN = z[N - j].cpu().numpy() / np.sqrt(np.float32(1) - acp[tN[j]])
        eH = h[N // 2 - j].cpu().numpy() / np.sqrt(np.float32(1) - acp[tH[j]])
        assert rel_l2(eN, eH) < 1e-6, j
        # ... and it is Philox stream 2 (not the step noise's 0 or the initial latents' 1) of the restated generator; the device's logf /
        # sinf / cosf differ from numpy's by a few ulp
        e2 = rel_l2(eN, philox_ref.normal_tensor(7, j, range(case["B"]), 2, case["L"]))
        others = [rel_l2(eN, philox_ref.normal_tensor(7, j, range(case["B"]), st, case["L"])) for st in (0, 1)]
        print(f"level {j}: draw vs philox_ref stream 2 {e2:.2e}; vs streams 0 / 1 {others[0]:.2f} / {others[1]:.2f}")
        assert e2 < 1e-5 and min(others) > 0.5, (j, e2, others)
    # a replay from k0 starts where an edit run at k0 with the same draw starts: bit for bit
    from convofusion_amd.sampler import SamplingRun
    k0 = case["k0"]
    with SamplingRun(m, _sched(), *case["src"], case["B"], case["L"], N, init_latents=to_dev(case["eps"][k0]), source_latents=src,
                     strength=(N - k0) / N) as run:
        assert run.first_iteration == k0 and torch.equal(run.read(), traj[N - k0])
    with SamplingRun(m, _sched(), *case["src"], case["B"], case["L"], N, noise_space=(traj, noise), strength=(N - k0) / N) as run:
        assert run.first_iteration == k0 and run.N == N - k0 and torch.equal(run.read(), traj[N - k0])


def test_noise_matches_reference(case, space):
    """noise against the golden's rows (relative L2 over all stored rows; every row's norm), exactly 0 in the last iteration, and
    levels_per_batch 1 / 7 / N against each other."""
    import torch
    from convofusion_amd.sampler import invert_ddpm
    from tests.gpu_helpers import to_dev
    m, traj, noise = space
    g, N = case["g"], case["N"]
    rows = sorted(int(k[5:]) for k in g.files if k.startswith("noise") and k[5:].isdigit())
    got = np.concatenate([noise[i].cpu().numpy().ravel() for i in rows])
    want = np.concatenate([g[f"noise{i}"].ravel() for i in rows])
    e = rel_l2(got, want)
    norms = np.array([np.linalg.norm(noise[i].cpu().numpy().astype(np.float64)) for i in range(N)])
    en = float(np.abs(norms - g["noise_norms"]).max() / g["noise_norms"].max())
    print(f"noise vs golden rows {rows}: {e:.2e}; row norms {en:.2e}")
    assert len(rows) >= 4 and e < TOL and en < TOL, (e, en)
    assert not bool(noise[N - 1].any()) and bool(torch.isfinite(noise).all())
    full = None
    for J in (N, 1, 7):
        _, z = invert_ddpm(m, _sched(), *case["src"], source_latents=to_dev(case["source"]), num_inference_steps=N,
                           level_noise=to_dev(case["eps"]), levels_per_batch=J)
        assert invert_ddpm.last["levels_per_batch"] == J
        if full is None:
            full = z
            continue
        ej = rel_l2(z.cpu().numpy(), full.cpu().numpy())
        print(f"levels_per_batch {J} vs {N}: {ej:.2e}")
        assert ej < TOL, (J, ej)


def test_replay_closes_under_the_source_conditioning(case, space):
    """N - 1 iterations of the replay under the source conditioning return trajectory[1]; the final read is the golden's last snapshot;
    the same replay with Philox step noise lands at least 100x further away."""
    from convofusion_amd.sampler import INVERSION_WEIGHTS, SamplingRun
    m, traj, noise = space
    g, B, L, N = case["g"], case["B"], case["L"], case["N"]
    with SamplingRun(m, _sched(), *case["src"], B, L, N, guidance_scale=1.0, modality_weights=INVERSION_WEIGHTS,
                     noise_space=(traj, noise)) as run:
        run.steps(N - 1)
        near = run.read().cpu().numpy()
        run.steps(1)
        last = run.read(close=True).cpu().numpy()
    closure = rel_l2(near, traj[1].cpu().numpy())
    e19, e20 = rel_l2(near, g["src_step19"]), rel_l2(last, g["src_step20"])
    with SamplingRun(m, _sched(), *case["src"], B, L, N, guidance_scale=1.0, modality_weights=INVERSION_WEIGHTS, init_latents=traj[N],
                     seed=11, operands=0) as run:
        run.steps(N - 1)
        contrast = rel_l2(run.read(close=True).cpu().numpy(), traj[1].cpu().numpy())
    print(f"closure {closure:.2e} (closure_ref {float(g['closure_ref']):.2e}); vs golden after N - 1 / N: {e19:.2e} / {e20:.2e}; "
          f"Philox step noise instead: {contrast:.2e} (contrast_ref {float(g['contrast_ref']):.2e})")
    assert closure < TOL and e19 < TOL and e20 < TOL, (closure, e19, e20)
    assert contrast >= 100 * closure, (contrast, closure)


def test_reconditioned_replays_match_reference(case, space):
    """Replays under the second conditioning at guidance scale 7.5 against the golden: plain, with the keep mask, from k0, and with a
    weight table that prunes a chunk.  The replay with no kept token from iteration 0 is bit-identical to the plain DDPM run on the same
    initial latents and step noise."""
    import torch
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import to_dev
    m, traj, noise = space
    g, B, L, N, k0 = case["g"], case["B"], case["L"], case["N"], case["k0"]
    keep = to_dev(g["keep"])
    kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=7.5)
    plain = sample(m, _sched(), *case["tgt"], noise_space=(traj, noise), **kw)
    kept = sample(m, _sched(), *case["tgt"], noise_space=(traj, noise), keep_mask=keep, **kw)
    strength = (N - k0) / N
    late = sample(m, _sched(), *case["tgt"], noise_space=(traj, noise), strength=strength, **kw)
    w = modality_ref.golden_weights(N)
    with SamplingRun(m, _sched(), *case["tgt"], B, L, N, guidance_scale=7.5, modality_weights=torch.from_numpy(w),
                     noise_space=(traj, noise)) as run:
        pruned = run.chunks_evaluated
        run.steps(run.N)
        weighted = run.read(close=True)
    # keep mask, k0 > 0 and the weight table together: the anchored instance reads slot N - *d_step with d_step started at k0, and the
    # table row is the full table's
    both = sample(m, _sched(), *case["tgt"], noise_space=(traj, noise), keep_mask=keep, strength=strength,
                  modality_weights=torch.from_numpy(w), **kw)
    errs = dict(plain=rel_l2(plain.cpu().numpy(), g["tgt_plain"]), keep=rel_l2(kept.cpu().numpy(), g["tgt_keep"]),
                k0=rel_l2(late.cpu().numpy(), g["tgt_k0"]), weighted=rel_l2(weighted.cpu().numpy(), g["tgt_weighted"]),
                keep_k0_weighted=rel_l2(both.cpu().numpy(), g["tgt_all"]))
    print("re-conditioned replays vs golden", {k: f"{v:.2e}" for k, v in errs.items()}, "chunks evaluated (weighted)", pruned)
    assert all(v < TOL for v in errs.values()), errs
    assert pruned < 7
    kb = g["keep"].astype(bool)
    ek = rel_l2(kept.cpu().numpy()[kb], g["tgt_keep"][kb])
    print(f"kept tokens of the finished keep-mask run vs golden {ek:.2e}")
    assert ek < TOL
    same = sample(m, _sched(), *case["tgt"], init_latents=traj[N], step_noise=noise, operands=0, **kw)
    assert torch.equal(plain, same)
    # return_attention with a noise space: the same latents, one entry per EXECUTED iteration, keyed by its timestep
    lat_a, atts = sample(m, _sched(), *case["tgt"], noise_space=(traj, noise), strength=strength, return_attention="all", **kw)
    table = [int(t) for t in _sched().timestep_table(N)[1]]
    ea = rel_l2(lat_a.cpu().numpy(), g["tgt_k0"])
    print(f"return_attention='all' from k0: {len(atts)} entries, latents vs golden {ea:.2e}")
    assert sorted(atts, reverse=True) == table[k0:] and ea < TOL
    assert all(len(v) == 5 and bool(torch.isfinite(v[1]).all()) for v in atts.values())


def test_default_guidance_arm_equals_weighted(case, space):
    """cfd_ddpm_invert with weights == NULL (args->guidance_weight; ddpm_extract_kernel's default instance) against the weighted call on
    the same level noise.  All 7 chunks evaluated on both sides: same rows, same terms in the same order (a zero weight contributes a
    zero) -- bit for bit.  With skip_zero_weight_chunks the default arm trims the trailing zero-weight chunks, the weighted call prunes
    the same ones: the same two chunks' rows -- bit for bit again.  The pruned weighted call is ``invert_ddpm``'s own."""
    import ctypes as C
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import to_dev
    m, traj, noise = space
    B, L, N = case["B"], case["L"], case["N"]
    run = SamplingRun(m, _sched(), *case["src"], B, L, N)      # (its argument struct: the memories with their row maps, the tables)
    a = run._args
    run.close()
    lib, h = _lib.load(), run.handle
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src, eps = to_dev(case["source"]), to_dev(case["eps"])

    def call(weights7, table, prune, skip):
        iv = _lib.DdpmInvertArgs()
        t, z = torch.empty_like(traj), torch.empty_like(noise)
        iv.source, iv.level_noise, iv.trajectory, iv.noise = src.data_ptr(), eps.data_ptr(), t.data_ptr(), z.data_ptr()
        a.guidance_weight = (C.c_float * 8)(*weights7)
        a.skip_zero_weight_chunks = skip
        wt = None
        if table:
            wt = np.zeros((N, B, 8), np.float32)
            wt[:, :, :] = np.asarray(weights7, np.float32)
            iv.weights, iv.prune = wt.ctypes.data_as(C.c_void_p), prune
        ge = C.c_int(0)
        torch.cuda.synchronize()
        _lib.check(lib.cfd_ddpm_invert(h, C.byref(a), C.byref(iv), C.byref(ge), None, st))
        torch.cuda.synchronize()
        assert torch.equal(t, traj)
        return z, ge.value

    cond = [0.0] * 6 + [1.0, 0.0]               # INVERSION_WEIGHTS at guidance_scale 1: the full-conditioning chunk alone
    d7, g1 = call(cond, False, 0, 0)
    w7, g2 = call(cond, True, 0, 0)
    w2, g3 = call(cond, True, 1, 0)
    print(f"default vs weighted, 7 chunks: {rel_l2(d7.cpu().numpy(), w7.cpu().numpy()):.2e}; pruned weighted vs 7 chunks "
          f"{rel_l2(w2.cpu().numpy(), w7.cpu().numpy()):.2e}; chunks {g1} {g2} {g3}")
    assert (g1, g2, g3) == (7, 7, 2) and torch.equal(d7, w7) and torch.equal(w2, noise)
    assert rel_l2(w2.cpu().numpy(), w7.cpu().numpy()) < TOL
    text = [0.0, 2.5] + [0.0] * 6               # the text-only chunk at 2.5: chunks 2 - 6 trail with weight 0
    ds, g4 = call(text, False, 0, 1)
    ws, g5 = call(text, True, 1, 0)
    df, g6 = call(text, False, 0, 0)
    print(f"default with skip_zero_weight_chunks vs pruned weighted: {rel_l2(ds.cpu().numpy(), ws.cpu().numpy()):.2e}; vs all 7 chunks "
          f"{rel_l2(ds.cpu().numpy(), df.cpu().numpy()):.2e}; chunks {g4} {g5} {g6}")
    assert (g4, g5, g6) == (2, 2, 7) and torch.equal(ds, ws) and rel_l2(ds.cpu().numpy(), df.cpu().numpy()) < TOL
    assert not torch.equal(ds, d7)


def test_closure_on_the_schedulers_own_table(case):
    """invert_ddpm and the replay on the table users get (the scheduler's own alphas_cumprod, not the oracle's): the replay under the
    source conditioning returns the recorded trajectory[1] within the budget, Philox step noise does not."""
    from convofusion_amd.sampler import INVERSION_WEIGHTS, SamplingRun, invert_ddpm
    from tests.gpu_helpers import hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    B, L, N = case["B"], case["L"], case["N"]
    traj, noise = invert_ddpm(m, _sched(False), *case["src"], source_latents=to_dev(case["source"]), num_inference_steps=N, seed=3)
    kw = dict(guidance_scale=1.0, modality_weights=INVERSION_WEIGHTS)
    with SamplingRun(m, _sched(False), *case["src"], B, L, N, noise_space=(traj, noise), **kw) as run:
        run.steps(N - 1)
        closure = rel_l2(run.read(close=True).cpu().numpy(), traj[1].cpu().numpy())
    with SamplingRun(m, _sched(False), *case["src"], B, L, N, init_latents=traj[N], seed=11, operands=0, **kw) as run:
        run.steps(N - 1)
        contrast = rel_l2(run.read(close=True).cpu().numpy(), traj[1].cpu().numpy())
    print(f"scheduler's own table: closure {closure:.2e}, Philox step noise instead {contrast:.2e}")
    assert closure < TOL and contrast >= 100 * closure and not bool(noise[N - 1].any())


def test_composition_and_refusals(case, space):
    """sample_sharded over two simulated slices equals the single run; the refusals raise; a run left open by an exception is closed."""
    import ctypes as C
    import torch
    from convofusion_amd import _lib, distributed
    from convofusion_amd.sampler import SamplingRun, invert_ddpm, sample, sample_with_weg
    from tests.gpu_helpers import to_dev
    m, traj, noise = space
    B, L, N = case["B"], case["L"], case["N"]
    kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=7.5)
    one = sample(m, _sched(), *case["tgt"], noise_space=(traj, noise), **kw)
    parts = []
    for r in range(2):   # each simulated rank gets its rows of both rings
        lo, hi = distributed.shard_range(B, r, 2)
        enc = [distributed.shard_cfg_batch(x, lo, hi, B) for x in case["tgt"][0]]
        masks = {k: distributed.shard_cfg_batch(v, lo, hi, B) for k, v in case["tgt"][1].items()}
        parts.append(sample(m, _sched(), enc, masks, noise_space=distributed.shard_noise_space((traj, noise), lo, hi, B),
                            **dict(kw, B=hi - lo)))
    sharded = distributed.sample_sharded(lambda e, k, **x: sample(m, _sched(), e, k, **dict(kw, **x)), *case["tgt"], B,
                                         noise_space=(traj, noise))
    assert torch.equal(sharded, one)
    assert torch.equal(torch.cat(parts), one)
    src = to_dev(case["source"])
    for bad in (dict(tie=torch.full((B, L), -1, dtype=torch.int32)), dict(preseq=src[:, :2]), dict(anchor_trajectory=traj),
                dict(source_latents=src), dict(init_latents=src), dict(strength=0.0)):
        with pytest.raises(ValueError):
            sample(m, _sched(), *case["tgt"], noise_space=(traj, noise), **kw, **bad)
    with pytest.raises(ValueError):
        sample(m, _sched(), *case["tgt"], noise_space=(traj[1:], noise), **kw)
    with pytest.raises(NotImplementedError):
        sample_with_weg(m, _sched(), *case["tgt"], [[1]], {}, noise_space=(traj, noise), **kw)
    # the library's own refusals (CFD_E_ARG) ...
    run = SamplingRun(m, _sched(), *case["tgt"], B, L, N, noise_space=(traj, noise))
    a = run._args
    run.close()
    lib, h = _lib.load(), run.handle
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rp = _lib.ReplayArgs()
    rp.trajectory, rp.noise, rp.steps, rp.B, rp.L = traj.data_ptr(), noise.data_ptr(), N, B, L

    def refused(call):
        with pytest.raises(_lib.CfdError) as e:
            _lib.check(call())
        assert e.value.code == -1, e.value

    for field, value in (("steps", N - 1), ("B", B + 1), ("first_iteration", N), ("trajectory", None), ("noise", None)):
        old = getattr(rp, field)
        setattr(rp, field, value)
        refused(lambda: lib.cfd_sample_begin_replay(h, C.byref(a), C.byref(rp), None, 0, None, st))
        setattr(rp, field, old)
    a.scheduler = 1
    refused(lambda: lib.cfd_sample_begin_replay(h, C.byref(a), C.byref(rp), None, 0, None, st))
    iv = _lib.DdpmInvertArgs()
    out_t, out_z = torch.empty_like(traj), torch.empty_like(noise)
    iv.source, iv.trajectory, iv.noise = src.data_ptr(), out_t.data_ptr(), out_z.data_ptr()
    refused(lambda: lib.cfd_ddpm_invert(h, C.byref(a), C.byref(iv), None, None, st))       # kind 1
    a.scheduler = 0
    a.dynamic_memory_mask = 1
    refused(lambda: lib.cfd_ddpm_invert(h, C.byref(a), C.byref(iv), None, None, st))
    refused(lambda: lib.cfd_sample_begin_replay(h, C.byref(a), C.byref(rp), None, 0, None, st))
    a.dynamic_memory_mask = 0
    a.preseq, a.preseq_len = src.data_ptr(), 2
    refused(lambda: lib.cfd_ddpm_invert(h, C.byref(a), C.byref(iv), None, None, st))
    refused(lambda: lib.cfd_sample_begin_replay(h, C.byref(a), C.byref(rp), None, 0, None, st))
    a.preseq, a.preseq_len = None, 0
    ring = torch.empty(16, device=src.device)
    a.att_ring = (C.c_void_p * _lib.NUM_MEM)(*[ring.data_ptr()] * _lib.NUM_MEM)
    refused(lambda: lib.cfd_ddpm_invert(h, C.byref(a), C.byref(iv), None, None, st))
    a.att_ring = (C.c_void_p * _lib.NUM_MEM)()
    iv.noise = None
    refused(lambda: lib.cfd_ddpm_invert(h, C.byref(a), C.byref(iv), None, None, st))
    iv.noise = out_z.data_ptr()
    wt = np.zeros((N, B, 8), np.float32)
    wt[3, 1, 2] = np.inf
    iv.weights = wt.ctypes.data_as(C.c_void_p)
    refused(lambda: lib.cfd_ddpm_invert(h, C.byref(a), C.byref(iv), None, None, st))
    with SamplingRun(m, _sched(), *case["tgt"], B, L, N, noise_space=(traj, noise)) as rr:      # the library refuses a WEG update too
        refused(lambda: lib.cfd_sample_write(rr.handle, C.c_void_p(src.data_ptr())))
        with pytest.raises(ValueError):
            rr.write(src)
    # ... and nothing of it left a run open: the next run opens and closes
    with pytest.raises(ValueError):
        invert_ddpm(m, _sched(), *case["src"], source_latents=src, num_inference_steps=N, modality_weights=dict(text=float("nan")))
    again = sample(m, _sched(), *case["tgt"], noise_space=(traj, noise), **kw)
    assert torch.equal(again, one)


def test_reperform_motion_ddpm_end_to_end():
    """reperform_motion(method="ddpm") = HIP encode -> invert_ddpm (source conditioning, the model's own DDPM scheduler and step count) ->
    replay (target conditioning) -> HIP decode, bit for bit its steps by hand; with target = source conditioning the latents are the
    closure result (printed: their distance from the source; the last step returns the model's x0 estimate).  method="ddim" given
    explicitly takes the default's path (same result); that this path still computes what it did before the DDPM method existed is
    what tests/test_gpu_inversion.py::test_reperform_motion_equals_its_steps_by_hand holds it to, against the DDIM steps done by hand."""
    import torch
    from types import SimpleNamespace
    from convofusion_amd import scheduler
    from convofusion_amd.edit import loop_to_vae, reperform_motion, token_mask, vae_to_loop
    from convofusion_amd.sampler import invert_ddpm, sample
    from tests.gpu_helpers import SCHED_KW, hip_denoiser
    from tests.test_gpu_inversion import SMALL, _inputs, _vae
    B, n, seed = 2, 20, 17
    src_c, src_m = _inputs(B, 16, *SMALL, seed)
    tgt_c, tgt_m = _inputs(B, 16, *SMALL, seed + 1)
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    cfg = SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=n)))
    model = SimpleNamespace(vae=_vae(), denoiser=hip_denoiser(1234, 1.0), scheduler=sch, guidance_scale=7.5, clf_guidance_drops=6,
                            do_classifier_free_guidance=True, cfg=cfg)
    g = torch.Generator().manual_seed(seed)
    feats = (0.5 * torch.randn((B, 128, 189), generator=g)).cuda()
    lengths = [128, 128]
    keep = token_mask(B, keep_frames=[(0, 32)], keep_parts=("body",)).cuda()
    out, lat, x_T = reperform_motion(model, feats, lengths, src_c, tgt_c, source_masks=src_m, target_masks=tgt_m, keep_mask=keep,
                                     method="ddpm", strength=0.8, seed=5)
    _, dist, _ = model.vae.encode(feats, lengths)
    src = vae_to_loop(dist.mean.reshape(2, B, 8, 128))
    space = invert_ddpm(model.denoiser, sch, src_c, src_m, source_latents=src, num_inference_steps=n, seed=5)
    want_lat = sample(model.denoiser, sch, tgt_c, tgt_m, B=B, L=16, num_inference_steps=n, guidance_scale=7.5, skip_zero_weight_chunks=True,
                      noise_space=space, keep_mask=keep, strength=0.8)
    want = model.vae.decode(loop_to_vae(want_lat), lengths)
    assert tuple(out.shape) == (B, 128, 189) and torch.isfinite(out).all()
    assert torch.equal(x_T, space[0][n]) and torch.equal(lat, want_lat) and torch.equal(out, want)
    # target = source conditioning and guidance: the closure result
    _, same, _ = reperform_motion(model, feats, lengths, src_c, src_c, source_masks=src_m, target_masks=src_m, method="ddpm", seed=5,
                                  modality_weights=dict(text=0.0, audio=0.0, spk=0.0, apb=0.0, lsnid=0.0, all=1.0 / 7.5))
    with sampler_run(model.denoiser, sch, src_c, src_m, B, n, space) as run:
        run.steps(n)
        closed = run.read(close=True)
    e = rel_l2(same.cpu().numpy(), closed.cpu().numpy())
    print(f"ddpm round trip: latents vs the closure result {e:.2e}; vs the source {rel_l2(same.cpu().numpy(), src.cpu().numpy()):.2e}")
    assert e < TOL
    a = reperform_motion(model, feats, lengths, src_c, tgt_c, source_masks=src_m, target_masks=tgt_m, num_inference_steps=10, keep_mask=keep)
    b = reperform_motion(model, feats, lengths, src_c, tgt_c, source_masks=src_m, target_masks=tgt_m, num_inference_steps=10, keep_mask=keep,
                         method="ddim")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def sampler_run(denoiser, sch, enc, masks, B, n, space):
    from convofusion_amd.sampler import INVERSION_WEIGHTS, SamplingRun
    return SamplingRun(denoiser, sch, enc, masks, B, 16, n, guidance_scale=1.0, modality_weights=INVERSION_WEIGHTS, noise_space=space)


# levels_per_batch 2 against 3 at the shape of test_identity_row_map_equals_none (rel. L2 of the noise rows): 4 x the figure measured on
# an MI355X on the commit before the three row-map sites shared one helper.  Two batch compositions may re-associate the forward's sums
# (4.3e-7 at the golden's shape, test_noise_matches_reference); at B = 2, L = 2, N = 4 that commit's two compositions give the same bits:
# the figure is 0.0, and so is the bound.
PARENT_LPB_2_VS_3 = 0.0
LPB_BOUND = 4 * PARENT_LPB_2_VS_3


def test_identity_row_map_equals_none():
    """Memories with U = 7 * B and no row_map against the same memories with an explicit identity row_map, through a pruned weighted level
    batch (the audio column 0 throughout: 6 of the 7 chunks are evaluated) at the level batches' smallest shape, B = 2, L = 2, N = 4:
    cfd_ddpm_invert with levels_per_batch 2 and 3 (N % J != 0: the last batch overlaps the one before) and cfd_sample_parallel at tolerance
    0 agree bit for bit between the two forms.  levels_per_batch 2 against 3: the trajectory bit for bit, the noise rows within LPB_BOUND
    (measured on an MI355X: 0.0 on the commit before, 0.0 on this one)."""
    import torch
    from convofusion_amd.sampler import invert_ddpm, sample_parallel
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, N = 2, 2, 4
    m = hip_denoiser(1234, 1.0)
    cb = inputs.make_cfg_batch(seed=5, B=B, L=L, S=(6, 20, 6, 8, 1), pad_tail=(2, 0, 1, 0, 0))
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    assert all(int(x.shape[0]) == 7 * B for x in mems)
    ident = [torch.arange(7 * B, dtype=torch.int32, device="cuda") for _ in mems]
    w = dict(text=1.0, audio=0.0, spk=0.5, apb=1.5, lsnid=1.0, all=0.25)
    src = to_dev((0.8 * philox_ref.normal_tensor(11, 0, range(B), 2, L)).astype(np.float32))
    forms = (dict(dedup=False), dict(row_maps=ident))
    noise_of = {}
    for J in (2, 3):
        got = []
        for form in forms:
            got.append(invert_ddpm(m, _sched(), mems, masks, source_latents=src, num_inference_steps=N, guidance_scale=2.0,
                                   modality_weights=w, seed=3, levels_per_batch=J, **form))
            assert invert_ddpm.last == dict(chunks_evaluated=6, levels_per_batch=J)
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), J
        assert bool(torch.isfinite(got[0][1]).all()) and bool(got[0][1][:N - 1].any())
        noise_of[J] = got[0]
    assert torch.equal(noise_of[2][0], noise_of[3][0])
    e = rel_l2(noise_of[3][1].cpu().numpy(), noise_of[2][1].cpu().numpy())
    print(f"levels_per_batch 3 vs 2, noise rows: {e:.3e} (bound {LPB_BOUND:.3e})")
    lat = []
    for form in forms:
        x, stats = sample_parallel(m, _sched(), mems, masks, B=B, L=L, num_inference_steps=N, tolerance=0.0, guidance_scale=2.0,
                                   modality_weights=w, seed=3, levels_per_batch=2, **form)
        assert stats.chunks_evaluated == 6 and stats.levels_per_batch == 2
        lat.append(x)
    assert torch.equal(lat[0], lat[1]) and bool(torch.isfinite(lat[0]).all())
    assert e <= LPB_BOUND, (e, LPB_BOUND)
