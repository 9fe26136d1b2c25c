"""-m gpu: parallel-in-time DDPM sampling (cfd_sample_parallel, ``sampler.sample_parallel``): Picard sweeps over level batches.

Tolerance 0 against the trajectories made with the REFERENCE denoiser (tests/golden/traj_ddpm20_b2, traj_ddpm1000, traj_modality_ddpm20;
inputs loaded as tests/test_gpu_sampler.py::test_sampler_matches_reference_trajectory loads them), the Philox draws against the tensors
passed in, run-to-run determinism, the bookkeeping, the refusals, and cfd_ddpm_invert around a parallel call on the same handle.
Tolerance > 0 against the restated sweeps (tests/parallel_ref) on the HIP forward of single levels, with planted-bug sensitivity.
Distances and sweep counts are printed.

Measured on an MI355X: tolerance 0 is 1.05e-5 / 9.05e-6 / 6.90e-6 from the goldens' final latents (ddpm20_b2 /
ddpm1000 / modality_ddpm20) and 7.07e-6 / 2.19e-6 / 3.92e-6 from the sequential fused run on split-pair operands; tolerance 0.1 on the
ddpm1000 inputs takes 26 sweeps at the default 283 levels per batch and ends 1.72e-3 from the golden."""
import ctypes as C

import numpy as np
import pytest

from oracle import inputs, philox_ref
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-3          # the project's trajectory budget, as tests/test_gpu_sampler.py


def _sched(kind="ddpm"):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    return scheduler.DDIMScheduler(**SCHED_KW) if kind == "ddim" else scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)


def _case(name):
    """The golden's inputs on the device: memories, masks, Philox initial latents (stream 1) and step noise (stream 0, step index i)."""
    from tests.gpu_helpers import to_dev
    g = load_golden("traj_" + name)
    meta = [int(x) for x in g["meta"]]
    B, L, S, pad, n, seed = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    noise = np.stack([philox_ref.normal_tensor(seed, i, range(B), 0, L) for i in range(n)])
    return dict(g=g, B=B, L=L, N=n, seed=seed, mems=[to_dev(x) for x in cb["memories"]], masks={k: to_dev(v) for k, v in cb["masks"].items()},
                init=to_dev(init), noise=to_dev(noise), weights=g["weights"] if "weights" in g.files else None)


@pytest.fixture(scope="module")
def small():
    return _case("ddpm20_b2")


def _par(c, **kw):
    from convofusion_amd.sampler import sample_parallel
    from tests.gpu_helpers import hip_denoiser
    args = dict(B=c["B"], L=c["L"], num_inference_steps=c["N"], guidance_scale=7.5, modality_weights=c["weights"], init_latents=c["init"],
                step_noise=c["noise"])
    args.update(kw)
    return sample_parallel(hip_denoiser(1234, 1.0), _sched(), c["mems"], c["masks"], **args)


@pytest.mark.parametrize("name,J", [("ddpm20_b2", 7), ("ddpm1000", 12), ("modality_ddpm20", 7)])
def test_tolerance_zero_matches_reference_trajectory(name, J):
    """tau = 0: the final latents and every stored snapshot, read from the returned trajectory (slot N - k: the latents after k
    iterations), within TRAJ_TOL of the reference-generated golden.  Printed: the distance from the sequential fused run on split-pair
    operands (operands=0) with the same initial latents and step noise, and the sweeps."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    c = _case(name)
    g, N = c["g"], c["N"]
    lat, traj, stats = _par(c, tolerance=0.0, levels_per_batch=J, trajectory=True)
    assert tuple(lat.shape) == (c["B"], c["L"], 128) and tuple(traj.shape) == (N + 1, c["B"], c["L"], 128)
    assert torch.equal(traj[0], lat) and torch.equal(traj[N], c["init"])
    errs = {k: rel_l2(traj[N - k].cpu().numpy(), g[f"step{k}"]) for k in sorted(int(f[4:]) for f in g.files if f.startswith("step"))}
    errs["final"] = rel_l2(lat.permute(1, 0, 2).cpu().numpy(), g["latents"])
    seq = sample(hip_denoiser(1234, 1.0), _sched(), c["mems"], c["masks"], B=c["B"], L=c["L"], num_inference_steps=N, guidance_scale=7.5,
                 init_latents=c["init"], step_noise=c["noise"], operands=0, modality_weights=c["weights"])
    d_seq = rel_l2(lat.cpu().numpy(), seq.cpu().numpy())
    print(f"parallel tau=0 {name} J={J}:", {k: f"{v:.2e}" for k, v in errs.items()}, f"vs sequential operands=0: {d_seq:.2e};", stats)
    assert stats.levels_per_batch == J and stats.chunks_evaluated == 6
    assert sum(stats.strides) == N and stats.sweeps == len(stats.strides) <= N
    assert bool(torch.isfinite(traj).all())
    assert all(v < TRAJ_TOL for v in errs.values()), errs


def _library_draws(c):
    """The library's own Philox draws (cfd_philox_normal) of the tensors ``_case`` restates in numpy: the initial latents (stream 1, step
    index 0) and the noise of every iteration (stream 0, step index i)."""
    import torch
    from convofusion_amd import _lib
    lib, h = _lib.load(), _lib.create_handle(0)
    B, per = c["B"], c["L"] * 128
    init, noise = torch.empty_like(c["init"]), torch.empty_like(c["noise"])
    _lib.check(lib.cfd_philox_normal(h, C.c_void_p(init.data_ptr()), B, per, c["seed"], 0, 0, 1, None))
    for i in range(c["N"]):
        _lib.check(lib.cfd_philox_normal(h, C.c_void_p(noise[i].data_ptr()), B, per, c["seed"], i, 0, 0, None))
    torch.cuda.synchronize()
    lib.cfd_destroy(h)
    return init, noise


def test_same_seed_draws_the_captured_loops_noise(small):
    """Without init_latents / step_noise the call draws Philox stream 1 and stream 0 with step index i under ``seed``: bit for bit the
    result with those tensors passed in -- at tau = 0 and at a tolerance that takes strides > 1.  The tensors passed in are the library's
    draws (cfd_philox_normal): the numpy restatement differs from the device's logf / cosf / sinf in the last bits (within 2e-5,
    tests/test_gpu_kernels.py::test_philox_matches_oracle, checked here for these streams and indices too), which a chain amplifies."""
    import torch
    init, noise = _library_draws(small)
    for got, want in ((init, small["init"]), (noise, small["noise"])):
        assert float((got - want).abs().max()) <= 2e-5
    for tau in (0.0, 0.1):
        a, sa = _par(small, tolerance=tau, levels_per_batch=6, init_latents=init, step_noise=noise)
        b, sb = _par(small, tolerance=tau, levels_per_batch=6, init_latents=None, step_noise=None, seed=small["seed"])
        assert torch.equal(a, b) and sa.strides == sb.strides, (tau, float((a - b).abs().max()))
    other, _ = _par(small, tolerance=0.0, levels_per_batch=6, init_latents=None, step_noise=None, seed=small["seed"] + 1)
    assert not torch.equal(other, a)


def test_one_level_per_batch_ignores_the_tolerance(small):
    import torch
    a, sa = _par(small, tolerance=0.0, levels_per_batch=1)
    b, sb = _par(small, tolerance=1e9, levels_per_batch=1)
    assert torch.equal(a, b) and sa.strides == sb.strides == [1] * small["N"] and sa.sweeps == small["N"]
    err = rel_l2(a.permute(1, 0, 2).cpu().numpy(), small["g"]["latents"])
    print(f"parallel J=1 vs golden: {err:.2e}")
    assert err < TRAJ_TOL


def test_two_calls_are_bit_identical(small):
    """tau = 0.1, J > 1: the error sums that decide the strides are reduced in a fixed order -- the same strides, the same bits, with and
    without the caller's trajectory buffer (the ring of J + 1 slots is the same code)."""
    import torch
    a, ta, sa = _par(small, tolerance=0.1, levels_per_batch=8, trajectory=True)
    b, tb, sb = _par(small, tolerance=0.1, levels_per_batch=8, trajectory=True)
    c, sc = _par(small, tolerance=0.1, levels_per_batch=8)
    print("parallel tau=0.1 J=8:", sa, sa.strides)
    assert torch.equal(a, b) and torch.equal(ta, tb) and sa.strides == sb.strides
    assert torch.equal(a, c) and sa.strides == sc.strides
    assert sum(sa.strides) == small["N"] and max(sa.strides) <= 8


def test_stats_and_max_sweeps(small):
    import torch
    from convofusion_amd import _lib
    N = small["N"]
    lat, st = _par(small, tolerance=0.0)                      # J from the default budget: clamped to N
    assert st.levels_per_batch == N and sum(st.strides) == N and st.sweeps == len(st.strides) <= N and st.chunks_evaluated == 6
    lat2, st2 = _par(small, tolerance=0.0, workspace_bytes=1)   # a budget below one level: J = 1
    assert st2.levels_per_batch == 1 and st2.sweeps == N
    assert rel_l2(lat.cpu().numpy(), lat2.cpu().numpy()) < TRAJ_TOL
    with pytest.raises(_lib.CfdError) as e:
        _par(small, tolerance=0.0, levels_per_batch=4, max_sweeps=3)
    assert e.value.code == -3 and "max_sweeps = 3" in str(e.value) and "levels final" in str(e.value), e.value
    lat3, st3 = _par(small, tolerance=0.0, levels_per_batch=4, max_sweeps=N)   # ... and the handle is usable afterwards
    assert st3.sweeps <= N and bool(torch.isfinite(lat3).all())


def test_tolerance_on_the_thousand_step_chain():
    """tau = 0.1 on the ddpm1000 inputs: a finite result whose strides stay within the batch; its sweeps and its distance from the golden
    are printed (no gate on either: nobody has measured what quality the tolerance buys)."""
    import torch
    c = _case("ddpm1000")
    lat, st = _par(c, tolerance=0.1)
    d = rel_l2(lat.permute(1, 0, 2).cpu().numpy(), c["g"]["latents"])
    print(f"parallel tau=0.1 ddpm1000: {st}, mean stride {c['N'] / st.sweeps:.2f}, vs golden {d:.2e}")
    assert bool(torch.isfinite(lat).all()) and sum(st.strides) == c["N"] and st.sweeps <= c["N"]
    assert max(st.strides) <= st.levels_per_batch


# B, L, N, J, tau, whether a fill from the wrong slot moves the result of the case (the third is blind to it)
RESTATED = [(2, 20, 20, 6, 0.3, True), (1, 4, 20, 7, 0.3, True), (3, 16, 10, 4, 0.5, False)]
GUARD_BAND = (0.95, 1.05)
ERR_GPU_GATE = 4 * 8.17e-6      # 4 x the largest err_gpu measured on an MI355X (the docstring below has the three)


@pytest.mark.parametrize("B,L,N,J,tau,fill_visible", RESTATED)
def test_tolerance_runs_match_the_restated_sweeps(B, L, N, J, tau, fill_visible):
    """tau > 0 against tests/parallel_ref.sample_parallel: scan, error sums, stride rule and fill in numpy, the guided prediction of a
    level from the HIP Denoiser forward on the 7-chunk batch (tested against the reference on its own) under
    oracle.sampler_ref.cfg_combine.  Asserted: the same strides -- fair because every err / bound ratio the restated rule evaluated lies
    outside GUARD_BAND (the device's predictions of a level-batched and a single forward differ in the last bits); the final latents and
    every trajectory slot within ERR_GPU_GATE (relative L2; err_gpu: the largest of them); the restated loop with the scan's carry
    dropped, and (first two cases) with the entering levels filled from X(i1), further than 10 err_gpu from the correct one, the carry
    mutant with other strides than the library's; and the call without a trajectory (the private J + 1 ring) bit-identical to the one
    with it, at L = 20 and L = 4.

    Measured on an MI355X, in the order of RESTATED: err_gpu 5.25e-6 / 5.96e-6 / 8.17e-6 (the gate: 4 x the
    largest; the tolerance 0 distance from the sequential run is up to 7e-6); the nearest err / bound ratios 1.095 / 1.127 / 0.785;
    strides 1 2 2 3 3 2 2 2 1 1 1 (twice) and 1 2 2 1 2 1 1; the carry mutant moves the result 1.12e-2 / 9.13e-3 / 5.03e-2 with strides
    all 1, the fill mutant 4.00e-3 / 6.28e-3."""
    import torch
    from oracle.sampler_ref import cfg_combine
    from oracle.scheduler_ref import DDPMSchedulerRef
    from tests import parallel_ref as ref
    from tests.gpu_helpers import hip_denoiser, to_dev
    seed = 11
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=(6, 20, 12, 8, 1), pad_tail=(2, 0, 3, 0, 0))
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    noise = np.stack([philox_ref.normal_tensor(seed, i, range(B), 0, L) for i in range(N)])
    c = dict(B=B, L=L, N=N, mems=[to_dev(x) for x in cb["memories"]], masks={k: to_dev(v) for k, v in cb["masks"].items()}, init=to_dev(init),
             noise=to_dev(noise), weights=None)
    m = hip_denoiser(1234, 1.0)

    def eps_fn(x, i, t):
        with torch.no_grad():
            out = m(to_dev(np.concatenate([x] * 7, axis=0)), torch.tensor(int(t)), c["mems"], mem_mask_dict=c["masks"])[0]
        return cfg_combine(out.cpu().numpy(), 7.5)

    ratios = []
    want_lat, want_traj, want_strides = ref.sample_parallel(eps_fn, DDPMSchedulerRef(), init, noise, N, J, tau, ratios=ratios)
    lat, traj, stats = _par(c, tolerance=tau, levels_per_batch=J, trajectory=True)
    ratios = np.array(ratios)
    nearest = float(ratios[np.argmin(np.abs(np.log(np.maximum(ratios, 1e-300))))])
    slots = [rel_l2(traj[k].cpu().numpy(), want_traj[k]) for k in range(N + 1)]
    err_gpu = max(slots + [rel_l2(lat.cpu().numpy(), want_lat)])
    mutants = {"carry": ref.sample_parallel(eps_fn, DDPMSchedulerRef(), init, noise, N, J, tau, drop_carry=True)}
    if fill_visible:
        mutants["fill"] = ref.sample_parallel(eps_fn, DDPMSchedulerRef(), init, noise, N, J, tau, fill_from_next_window=True)
    moved = {k: rel_l2(v[0], want_lat) for k, v in mutants.items()}
    print(f"\nparallel tau={tau} B={B} L={L} N={N} J={J}: strides {stats.strides} (restated {want_strides}), nearest err/bound ratio "
          f"{nearest:.3f}, err_gpu {err_gpu:.2e} (final {rel_l2(lat.cpu().numpy(), want_lat):.2e}), mutants moved "
          + ", ".join(f"{k} {v:.2e} strides {mutants[k][2]}" for k, v in moved.items()))
    assert stats.levels_per_batch == J and stats.chunks_evaluated == 6
    assert not ((ratios >= GUARD_BAND[0]) & (ratios <= GUARD_BAND[1])).any(), sorted(ratios, key=lambda q: abs(np.log(max(q, 1e-300))))[:4]
    assert stats.strides == want_strides
    assert max(want_strides) > 1 and torch.equal(traj[0], lat) and torch.equal(traj[N], c["init"])
    assert err_gpu <= ERR_GPU_GATE, (err_gpu, slots)
    for k, v in moved.items():
        assert v > 10 * err_gpu, (k, v, err_gpu)
    assert mutants["carry"][2] != stats.strides
    if L in (20, 4):
        lat2, stats2 = _par(c, tolerance=tau, levels_per_batch=J)
        assert torch.equal(lat2, lat) and stats2.strides == stats.strides


def _raw(c):
    """The handle, the cfd_sample_args of the DDPM run (from a run opened and closed) and a fresh cfd_parallel_args."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched(), c["mems"], c["masks"], c["B"], c["L"], c["N"], init_latents=c["init"],
                      step_noise=c["noise"], skip_zero_weight_chunks=True)
    a = run._args
    run.close()
    out = torch.empty_like(c["init"])
    pa = _lib.ParallelArgs()
    pa.latents, pa.levels_per_batch = out.data_ptr(), 5
    return run, a, pa, out


def test_refusals(small):
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun, sample_parallel
    from tests.gpu_helpers import hip_denoiser
    c = small
    m = hip_denoiser(1234, 1.0)
    with pytest.raises(TypeError):
        sample_parallel(m, _sched("ddim"), c["mems"], c["masks"], B=c["B"], L=c["L"], num_inference_steps=c["N"])
    with pytest.raises(ValueError):       # the conditioning batch is 7 chunks of B rows
        sample_parallel(m, _sched(), c["mems"], c["masks"], B=c["B"] + 1, L=c["L"], num_inference_steps=c["N"])
    run, a, pa, out = _raw(c)
    lib, h = _lib.load(), run.handle
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(code=-1):
        with pytest.raises(_lib.CfdError) as e:
            _lib.check(lib.cfd_sample_parallel(h, C.byref(a), C.byref(pa), None, st))
        assert e.value.code == code, e.value
        return str(e.value)

    torch.cuda.synchronize()
    _lib.check(lib.cfd_sample_parallel(h, C.byref(a), C.byref(pa), None, st))      # (the arguments are good: stats may be NULL)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    a.scheduler = 1
    assert "scheduler 0" in refused()
    a.scheduler = 0
    a.preseq, a.preseq_len = c["init"].data_ptr(), 2
    assert "preseq" in refused()
    a.preseq, a.preseq_len = None, 0
    a.dynamic_memory_mask = 1
    assert "dynamic" in refused()
    a.dynamic_memory_mask = 0
    ring = torch.empty(16, device=out.device)
    a.att_ring = (C.c_void_p * _lib.NUM_MEM)(*[ring.data_ptr()] * _lib.NUM_MEM)
    assert "att_ring" in refused()
    a.att_ring = (C.c_void_p * _lib.NUM_MEM)()
    for tol in (-0.5, float("nan"), float("inf")):
        pa.tolerance = tol
        assert "tolerance" in refused()
    pa.tolerance = 0.0
    pa.levels_per_batch = -1
    assert "levels_per_batch" in refused()
    pa.levels_per_batch = 5
    pa.latents = None
    assert "NULL" in refused()
    pa.latents = out.data_ptr()
    wt = np.zeros((c["N"], c["B"], 8), np.float32)
    wt[3, 1, 2] = np.inf
    pa.weights = wt.ctypes.data_as(C.c_void_p)
    refused()
    pa.weights = None
    with SamplingRun(m, _sched(), c["mems"], c["masks"], c["B"], c["L"], c["N"]) as open_run:      # a run is open on the handle
        assert open_run.handle.value == h.value
        assert "open" in refused(-3)
    torch.cuda.synchronize()
    _lib.check(lib.cfd_sample_parallel(h, C.byref(a), C.byref(pa), None, st))      # ... and none of it left anything behind
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


def test_inversion_around_a_parallel_call_keeps_its_bits(small):
    """cfd_ddpm_invert before and after a cfd_sample_parallel on the same handle (other J, other guidance): the shared level-batch set-up
    leaves no state behind -- the same trajectory and noise, bit for bit; and the parallel call between two inversions likewise."""
    import torch
    from convofusion_amd.sampler import invert_ddpm
    from tests.gpu_helpers import hip_denoiser
    c = small
    m = hip_denoiser(1234, 1.0)
    src = 0.8 * c["init"]
    inv = lambda: invert_ddpm(m, _sched(), c["mems"], c["masks"], source_latents=src, num_inference_steps=c["N"], seed=5, levels_per_batch=6)
    t0, z0 = inv()
    p0, s0 = _par(c, tolerance=0.1, levels_per_batch=4)
    t1, z1 = inv()
    p1, s1 = _par(c, tolerance=0.1, levels_per_batch=4)
    assert torch.equal(t0, t1) and torch.equal(z0, z1)
    assert torch.equal(p0, p1) and s0.strides == s1.strides
    assert bool(torch.isfinite(z1).all()) and not bool(z1[c["N"] - 1].any())
