"""-m gpu: tied tokens in the captured loop (cfd_sample_begin_tied, ``SamplingRun(tie=)``) and long-form synthesis on top of them
(``convofusion_amd.longform``).

The tied loop against trajectories made with the REFERENCE denoiser and the restated tied loop (tests/golden/traj_longform_*.npz,
make_golden_longform.py), the exactness of the copy, the all -1 table against the run without one (bit for bit), causality, grouping with a
carry against ``sample`` calls by hand, composition with weight tables, pruning and the attention ring, ``synthesize_motion`` on seeded
weights, and the ABI's refusals (host-side argument checks: nothing here provokes a fault).  Errors are printed."""
import ctypes as C

import numpy as np
import pytest

from oracle import inputs, philox_ref, vae_weights
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-3          # the project's trajectory budget, as tests/test_gpu_edit.py
DPM_KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SMALL = ((6, 20, 6, 8, 1), (2, 0, 1, 0, 0))


def _sched(kind):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    if kind == "dpmpp":
        return scheduler.DPMSolverMultistepScheduler(**DPM_KW)
    return scheduler.DDIMScheduler(**SCHED_KW) if kind == "ddim" else scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)


def _inputs(B, seed, L=16, S=SMALL[0], pad=SMALL[1]):
    from tests.gpu_helpers import to_dev
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    return [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}


def _rows(mems, masks, a, b, B):
    from convofusion_amd.distributed import shard_cfg_batch
    return [shard_cfg_batch(x, a, b, B) for x in mems], {k: shard_cfg_batch(v, a, b, B) for k, v in masks.items()}


def _ties(U, W, L=16):
    from convofusion_amd.longform import window_ties
    return window_ties(U, W, L).cuda()


def _assert_tied(lat, tie):
    import torch
    L = lat.shape[1]
    flat = lat.reshape(-1, 128)
    idx = torch.nonzero(tie.reshape(-1) >= 0).reshape(-1)
    assert idx.numel() > 0
    assert torch.equal(flat[idx], flat[tie.reshape(-1)[idx].long()]), "a tied token differs from its source"
    return L


@pytest.mark.parametrize("operands", [None, 0])
@pytest.mark.parametrize("name", ["ddpm20", "dpmpp10"])
def test_tied_loop_matches_reference_trajectory(name, operands):
    """2 utterances x 3 windows as 6 rows of one tied run, memories different per row, against the restated tied loop on the reference
    denoiser: every snapshot (the latents as stepped) and the final latents (after the final copy) within TRAJ_TOL relative L2."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g = load_golden("traj_longform_" + name)
    meta = [int(x) for x in g["meta"]]
    U, W, L, S, pad, n, seed = meta[0], meta[1], meta[2], tuple(meta[3:8]), tuple(meta[8:13]), meta[13], meta[14]
    B = U * W
    mems, masks = _inputs(B, seed, L, S, pad)
    kind = "dpmpp" if "dpmpp" in name else "ddpm"
    init = to_dev(philox_ref.normal_tensor(seed, 0, range(B), 1, L))
    noise = None if kind == "dpmpp" else to_dev(np.stack([philox_ref.normal_tensor(seed, i, range(B), 0, L) for i in range(n)]))
    tie = torch.from_numpy(g["tie"]).cuda()
    assert torch.equal(tie, _ties(U, W, L))
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched(kind), mems, masks, B, L, n, guidance_scale=7.5, init_latents=init, step_noise=noise,
                      operands=operands, tie=tie)
    errs = {}
    for k in sorted(int(f[4:]) for f in g.files if f.startswith("step")):
        run.steps(k - run.position)
        errs[k] = rel_l2(run.read().cpu().numpy(), g[f"step{k}"])
    run.steps(run.N - run.position)
    lat = run.read(close=True)
    errs["final"] = rel_l2(lat.cpu().numpy(), g["latents"])
    print("longform", name, "operands", operands, {k: f"{v:.2e}" for k, v in errs.items()})
    _assert_tied(lat, tie)
    assert torch.isfinite(lat).all() and all(v < TRAJ_TOL for v in errs.values()), errs


@pytest.mark.parametrize("operands", [None, 0])
def test_grouped_runs_with_carry_match_reference_trajectory(operands):
    """1 utterance x 4 windows in two runs of 2 (DDIM-10): a tie inside each run, the second run's first window keeping its first half
    from the first run's finished last window.  Each run's snapshots and final latents against the golden within TRAJ_TOL, the second run
    fed with the GOLDEN's carry (so that its error is its own); then ``synthesize_latents(max_rows=2)`` end to end against all 4 rows."""
    import torch
    from convofusion_amd.longform import synthesize_latents
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    g = load_golden("traj_longform_carry_ddim10")
    meta = [int(x) for x in g["meta"]]
    U, W, L, S, pad, n, seed = meta[0], meta[1], meta[2], tuple(meta[3:8]), tuple(meta[8:13]), meta[13], meta[14]
    B = U * W
    mems, masks = _inputs(B, seed, L, S, pad)
    m = hip_denoiser(1234, 1.0)
    errs = {}
    for grp, (a, b) in enumerate([(0, 2), (2, 4)]):
        enc, mk = _rows(mems, masks, a, b, B)
        keep = torch.from_numpy(g[f"keep{grp}"]).bool().cuda()
        kw = dict(source_latents=to_dev(g[f"source{grp}"]), keep_mask=keep) if bool(keep.any()) else {}
        run = SamplingRun(m, _sched("ddim"), enc, mk, b - a, L, n, guidance_scale=7.5, seed=seed, first_utterance=a, operands=operands,
                          tie=torch.from_numpy(g[f"tie{grp}"]).cuda(), **kw)
        for k in (1, 3, 5):
            run.steps(k - run.position)
            errs[f"run{grp} step{k}"] = rel_l2(run.read().cpu().numpy(), g[f"step{k}_{grp}"])
        run.steps(run.N - run.position)
        lat = run.read(close=True)
        errs[f"run{grp} final"] = rel_l2(lat.cpu().numpy(), g[f"latents{grp}"])
        _assert_tied(lat, torch.from_numpy(g[f"tie{grp}"]).cuda())
    win, seq = synthesize_latents(m, _sched("ddim"), mems, masks, n_utterances=U, n_windows=W, L=L, num_inference_steps=n, guidance_scale=7.5,
                                  seed=seed, max_rows=int(g["max_rows"]), skip_zero_weight_chunks=False, operands=operands)
    errs["end to end"] = rel_l2(win.reshape(B, L, 128).cpu().numpy(), g["latents"])
    print("longform carry_ddim10 operands", operands, {k: f"{v:.2e}" for k, v in errs.items()})
    assert tuple(seq.shape) == (U, (W + 1) * L // 2, 128)
    assert all(v < TRAJ_TOL for v in errs.values()), errs


@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpmpp"])
def test_tied_tokens_are_bit_identical_to_their_sources(kind):
    """After the run read()[b, l] equals read()[b', l'] bit for bit for every tie; after run.inpaint() at an arbitrary position likewise
    (and nothing else moved); a read in between returns the latents as the scheduler left them."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    U, W, L, n, seed = 2, 3, 16, 10, 41
    B = U * W
    mems, masks = _inputs(B, seed)
    tie = _ties(U, W)
    tied = tie >= 0
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched(kind), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, tie=tie)
    for pos in (0, 3, 7):
        run.steps(pos - run.position)
        before = run.read()
        if pos > 0 and kind == "ddpm":        # as stepped: every token got its own step noise
            assert not torch.equal(before.reshape(-1, 128)[tied.reshape(-1)], before.reshape(-1, 128)[tie.reshape(-1)[tied.reshape(-1)].long()])
        run.inpaint()
        after = run.read()
        _assert_tied(after, tie)
        assert torch.equal(after[~tied], before[~tied]), pos
        run.steps(1)                           # (the captured iteration skips the copy it has had)
    run.steps(run.N - run.position)
    lat = run.read()
    _assert_tied(lat, tie)
    assert torch.equal(run.read(close=True), lat) and torch.isfinite(lat).all()
    with SamplingRun(hip_denoiser(1234, 1.0), _sched(kind), mems, masks, B, L, n, seed=seed, tie=tie) as again:
        with pytest.raises(ValueError):
            again.write(lat)                   # (no WEG update inside a tied run)


@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpmpp"])
def test_a_table_without_ties_is_bit_identical_to_no_table(kind):
    """tie all -1: the same run without tie, bit for bit -- plain and with a keep mask (the tied instance's kept tokens are the edit
    instance's)."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    from tests.test_gpu_edit import _keep, _source
    m = hip_denoiser(1234, 1.0)
    B, L, n, seed = 3, 16, 10, 6
    mems, masks = _inputs(B, seed)
    none = torch.full((B, L), -1, dtype=torch.int32, device="cuda")
    kw = dict(B=B, L=L, num_inference_steps=n, seed=seed, skip_zero_weight_chunks=True)
    plain = sample(m, _sched(kind), mems, masks, **kw)
    assert torch.isfinite(plain).all() and torch.equal(sample(m, _sched(kind), mems, masks, tie=none, **kw), plain)
    ekw = dict(kw, source_latents=_source(B, seed), keep_mask=_keep(B, seed))
    edit = sample(m, _sched(kind), mems, masks, **ekw)
    assert not torch.equal(edit, plain) and torch.equal(sample(m, _sched(kind), mems, masks, tie=none, **ekw), edit)


def test_ties_are_causal():
    """Window 0 of each utterance is a source only: bit-identical to the same rows' run without ties, and within 1e-5 of its own one-row
    run (the tolerance of test_per_utterance_masks_match_one_utterance_runs); the windows w > 0 differ from their untied run by more than
    1e-3."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    U, W, L, n, seed = 2, 3, 16, 20, 23
    B = U * W
    mems, masks = _inputs(B, seed)
    kw = dict(B=B, L=L, num_inference_steps=n, seed=seed)
    tied = sample(m, _sched("ddpm"), mems, masks, tie=_ties(U, W), **kw)
    free = sample(m, _sched("ddpm"), mems, masks, **kw)
    for u in range(U):
        r = u * W
        assert torch.equal(tied[r], free[r])
        enc, mk = _rows(mems, masks, r, r + 1, B)
        one = sample(m, _sched("ddpm"), enc, mk, B=1, L=L, num_inference_steps=n, seed=seed, first_utterance=r)
        e = float((one[0] - tied[r]).norm() / tied[r].norm())
        d = [float((tied[r + w] - free[r + w]).norm() / free[r + w].norm()) for w in range(1, W)]
        print(f"utterance {u}: window 0 vs its one-row run {e:.2e}; windows 1.. vs untied {d}")
        assert e < 1e-5 and all(x > 1e-3 for x in d)


def test_groups_of_one_window_are_sample_calls_by_hand():
    """max_rows = 1 with a carry: every window its own run, its first half kept from the window before (window 0: from `carry`) -- the
    hand-written loop of sample(..., source_latents=, keep_mask=) calls, bit for bit; and max_rows = 2 equals its steps by hand too."""
    import torch
    from convofusion_amd.longform import stitch_tokens, synthesize_latents
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    U, W, L, n, seed = 1, 4, 16, 10, 77
    B, H = U * W, 8
    mems, masks = _inputs(B, seed)
    carry = (0.5 * torch.randn((U, H, 128), generator=torch.Generator().manual_seed(1))).cuda()
    kw = dict(L=L, num_inference_steps=n, guidance_scale=7.5, seed=seed, skip_zero_weight_chunks=True)
    keep = torch.zeros((1, L), dtype=torch.bool, device="cuda")
    keep[:, :H] = True

    def by_hand(a, b, prev, tie=None):
        enc, mk = _rows(mems, masks, a, b, B)
        src = torch.zeros((b - a, L, 128), device="cuda")
        src[0, :H] = prev
        km = torch.zeros((b - a, L), dtype=torch.bool, device="cuda")
        km[0, :H] = True
        return sample(m, _sched("ddpm"), enc, mk, B=b - a, first_utterance=a, source_latents=src, keep_mask=km, tie=tie, **kw)

    win, seq = synthesize_latents(m, _sched("ddpm"), mems, masks, n_utterances=U, n_windows=W, max_rows=1, carry=carry, **kw)
    prev, want = carry[0], []
    for w in range(W):
        want.append(by_hand(w, w + 1, prev)[0])
        prev = want[-1][H:]
    want = torch.stack(want)
    assert torch.isfinite(win).all() and torch.equal(win[0], want) and torch.equal(seq, stitch_tokens(win))
    win2, _ = synthesize_latents(m, _sched("ddpm"), mems, masks, n_utterances=U, n_windows=W, max_rows=2, carry=carry, **kw)
    pair = torch.full((2, L), -1, dtype=torch.int32, device="cuda")
    pair[1, :H] = torch.arange(H, 2 * H, dtype=torch.int32)
    first = by_hand(0, 2, carry[0], pair)
    second = by_hand(2, 4, first[1, H:], pair)
    assert torch.equal(win2[0], torch.cat([first, second]))
    assert torch.equal(win2[0, 1, :H], win2[0, 0, H:]) and not torch.equal(win2[0], win[0])       # the grouping is part of the meaning


def test_tied_run_composes_with_a_weight_table_pruning_and_the_ring():
    """An [N, B, 6] weight table whose apb / lsnid / all columns are 0: the pruned tied run (4 chunks) within 1e-6 of the unpruned one
    (7 chunks); return_attention="all" on a tied run: one finite entry per executed iteration, latents within 1e-6 of the run without."""
    import torch
    from convofusion_amd.sampler import SamplingRun, sample
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    U, W, L, n, seed = 1, 3, 16, 20, 31
    B = U * W
    mems, masks = _inputs(B, seed)
    tie = _ties(U, W)
    w = np.random.default_rng(7).uniform(0.0, 2.0, size=(n, B, 6))
    w[:, :, 3:] = 0.0
    outs = {}
    for prune in (True, False):
        with SamplingRun(m, _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, modality_weights=torch.from_numpy(w),
                         prune_zero_weight_chunks=prune, tie=tie) as run:
            assert run.chunks_evaluated == (4 if prune else 7)
            run.steps(run.N)
            outs[prune] = run.read(close=True)
    e = float((outs[True] - outs[False]).norm() / outs[False].norm())
    kw = dict(B=B, L=L, num_inference_steps=n, seed=seed, tie=tie)
    lat, atts = sample(m, _sched("ddpm"), mems, masks, return_attention="all", **kw)
    want = sample(m, _sched("ddpm"), mems, masks, **kw)
    r = float((lat - want).norm() / want.norm())
    d = float((outs[False] - want).norm() / want.norm())
    print(f"tied: pruned vs unpruned {e:.2e}; ring vs no ring {r:.2e}; weighted vs reference weights {d:.2e}")
    _assert_tied(outs[True], tie)
    _assert_tied(lat, tie)
    assert torch.isfinite(outs[True]).all() and e < 1e-6 and d > 1e-3
    assert sorted(atts, reverse=True) == list(range(950, -1, -50))      # DDPM-20's table: every executed iteration has its slot
    assert all(len(v) == 5 and all(tuple(a.shape[:2]) == (B, 9) and np.isfinite(a.cpu().numpy()).all() for a in v) for v in atts.values())
    assert r < 1e-6, r


def _vae():
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    from tests.test_vae_encode_host import ABL, KW
    v = ConvoFusionVae(ablation=ABL, **KW)
    v.load_state_dict({k: torch.from_numpy(a) for k, a in vae_weights.make_state_dict().items()}, strict=True)
    return v.cuda().eval()


def test_synthesize_motion_on_seeded_weights():
    """synthesize_motion = synthesize_latents -> one HIP decode of all windows -> the reference's frame stitching: [U, (W + 1) * 64, nfeats],
    finite; window 0's frames equal decode of row 0 alone within 1e-4 max abs (what tests/test_gpu_vae.py holds decode to); the whole output
    equals its steps by hand bit for bit."""
    import torch
    from types import SimpleNamespace
    from convofusion_amd.edit import loop_to_vae
    from convofusion_amd.longform import stitch_frames, synthesize_latents, synthesize_motion
    from tests.gpu_helpers import hip_denoiser
    U, W, n, seed = 2, 3, 10, 17
    B = U * W
    mems, masks = _inputs(B, seed)
    model = SimpleNamespace(vae=_vae(), denoiser=hip_denoiser(1234, 1.0), scheduler=_sched("ddpm"), guidance_scale=7.5, clf_guidance_drops=6,
                            do_classifier_free_guidance=True,
                            cfg=SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=n, eta=0.0))))
    out, win, seq = synthesize_motion(model, mems, masks, n_utterances=U, n_windows=W, seed=seed)
    nf = out.shape[-1]
    assert tuple(out.shape) == (U, (W + 1) * 64, nf) and nf == 189 and torch.isfinite(out).all()
    assert tuple(win.shape) == (U, W, 16, 128) and tuple(seq.shape) == (U, (W + 1) * 8, 128)
    for u in range(U):
        alone = model.vae.decode(loop_to_vae(win[u, :1]), [128])[0]
        err = float((out[u, :128] - alone).abs().max())
        print(f"utterance {u}: window 0 of the stitched motion vs decode of its row alone: max abs {err:.2e}")
        assert err < 1e-4
    want_win, want_seq = synthesize_latents(model.denoiser, _sched("ddpm"), mems, masks, n_utterances=U, n_windows=W, num_inference_steps=n,
                                            guidance_scale=7.5, seed=seed)
    feats = model.vae.decode(loop_to_vae(want_win.reshape(B, 16, 128)), [128] * B)
    assert torch.equal(win, want_win) and torch.equal(seq, want_seq) and torch.equal(out, stitch_frames(feats.reshape(U, W, 128, nf)))


def test_abi_refusals():
    """cfd_sample_begin_tied refuses (CFD_E_ARG, the message naming the token) an entry out of range, a self-tie, a chain, a kept source, a
    token both kept and tied, a NULL tie / table / edit source, a first iteration > 0, DDIM inversion, preseq and dynamic memories; a
    good call afterwards opens a run on the same handle."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser
    from tests.test_gpu_edit import _source
    B, L, n = 2, 16, 10
    mems, masks = _inputs(B, 4)
    src = _source(B, 4)
    run = SamplingRun(hip_denoiser(1234, 1.0), _sched("ddpm"), mems, masks, B, L, n, guidance_scale=7.5, seed=1)
    run.close()
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g_eval = C.c_int(-7)
    preseq = torch.zeros((B, 4, 128), device="cuda")

    def table(**entries):
        t = torch.full((B, L), -1, dtype=torch.int32)
        for k, v in entries.items():
            b, l = (int(x) for x in k[1:].split("_"))
            t[b, l] = v
        return t.cuda()

    def keep_at(*tokens):
        k = torch.zeros((B, L), dtype=torch.uint8)
        for t in tokens:
            k.view(-1)[t] = 1
        return k.cuda()

    def call(tie, keep=None, source=src, k0=0, edit=True, null_tie=False, **args):
        a = _lib.SampleArgs.from_buffer_copy(run._args)
        for k, v in args.items():
            setattr(a, k, v)
        e = _lib.EditArgs()
        e.source = source.data_ptr() if source is not None else None
        e.keep = keep.data_ptr() if keep is not None else None
        e.first_iteration = k0
        t = _lib.TieArgs()
        t.tie = tie.data_ptr() if tie is not None else None
        return lib.cfd_sample_begin_tied(run.handle, C.byref(a), C.byref(e) if edit else None, None if null_tie else C.byref(t), None, 1,
                                         C.byref(g_eval), stream)

    good = table(t1_0=8, t1_1=9)
    ts = (C.c_int32 * n)(*range(0, 1000, 100))
    cases = (("NULL tie", dict(tie=good, null_tie=True), "null"), ("NULL table", dict(tie=None), "NULL"),
             ("NULL source", dict(tie=good, source=None), "source"), ("k0 = 3", dict(tie=good, k0=3), "first_iteration"),
             ("out of range", dict(tie=table(t1_0=B * L)), "tie[1][0]"), ("below -1", dict(tie=table(t0_3=-2)), "tie[0][3]"),
             ("self-tie", dict(tie=table(t1_2=L + 2)), "tie[1][2]"), ("chain", dict(tie=table(t1_0=8, t0_8=3)), "itself tied"),
             ("source kept", dict(tie=good, keep=keep_at(8)), "tie[1][0]"), ("kept and tied", dict(tie=good, keep=keep_at(L)), "(1, 0)"),
             ("preseq", dict(tie=good, preseq=preseq.data_ptr(), preseq_len=4), "preseq"),
             ("dynamic memories", dict(tie=good, dynamic_memory_mask=1), "dynamic"),
             ("inversion", dict(tie=good, edit=False, scheduler=3, clip_sample=0, timesteps=C.cast(ts, C.c_void_p), num_timesteps=n),
              "inversion"))
    for what, kw, msg in cases:
        rc = call(**kw)
        err = lib.cfd_last_error().decode()
        print(what, "->", rc, err)
        assert rc == -1 and msg in err, what
        assert lib.cfd_sample_position(run.handle) == -1               # no run was opened
    assert call(good, keep=keep_at(0, 20)) == 0 and g_eval.value == 7
    out = torch.empty((B, L, 128), device="cuda")
    assert lib.cfd_sample_steps(run.handle, n) == 0
    assert lib.cfd_sample_read(run.handle, C.c_void_p(out.data_ptr()), 1) == 0
    assert torch.isfinite(out).all() and torch.equal(out[1, :2], out[0, 8:10])
    assert call(good, edit=False) == 0                                  # no edit: no kept token, no source needed
    assert lib.cfd_sample_steps(run.handle, 2) == 0 and lib.cfd_sample_read(run.handle, C.c_void_p(out.data_ptr()), 1) == 0
