"""CPU: the stages ``SamplingRun.__init__`` is made of that need no device -- the kind of a run (``resolve_run_kind``: every refusal
between kinds with its full message, their precedence, the record of each accepted kind), the opener a kind maps to
(``select_opener``, on a stand-in for the library), the default guidance weights, the plain opener's evaluated chunks, the guidance
memories and the scheduler part of cfd_sample_args.  CPU tensors, ``device=None``: nothing here loads the library."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from convofusion_amd import _lib, sampler, scheduler
from convofusion_amd.sampler import (RunKind, default_guidance_weights, fill_scheduler_args, plain_chunks_evaluated, resolve_run_kind,
                                     select_memories, select_opener)
from oracle import inputs

YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
B, L, N = 2, 16, 10

INVERSION = ("a DDIM inversion run takes no preseq, edit (source_latents / keep_mask / strength), anchor_trajectory or dynamic memories: "
             "give the source as init_latents")
TRAJECTORY = "trajectory=True records a DDIM inversion: it needs a DDIMInverseScheduler"
ANCHOR_SCHEDULER = "an anchored run is a deterministic, unclipped DDIM run: DDIMScheduler(clip_sample=False) and eta = 0"
ANCHOR_ARGS = "an anchored run takes no source_latents, strength or preseq (its kept tokens come from the trajectory)"
REPLAY_NOISE = "noise_space: the replay takes its initial latents and step noise from the noise space (no init_latents / step_noise)"
OPENERS = ("cfd_sample_begin", "cfd_sample_begin_weighted", "cfd_sample_begin_edit", "cfd_sample_begin_invert", "cfd_sample_begin_anchored",
           "cfd_sample_begin_tied", "cfd_sample_begin_replay")


def _sched(kind, **kw):
    if kind == "ddpm":
        return scheduler.DDPMScheduler(**YAML, variance_type="fixed_small", clip_sample=True)
    if kind == "inverse":
        return scheduler.DDIMInverseScheduler(**YAML)
    return scheduler.DDIMScheduler(**YAML, **dict(dict(clip_sample=False), **kw))


SOURCE = torch.arange(B * L * 128, dtype=torch.float64).reshape(B, L, 128) / 1000.0
PRESEQ = torch.zeros((B, 4, 128))
RING = torch.zeros((N + 1, B, L, 128), dtype=torch.float64)
NOISE = torch.ones((N, B, L, 128))
KEEP = torch.zeros((B, L), dtype=torch.bool)
KEEP[0, :4] = KEEP[1, 12:] = True
TIE = torch.full((B, L), -1, dtype=torch.int64)
TIE[1, :8] = torch.arange(8, 16)          # row 1's first half copies row 0's second half


def _resolve(kind="ddpm", eta=0.0, sched_kw=None, **kw):
    sch = _sched(kind, **(sched_kw or {}))
    return resolve_run_kind(sch, sch.timestep_table(N)[1], eta, B=B, L=L, **kw)


REFUSALS = {
    "inverse + preseq": (INVERSION, dict(kind="inverse", preseq=PRESEQ)),
    "inverse + source_latents": (INVERSION, dict(kind="inverse", source_latents=SOURCE)),
    "inverse + anchor_trajectory": (INVERSION, dict(kind="inverse", anchor_trajectory=RING)),
    "inverse + dynamic_memories": (INVERSION, dict(kind="inverse", dynamic_memories=(0,))),
    "trajectory + ddpm": (TRAJECTORY, dict(kind="ddpm", trajectory=True)),
    "anchored + ddpm": (ANCHOR_SCHEDULER, dict(kind="ddpm", anchor_trajectory=RING)),
    "anchored + eta": (ANCHOR_SCHEDULER, dict(kind="ddim", eta=0.5, anchor_trajectory=RING)),
    "anchored + clip_sample": (ANCHOR_SCHEDULER, dict(kind="ddim", sched_kw=dict(clip_sample=True), anchor_trajectory=RING)),
    "anchored + source_latents": (ANCHOR_ARGS, dict(kind="ddim", anchor_trajectory=RING, source_latents=SOURCE)),
    "anchored + preseq": (ANCHOR_ARGS, dict(kind="ddim", anchor_trajectory=RING, preseq=PRESEQ)),
    "anchored + strength": (ANCHOR_ARGS, dict(kind="ddim", anchor_trajectory=RING, strength=0.5)),
    "replay + init_latents": (REPLAY_NOISE, dict(kind="ddpm", noise_space=(RING, NOISE), init_latents=SOURCE)),
    "replay + step_noise": (REPLAY_NOISE, dict(kind="ddpm", noise_space=(RING, NOISE), step_noise=NOISE)),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_between_kinds(case):
    """Every refusal ``SamplingRun.__init__`` itself raised before its stages were split out: a ValueError with the same full text."""
    msg, kw = REFUSALS[case]
    with pytest.raises(ValueError) as e:
        _resolve(**kw)
    assert type(e.value) is ValueError and str(e.value) == msg


def test_replay_operands():
    """A replay turns operands None / "auto" (and the first attempt of an "auto" loop) into 0 and leaves a policy alone; no other kind
    touches them."""
    for given, want in ((None, 0), ("auto", 0), (sampler._AUTO_RUN, 0), (15, 15), (0, 0)):
        assert _resolve(noise_space=(RING, NOISE), operands=given).operands == want
    for given in (None, "auto", 15):
        assert _resolve(operands=given).operands == given


def test_precedence_of_refusals():
    """Where two refusals apply the parent's order decides.  An inversion with preseq and trajectory=True: the scheduler's own checks
    (``check_inversion``: here eta) come before the inversion's refusal of preseq, and that one before ``check_tie``'s refusal of an
    inversion or of preseq; trajectory=True adds none with the inverse scheduler.  An anchored run with a tie: the anchored run's own
    refusals (here strength < 1) come before ``check_tie``, whose "an anchored run takes no tied tokens" is what a valid anchored run with
    a tie gets -- not its refusal of strength < 1."""
    with pytest.raises(ValueError, match="eta must be 0"):
        _resolve("inverse", eta=0.5, preseq=PRESEQ, trajectory=True)
    with pytest.raises(ValueError) as e:
        _resolve("inverse", preseq=PRESEQ, trajectory=True, tie=TIE)
    assert str(e.value) == INVERSION
    with pytest.raises(ValueError) as e:
        _resolve("ddim", anchor_trajectory=RING, tie=TIE, strength=0.5)
    assert str(e.value) == ANCHOR_ARGS
    with pytest.raises(ValueError) as e:
        _resolve("ddim", anchor_trajectory=RING, tie=TIE)
    assert str(e.value) == "tie: an anchored run (anchor_trajectory) takes no tied tokens"


def _kinds():
    """The accepted kinds: name -> (RunKind, trajectory ring or None, weighted)."""
    return {"plain": (_resolve(), None, False),
            "weighted": (_resolve(), None, True),
            "edit": (_resolve(source_latents=SOURCE, keep_mask=KEEP, strength=0.5), None, False),
            "tied": (_resolve(tie=TIE), None, False),
            "tied edit": (_resolve(tie=TIE, source_latents=SOURCE, keep_mask=KEEP), None, True),
            "inversion": (_resolve("inverse", init_latents=SOURCE, trajectory=True), torch.zeros((N + 1, B, L, 128)), True),
            "anchored": (_resolve("ddim", anchor_trajectory=RING, keep_mask=KEEP), None, False),
            "replay": (_resolve(noise_space=(RING, NOISE), keep_mask=KEEP, strength=0.5), None, True)}


def test_accepted_kinds():
    kinds = {k: v[0] for k, v in _kinds().items()}
    assert kinds["plain"] == RunKind(None, None, None, None, 0, False, None)
    k = kinds["edit"]
    assert k.first_iteration == N - int(N * 0.5) == k.edit[2] and (k.anchor, k.replay, k.tie, k.trajectory) == (None, None, None, False)
    assert k.edit[0].dtype == torch.float32 and torch.equal(k.edit[0], SOURCE.float()) and k.edit[0].is_contiguous()
    assert k.edit[1].dtype == torch.uint8 and torch.equal(k.edit[1].bool(), KEEP)
    k = kinds["tied"]
    assert k.tie.dtype == torch.int32 and torch.equal(k.tie.long(), TIE) and (k.edit, k.anchor, k.replay, k.first_iteration) == (None,) * 3 + (0,)
    k = kinds["tied edit"]
    assert torch.equal(k.tie.long(), TIE) and torch.equal(k.edit[1].bool(), KEEP) and k.edit[2] == 0 and k.first_iteration == 0
    k = kinds["inversion"]
    assert k.trajectory is True and (k.edit, k.anchor, k.replay, k.tie, k.first_iteration) == (None,) * 4 + (0,)
    assert _resolve("inverse", init_latents=SOURCE).trajectory is False
    k = kinds["anchored"]      # (the keep mask goes to the anchor: no edit is made of it)
    assert k.anchor[0].dtype == torch.float32 and tuple(k.anchor[0].shape) == (N + 1, B, L, 128) and torch.equal(k.anchor[1].bool(), KEEP)
    assert (k.edit, k.replay, k.tie, k.first_iteration) == (None, None, None, 0)
    assert _resolve("ddim", anchor_trajectory=RING).anchor[1] is None
    k = kinds["replay"]
    assert k.first_iteration == N - int(N * 0.5) == k.replay[3] and k.operands == 0 and (k.edit, k.anchor, k.tie) == (None, None, None)
    assert tuple(k.replay[0].shape) == (N + 1, B, L, 128) and torch.equal(k.replay[1], NOISE) and torch.equal(k.replay[2].bool(), KEEP)


def test_opener_of_every_kind():
    """The library function and the number of arguments between cfd_sample_args and the weight table that the parent's if-chain picked."""
    lib = SimpleNamespace(**{name: name for name in OPENERS})
    want = {"plain": ("cfd_sample_begin", 0), "weighted": ("cfd_sample_begin_weighted", 0), "edit": ("cfd_sample_begin_edit", 1),
            "tied": ("cfd_sample_begin_tied", 2), "tied edit": ("cfd_sample_begin_tied", 2), "inversion": ("cfd_sample_begin_invert", 1),
            "anchored": ("cfd_sample_begin_anchored", 1), "replay": ("cfd_sample_begin_replay", 1)}
    for name, (kind, ring, weighted) in _kinds().items():
        opener, extra, keep = select_opener(lib, kind, B, L, N, ring, weighted)
        assert (opener, len(extra)) == want[name], name
        structs = [k for k in keep if isinstance(k, C.Structure)]
        if name == "tied":
            assert extra[0] is None and [type(s) for s in structs] == [_lib.TieArgs] and structs[0].tie == kind.tie.data_ptr()
        if name == "tied edit":
            assert extra[0] is not None and {type(s) for s in structs} == {_lib.EditArgs, _lib.TieArgs}
        if name == "edit":
            assert (structs[0].source, structs[0].keep, structs[0].first_iteration) == (kind.edit[0].data_ptr(), kind.edit[1].data_ptr(), 5)
        if name == "replay":
            r = structs[0]
            assert (r.trajectory, r.noise, r.keep) == tuple(t.data_ptr() for t in kind.replay[:3])
            assert (r.steps, r.B, r.L, r.first_iteration) == (N, B, L, 5)
        if name == "anchored":
            an = structs[0]
            assert (an.trajectory, an.keep, an.steps, an.B, an.L) == (kind.anchor[0].data_ptr(), kind.anchor[1].data_ptr(), N, B, L)
        if name == "inversion":
            assert extra[0].value == ring.data_ptr()
        # the tensors the library reads in place stay alive with the run
        for piece in (kind.edit, kind.anchor, kind.replay):
            for t in piece or ():
                assert not isinstance(t, torch.Tensor) or any(t is k for k in keep), name
    # an inversion that records nothing is a plain or weighted run
    assert select_opener(lib, _resolve("inverse", init_latents=SOURCE), B, L, N, None, True)[:2] == ("cfd_sample_begin_weighted", ())


def test_default_guidance_weights():
    assert default_guidance_weights(7, 7.5) == [0.0, 7.5, 7.5, 7.5, 7.5, 7.5, 0.0, 0.0]
    assert default_guidance_weights(3, 2) == [0.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert default_guidance_weights(1, 7.5) == [0.0] * 8
    assert all(isinstance(v, float) for g in (7, 3, 1) for v in default_guidance_weights(g, 3))


def test_plain_opener_evaluated_chunks():
    """The trailing zero-weight chunks go with skip_zero_weight_chunks only; chunk 0 always stays."""
    w7, w3 = default_guidance_weights(7, 7.5), default_guidance_weights(3, 7.5)
    assert plain_chunks_evaluated(7, w7, True) == 6 and plain_chunks_evaluated(7, w7, False) == 7
    assert plain_chunks_evaluated(3, w3, True) == 3 and plain_chunks_evaluated(3, w3, False) == 3
    assert plain_chunks_evaluated(1, default_guidance_weights(1, 7.5), True) == 1
    assert plain_chunks_evaluated(7, default_guidance_weights(7, 0.0), True) == 1
    assert plain_chunks_evaluated(7, [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], True) == 4     # (a zero in the middle is evaluated)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return (a is None and b is None) or torch.equal(a, b)


def test_guidance_memories():
    """The three paths return what the constructor's inline block returned: the distinct memories with their maps as they are, the
    replicated batch de-duplicated (``dedup_memories``), or as it is without maps; and its two refusals."""
    cb = inputs.make_cfg_batch(seed=1, B=B, L=L, S=(6, 20, 6, 8, 1), pad_tail=(2, 0, 1, 0, 0))
    enc = [torch.from_numpy(m) for m in cb["memories"]]
    masks = {k: (torch.from_numpy(v) if v is not None else None) for k, v in cb["masks"].items()}
    maps = [torch.from_numpy(m) for m in cb["row_map"]]
    uniq = [torch.from_numpy(u) for u in cb["unique"]]
    got = select_memories(uniq, masks, 7, B, row_maps=maps)
    assert _same(got, (uniq, maps, masks)) and all(g is u for g, u in zip(got[0], uniq)) and got[2] is not masks
    got = select_memories(enc, masks, 7, B, dedup=True)
    assert _same(got, sampler.dedup_memories(enc, masks)) and [int(m.shape[0]) for m in got[0]] == [B + 1] * 5
    assert all(np.array_equal(g.numpy(), m) for g, m in zip(got[1], cb["row_map"]))
    got = select_memories(enc, masks, 7, B, dedup=False)
    assert _same(got, (enc, None, masks)) and got[1] is None
    assert _same(select_memories(enc, None, 7, B, dedup=False), (enc, None, {}))
    with pytest.raises(ValueError) as e:
        select_memories(uniq, masks, 7, B, row_maps=[m[:-1] for m in maps])
    assert str(e.value) == "row_maps must have G*B = 14 entries"
    with pytest.raises(ValueError) as e:
        select_memories([m[:7] for m in enc], masks, 7, B)
    assert str(e.value) == "conditioning batch is 7 rows, expected G*B = 14"


def test_scheduler_part_of_the_args():
    sch = scheduler.DDIMScheduler(**YAML, clip_sample=True, set_alpha_to_one=False, steps_offset=1)
    n, table = sch.timestep_table(N)
    a = _lib.SampleArgs()
    acp, ts = fill_scheduler_args(a, sch, n, table, 0.25)
    assert (a.scheduler, a.num_train_timesteps, a.num_inference_steps, a.clip_sample, a.eta) == (1, 1000, N, 1, 0.25)
    assert (a.set_alpha_to_one, a.steps_offset, a.num_timesteps) == (0, 1, N)
    assert a.alphas_cumprod == acp.data_ptr() and acp.dtype == torch.float32 and torch.equal(acp, sch.alphas_cumprod.float())
    assert a.timesteps == C.addressof(ts) and list(ts) == [int(t) for t in table]
    ddpm = _sched("ddpm")
    b = _lib.SampleArgs()
    fill_scheduler_args(b, ddpm, *ddpm.timestep_table(N))
    assert (b.scheduler, b.clip_sample, b.eta, b.set_alpha_to_one, b.steps_offset) == (0, 1, 0.0, 1, 0)
