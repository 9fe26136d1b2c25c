"""The pure half of opening a sampling run (``convofusion_amd.sampler.SamplingRun``): the argument checks of every run kind and
``resolve_run_kind``, which turns the constructor's arguments into one ``RunKind`` record or the refusal that applies.  No library and no
device is needed: tensors are moved to ``device`` only where one is given.  Every name here is also importable from the sampler module."""
import typing

import torch


def edit_first_iteration(strength, N):
    """The first iteration k0 of an edit run over a table of N iterations at img2img ``strength`` -- diffusers' img2img convention
    (``get_timesteps``): k = min(int(N * strength), N) iterations are executed, k0 = N - k.  strength outside (0, 1], or one that executes
    no iteration (k == 0), raises ValueError."""
    try:
        st = float(strength)
    except (TypeError, ValueError):
        raise ValueError(f"strength must be a number in (0, 1], not {strength!r}") from None
    if not 0.0 < st <= 1.0:
        raise ValueError(f"strength = {strength!r} is not in (0, 1]")
    k = min(int(N * st), N)
    if k == 0:
        raise ValueError(f"strength = {strength!r} executes no iteration of the {N}-iteration schedule (int({N} * strength) = 0)")
    return N - k


def _check_keep_mask(keep_mask, B, L, device):
    """The keep mask of an edit or an anchored run as uint8 [B, L] on ``device`` (None stays None); ValueError for anything but a bool or
    integer [B, L] tensor of 0 / 1."""
    if keep_mask is None:
        return None
    if not isinstance(keep_mask, torch.Tensor) or keep_mask.is_floating_point() or keep_mask.is_complex():
        raise ValueError("keep_mask must be a bool or integer (0 / 1) tensor [B, L]")
    if tuple(keep_mask.shape) != (B, L):
        raise ValueError(f"keep_mask must be [B, L] = [{B}, {L}], not {list(keep_mask.shape)}")
    if keep_mask.dtype != torch.bool and bool(((keep_mask != 0) & (keep_mask != 1)).any()):
        raise ValueError("keep_mask holds values other than 0 and 1")
    return keep_mask.detach().to(device=device, dtype=torch.uint8).contiguous()


def check_edit(source_latents, keep_mask, strength, B, L, N, preseq=None, device=None):
    """The edit arguments of a run (``SamplingRun``): None when the run is no edit (no source, strength 1), else (source float32 [B, L, 128]
    contiguous on ``device``, keep mask uint8 [B, L] on ``device`` or None, k0).  Refusals (ValueError): keep_mask or strength < 1 without
    source_latents, preseq together with an edit, a source other than a floating-point [B, L, 128] tensor, a keep mask other than a bool or
    integer [B, L] tensor of 0 / 1, strength outside (0, 1] or executing no iteration (``edit_first_iteration``)."""
    k0 = edit_first_iteration(strength, N)
    if source_latents is None:
        if keep_mask is not None:
            raise ValueError("keep_mask needs source_latents: the kept tokens are re-noised from them")
        if k0 != 0:
            raise ValueError(f"strength = {strength!r} < 1 needs source_latents: the run starts part-way down the schedule from them")
        return None
    if preseq is not None:
        raise ValueError("preseq (the rollout's prefix in-painting) and an edit (source_latents) do not go together: give the prefix as a "
                         "keep_mask over its tokens instead")
    if not isinstance(source_latents, torch.Tensor) or not source_latents.is_floating_point():
        raise ValueError("source_latents must be a floating-point tensor [B, L, 128]")
    if tuple(source_latents.shape) != (B, L, 128):
        raise ValueError(f"source_latents must be [B, L, 128] = [{B}, {L}, 128], not {list(source_latents.shape)}")
    src = source_latents.detach().to(device=device, dtype=torch.float32).contiguous()
    return src, _check_keep_mask(keep_mask, B, L, device), k0


def check_inversion(scheduler, table, eta=0.0):
    """The arguments of a DDIM inversion run (scheduler kind 3, ``DDIMInverseScheduler``): the timestep table strictly increasing in
    [0, T), eta 0 and no clipping (the step is deterministic; a clipped x0 is not invertible).  Anything else raises ValueError."""
    import numpy as np
    T = int(scheduler.config.num_train_timesteps)
    ts = np.asarray(table, dtype=np.int64).reshape(-1)
    if ts.size < 1 or (ts.size > 1 and not bool((np.diff(ts) > 0).all())) or int(ts.min()) < 0 or int(ts.max()) >= T:
        raise ValueError(f"DDIM inversion needs a strictly increasing timestep table in [0, {T}), not {ts.tolist()[:8]}...")
    if float(eta) != 0.0:
        raise ValueError(f"DDIM inversion is deterministic: eta must be 0, not {eta!r}")
    if scheduler.config.get("clip_sample", False):
        raise ValueError("DDIM inversion runs without clip_sample (a clipped x0 is not invertible)")


def check_anchor(trajectory, keep_mask, B, L, N, device=None):
    """The anchor of a re-conditioning run (``SamplingRun(anchor_trajectory=)``): (trajectory float32 [N + 1, B, L, 128] contiguous on
    ``device``, keep mask uint8 [B, L] on ``device`` or None).  Refusals (ValueError): a trajectory other than a floating-point
    [N + 1, B, L, 128] tensor (N = the run's iterations: the inversion must have as many), a keep mask other than a bool or integer [B, L]
    tensor of 0 / 1."""
    if not isinstance(trajectory, torch.Tensor) or not trajectory.is_floating_point():
        raise ValueError("anchor_trajectory must be a floating-point tensor [N + 1, B, L, 128]")
    if tuple(trajectory.shape) != (N + 1, B, L, 128):
        raise ValueError(f"anchor_trajectory must be [N + 1, B, L, 128] = [{N + 1}, {B}, {L}, 128] (an inversion with the run's N = {N} "
                         f"iterations, B and L), not {list(trajectory.shape)}")
    return trajectory.detach().to(device=device, dtype=torch.float32).contiguous(), _check_keep_mask(keep_mask, B, L, device)


def check_noise_space(noise_space, keep_mask, strength, B, L, N, device=None, *, scheduler_kind=0, preseq=None, source_latents=None,
                      anchor_trajectory=None, tie=None, dynamic_memories=()):
    """The noise space of a replay run (``SamplingRun(noise_space=)``, cfd_sample_begin_replay): (trajectory float32 [N + 1, B, L, 128] and
    noise float32 [N, B, L, 128] contiguous on ``device``, keep mask uint8 [B, L] or None, k0 = ``edit_first_iteration(strength, N)``).
    Refusals (ValueError), each before any device work: a scheduler other than DDPM, preseq, source_latents, anchor_trajectory, tie or
    dynamic memories next to it, a pair other than two floating-point tensors of those shapes (N = the run's iterations: the inversion must
    have as many), a keep mask other than a bool or integer [B, L] tensor of 0 / 1, a strength outside (0, 1]."""
    if scheduler_kind != 0:
        raise ValueError("noise_space: an edit-friendly DDPM noise space is replayed by a DDPMScheduler run")
    for name, v in (("preseq", preseq), ("source_latents", source_latents), ("anchor_trajectory", anchor_trajectory), ("tie", tie)):
        if v is not None:
            raise ValueError(f"noise_space and {name} do not go together (the replay's kept tokens and its start come from the trajectory)")
    if dynamic_memories:
        raise ValueError("noise_space: a replay takes no dynamic memories (a dyadic run)")
    try:
        trajectory, noise = noise_space
    except (TypeError, ValueError):
        raise ValueError("noise_space must be the pair (trajectory, noise) of invert_ddpm") from None
    for name, t, shape in (("trajectory", trajectory, (N + 1, B, L, 128)), ("noise", noise, (N, B, L, 128))):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"noise_space: {name} must be a floating-point tensor {list(shape)}")
        if tuple(t.shape) != shape:
            raise ValueError(f"noise_space: {name} must be {list(shape)} (an inversion with the run's N = {N} iterations, B and L), not "
                             f"{list(t.shape)}")
    k0 = edit_first_iteration(strength, N)
    return (trajectory.detach().to(device=device, dtype=torch.float32).contiguous(),
            noise.detach().to(device=device, dtype=torch.float32).contiguous(), _check_keep_mask(keep_mask, B, L, device), k0)


def check_tie(tie, keep_mask, B, L, device=None, *, preseq=None, strength=1.0, scheduler_kind=None, anchored=False, dynamic_memories=()):
    """The tie table of a tied run (``SamplingRun(tie=)``, cfd_sample_begin_tied): None when the run has none, else the table as int32
    [B, L] contiguous on ``device``.  Entry [b, l] is -1 (a free token) or the flat index b' * L + l' of the token whose value token (b, l)
    takes at the start of every iteration and once more after the last.  Refusals (ValueError), each before any device work and each
    naming the first offending (b, l): a table other than an integer [B, L] tensor, an entry outside [-1, B * L), a token tied to itself, a
    source that is itself tied (no chains, so no cycles), a source that ``keep_mask`` keeps, a token both kept and tied; and the runs that
    take no ties: preseq, strength < 1, DDIM inversion (scheduler kind 3), an anchored run, dynamic memories (dyadic runs)."""
    if tie is None:
        return None
    if scheduler_kind == 3:
        raise ValueError("tie: a DDIM inversion run (DDIMInverseScheduler) takes no tied tokens")
    if anchored:
        raise ValueError("tie: an anchored run (anchor_trajectory) takes no tied tokens")
    if preseq is not None:
        raise ValueError("tie: preseq (the rollout's prefix in-painting) and tied tokens do not go together: give the prefix as kept "
                         "tokens (source_latents / keep_mask)")
    if float(strength) != 1.0:
        raise ValueError(f"tie: a tied run starts at iteration 0 (strength = {strength!r} is not 1)")
    if dynamic_memories:
        raise ValueError("tie: a run with dynamic memories (a dyadic run) takes no tied tokens")
    if not isinstance(tie, torch.Tensor) or tie.is_floating_point() or tie.is_complex() or tie.dtype == torch.bool:
        raise ValueError("tie must be an integer tensor [B, L] (-1, or the flat index b' * L + l' of the source token)")
    if tuple(tie.shape) != (B, L):
        raise ValueError(f"tie must be [B, L] = [{B}, {L}], not {list(tie.shape)}")
    t = tie.detach().to("cpu", torch.int64).reshape(-1)
    keep = None
    if keep_mask is not None:
        if not isinstance(keep_mask, torch.Tensor) or tuple(keep_mask.shape) != (B, L):
            raise ValueError(f"keep_mask must be a tensor [B, L] = [{B}, {L}]")
        keep = (keep_mask.detach().to("cpu") != 0).reshape(-1)
    n = B * L
    for e in torch.nonzero(t != -1).reshape(-1).tolist():
        v, b, l = int(t[e]), e // L, e % L
        if v < -1 or v >= n:
            raise ValueError(f"tie[{b}][{l}] = {v} is not -1 or a token in [0, {n})")
        if v == e:
            raise ValueError(f"tie[{b}][{l}] = {v} ties the token to itself")
        if int(t[v]) != -1:
            raise ValueError(f"tie[{b}][{l}] = {v} names a source ({v // L}, {v % L}) that is itself tied (no chains)")
        if keep is not None and bool(keep[v]):
            raise ValueError(f"tie[{b}][{l}] = {v} names a source ({v // L}, {v % L}) that keep_mask keeps (a source must be free)")
        if keep is not None and bool(keep[e]):
            raise ValueError(f"token ({b}, {l}) is both kept (keep_mask) and tied")
    return tie.detach().to(device=device, dtype=torch.int32).contiguous()


def sample_prediction(scheduler):
    """Whether the scheduler's denoiser predicts the clean latent (``prediction_type="sample"``) rather than the noise."""
    return (getattr(scheduler, "config", None) or {}).get("prediction_type", "epsilon") == "sample"


def refuse_sample_prediction(scheduler, what):
    """NotImplementedError when ``scheduler`` has ``prediction_type="sample"``: ``what`` (the start of the message) is built and checked for
    epsilon-predicting models only -- there is no trajectory of an x0-predicting model to check it against."""
    if sample_prediction(scheduler):
        raise NotImplementedError(f"{what} with prediction_type='epsilon' only: with prediction_type='sample' it has no reference "
                                  "trajectory to be checked against")


def _check_guided_loop(scheduler, name, loop, noise_space, anchor_trajectory, trajectory):
    """The refusals the two guided loops share (``check_loss_guidance``, ``check_keyframe_guidance``): every one but the tied run's.
    ``name``: the loop's function; ``loop``: the phrase that names it in a sentence."""
    what = f"{name}: {loop} runs"
    kind = getattr(scheduler, "KIND", None)
    if kind == 3 or trajectory:
        raise NotImplementedError(f"{name}: a DDIM inversion (DDIMInverseScheduler) takes no loss guidance -- its latents "
                                  "are its own; use invert() or sample()")
    if kind == 2:
        raise NotImplementedError(f"{what} with DDPMScheduler / DDIMScheduler; with DPMSolverMultistepScheduler it has no reference "
                                  "trajectory to be checked against -- use sample()")
    refuse_sample_prediction(scheduler, what)
    if noise_space is not None:
        raise NotImplementedError(f"{name}: the replay of a noise space (noise_space) takes no loss guidance")
    if anchor_trajectory is not None:
        raise NotImplementedError(f"{name}: an anchored run (anchor_trajectory) takes no loss guidance: its kept tokens "
                                  "come from the trajectory")


def check_loss_guidance(scheduler, *, noise_space=None, anchor_trajectory=None, tie=None, trajectory=False):
    """The runs ``sampler.sample_with_loss_guidance`` takes: DDPMScheduler / DDIMScheduler with epsilon prediction, plain, weighted, edit
    and preseq runs.  NotImplementedError, before any device work, for DPM-Solver++ (its multistep history would carry the moved latents
    of one iteration into the next with nothing to check it against), prediction_type="sample", a DDIM inversion, the replay of a noise
    space, an anchored and a tied run (their latents are overwritten from recorded levels or from each other every iteration)."""
    _check_guided_loop(scheduler, "sample_with_loss_guidance", "the loss-guided loop (loss_fn)", noise_space, anchor_trajectory, trajectory)
    if tie is not None:
        raise NotImplementedError("sample_with_loss_guidance: a tied run (tie) takes no loss guidance (write): its tied tokens are "
                                  "overwritten from their sources every iteration -- key poses on a tied run: sample_with_keyframes, "
                                  "which folds their gradients onto the sources")


def check_keyframe_guidance(scheduler, *, noise_space=None, anchor_trajectory=None, tie=None, trajectory=False):
    """The runs ``sampler.sample_with_keyframes`` takes: those of ``check_loss_guidance`` and the tied run (``tie`` is accepted and not
    looked at: ``check_tie`` has the table's own refusals) -- the device call folds a tied token's gradient onto its source and leaves
    the latents satisfying the tie.  The refusals, NotImplementedError before any device work, are ``check_loss_guidance``'s others."""
    _check_guided_loop(scheduler, "sample_with_keyframes", "the key-pose guided loop", noise_space, anchor_trajectory, trajectory)


def check_weg_rows(per_row, tie, B, L, S):
    """What ``sampler.sample_with_weg`` asks of ``per_row`` and ``tie``, before any device work.  ``tie`` without ``per_row=True`` is
    refused (ValueError naming the keyword): the reference's loop has one loss for the batch and nothing that folds a tied token's
    gradient onto its source.  With ``per_row=True`` the B rows of L tokens against memory lengths ``S`` must fit the row-tile gradient
    engine (``weg.step_refusal``), NotImplementedError otherwise; the table itself is ``check_tie``'s to refuse when the run opens."""
    if not per_row:
        if tie is not None:
            raise ValueError("sample_with_weg: tie= needs per_row=True -- the batch-of-one loop (per_row=False) writes its update over the "
                             "tied tokens; the per-row loop folds their gradients onto their sources")
        return
    from .weg import step_refusal
    why = step_refusal(B, L, S)
    if why is not None:
        raise NotImplementedError(f"sample_with_weg(per_row=True): per-row word-excitation guidance runs on the row-tile gradient engine "
                                  f"only: {why}")


_AUTO_RUN = object()   # the first attempt of an "auto" loop (``_with_auto_operands``): a guarded run, not another "auto" loop


def check_pose_keyframes(who, target, frame_mask, feature_mask=None, lengths=None):
    """What ``edit.pose_keyframe_loss`` and ``sampler.sample_with_pose_keyframes`` (``who``) ask of key poses in pose space: ``target``
    [B, F, nfeats], ``frame_mask`` [B, F], ``feature_mask`` [nfeats] or None (all), ``lengths`` B values in [1, F] whose largest is F
    (None: F each), and at least one selected frame and feature.  Returns (B, F, nfeats, the frame mask as bool [B, F], the feature mask
    as bool [nfeats] on the CPU, the lengths as a list, selected frames * selected features)."""
    if not isinstance(target, torch.Tensor) or target.dim() != 3:
        raise ValueError(f"{who}: target must be [B, F, nfeats], got {tuple(getattr(target, 'shape', ()))}")
    B, F, nf = (int(v) for v in target.shape)
    fm = (frame_mask != 0)
    if tuple(fm.shape) != (B, F):
        raise ValueError(f"{who}: frame_mask must be [B, F] = [{B}, {F}] like target, got {tuple(fm.shape)}")
    cm = torch.ones(nf, dtype=torch.bool) if feature_mask is None else (feature_mask != 0)
    if tuple(cm.shape) != (nf,):
        raise ValueError(f"{who}: feature_mask must be [{nf}], got {tuple(cm.shape)}")
    lens = [F] * B if lengths is None else [int(v) for v in (lengths.reshape(-1).tolist() if torch.is_tensor(lengths) else lengths)]
    if len(lens) != B or min(lens) < 1 or max(lens) != F:
        raise ValueError(f"{who}: lengths must be {B} values in [1, {F}] whose largest is {F}, got {lens}")
    n = int(fm.sum().item()) * int(cm.sum().item())
    if n == 0:
        raise ValueError(f"{who}: the masks select no frame or no feature")
    return B, F, nf, fm, cm, lens, n


def check_operands(operands):
    """None, an operand policy (int), or "auto"; anything else is refused."""
    if operands is None or operands is _AUTO_RUN or operands == "auto":
        return operands
    if isinstance(operands, (str, bytes, bool)):
        raise ValueError(f"operands must be None, an operand policy (int) or 'auto', not {operands!r}")
    try:
        return int(operands)
    except (TypeError, ValueError):
        raise ValueError(f"operands must be None, an operand policy (int) or 'auto', not {operands!r}") from None


class RunKind(typing.NamedTuple):
    """What ``resolve_run_kind`` makes of a run's arguments: the validated pieces of the kinds (None: the run is not of that kind)."""
    edit: typing.Optional[tuple]       # (source, keep mask or None, k0): ``check_edit``
    anchor: typing.Optional[tuple]     # (trajectory, keep mask or None): ``check_anchor``
    replay: typing.Optional[tuple]     # (trajectory, noise, keep mask or None, k0): ``check_noise_space``
    tie: typing.Optional[torch.Tensor]   # the tie table: ``check_tie``
    first_iteration: int               # k0 of an edit or a replay, else 0
    trajectory: bool                   # a DDIM inversion that records its trajectory
    operands: object                   # as given; a replay and a prediction_type="sample" run turn None / "auto" into 0


def resolve_run_kind(scheduler, table, eta=0.0, *, B, L, preseq=None, source_latents=None, keep_mask=None, strength=1.0, trajectory=False,
                     anchor_trajectory=None, tie=None, noise_space=None, init_latents=None, step_noise=None, dynamic_memories=(),
                     operands=None, device=None):
    """Which kind of run the arguments of ``SamplingRun`` describe, over the scheduler's full ``table``: every refusal between kinds and
    the leaf checks (``check_inversion`` / ``check_anchor`` / ``check_tie`` / ``check_noise_space`` / ``check_edit``), in the order
    prediction type, inversion, anchor, tie, replay, edit: where two refusals apply, the earlier one is raised.  A new kind adds its
    block here.  ``prediction_type="sample"`` (the scheduler's config) goes with the plain, weighted, edit, tied and preseq runs of DDPM,
    DDIM and DPM-Solver++; inversion, an anchored run, a replay and dynamic memories (dyadic runs) refuse it, and its default operand
    policy is 0 (None / "auto" become 0: the single-fp16 policy was adopted on epsilon trajectories)."""
    n_full, kind = len(table), scheduler.KIND
    if sample_prediction(scheduler):
        for what, given in (("a DDIM inversion run (DDIMInverseScheduler) runs", kind == 3),
                            ("an anchored run (anchor_trajectory) runs", anchor_trajectory is not None),
                            ("the replay of a noise space (noise_space) runs", noise_space is not None),
                            ("a run with dynamic memories (a dyadic run) runs", bool(dynamic_memories))):
            if given:
                refuse_sample_prediction(scheduler, what)
        if operands is None or operands is _AUTO_RUN or operands == "auto":
            operands = 0
    if kind == 3:
        check_inversion(scheduler, table, eta)
        if preseq is not None or source_latents is not None or anchor_trajectory is not None or dynamic_memories:
            raise ValueError("a DDIM inversion run takes no preseq, edit (source_latents / keep_mask / strength), anchor_trajectory or "
                             "dynamic memories: give the source as init_latents")
    elif trajectory:
        raise ValueError("trajectory=True records a DDIM inversion: it needs a DDIMInverseScheduler")
    anchor = None
    if anchor_trajectory is not None:
        if kind != 1 or float(eta) != 0.0 or scheduler.config.get("clip_sample", False):
            raise ValueError("an anchored run is a deterministic, unclipped DDIM run: DDIMScheduler(clip_sample=False) and eta = 0")
        if source_latents is not None or preseq is not None or float(strength) != 1.0:
            raise ValueError("an anchored run takes no source_latents, strength or preseq (its kept tokens come from the trajectory)")
        anchor = check_anchor(anchor_trajectory, keep_mask, B, L, n_full, device)
        keep_mask = None
    tie_table = check_tie(tie, keep_mask, B, L, device, preseq=preseq, strength=strength, scheduler_kind=kind,
                          anchored=anchor_trajectory is not None, dynamic_memories=dynamic_memories)
    replay = None
    if noise_space is not None:
        if init_latents is not None or step_noise is not None:
            raise ValueError("noise_space: the replay takes its initial latents and step noise from the noise space (no init_latents / "
                             "step_noise)")
        replay = check_noise_space(noise_space, keep_mask, strength, B, L, n_full, device, scheduler_kind=kind, preseq=preseq,
                                   source_latents=source_latents, anchor_trajectory=anchor_trajectory, tie=tie,
                                   dynamic_memories=dynamic_memories)
        keep_mask, strength = None, 1.0
        if operands is None or operands is _AUTO_RUN or operands == "auto":
            operands = 0
    edit = check_edit(source_latents, keep_mask, strength, B, L, n_full, preseq, device)
    k0 = edit[2] if edit is not None else (replay[3] if replay is not None else 0)
    return RunKind(edit, anchor, replay, tie_table, k0, bool(trajectory), operands)
