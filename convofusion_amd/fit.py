"""Fitting CONDITIONING to data through the memory gradient of the HIP denoiser (``Denoiser.vjp_memories`` / ``cfd_denoise_vjp_mem``).

No weight of the DENOISER is trained.  ``fit_audio_encoder`` trains the one module whose output is a memory -- the audio encoder that
turns Mel frames into ``alsn`` -- by carrying that memory's gradient through the encoder's own backward pass
(``conditioning.audio_encoder_vjp`` / ``cfd_audio_encoder_vjp``): adapting the model to a microphone, a room, a voice.  Everywhere else
the network stays as loaded, and what is optimised is one or more of the five memories themselves -- textual
inversion applied to a memory.  The first use is a new listener identity: the reference's ``condition_fuser.lsn_id_emb`` is an
``nn.Embedding(36, 512)`` (condfuser.py:21,49), and a participant who is not one of its rows needs a new 512-vector fitted to a few of
their motions (``fit_identity``); the fitted row goes back into ``lsn_id_emb.weight``.

The objective is the reference's training loss with everything but the fitted memories held fixed (``_diffusion_process``,
convofusion.py:552-584): ``x_t = add_noise(latents, noise, t)``, one CONDITIONAL forward (no guidance batch), mean-squared error
against the noise (``prediction_type="epsilon"``) or the clean latents (``"sample"``).

One timestep is shared by all rows of a step.  The reference draws one timestep per row; the row-tile VJP takes one per call, so a step
here is the reference's step with the B draws tied together (the expectation of the loss over timesteps is the same, its variance per
step larger).  Fitting quality on a trained checkpoint is not measured by the project's tests: their weights are seeded.
"""
import torch

from .denoiser import MEM_NAMES, vjp_refusal


def denoising_loss_cotangent(out, target):
    """(mean-squared error of ``out`` against ``target``, its gradient with respect to ``out``: 2 (out - target) / numel)."""
    diff = out.detach().to(torch.float32) - target.detach().to(device=out.device, dtype=torch.float32)
    return (diff * diff).mean(), diff * (2.0 / diff.numel())


def _check(latents, encoder_hidden_states, fit, init, steps, timesteps, scheduler):
    """Every refusal of ``fit_conditioning``, before any device work.  Returns the names to fit, in the order given."""
    if latents.dim() != 3:
        raise ValueError(f"latents must be [B, L, latent_dim] in the loop's token layout (edit.vae_to_loop), got {list(latents.shape)}")
    B, L, _ = latents.shape
    if len(encoder_hidden_states) != len(MEM_NAMES):
        raise ValueError("encoder_hidden_states must be the 5-tuple (spk_emb, alsn, tlsn, apb, lsnemb)")
    fit = tuple(fit)
    if not fit:
        raise ValueError("fit names no memory")
    for name in fit:
        if name not in MEM_NAMES:
            raise ValueError(f"fit names a memory that does not exist: {name!r} (the memories are {', '.join(MEM_NAMES)})")
    if len(set(fit)) != len(fit):
        raise ValueError(f"fit names a memory twice: {fit}")
    for name, m in zip(MEM_NAMES, encoder_hidden_states):
        if m.dim() != 3 or m.shape[0] != B or m.shape[-1] != 512:
            raise ValueError(f"memory {name}: expected the examples' own conditional memory [{B}, S, 512], got {list(m.shape)}")
    for name, v in (init or {}).items():
        if name not in fit:
            raise ValueError(f"init has a tensor for {name!r}, which is not fitted")
        S = int(encoder_hidden_states[MEM_NAMES.index(name)].shape[1])
        if tuple(v.shape) != (1, S, 512):
            raise ValueError(f"init[{name!r}] must be [1, {S}, 512], got {list(v.shape)}")
    if int(steps) < 1:
        raise ValueError(f"steps = {steps} must be at least 1")
    T = int(scheduler.config.num_train_timesteps)
    if timesteps is not None:
        if len(timesteps) < int(steps):
            raise ValueError(f"timesteps has {len(timesteps)} entries for {steps} steps")
        for t in timesteps:
            if not 0 <= int(t) < T:
                raise ValueError(f"timestep {int(t)} outside [0, {T})")
    if scheduler.config.prediction_type not in ("epsilon", "sample"):
        raise NotImplementedError(f"fit_conditioning: prediction_type {scheduler.config.prediction_type!r} has no target")
    why = vjp_refusal(B, L, [int(m.shape[1]) for m in encoder_hidden_states])
    if why is not None:
        raise NotImplementedError(f"fitting runs on the memory gradient of the row-tile path only: {why}")
    return fit


def fit_conditioning(denoiser, scheduler, latents, encoder_hidden_states, cond_masks=None, *, fit=("lsnemb",), init=None, steps, lr,
                     optimizer=None, timesteps=None, seed=0):
    """Fit the memories named in ``fit`` to the clean example ``latents [B, L, 128]`` (the loop's token layout, ``edit.vae_to_loop``).

    ``encoder_hidden_states``: the examples' own five conditional memories ``[B, S_j, 512]``; ``cond_masks``: their key-padding masks.
    Every fitted memory is ONE tensor ``[1, S_j, 512]`` shared by all B rows (a single instance with an all-zero row map: the kernel
    sums the rows' gradients); it starts at ``init[name]`` or at the mean of the given rows.  The mask of a fitted memory is that of
    example 0.  A step: a timestep (``timesteps[i]``, or a draw of a CPU generator seeded with ``seed`` over ``num_train_timesteps``) --
    ONE for all rows, see the module docstring --, noise from the same generator, ``x_t = scheduler.add_noise(latents, noise, t)``, the
    target by ``scheduler.config.prediction_type``, the forward, ``denoising_loss_cotangent`` of its output, one ``vjp_memories`` call
    with ``wrt=fit`` (the mean-squared error's cotangent depends on the output, so it cannot be handed to the call that computes it),
    one optimiser step.
    ``optimizer``: a callable ``params -> torch.optim.Optimizer``; default ``Adam(params, lr=lr)``.

    Returns ``({name: fitted [1, S_j, 512]}, losses)``: the loss of step i is measured BEFORE its update."""
    fit = _check(latents, encoder_hidden_states, fit, init, steps, timesteps, scheduler)
    B, L, _ = latents.shape
    dev = latents.device
    x0 = latents.detach().to(torch.float32).contiguous()
    masks = dict(cond_masks or {})
    params = {}
    for name in fit:
        j = MEM_NAMES.index(name)
        start = init[name] if init and name in init else encoder_hidden_states[j].detach().to(torch.float32).mean(dim=0, keepdim=True)
        params[name] = start.detach().to(device=dev, dtype=torch.float32).clone().contiguous().requires_grad_(True)
    opt = optimizer(list(params.values())) if optimizer is not None else torch.optim.Adam(list(params.values()), lr=lr)
    zero_map = torch.zeros(B, dtype=torch.int32, device=dev)
    row_maps = [zero_map if name in fit else None for name in MEM_NAMES]
    call_masks = {}
    for name in MEM_NAMES:
        mk = masks.get(name)
        call_masks[name] = mk if mk is None or name not in fit else mk[:1]
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    T = int(scheduler.config.num_train_timesteps)
    losses = []
    for i in range(int(steps)):
        t = int(timesteps[i]) if timesteps is not None else int(torch.randint(0, T, (1,), generator=gen).item())
        noise = torch.randn(x0.shape, generator=gen, dtype=torch.float32).to(dev)
        xt = scheduler.add_noise(x0, noise, t)
        target = noise if scheduler.config.prediction_type == "epsilon" else x0
        mems = [params[name].detach() if name in fit else encoder_hidden_states[j] for j, name in enumerate(MEM_NAMES)]
        # The loss's cotangent depends on the output, so a step is the inference forward (memories expanded to one per row) and one
        # vjp_memories call on the shared instances; the call's own recomputed forward is not read back (want_out=False).
        with torch.no_grad():
            out, _ = denoiser(xt, t, [m.expand(B, -1, -1) if name in fit else m for name, m in zip(MEM_NAMES, mems)],
                              mem_mask_dict={k: (v.expand(B, -1) if v is not None and k in fit else v) for k, v in call_masks.items()})
        loss, cot = denoising_loss_cotangent(out, target)
        _, _, d_mem = denoiser.vjp_memories(xt, t, mems, call_masks, cot, wrt=fit, row_maps=row_maps, want_out=False, want_grad=False)
        losses.append(float(loss))
        opt.zero_grad(set_to_none=True)
        for name in fit:
            params[name].grad = d_mem[name]
        opt.step()
    return {name: p.detach().clone() for name, p in params.items()}, losses


def _check_audio(audio_encoder, latents, mel, encoder_hidden_states, train, steps, timesteps, scheduler):
    """Every refusal of ``fit_audio_encoder``, before any device work.  Returns the keys to train, in the order given."""
    from .conditioning import AUDIO_ENC_KEYS
    if audio_encoder.training:
        raise NotImplementedError("fit_audio_encoder: the encoder must be in eval mode (dropout is not implemented; fitting runs with it as the identity)")
    train = AUDIO_ENC_KEYS if train is None else tuple(train)
    if not train:
        raise ValueError("train names no parameter")
    for k in train:
        if k not in AUDIO_ENC_KEYS:
            raise ValueError(f"train names a parameter that does not exist: {k!r} (the parameters are {', '.join(AUDIO_ENC_KEYS)})")
    if len(set(train)) != len(train):
        raise ValueError(f"train names a parameter twice: {train}")
    in_dim, latent = audio_encoder.main[0].in_features, audio_encoder.out_net.out_features
    if mel.dim() != 3 or mel.shape[-1] != in_dim:
        raise ValueError(f"mel must be [B, S, {in_dim}] (the encoder's input_size), got {list(mel.shape)}")
    if latents.dim() == 3 and mel.shape[0] != latents.shape[0]:
        raise ValueError(f"mel has {mel.shape[0]} examples, latents {latents.shape[0]}")
    if len(encoder_hidden_states) != len(MEM_NAMES):
        raise ValueError("encoder_hidden_states must be the 5-tuple (spk_emb, alsn, tlsn, apb, lsnemb)")
    # the alsn entry is what the encoder makes of mel: its shape is known without running it
    j = MEM_NAMES.index("alsn")
    mems = list(encoder_hidden_states)
    mems[j] = torch.empty((mel.shape[0], mel.shape[1], latent), device="meta")
    _check(latents, mems, ("alsn",), None, steps, timesteps, scheduler)
    for p in audio_encoder.parameters():
        if p.device != latents.device or p.dtype != torch.float32:
            raise ValueError(f"the encoder's parameters must be float32 on the latents' device {latents.device}: they are updated in place "
                             f"(found {p.dtype} on {p.device})")
    return train


def fit_audio_encoder(denoiser, scheduler, audio_encoder, latents, mel, encoder_hidden_states, cond_masks=None, *, steps, lr, optimizer=None,
                      timesteps=None, seed=0, train=None):
    """Train ``audio_encoder`` (a ``conditioning.AudioConvEncoder`` in eval mode) against the FROZEN denoiser: the reference's training
    loss with every weight but the encoder's held fixed.  ``latents [B, L, 128]`` the clean examples, ``mel [B, S, input_size]`` their Mel
    frames in dB, ``encoder_hidden_states`` the examples' five conditional memories -- the ``alsn`` entry is not read (it may be None):
    it is ``audio_encoder(mel)`` at every step.  Objective and draws are ``fit_conditioning``'s: one timestep for all rows, a CPU
    generator seeded with ``seed``, the target by ``scheduler.config.prediction_type``.

    A step: ``alsn = audio_encoder(mel)``; the inference forward with every example's own memories; ``denoising_loss_cotangent``; one
    ``vjp_memories(..., wrt=("alsn",), want_out=False, want_grad=False)``; one ``conditioning.audio_encoder_vjp``; one optimiser step on
    the module's parameters IN PLACE.  ``train``: the state-dict keys to train (default all six of ``conditioning.AUDIO_ENC_KEYS``);
    the others keep their bits.  ``optimizer``: a callable ``params -> torch.optim.Optimizer``; default ``Adam(params, lr=lr)``.
    Dropout(0.1) and the reference's random modality drops are not applied.  Fitting quality on a trained checkpoint is not measured by
    the project's tests: their weights are seeded.

    Returns the losses: the loss of step i is measured BEFORE its update."""
    from .conditioning import AUDIO_ENC_KEYS, _audio_enc_params, audio_encoder_vjp
    train = _check_audio(audio_encoder, latents, mel, encoder_hidden_states, train, steps, timesteps, scheduler)
    dev = latents.device
    x0 = latents.detach().to(torch.float32).contiguous()
    mel = mel.detach().to(device=dev, dtype=torch.float32).contiguous()
    masks = dict(cond_masks or {})
    by_key = dict(zip(AUDIO_ENC_KEYS, _audio_enc_params(audio_encoder)))
    params = [by_key[k] for k in train]
    opt = optimizer(params) if optimizer is not None else torch.optim.Adam(params, lr=lr)
    j_alsn = MEM_NAMES.index("alsn")
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    T = int(scheduler.config.num_train_timesteps)
    losses = []
    for i in range(int(steps)):
        t = int(timesteps[i]) if timesteps is not None else int(torch.randint(0, T, (1,), generator=gen).item())
        noise = torch.randn(x0.shape, generator=gen, dtype=torch.float32).to(dev)
        xt = scheduler.add_noise(x0, noise, t)
        target = noise if scheduler.config.prediction_type == "epsilon" else x0
        with torch.no_grad():
            alsn = audio_encoder(mel)
            mems = [alsn if j == j_alsn else m for j, m in enumerate(encoder_hidden_states)]
            out, _ = denoiser(xt, t, mems, mem_mask_dict=masks)
        loss, cot = denoising_loss_cotangent(out, target)
        _, _, d_mem = denoiser.vjp_memories(xt, t, mems, masks, cot, wrt=("alsn",), want_out=False, want_grad=False)
        grads, _ = audio_encoder_vjp(audio_encoder, mel, d_mem["alsn"], want=train)
        losses.append(float(loss))
        opt.zero_grad(set_to_none=True)
        for k in train:
            by_key[k].grad = grads[k]
        opt.step()
    return losses


def fit_identity(denoiser, scheduler, latents, encoder_hidden_states, cond_masks=None, *, init=None, steps, lr, optimizer=None,
                 timesteps=None, seed=0):
    """A new listener identity: ``fit_conditioning`` with ``fit=("lsnemb",)``.  ``init``: a start vector ``[1, 1, 512]`` (or anything that
    reshapes to it); default the mean of the given ``lsnemb`` rows.  Returns ``(identity [1, S, 512], losses)``."""
    start = None
    if init is not None:
        S = int(encoder_hidden_states[MEM_NAMES.index("lsnemb")].shape[1])
        start = {"lsnemb": torch.as_tensor(init).reshape(1, S, 512)}
    fitted, losses = fit_conditioning(denoiser, scheduler, latents, encoder_hidden_states, cond_masks, fit=("lsnemb",), init=start, steps=steps,
                                      lr=lr, optimizer=optimizer, timesteps=timesteps, seed=seed)
    return fitted["lsnemb"], losses
