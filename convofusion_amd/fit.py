"""Fitting CONDITIONING to data through the memory gradient of the HIP denoiser (``Denoiser.vjp_memories`` / ``cfd_denoise_vjp_mem``).

No weight is trained: the network stays as loaded, and what is optimised is one or more of the five memories themselves -- textual
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
