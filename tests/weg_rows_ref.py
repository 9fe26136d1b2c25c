"""Restatement of per-row word-excitation guidance (cfd_weg_step, ``weg.weg_update_rows``) -- TEST INFRASTRUCTURE.

Every row of a batch is its own utterance, so the restatement composes ``oracle.weg_ref`` at B = 1, row by row: ``focus_loss`` /
``loss_and_grad`` / ``weg_update`` with ``normalize_eot=True`` and the row's own EOT.  What the rows share in a tied run -- the
evaluation at x~, the fold of a tied token's gradient onto its source weighted by the tied token's row step, the lock-step rounds --
is written out in numpy float32 in the order the kernel sums in (ascending CSR order), so that the fold can be compared bit for bit.
"""
import numpy as np

from oracle import weg_ref
from oracle.sampler_ref import CFG_CHUNKS, cfg_combine

F32 = np.float32


def row_eots(masks):
    """argmax(mask_tlsn[b]) - 1 per row (convofusion.py:460)."""
    return [int(v) for v in np.argmax(np.asarray(masks["tlsn"]).astype(np.int64), axis=1) - 1]


def one_row(states, masks, b):
    return [np.asarray(m)[b:b + 1] for m in states], {k: (np.asarray(v)[b:b + 1] if v is not None else None) for k, v in masks.items()}


def focus_loss_rows(att, focus, eots):
    """``weg_ref.focus_loss`` per row with that row's EOT: (losses [B], max_att list of lists, d losses[b] / d att[b] stacked)."""
    losses, mx, d = [], [], []
    for b in range(att.shape[0]):
        _, ls, m, g = weg_ref.focus_loss(att[b:b + 1], [focus[b]], True, [eots[b]])
        losses.append(ls[0])
        mx.append(m[0])
        d.append(g[0])
    return np.asarray(losses, dtype=F32), mx, np.stack(d)


def loss_and_grad_rows(sd, latents, t, states, masks, focus):
    """``weg_ref.loss_and_grad`` at B = 1 per row: (losses [B], grad [B, L, 128]); a row without focus tokens: 0 and zeros."""
    losses, grads = [], []
    for b in range(latents.shape[0]):
        if not focus[b]:
            losses.append(F32(0))
            grads.append(np.zeros_like(latents[b]))
            continue
        st, mk = one_row(states, masks, b)
        loss, _, _, g = weg_ref.loss_and_grad(sd, latents[b:b + 1], t, st, mk, [focus[b]], True)
        losses.append(F32(loss))
        grads.append(g[0])
    return np.asarray(losses, dtype=F32), np.stack(grads).astype(F32)


# ----------------------------------------------------------------------------- the tie: x~, the CSR table, the fold
def tie_copy(latents, tie):
    B, L, D = latents.shape
    flat = np.asarray(tie).reshape(-1)
    tied = np.nonzero(flat >= 0)[0]
    out = latents.reshape(B * L, D).copy()
    out[tied] = latents.reshape(B * L, D)[flat[tied]]
    return out.reshape(B, L, D)


def tied_lists(tie):
    """Per source token the tokens tied to it, ascending (the CSR table's content)."""
    flat = np.asarray(tie).reshape(-1)
    lists = {}
    for e in np.nonzero(flat >= 0)[0]:
        lists.setdefault(int(flat[e]), []).append(int(e))
    return lists


def fold(x_tilde, g_tilde, tie, steps):
    """(grad, x_new) of the gated, tied update from g~ = the per-row gradients at x~, in float32 and the kernel's order:
    grad[s] = g~[s] + sum_t g~[t]; x_new[s] = x~[s] - (step[r(s)] g~[s] + sum_t step[r(t)] g~[t]); a tied token: grad 0, its source's
    x_new."""
    B, L, D = x_tilde.shape
    flat = np.asarray(tie).reshape(-1) if tie is not None else np.full(B * L, -1)
    steps = np.asarray(steps, dtype=F32)
    g = g_tilde.reshape(B * L, D).astype(F32)
    x = x_tilde.reshape(B * L, D).astype(F32)
    lists = tied_lists(flat)
    grad, x_new = np.zeros_like(g), np.zeros_like(x)
    for s in range(B * L):
        if flat[s] >= 0:
            continue
        gu = g[s].copy()
        gs = (steps[s // L] * g[s]).astype(F32)
        for t in lists.get(s, []):
            gu = (gu + g[t]).astype(F32)
            gs = (gs + (steps[t // L] * g[t]).astype(F32)).astype(F32)
        grad[s] = gu
        x_new[s] = (x[s] - gs).astype(F32)
    tied = np.nonzero(flat >= 0)[0]
    x_new[tied] = x_new[flat[tied]]
    return grad.reshape(B, L, D), x_new.reshape(B, L, D)


# ----------------------------------------------------------------------------- the loop branch
def reference_row(seq, threshold, max_refinement_steps, closing):
    """``weg_ref.weg_update``'s control flow for ONE row on a recorded loss sequence: seq[k] is the row's loss after k effective steps
    (a step at loss 0 has gradient 0 and moves nothing).  threshold None: no threshold iteration.  Returns (steps taken, rounds, the
    loss the branch returns, evaluations)."""
    k, loss, evals, rounds = 0, seq[0], 1, 0
    if threshold is not None and loss > 1.0 - threshold:
        target = max(0.0, 1.0 - threshold)
        while loss > target:
            rounds += 1
            loss = seq[k]
            evals += 1
            if loss != 0:
                k += 1
            if rounds >= max_refinement_steps:
                break
        loss = seq[k]
        evals += 1
    if closing and loss != 0:
        k += 1
    return k, rounds, loss, evals


def weg_update_rows(sd, latents, i, t, states, masks, focus, params, num_steps, scale_carry=None, log=None):
    """``weg_ref.weg_update`` applied per row at B = 1 (untied rows are independent).  The scale-range carry is one table for the run:
    every row reads a copy, the run's own advances once.  ``log``: a list that receives dict(i, losses, rounds, evaluated) -- the
    rows' returned losses, their refinement rounds (evaluations - 2 of a row that entered) and every loss a decision compared."""
    out, losses, rounds, seen = [], [], [], []
    real = weg_ref.loss_and_grad
    for b in range(latents.shape[0]):
        if not focus[b]:
            out.append(latents[b:b + 1])
            losses.append(0.0)
            rounds.append(0)
            seen.append([])
            continue
        st, mk = one_row(states, masks, b)
        evaluated = []

        def counting(*a, **kw):
            r = real(*a, **kw)
            evaluated.append(float(r[0]))
            return r
        weg_ref.loss_and_grad = counting
        try:
            new, loss = weg_ref.weg_update(sd, latents[b:b + 1], i, t, st, mk, [focus[b]], params, num_steps,
                                           scale_carry=None if scale_carry is None else list(scale_carry))
        finally:
            weg_ref.loss_and_grad = real
        out.append(new)
        losses.append(loss)
        rounds.append(max(0, len(evaluated) - 2))
        seen.append(evaluated)
    if scale_carry is not None:
        weg_ref.scale_range_schedule(params, num_steps, scale_carry)
    if log is not None:
        log.append(dict(i=i, losses=losses, rounds=rounds, evaluated=seen))
    return np.concatenate(out, axis=0).astype(F32)


def weg_update_rows_tied(sd, latents, i, t, states, masks, focus, params, num_steps, tie, scale_carry=None, log=None):
    """The same branch for the rows of a tied run, where the rows meet in the fold: lock-step rounds.  Every evaluation is per row
    at x~; row b takes its step in a round while it entered refinement, its previous loss exceeds the target and it has taken fewer
    than max_refinement_steps rounds; one closing evaluation with the closing step follows (a row at loss 0 has gradient 0)."""
    sr = weg_ref.scale_range_schedule(params, num_steps, scale_carry)
    step = F32(params["scale_factor"] * np.sqrt(sr[i]))
    closing = step if i < params["max_iter_to_alter"] else F32(0)
    B = latents.shape[0]
    x = tie_copy(np.asarray(latents, dtype=F32), tie)

    def call(steps):
        nonlocal x
        losses, g = loss_and_grad_rows(sd, x, t, states, masks, focus)
        _, x = fold(x, g, tie, steps)
        seen.append([float(v) for v in losses])
        return losses
    thr = params["thresholds"].get(i)
    rounds, seen = [0] * B, []
    if thr is None:
        losses = call([closing] * B)
    else:
        losses = call([0] * B)
        target = max(0.0, 1.0 - thr)
        entered = [float(l) > 1.0 - thr for l in losses]
        while True:
            active = [entered[b] and float(losses[b]) > target and rounds[b] < params["max_refinement_steps"] for b in range(B)]
            if not any(active):
                break
            losses = call([step if a else F32(0) for a in active])
            rounds = [r + int(a) for r, a in zip(rounds, active)]
        if any(entered) or closing != 0:
            losses = call([closing] * B)
    if log is not None:
        log.append(dict(i=i, losses=[float(v) for v in losses], rounds=rounds, evaluated=seen))
    return x


def tied_reverse(denoise_fn, scheduler, encoder_hidden_states, cond_masks, init_noise, tie, pre_step=None, guidance_scale=7.5,
                 num_inference_steps=5, eta=0.0):
    """tests/longform_ref.py's tied loop (DDIM, eta 0, no kept tokens) with ``pre_step(i, t, latents)`` behind the copy of the tied
    tokens: the WEG branch of a tied run.  Returns the latents [B, L, 128] after the final copy."""
    latents = (np.asarray(init_noise, dtype=F32) * F32(scheduler.init_noise_sigma)).astype(F32)
    scheduler.set_timesteps(num_inference_steps)
    for i, t in enumerate(scheduler.timesteps):
        latents = tie_copy(latents, tie)
        if pre_step is not None:
            latents = pre_step(i, int(t), latents)
        noise_pred, _ = denoise_fn(np.concatenate([latents] * CFG_CHUNKS, axis=0), int(t), encoder_hidden_states, cond_masks)
        latents = scheduler.step(cfg_combine(noise_pred, guidance_scale), t, latents, eta=eta, noise=None)
    return tie_copy(latents, tie)


# ----------------------------------------------------------------------------- the loop case of tests/test_gpu_weg_rows.py
# Five DDPM iterations at B = 3 with EOTs 8 / 7 / 6, one threshold iteration.  Seed, scale factor and threshold were chosen with the
# oracle on the CPU so that (a) the rows need different numbers of rounds -- row 0 runs into max_refinement_steps, row 1 leaves after two
# rounds, row 2 never enters -- and (b) every oracle loss a decision compares lies at least 1e-3 from the target 1 - 0.1695 = 0.8305
# (closest: row 1's 0.82939 and 0.83177), so that no decision can flip on float32 noise.  tests/golden/weg_rows_loop.npz records it
# (make_golden_weg_rows.py).
LOOP = dict(B=3, L=16, S=(6, 20, 12, 8, 1), pad=(2, 0, 3, 0, 0), n_steps=5, seed=11, focus=[[2, 5], [3], [1, 4]],
            params=dict(scale_factor=5000, scale_range=[1.0, 0.5], max_iter_to_alter=3, thresholds={1: 0.1695}, max_refinement_steps=3))
_loop = {}


def loop_inputs():
    from oracle import inputs, philox_ref
    c = LOOP
    cb = inputs.make_cfg_batch(seed=c["seed"], B=c["B"], L=c["L"], S=c["S"], pad_tail=c["pad"])
    init = philox_ref.normal_tensor(c["seed"], 0, range(c["B"]), 1, c["L"])
    noise = np.stack([philox_ref.normal_tensor(c["seed"], i, range(c["B"]), 0, c["L"]) for i in range(c["n_steps"])])
    text_states = [np.split(x, 7, axis=0)[1] for x in cb["memories"]]
    text_masks = {k: (np.split(v, 7, axis=0)[1] if v is not None else None) for k, v in cb["masks"].items()}
    return cb, init, noise, text_states, text_masks


def loop_oracle():
    """(guided latents [L, B, 128], unguided latents, log) of the loop case: ``sampler_ref.diffusion_reverse`` with the per-row
    ``pre_step``; computed once per process."""
    if not _loop:
        from oracle import denoiser_ref, sampler_ref, scheduler_ref
        from tests.helpers import state_dict
        c = LOOP
        sd = state_dict(1234, 1.0)
        cb, init, noise, ts, tm = loop_inputs()
        log, carry = [], list(c["params"]["scale_range"])
        fwd = lambda x, t, enc, masks: denoiser_ref.denoiser_forward(sd, x, t, enc, masks)
        kw = dict(guidance_scale=7.5, num_inference_steps=c["n_steps"])
        ref, _, _ = sampler_ref.diffusion_reverse(
            fwd, scheduler_ref.DDPMSchedulerRef(), cb["memories"], cb["masks"], init, lambda i, t: noise[i],
            pre_step=lambda i, t, lat: weg_update_rows(sd, lat, i, t, ts, tm, c["focus"], c["params"], c["n_steps"], scale_carry=carry, log=log), **kw)
        plain, _, _ = sampler_ref.diffusion_reverse(fwd, scheduler_ref.DDPMSchedulerRef(), cb["memories"], cb["masks"], init, lambda i, t: noise[i], **kw)
        _loop["r"] = (ref, plain, log)
    return _loop["r"]
