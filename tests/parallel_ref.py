"""Restated parallel-in-time DDPM sampling (ParaDiGMS, Shih et al., NeurIPS 2023) -- TEST INFRASTRUCTURE (numpy, float32).

The reference has no parallel sampler.  Restated here is the sweep / scan / slide loop of cfd_sample_parallel over ANY eps function, on
oracle.scheduler_ref.DDPMSchedulerRef's float32 step:

    X(i): the current estimate of the latent ENTERING iteration i; window i0 .. i0 + p - 1, p = min(J, N - i0); X(i0) is final
    sweep:  s_j  = DDPMSchedulerRef.step(eps_fn(X(j), j, t_j), t_j, X(j), noise_j)          for every j of the window, from the OLD X
    scan:   Xn(i0) = X(i0);  Xn(j + 1) = fl(s_j + fl(Xn(j) - X(j)))                         serially over the window
    err:    e[k][b] = sum_{l,d} (Xn(i0 + k) - X(i0 + k))^2                                  k = 1 .. p - 1
    slide:  the largest s in [1, p] with e[k][b] / (L * 128) <= tau^2 * v(i0 + k) for every 1 <= k < s and every b (``stride``)

v(i) = sigma_i^2 of iteration i's step; an iteration that adds no noise (t = 0) takes the value of the iteration before it.  The levels
that enter the window start from its last value.  X(i0 + 1) is exact after every sweep (it is the sequential step of the final X(i0)),
and a level whose predecessor did not change receives s_j + 0 = s_j: at tau = 0 a level is passed only when every level in front of it
was left unchanged by the sweep, i.e. when it is the sequential chain's value -- by induction the whole run is, in at most N sweeps.
The trajectory uses the ring convention of the inversions: slot N - i is X(i), slot 0 the result.
"""
import numpy as np

from oracle.sampler_ref import CFG_CHUNKS, cfg_combine

F32 = np.float32


def guided(denoise_fn, encoder_hidden_states=None, cond_masks=None, guidance_scale=7.5):
    """eps_fn(x [B, L, 128], i, t) of a 7-chunk denoise_fn(sample [7B, L, 128], t, enc, masks) -> (eps, att) under the reference's combine."""
    def eps_fn(x, i, t):
        noise_pred, _ = denoise_fn(np.concatenate([x] * CFG_CHUNKS, axis=0), int(t), encoder_hidden_states, cond_masks)
        return cfg_combine(noise_pred, guidance_scale)
    return eps_fn


def variances(scheduler, timesteps):
    """v(i) of the stride rule, float32 [N]."""
    sig = np.array([scheduler.coefficients(int(t))[4] for t in timesteps], F32)
    v = (sig * sig).astype(F32)
    for i, t in enumerate(timesteps):
        if int(t) == 0 and i > 0:
            v[i] = v[i - 1]
    return v


def stride(err, p, i0, v, tau, n_el):
    """err float32 [>= p][B] (row k: the squared change of X(i0 + k); row 0 unused); v: ``variances``; n_el = L * 128.  float32 throughout,
    as the library decides it; a NaN fails the comparison."""
    err = np.asarray(err, F32)
    s = 1
    while s < p:
        bound = F32(F32(tau) * F32(tau)) * v[i0 + s]
        if not np.all(err[s] / F32(n_el) <= bound):
            break
        s += 1
    return s


def stride_ratios(err, p, i0, v, tau, n_el):
    """The err / bound ratios ``stride`` evaluates (float64 of its float32 operands), every utterance of every window position up to and
    including the one that stops the window; empty at tau = 0.  A ratio near 1 is a stride that a last-bit difference can change."""
    err = np.asarray(err, F32)
    s = stride(err, p, i0, v, tau, n_el)
    out = []
    for k in range(1, min(s + 1, p)):
        bound = F32(F32(tau) * F32(tau)) * v[i0 + k]
        if bound > 0:
            out.extend(float(q) for q in (err[k] / F32(n_el)).astype(np.float64) / np.float64(bound))
    return out


def sequential(eps_fn, scheduler, init_latents, step_noise, num_inference_steps):
    """The DDPM loop; returns the trajectory [N + 1, B, L, 128] (slot N - i: the latent entering iteration i; slot 0: the result)."""
    scheduler.set_timesteps(num_inference_steps)
    ts = [int(t) for t in scheduler.timesteps]
    N = len(ts)
    x = np.asarray(init_latents, F32).copy()
    traj = np.empty((N + 1,) + x.shape, F32)
    traj[N] = x
    for i, t in enumerate(ts):
        x = scheduler.step(eps_fn(x, i, t), t, x, noise=step_noise[i] if t > 0 else None)
        traj[N - i - 1] = x
    return traj


def sample_parallel(eps_fn, scheduler, init_latents, step_noise, num_inference_steps, levels_per_batch, tolerance, max_sweeps=None,
                    ratios=None, drop_carry=False, fill_from_next_window=False):
    """Returns (latents [B, L, 128], trajectory [N + 1, B, L, 128], strides).  Raises RuntimeError when max_sweeps is reached.
    ratios: a list that receives ``stride_ratios`` of every sweep.  Planted bugs, for the sensitivity of the tests that compare with this
    loop: drop_carry -- the scan forgets Xn(j) - X(j) (Xn(j + 1) = s_j); fill_from_next_window -- the entering levels start from
    X(i1), the next window's first latent, instead of X(i0 + p).  Both keep the sequential chain as the fixed point at tolerance 0."""
    scheduler.set_timesteps(num_inference_steps)
    ts = [int(t) for t in scheduler.timesteps]
    N = len(ts)
    J = max(1, min(int(levels_per_batch), N))
    v = variances(scheduler, ts)
    x0 = np.asarray(init_latents, F32)
    n_el = x0.shape[1] * x0.shape[2]
    X = np.empty((N + 1,) + x0.shape, F32)     # X[i]: indexed by iteration here; turned into the ring on return
    X[:min(J, N) + 1] = x0
    i0, strides = 0, []
    while i0 < N:
        if max_sweeps is not None and len(strides) >= max_sweeps:
            raise RuntimeError(f"max_sweeps = {max_sweeps} reached with {i0} of {N} levels final")
        p = min(J, N - i0)
        s = [scheduler.step(eps_fn(X[j], j, ts[j]), ts[j], X[j], noise=step_noise[j] if ts[j] > 0 else None) for j in range(i0, i0 + p)]
        err = np.zeros((p + 1, x0.shape[0]), F32)
        d = np.zeros_like(x0)
        for k in range(1, p + 1):
            xn = s[k - 1].astype(F32) if drop_carry else (s[k - 1] + d).astype(F32)
            d = (xn - X[i0 + k]).astype(F32)
            err[k] = np.sum((d * d).astype(F32), axis=(1, 2), dtype=F32)
            X[i0 + k] = xn
        st = stride(err, p, i0, v, tolerance, n_el)
        strides.append(st)
        if ratios is not None:
            ratios.extend(stride_ratios(err, p, i0, v, tolerance, n_el))
        i1 = i0 + st
        hi = i1 + min(J, N - i1)
        X[i0 + p + 1:hi + 1] = X[i1] if fill_from_next_window else X[i0 + p]
        i0 = i1
    traj = X[::-1].copy()
    return traj[0].copy(), traj, strides
