"""High-precision restatement of one guided update by a key-pose loss in POSE space (``cfd_denoise_guide_pose``,
``Denoiser.guide_pose``) -- TEST INFRASTRUCTURE.

Plain numpy in one dtype chosen by the caller (float64: what the call is measured against; float32: the yardstick), composed from
``tests/guide_ref`` (tie gather, combine, fold, update), ``tests/vjp_ref.out_and_vjp`` (the denoiser's forward and its vector-Jacobian
product) and ``tests/vae_vjp_ref`` (the decoder's forward and its sweep, fed the loss's own cotangent).  Nothing here is copied from the
code under test; the layout map and the loss are pinned against torch autograd by tests/test_pose_guide_host.py.
"""
import numpy as np

from tests import guide_ref, vae_vjp_ref, vjp_ref


def loop_to_vae(x0):
    """[B, L, C] -> [2, B, L / 2, C]: token l = 2 p + part of row b goes to z[part, b, p]."""
    B, L, C = x0.shape
    return np.ascontiguousarray(x0.reshape(B, L // 2, 2, C).transpose(2, 0, 1, 3))


def vae_to_loop(z):
    """The inverse map (and, being a permutation, the transpose that carries d_z back to d_x0)."""
    two, B, T, C = z.shape
    return np.ascontiguousarray(z.transpose(1, 2, 0, 3).reshape(B, 2 * T, C))


def loss_and_cotangent(feats, target, frame_mask, feature_mask, inv_n):
    """(loss, d_feats) of loss = inv_n sum (frame_mask feature_mask (feats - target))^2."""
    r = frame_mask[:, :, None] * feature_mask[None, None, :] * (feats - target)
    return inv_n * (r * r).sum(), 2.0 * inv_n * r


def forward(sd, vsd, x, t, mems_rows, masks_rows, w, lengths, target, frame_mask, feature_mask, s0, s1, inv_n, tie=None, num_layers=5,
            dtype=np.float64):
    """The loss alone, as a function of the latents x in ``dtype`` (x is NOT rounded to float32 on the way into the denoiser: the
    function central differences are taken of)."""
    dt = np.dtype(dtype)
    x, w, target, frame_mask, feature_mask = (np.asarray(v, dtype=dt) for v in (x, w, target, frame_mask, feature_mask))
    B, L, C = x.shape
    n = w.shape[1]
    xt = guide_ref.gather_tie(x, tie)
    out = vjp_ref.out_and_vjp(sd, np.concatenate([xt] * n), t, mems_rows, masks_rows, np.zeros((n * B, L, C), dtype=dt), dtype=dt)[0]
    x0 = (xt - dt.type(s1) * guide_ref.combine(np.asarray(out, dtype=dt).reshape(n, B, L, C), w)) / dt.type(s0)
    feats = vae_vjp_ref.decode_forward(vsd, loop_to_vae(x0), lengths, num_layers, dt)[0]
    return float(loss_and_cotangent(np.asarray(feats, dtype=dt), target, frame_mask, feature_mask, dt.type(inv_n))[0])


def guide_pose(sd, vsd, x, t, mems_rows, masks_rows, w, lengths, target, frame_mask, feature_mask, s0, s1, inv_n, step, tie=None,
               num_layers=5, dtype=np.float64, round_input=True):
    """dict(loss, feats [B, F, 189], d_out [n * B, L, 128], grad, x_new) of one guided update.  sd / vsd: the denoiser's and the VAE's
    state dicts; x [B, L, 128]; mems_rows / masks_rows: the memories and masks of the n * B forward rows, chunk-major; w [B, n];
    lengths: B frame counts whose largest F is target's; target [B, F, 189]; frame_mask [B, F]; feature_mask [189].
    round_input False: the forward is given x in ``dtype`` (for central differences)."""
    dt = np.dtype(dtype)
    x, w, target, frame_mask, feature_mask = (np.asarray(v, dtype=dt) for v in (x, w, target, frame_mask, feature_mask))
    s0, s1, inv_n, step = (dt.type(v) for v in (s0, s1, inv_n, step))
    B, L, C = x.shape
    n = w.shape[1]
    xt = guide_ref.gather_tie(x, tie)
    xin = np.concatenate([xt] * n)
    if round_input:
        xin = xin.astype(np.float32)      # (what the forward is given: the float32 latents)
    out = vjp_ref.out_and_vjp(sd, xin, t, mems_rows, masks_rows, np.zeros_like(xin), dtype=dt)[0]
    x0 = (xt - s1 * guide_ref.combine(np.asarray(out, dtype=dt).reshape(n, B, L, C), w)) / s0
    feats, state, _ = vae_vjp_ref.decode_forward(vsd, loop_to_vae(x0), lengths, num_layers, dt)
    feats = np.asarray(feats, dtype=dt)
    loss, d_feats = loss_and_cotangent(feats, target, frame_mask, feature_mask, inv_n)
    d_x0 = vae_to_loop(np.asarray(vae_vjp_ref.decode_sweep(state, d_feats), dtype=dt))
    back = -(s1 / s0)
    wsum = w[:, 1:].sum(axis=1)
    d_out = np.stack([back * (1.0 - wsum)[:, None, None] * d_x0] + [back * w[:, k, None, None] * d_x0 for k in range(1, n)])
    g_rows = vjp_ref.out_and_vjp(sd, xin, t, mems_rows, masks_rows, d_out.reshape(n * B, L, C), dtype=dt)[1]
    gt = d_x0 / s0
    for c in range(n):
        gt = gt + np.asarray(g_rows, dtype=dt).reshape(n, B, L, C)[c]
    g = guide_ref.fold(gt, tie)
    return dict(loss=float(loss), feats=feats, d_out=d_out.reshape(n * B, L, C), grad=g, x_new=guide_ref.update(xt, g, tie, step))
