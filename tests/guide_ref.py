"""High-precision restatement of one key-pose guided update (``cfd_denoise_guide``, ``Denoiser.guide``) -- TEST INFRASTRUCTURE.

Plain numpy in one dtype chosen by the caller (float64: what the call is measured against; float32: the yardstick), composed from
``tests/vjp_ref.out_and_vjp`` (the forward and the vector-Jacobian product of one denoiser forward): the tie gather, the guidance
combine, the predicted clean latents, the key-pose loss, the cotangent rows, the sum over the chunks, the fold of tied tokens onto
their sources and the update.  Nothing here is copied from the code under test; the fold is pinned against torch autograd through an
index gather by tests/test_keyframes_host.py.
"""
import numpy as np

from tests import vjp_ref


def gather_tie(x, tie):
    """x~: x [B, L, C] with every tied token (tie [B, L] >= 0: the flat index of its source) replaced by its source's value."""
    if tie is None:
        return x
    B, L, C = x.shape
    flat = x.reshape(B * L, C)
    t = np.asarray(tie).reshape(-1)
    idx = np.where(t >= 0, t, np.arange(B * L))
    return flat[idx].reshape(B, L, C)


def combine(e, w):
    """eps = e_0 + sum_{k >= 1} w[:, k] (e_k - e_0), in ascending k; e [n, B, L, C], w [B, n]."""
    eps = e[0]
    for k in range(1, e.shape[0]):
        eps = eps + w[:, k, None, None] * (e[k] - e[0])
    return eps


def loss_and_cotangents(xt, e, w, target, mask, s0, s1, inv_n):
    """(loss, d_out [n, B, L, C], g_dir [B, L, C]) of loss = inv_n sum (mask (x0 - target))^2, x0 = (x~ - s1 eps) / s0."""
    n = e.shape[0]
    x0 = (xt - s1 * combine(e, w)) / s0
    r = mask[..., None] * (x0 - target)
    loss = inv_n * (r * r).sum()
    d_x0 = 2.0 * inv_n * r
    back = -(s1 / s0)
    wsum = w[:, 1:].sum(axis=1)
    d_out = np.stack([back * (1.0 - wsum)[:, None, None] * d_x0] + [back * w[:, k, None, None] * d_x0 for k in range(1, n)])
    return loss, d_out, d_x0 / s0


def fold(g, tie):
    """The gradient at x of a function whose gradient at x~ = gather_tie(x, tie) is g [B, L, C]: a source receives its own row plus the
    rows of the tokens tied to it (ascending), a tied token 0."""
    if tie is None:
        return g
    B, L, C = g.shape
    flat = g.reshape(B * L, C)
    out = flat.copy()
    t = np.asarray(tie).reshape(-1)
    for e in np.nonzero(t >= 0)[0]:
        out[t[e]] = out[t[e]] + flat[e]
    out[t >= 0] = 0
    return out.reshape(B, L, C)


def update(xt, g, tie, step):
    """x_new = x~ - step g on free tokens; a tied token takes its source's new value."""
    return gather_tie(xt - step * g, tie)


def guide(sd, x, t, mems_rows, masks_rows, w, target, mask, s0, s1, inv_n, step, tie=None, dtype=np.float64):
    """dict(loss, d_out [n * B, L, 128], grad, x_new) of one guided update.  x [B, L, 128]; mems_rows / masks_rows: the memories and
    masks of the n * B forward rows, chunk-major (row c * B + b), one per row; w [B, n]; s0 = sqrt(acp_t), s1 = sqrt(1 - acp_t)."""
    dt = np.dtype(dtype)
    x, w, target, mask = (np.asarray(v, dtype=dt) for v in (x, w, target, mask))
    s0, s1, inv_n, step = (dt.type(v) for v in (s0, s1, inv_n, step))
    B, L, C = x.shape
    n = w.shape[1]
    xt = gather_tie(x, tie)
    xin = np.concatenate([xt] * n).astype(np.float32)      # (what the forward is given: the float32 latents)
    out = vjp_ref.out_and_vjp(sd, xin, t, mems_rows, masks_rows, np.zeros_like(xin), dtype=dt)[0]
    loss, d_out, g_dir = loss_and_cotangents(xt, np.asarray(out, dtype=dt).reshape(n, B, L, C), w, target, mask, s0, s1, inv_n)
    g_rows = vjp_ref.out_and_vjp(sd, xin, t, mems_rows, masks_rows, d_out.reshape(n * B, L, C), dtype=dt)[1]
    gt = g_dir
    for c in range(n):
        gt = gt + np.asarray(g_rows, dtype=dt).reshape(n, B, L, C)[c]
    g = fold(gt, tie)
    return dict(loss=float(loss), d_out=d_out.reshape(n * B, L, C), grad=g, x_new=update(xt, g, tie, step))
