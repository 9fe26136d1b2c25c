"""Plain restatements of the kernels of a cfd_sample_parallel sweep around the forward -- TEST INFRASTRUCTURE (numpy).

``step64``: the DDPM step of one level under the guidance combine, float64, the formulas of oracle/sampler_ref.cfg_combine (u + the sum of
w_k (e_k - u) in the reference's order) and oracle/scheduler_ref.DDPMSchedulerRef.step (x0 = (x - sb eps) / sa, clipped to [-1, 1],
mu = c0 x0 + cx x, + sigma z where the row adds noise) on the float32 coefficient rows the library uploads.
``scan32``: the re-propagation of a sweep, float32 with every operation rounded on its own (tests/parallel_ref.sample_parallel's scan).
``split_planes``: the stored split pairs of a float32 row (cfd_test_gemm_epi's convention: per 32-column block 64 bytes of hi, 64 of lo).
"""
import numpy as np

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24


def step64(x, eps, coef_row, pos, w, clip, z):
    """x [B, L, 128], eps [G, B, L, 128] (the evaluated chunks), coef_row float32 [8] (sb, sa, c0, cx, sigma, use_noise, ..), pos: the
    evaluated chunk of every chunk of the combine, w: float [Gc] or per utterance [B, Gc] (w[.., 0] is not read), z [B, L, 128].
    Returns (s, x0 before the clip, mag) in float64; mag = |x| + sum_k |w_k| |e_k - e_0| + |e_0|, the magnitude the rounding errors of
    the float32 chain scale with."""
    x, eps, z = np.asarray(x, F64), np.asarray(eps, F64), np.asarray(z, F64)
    sb, sa, c0, cx, sigma, use_noise = (F64(v) for v in np.asarray(coef_row, F32)[:6])
    w = np.asarray(w, F64)
    wk = (lambda k: w[:, k].reshape(-1, 1, 1)) if w.ndim == 2 else (lambda k: w[k])
    u = eps[pos[0]]
    acc, mag = np.zeros_like(u), np.abs(x) + np.abs(u)
    for k in range(1, len(pos)):                       # ((((text + audio) + spk) + apb) + lsnid) + all
        term = wk(k) * (eps[pos[k]] - u)
        acc = acc + term
        mag = mag + np.abs(term)
    e = u + acc if len(pos) > 1 else u
    x0 = (x - sb * e) / sa
    x0c = np.clip(x0, -1.0, 1.0) if clip else x0
    s = c0 * x0c + cx * x
    if use_noise != 0:
        s = s + sigma * z
    return s, x0, mag


def step_bound(s, mag, coef_row, Gc):
    """|float32 chain - step64| <= C 2^-24 mag / sa + 2^-24 |s|, C = 8 + 2 Gc.  The chain: the combine's Gc - 1 terms take a subtraction
    and a product each and at most Gc - 1 additions in sequence (the last one onto e_0): <= Gc + 1 roundings of the running magnitude;
    sb eps, the subtraction and the division by sa: 3; c0 x0, cx x and their sum: 3 -- Gc + 7 roundings of quantities bounded by
    mag / sa (sa, sb, c0, cx <= 1; a clipped x0 has |x - sb eps| >= sa, so mag / sa >= 1 = |x0|).  The rest of C, Gc + 1 units, covers
    the product sigma z (sigma <= 0.6 in a 20-step table), the second-order terms and the float64 side.  The last addition rounds the
    result itself: 2^-24 |s|."""
    C = 8 + 2 * Gc
    return C * U24 * mag / F64(np.asarray(coef_row, F32)[1]) + U24 * np.abs(s)


def scan32(s, X, base, off):
    """s float32 [J, B, L, 128] (levels below off are not read), X: {iteration: float32 [B, L, 128]} with base + off .. base + J.
    Returns ({iteration: new X} for base + off + 1 .. base + J, d [J + 1, B, L, 128]: row k = the change of window position k)."""
    J = s.shape[0]
    d = np.zeros_like(s[0], dtype=F32)
    new, ds = {}, np.zeros((J + 1,) + s.shape[1:], F32)
    for lv in range(off, J):
        i, k = base + lv, lv - off + 1
        xn = (s[lv].astype(F32) + d).astype(F32)
        d = (xn - X[i + 1].astype(F32)).astype(F32)
        new[i + 1] = xn
        ds[k] = d
    return new, ds


def err64(ds):
    """The float64 sum per utterance of the float32 squares: ds [K, B, L, 128] -> [K, B]."""
    return np.sum((ds * ds).astype(F32).astype(F64), axis=(2, 3))


def split_planes(x):
    """float32 [..., 128] -> the stored row as uint8 [..., 512]."""
    x = np.clip(np.asarray(x, F32), -65504, 65504)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(F32)).astype(np.float16)
    blk = np.stack([hi.reshape(x.shape[:-1] + (-1, 32)), lo.reshape(x.shape[:-1] + (-1, 32))], axis=-2)     # [..., blocks, 2, 32]
    return np.ascontiguousarray(blk).view(np.uint8).reshape(x.shape[:-1] + (x.shape[-1] * 4,))
