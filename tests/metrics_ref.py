"""A from-scratch numpy restatement of the reference's motion evaluation (quant_eval/metric_eval.py, jitter_metric.py,
motion_autoencoder.py), in the precision the caller names (float64: the yardstick; float32: what the same formulas lose in single
precision, which is where the GPU tests' gates come from), and the seeded inputs the tests share.  No reference code is imported here;
tests/golden/make_golden_metrics.py holds this file to the reference itself and records its outputs in tests/golden/metrics.npz."""
import functools

import numpy as np

FACTOR = 4.0
FEAT, JOINTS, FPS = 189, 63, 25
TRACK_JOINTS = (5, 6, 7, 9, 10, 11)
ORDERS = (10, 12)
SIGMAS = {10: 0.3, 12: 1.25}
THRESHOLD = 0.3
MARGIN = 1e-4
SEMANTIC_SCALE = 1 / 0.165


# ------------------------------------------------------------------ seeded inputs
@functools.lru_cache(maxsize=None)
def motion(seed, T=128):
    """float32 [T, 189]: a seeded rest pose plus, per coordinate, four sinusoids of 0.3 - 2.5 Hz and amplitude 0.05 - 0.4, at 25 fps."""
    rng = np.random.default_rng(1000 + seed)
    base = rng.uniform(-1.0, 1.0, FEAT)
    f = rng.uniform(0.3, 2.5, (4, FEAT))
    a = rng.uniform(0.05, 0.4, (4, FEAT))
    p = rng.uniform(0.0, 2 * np.pi, (4, FEAT))
    t = np.arange(T)[:, None, None] / FPS
    x = (base + (a * np.sin(2 * np.pi * f * t + p)).sum(axis=1)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def target_of(seed, T=128):
    """float32 [T, 189]: the motion plus a smaller seeded motion, so the SRGR decisions fall on both sides of the threshold."""
    rng = np.random.default_rng(5000 + seed)
    f = rng.uniform(0.3, 2.5, (4, FEAT))
    a = rng.uniform(0.05, 0.4, (4, FEAT)) * 0.3
    p = rng.uniform(0.0, 2 * np.pi, (4, FEAT))
    t = np.arange(T)[:, None, None] / FPS
    x = (motion(seed, T).astype(np.float64) + (a * np.sin(2 * np.pi * f * t + p)).sum(axis=1)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def semantic_of(seed, T=128):
    s = np.random.default_rng(7000 + seed).uniform(0.0, 1.0, T).astype(np.float32)
    s.setflags(write=False)
    return s


def onsets_of(seed, count, T=128):
    """float64 [count]: sorted seeded onset times inside the sequence."""
    return np.sort(np.random.default_rng(9000 + seed).uniform(0.0, (T - 1) / FPS, count))


ONSET_COUNTS = (0, 1, 7, 7, 1)      # per sequence of a batch, cycled


# ------------------------------------------------------------------ per-sequence metrics
def l1div_partial(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return np.abs(x - x.mean(axis=0)).sum(dtype=dtype)


def srgr_partial(pred, target, semantic, threshold=THRESHOLD, dtype=np.float64):
    """(the weighted sum over frames and joints, the number of successes, the smallest distance of a comparison from the threshold)"""
    p = np.asarray(pred, dtype=dtype).reshape(-1, JOINTS, 3)
    t = np.asarray(target, dtype=dtype).reshape(-1, JOINTS, 3)
    diff = np.abs(p - t).sum(axis=2, dtype=dtype)
    ok = diff < dtype(threshold)
    w = np.asarray(semantic, dtype=dtype).reshape(-1) * dtype(SEMANTIC_SCALE)
    return (ok * w[:, None]).sum(dtype=dtype), int(ok.sum()), float(np.abs(diff.astype(np.float64) - threshold).min())


def jitter_sum(pred, target, dtype=np.float64):
    p, t = np.asarray(pred, dtype=dtype), np.asarray(target, dtype=dtype)
    return np.abs(np.abs(p[1:] - p[:-1]) - np.abs(t[1:] - t[:-1])).sum(dtype=dtype)


def speeds(x, dtype=np.float64):
    """[6, T - 1]: the frame-to-frame speed of the six tracked joints."""
    x = np.asarray(x, dtype=dtype).reshape(-1, JOINTS, 3)
    v = x[1:, TRACK_JOINTS, :] - x[:-1, TRACK_JOINTS, :]
    return np.sqrt((v * v).sum(axis=2, dtype=dtype)).T


def beats(x, order, dtype=np.float64):
    """(uint8 [6, T - 1], the smallest |min over the compared neighbours - v[i]| / max(v) over all decisions): i is a beat iff v[i] is
    strictly below v[clip(i +- s)] for every s = 1 .. order."""
    v = speeds(x, dtype)
    n = v.shape[1]
    idx = np.arange(n)
    lowest = np.full(v.shape, np.inf)
    for s in range(1, order + 1):
        lowest = np.minimum(lowest, np.minimum(v[:, np.clip(idx - s, 0, n - 1)], v[:, np.clip(idx + s, 0, n - 1)]))
    margin = (np.abs(lowest - v) / v.max(axis=1, keepdims=True))
    # a frame compared with itself (i - s or i + s clipped onto i) is no decision: the difference is exactly 0 in every precision
    self_cmp = (idx < 1) | (idx > n - 2)
    return (v < lowest).astype(np.uint8), float(margin[:, ~self_cmp].min())


def align_score(wrist_beats, onsets, sigma, fps=FPS, dtype=np.float64):
    """The mean over onsets of exp(-d^2 / 2 sigma^2), d to the nearest beat time; no beats: 0.  None without onsets."""
    onsets = np.asarray(onsets, dtype=dtype)
    if onsets.size == 0:
        return None
    times = np.nonzero(wrist_beats)[0].astype(dtype) / dtype(fps)
    if times.size == 0:
        return dtype(0)
    d = np.abs(onsets[:, None] - times[None, :]).min(axis=1)
    return np.exp(-(d * d) / dtype(2 * sigma * sigma)).mean(dtype=dtype)


def process_motion(x, dtype=np.float64):
    """[T, 189] -> [T, 189]: floor, XZ origin, facing +z from joints 18 13 9 5 of frame 0, root-relative joints, wrist-relative hands."""
    m = np.array(x, dtype=dtype).reshape(-1, JOINTS, 3)
    m[:, :, 1] -= m[:, :, 1].min()
    first = m[0].copy()
    m = m - first[0] * np.array([1, 0, 1], dtype=dtype)
    across = (first[18] - first[13]) + (first[9] - first[5])
    across = across / np.sqrt((across * across).sum(dtype=dtype))
    fwd = np.cross(np.array([0, 1, 0], dtype=dtype), across)
    fwd = fwd / np.sqrt((fwd * fwd).sum(dtype=dtype))
    z = np.array([0, 0, 1], dtype=dtype)
    q = np.concatenate([[np.sqrt((fwd * fwd).sum(dtype=dtype) * (z * z).sum(dtype=dtype)) + (fwd * z).sum(dtype=dtype)], np.cross(fwd, z)]).astype(dtype)
    q = q / np.sqrt((q * q).sum(dtype=dtype))
    uv = np.cross(q[1:], m)
    uuv = np.cross(q[1:], uv)
    m = (m + dtype(2) * (q[0] * uv + uuv)).astype(dtype)
    m[:, 1:] = m[:, 1:] - m[:, :1]
    m[:, 23:43] = m[:, 23:43] - m[:, 7:8]
    m[:, 43:] = m[:, 43:] - m[:, 11:12]
    return m.reshape(-1, FEAT)


def avg_distance(rows, dtype=np.float64):
    """The mean over all pairs i < j of the Euclidean distance between rows [N, D], from the differences."""
    r = np.asarray(rows, dtype=dtype).reshape(len(rows), -1)
    total, n = dtype(0), r.shape[0]
    for i in range(n - 1):
        d = r[i + 1:] - r[i]
        total += np.sqrt((d * d).sum(axis=1, dtype=dtype)).sum(dtype=dtype)
    return total / dtype(n * (n - 1) / 2)


# ------------------------------------------------------------------ the embedding net
def _leaky(x, slope):
    return np.where(x >= 0, x, x * x.dtype.type(slope))


def make_fgd_state(F, seed):
    """A seeded state dict (numpy float32) with HalfEmbeddingNet's pose-encoder keys: weights N(0, 1 / fan_in), BatchNorm statistics away
    from their defaults."""
    rng = np.random.default_rng(seed)
    s = {}

    def lin(name, shape):
        fan = int(np.prod(shape[1:]))
        s[name + ".weight"] = (rng.standard_normal(shape) / np.sqrt(fan)).astype(np.float32)
        s[name + ".bias"] = (0.1 * rng.standard_normal(shape[0])).astype(np.float32)

    def bn(name, n):
        s[name + ".weight"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
        s[name + ".bias"] = (0.1 * rng.standard_normal(n)).astype(np.float32)
        s[name + ".running_mean"] = (0.1 * rng.standard_normal(n)).astype(np.float32)
        s[name + ".running_var"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
        s[name + ".num_batches_tracked"] = np.array(7, dtype=np.int64)
    p = "pose_encoder."
    for i, (cin, cout, k) in enumerate(((FEAT, F, 3), (F, 2 * F, 3), (2 * F, 2 * F, 4))):
        lin(f"{p}net.{i}.0", (cout, cin, k))
        bn(f"{p}net.{i}.1", cout)
    lin(p + "net.3", (F, 2 * F, 3))
    for i, (cin, cout) in zip((0, 3, 6, 9), ((59 * F, 20 * F), (20 * F, 4 * F), (4 * F, 2 * F), (2 * F, F))):
        lin(f"{p}out_net.{i}", (cout, cin))
        if i < 9:
            bn(f"{p}out_net.{i + 1}", cout)
    lin(p + "fc_mu", (F, F))
    lin(p + "fc_logvar", (F, F))
    return s


def _bn(x, s, name, axis, dtype):
    shape = [1] * x.ndim
    shape[axis] = -1
    g, b, m, v = (s[f"{name}.{k}"].astype(dtype).reshape(shape) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(v + dtype(1e-5)) * g + b


def _conv(x, w, b, stride, dtype):
    """x [B, T, C], w [N, C, k] -> [B, T', N]"""
    k = w.shape[2]
    n = (x.shape[1] - k) // stride + 1
    win = np.stack([x[:, j:j + stride * (n - 1) + 1:stride] for j in range(k)], axis=2)      # [B, n, k, C]
    return np.einsum("bnkc,ock->bno", win, w.astype(dtype), optimize=True).astype(dtype) + b.astype(dtype)


def embed(state, x, dtype=np.float64):
    """HalfEmbeddingNet.forward in eval mode, layer by layer (nothing folded): x [B, 128, 189] -> mu [B, F]."""
    p = "pose_encoder."
    h = np.asarray(x, dtype=dtype)
    for i, stride in enumerate((1, 1, 2)):
        h = _conv(h, state[f"{p}net.{i}.0.weight"], state[f"{p}net.{i}.0.bias"], stride, dtype)
        h = _leaky(_bn(h, state, f"{p}net.{i}.1", 2, dtype), 0.2)
    h = _conv(h, state[p + "net.3.weight"], state[p + "net.3.bias"], 1, dtype)
    h = h.transpose(0, 2, 1).reshape(h.shape[0], -1)                                         # flatten(1) of [B, F, 59]
    for i in (0, 3, 6, 9):
        h = h @ state[f"{p}out_net.{i}.weight"].astype(dtype).T + state[f"{p}out_net.{i}.bias"].astype(dtype)
        if i < 9:
            h = _leaky(_bn(h, state, f"{p}out_net.{i + 1}", 1, dtype), 1.0)
    return h @ state[p + "fc_mu.weight"].astype(dtype).T + state[p + "fc_mu.bias"].astype(dtype)


def make_folded_parts(F, seed):
    """A seeded FOLDED pack (float32), for widths at which a whole state dict is too large to make in a test: [(W [N, K], b [N]) x 5]."""
    rng = np.random.default_rng(seed)
    parts = []
    for n, k in ((F, 3 * FEAT), (2 * F, 3 * F), (2 * F, 8 * F), (F, 6 * F), (F, 59 * F)):
        parts.append(((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)))
    return parts


def embed_folded(parts, x, dtype=np.float64):
    """The folded net: four products over overlapping frame-major windows (row stride C, 2 C for the third) and one affine map."""
    h = np.asarray(x, dtype=dtype)
    for (w, b), k, stride, slope in zip(parts[:4], (3, 3, 4, 3), (1, 1, 2, 1), (0.2, 0.2, 0.2, 1.0)):
        n = (h.shape[1] - k) // stride + 1
        win = np.concatenate([h[:, j:j + stride * (n - 1) + 1:stride] for j in range(k)], axis=2)   # [B, n, k C]
        h = _leaky((win @ w.astype(dtype).T).astype(dtype) + b.astype(dtype), slope)
    w, b = parts[4]
    return h.reshape(h.shape[0], -1) @ w.astype(dtype).T + b.astype(dtype)


# ------------------------------------------------------------------ Frechet distance
def stats_of(e):
    """[n | sum e | sum e e^T] in float64."""
    e = np.asarray(e, dtype=np.float64)
    return np.concatenate([[e.shape[0]], e.sum(axis=0), (e.T @ e).reshape(-1)])


def frechet(ea, eb):
    """From the samples: means, np.cov (ddof = 1), the matrix square root of the product by eigen-decomposition of the symmetrised form
    (a restatement that needs no scipy: tr sqrt(S1 S2) = sum of the square roots of the eigenvalues of S1^(1/2) S2 S1^(1/2))."""
    ea, eb = np.asarray(ea, dtype=np.float64), np.asarray(eb, dtype=np.float64)
    m1, m2 = ea.mean(axis=0), eb.mean(axis=0)
    s1, s2 = np.cov(ea, rowvar=False), np.cov(eb, rowvar=False)
    w, v = np.linalg.eigh(s1)
    r1 = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    ev = np.linalg.eigvalsh(r1 @ s2 @ r1)
    d = m1 - m2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(ev, 0, None)).sum())


def rel(got, want):
    """max |got - want| / max |want|"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())
