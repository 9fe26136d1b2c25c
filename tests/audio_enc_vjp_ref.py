"""AudioConvEncoder's forward and backward pass restated in numpy -- TEST INFRASTRUCTURE, the oracle of ``cfd_audio_encoder_vjp``.

Linear(in, hidden), LeakyReLU(0.1), Linear(hidden, latent), LeakyReLU(0.1), Linear(latent, latent), dropout the identity; the slope of
LeakyReLU at exactly 0 is 0.1 (torch's convention).  ``encoder_vjp`` runs at the dtype it is given: float64 is the oracle, float32 (numpy's
own float32 products) is the yardstick a float32 unit is held to -- the gate is ``GATE`` times what that run loses against float64 on the
same inputs.  tests/test_audio_enc_vjp_host.py checks the restatement against torch autograd at float64.
"""
import numpy as np

KEYS = ("main.0.weight", "main.0.bias", "main.3.weight", "main.3.bias", "out_net.weight", "out_net.bias")
GATE = 4.0      # the project's margin for its float32 units: the error of the float32 restatement on the same inputs, times 4


def leaky(z):
    return np.where(z > 0, z, z.dtype.type(0.1) * z)


def slope(z):
    return np.where(z > 0, z.dtype.type(1.0), z.dtype.type(0.1))


def encoder_vjp(x, params, d_out, dtype=np.float64):
    """``x [rows, in]``, ``params`` {state-dict key: array}, ``d_out [rows, latent]`` -> {"out", "d_x", and every key's gradient}, all
    computed at ``dtype`` from the inputs cast to it."""
    x, g = np.asarray(x, dtype=dtype), np.asarray(d_out, dtype=dtype)
    w0, b0, w1, b1, w2, b2 = (np.asarray(params[k], dtype=dtype) for k in KEYS)
    z1 = x @ w0.T + b0
    h1 = leaky(z1)
    z2 = h1 @ w1.T + b1
    h2 = leaky(z2)
    r = {"out": h2 @ w2.T + b2}
    r["out_net.weight"], r["out_net.bias"] = g.T @ h2, g.sum(axis=0)
    dz2 = (g @ w2) * slope(z2)
    r["main.3.weight"], r["main.3.bias"] = dz2.T @ h1, dz2.sum(axis=0)
    dz1 = (dz2 @ w1) * slope(z1)
    r["main.0.weight"], r["main.0.bias"] = dz1.T @ x, dz1.sum(axis=0)
    r["d_x"] = dz1 @ w0
    return r


def rel_l2(a, b):
    """|a - b| / |b|; 0 where both vanish, inf where only the reference does."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d, n = np.linalg.norm(a - b), np.linalg.norm(b)
    if n == 0:
        return 0.0 if d == 0 else float("inf")
    return float(d / n)


def seeded_params(in_dim, hidden, latent, seed, zero_bias=False):
    """Parameters as nn.Linear's default init draws them (uniform in +-1 / sqrt(fan_in)), float32, from a numpy generator."""
    r = np.random.Generator(np.random.PCG64(seed))
    p = {}
    for (kw, kb), (n, k) in zip((KEYS[0:2], KEYS[2:4], KEYS[4:6]), ((hidden, in_dim), (latent, hidden), (latent, latent))):
        a = 1.0 / np.sqrt(k)
        p[kw] = r.uniform(-a, a, (n, k)).astype(np.float32)
        p[kb] = np.zeros(n, np.float32) if zero_bias else r.uniform(-a, a, n).astype(np.float32)
    return p


def seeded_inputs(rows, in_dim, latent, seed):
    """(Mel-dB-like rows, a cotangent of the size a mean-squared error's is), float32."""
    r = np.random.Generator(np.random.PCG64(seed))
    x = (-40.0 + 25.0 * r.standard_normal((rows, in_dim))).astype(np.float32)
    d = (r.standard_normal((rows, latent)) / (rows * latent)).astype(np.float32)
    return x, d


def gate_report(got, x, params, d_out, names):
    """[(name, error of ``got`` against float64, error of the float32 restatement against float64)] for every name of ``names``."""
    want = encoder_vjp(x, params, d_out, np.float64)
    f32 = encoder_vjp(x, params, d_out, np.float32)
    return [(n, rel_l2(got[n], want[n]), rel_l2(f32[n], want[n])) for n in names]
