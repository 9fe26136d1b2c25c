"""-m gpu: the split-pair GEMM's epilogues (csrc/gemm_sp.hpp) against float64, one launch at a time (cfd_test_gemm_epi).

Covers what the product launches besides the plain float32 store of test_gpu_kernels.py: the bias store, the split-pair store with GELU and
the P-fragment column order, the residual update, the LayerNorm fold's producer (residual + split copy + slot statistics) and consumers
(EpiLn<E>), and the fused q | k | v^T store -- at ragged J, at K of one and two k-tiles (the 3-stage prologue's special cases) and in every
tile class the product reaches.  Split-pair outputs are decoded here from the stored bytes (per row and 32-column block: 32 fp16 hi, then
32 fp16 lo), so the layout is checked too.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U22 = 2.0 ** -22          # the split pair's operand error (fp16 hi + lo)
U24 = 2.0 ** -24
E_ARG = -1                # CFD_E_ARG
C_FOLD = 2                # the fold's error model: |err| <= C_FOLD 2^-22 (1 + |mu| / sqrt(var + eps)) x the row norms (measured: <= 0.74)
ROWS = 512                # features of a residual row (CFD_D)


@pytest.fixture(scope="module")
def ops():
    import torch
    from convofusion_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load(), _lib.create_handle(0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _launch(ops, kind, I, J, K, **kw):
    """One cfd_test_gemm_epi call; returns (status, tile class launched).  Tensors in kw are device tensors."""
    import torch
    from convofusion_amd import _lib
    lib, h = ops
    a = _lib.TestEpiArgs()
    a.kind, a.I, a.J, a.K = kind, I, J, K
    a.tile_cfg, a.gelu, a.perm32, a.natural = kw.get("cfg", 0), kw.get("gelu", 0), kw.get("perm32", 0), kw.get("natural", 0)
    a.ln_eps = kw.get("eps", 1e-5)
    for f in ("X", "Y", "y_sp", "bias", "gamma", "beta", "ln_stat", "x", "out", "out2", "stat"):
        setattr(a, f, _ptr(kw.get(f)))
    a.tile_cfg_used = -1
    r = lib.cfd_test_gemm_epi(h, C.byref(a), None)
    torch.cuda.synchronize()
    return r, a.tile_cfg_used


def _ok(ops, kind, I, J, K, **kw):
    from convofusion_amd import _lib
    r, used = _launch(ops, kind, I, J, K, **kw)
    _lib.check(r)
    return used


def sp_decode(raw, ncol):
    """Stored split pairs (uint8 [..., ncol * 4]) -> float64 hi + lo, and the hi / lo planes."""
    h = np.ascontiguousarray(raw).view(np.float16).reshape(raw.shape[:-1] + (ncol // 32, 2, 32))
    hi, lo = h[..., 0, :].reshape(raw.shape[:-1] + (ncol,)), h[..., 1, :].reshape(raw.shape[:-1] + (ncol,))
    return hi.astype(np.float64) + lo.astype(np.float64), hi, lo


def _sp_buf(rows, ncol, fill=0xFF):
    import torch
    return torch.full((rows, ncol * 4), fill, dtype=torch.uint8, device="cuda")


def gelu64(v):
    import torch
    return 0.5 * v * (1.0 + torch.special.erf(torch.from_numpy(v / np.sqrt(2.0))).numpy())


def _norms(Y, X):
    return np.sqrt((Y.astype(np.float64) ** 2).sum(1)), np.sqrt((X.astype(np.float64) ** 2).sum(1))


def _operands(rng, I, J, K, spread=True):
    X = rng.standard_normal((I, K)).astype(np.float32)
    Y = rng.standard_normal((J, K)) * (rng.uniform(0.01, 30, (J, 1)) if spread else 1.0)
    return X, Y.astype(np.float32), rng.standard_normal(I).astype(np.float32)


def _check(got, want, scale, what, bound=1e-5, extra=0.0):
    assert np.isfinite(got).all(), what
    err = np.abs(got - want) / scale
    lim = bound + extra / scale
    bad = err > lim
    assert not bad.any(), (what, float(err.max()), np.argwhere(bad)[:5].tolist())


# shapes: every J of the ragged-edge set and K in {32, 64, 512, 2048} (one / two k-tiles: the 3-stage prologue's special cases)
SHAPES = [(1, 32), (15, 64), (16, 512), (17, 2048), (63, 32), (65, 64), (1120, 512), (3584, 64)]


# ---- EpiF32 with a bias, every class ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [0, 1, 3, 6, 19, 20, 24])
@pytest.mark.parametrize("J,K", SHAPES)
def test_f32_bias(ops, cfg, J, K):
    import torch
    from convofusion_amd import _lib
    I = 192 if cfg == 20 else 320          # (ragged in I as well: 320 = 2.5 tiles of 128)
    rng = np.random.default_rng(J * 31 + K + cfg)
    X, Y, b = _operands(rng, I, J, K)
    out = torch.full((J + 3, I), float("nan"), dtype=torch.float32, device="cuda")
    _ok(ops, _lib.EPI_F32, I, J, K, cfg=cfg, X=_dev(X), Y=_dev(Y), bias=_dev(b), out=out)
    got = out.cpu().numpy()
    want = Y.astype(np.float64) @ X.astype(np.float64).T + b
    ny, nx = _norms(Y, X)
    _check(got[:J], want, ny[:, None] * nx[None, :] + np.abs(b)[None, :], "f32", extra=U24 * np.abs(want))
    assert np.isnan(got[J:]).all(), "rows beyond J written"


# ---- EpiSplit: bias, split store, classes 0 / 1 / 19 / 24 -------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [0, 1, 19, 24])
@pytest.mark.parametrize("J,K", SHAPES)
def test_split_bias(ops, cfg, J, K):
    from convofusion_amd import _lib
    I = 320
    rng = np.random.default_rng(J * 37 + K + cfg)
    X, Y, b = _operands(rng, I, J, K)
    out = _sp_buf(J + 2, I)
    _ok(ops, _lib.EPI_SPLIT, I, J, K, cfg=cfg, X=_dev(X), Y=_dev(Y), bias=_dev(b), out=out)
    raw = out.cpu().numpy()
    got, _, _ = sp_decode(raw[:J], I)
    want = Y.astype(np.float64) @ X.astype(np.float64).T + b
    ny, nx = _norms(Y, X)
    _check(got, want, ny[:, None] * nx[None, :] + np.abs(b)[None, :], "split", extra=U22 * np.abs(want))
    assert (raw[J:] == 0xFF).all(), "rows beyond J written"


def _exact_preact(rng, I, J):
    """X selects one column of Y per feature (K = 32); Y (multiples of 2^-10 in [-10, 10]) and the bias (multiples of 2^-6) carry at most
    15 significant bits: the split pairs, the product and the pre-activation D + bias are exact, and so is its split-pair store."""
    K = 32
    X = np.zeros((I, K), np.float32)
    X[np.arange(I), rng.permutation(np.arange(I)) % K] = 1.0
    Y = (rng.integers(-10240, 10241, (J, K)) / 1024.0).astype(np.float32)
    b = (rng.integers(-64, 65, I) / 64.0).astype(np.float32)
    v = Y.astype(np.float64) @ X.astype(np.float64).T + b
    return X, Y, b, v


def test_split_gelu_matches_erf_gelu(ops):
    """EpiSplit + GELU over pre-activations in [-10, 10]: |gelu_fast_f - erf GELU| <= 0.75e-7 |x| (the comment's claim) + split rounding."""
    from convofusion_amd import _lib
    rng = np.random.default_rng(5)
    I, J = 256, 1120
    X, Y, b, v = _exact_preact(rng, I, J)
    out = _sp_buf(J, I)
    _ok(ops, _lib.EPI_SPLIT, I, J, 32, gelu=1, X=_dev(X), Y=_dev(Y), bias=_dev(b), out=out)
    got, _, _ = sp_decode(out.cpu().numpy(), I)
    want = gelu64(v)
    err = np.abs(got - want)
    # hi + lo of the stored float32 value (lo may be an fp16 subnormal), and a few float32 roundings of the formula itself
    split = U22 * np.abs(want) + 4 * U24 * np.abs(want) + 2.0 ** -25
    excess = np.maximum(err - split, 0) / np.maximum(np.abs(v), 1e-30)
    print(f"\nGELU: max |err| - split rounding = {excess.max():.3g} |x| (claim 0.75e-7 |x|); max |err| {err.max():.3g}")
    assert np.isfinite(got).all()
    assert (err <= 0.75e-7 * np.abs(v) + split).all(), (float(excess.max()), np.argwhere(err > 0.75e-7 * np.abs(v) + split)[:5].tolist())


def test_split_perm32_column_order(ops):
    """perm32: column 32 S + 16 h + 4 q + r is stored at position 32 S + 8 q + 4 h + r (the P-fragment k-slot order)."""
    from convofusion_amd import _lib
    rng = np.random.default_rng(6)
    I, J = 128, 65
    X, Y, b, v = _exact_preact(rng, I, J)
    out = _sp_buf(J, I)
    _ok(ops, _lib.EPI_SPLIT, I, J, 32, perm32=1, X=_dev(X), Y=_dev(Y), bias=_dev(b), out=out)
    got, _, _ = sp_decode(out.cpu().numpy(), I)
    col = np.arange(I)
    S, h, q, r = col // 32, (col // 16) % 2, (col // 4) % 4, col % 4
    pos = 32 * S + 8 * q + 4 * h + r
    assert sorted(pos.tolist()) == col.tolist()
    np.testing.assert_array_equal(got[:, pos], v)          # (exact pre-activation, no GELU: the store is exact too)


# ---- EpiResid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [0, 1, 19, 24])
@pytest.mark.parametrize("J,K", SHAPES)
def test_resid(ops, cfg, J, K):
    from convofusion_amd import _lib
    rng = np.random.default_rng(J * 41 + K + cfg)
    X, Y, b = _operands(rng, ROWS, J, K)
    x0 = (rng.standard_normal((J, ROWS)) * 3).astype(np.float32)
    x = _dev(np.concatenate([x0, np.full((2, ROWS), np.nan, np.float32)]))
    _ok(ops, _lib.EPI_RESID, ROWS, J, K, cfg=cfg, X=_dev(X), Y=_dev(Y), bias=_dev(b), x=x)
    got = x.cpu().numpy()
    want = x0.astype(np.float64) + Y.astype(np.float64) @ X.astype(np.float64).T + b
    ny, nx = _norms(Y, X)
    _check(got[:J], want, ny[:, None] * nx[None, :] + np.abs(b)[None, :], "resid", extra=2 * U24 * (np.abs(want) + np.abs(x0)))
    assert np.isnan(got[J:]).all(), "rows beyond J written"


# ---- EpiResidStat: the fold's producer -------------------------------------------------------------------------------------------------
def slot_stats(x):
    """float64 (mean, M2) per row and 32-column slot of float32 rows [J][512]."""
    s = x.astype(np.float64).reshape(x.shape[0], ROWS // 32, 32)
    m = s.mean(-1)
    return m, ((s - m[..., None]) ** 2).sum(-1)


def _producer(ops, rng, J, K, x0, guard=2):
    """One EpiResidStat launch on rows x0 [J][512]; returns x_new, the raw split copy, the statistics and the class, plus device buffers."""
    import torch
    from convofusion_amd import _lib
    X = (rng.standard_normal((ROWS, K)) / np.sqrt(K)).astype(np.float32)
    Y = rng.standard_normal((J, K)).astype(np.float32)
    b = (rng.standard_normal(ROWS) * 0.1).astype(np.float32)
    x = _dev(np.concatenate([x0, np.full((guard, ROWS), np.nan, np.float32)]))
    xs = _sp_buf(J + guard, ROWS)
    st = torch.full((J + guard, ROWS // 32, 2), float("nan"), dtype=torch.float32, device="cuda")
    used = _ok(ops, _lib.EPI_RESID_STAT, ROWS, J, K, X=_dev(X), Y=_dev(Y), bias=_dev(b), x=x, out=xs, stat=st)
    return dict(X=X, Y=Y, b=b, x=x, xs=xs, stat=st, used=used)


@pytest.mark.parametrize("J,K", [(1, 32), (15, 64), (17, 2048), (65, 512), (1120, 512), (3584, 2048), (6208, 64)])
def test_resid_stat_producer(ops, J, K):
    rng = np.random.default_rng(J + K)
    x0 = (rng.standard_normal((J, ROWS)) * rng.uniform(0.5, 4, (J, 1)) + rng.uniform(-50, 50, (J, 1))).astype(np.float32)
    p = _producer(ops, rng, J, K, x0)
    assert p["used"] == (24 if 8 * -(-J // 64) > 768 else 19), p["used"]      # launch_gemm_midsize's rule at I = 512
    xn = p["x"].cpu().numpy()
    want = x0.astype(np.float64) + p["Y"].astype(np.float64) @ p["X"].astype(np.float64).T + p["b"]
    ny, nx = _norms(p["Y"], p["X"])
    _check(xn[:J], want, ny[:, None] * nx[None, :] + np.abs(p["b"])[None, :], "x", extra=2 * U24 * (np.abs(want) + np.abs(x0)))
    assert np.isnan(xn[J:]).all(), "x rows beyond J written"
    # the split copy: bit for bit what split_f32 makes of the returned rows
    raw = p["xs"].cpu().numpy()
    _, hi, lo = sp_decode(raw[:J], ROWS)
    x32 = xn[:J]
    whi = np.clip(x32, -65504, 65504).astype(np.float16)
    wlo = (np.clip(x32, -65504, 65504) - whi.astype(np.float32)).astype(np.float16)
    np.testing.assert_array_equal(hi.view(np.uint16), whi.view(np.uint16))
    np.testing.assert_array_equal(lo.view(np.uint16), wlo.view(np.uint16))
    assert (raw[J:] == 0xFF).all(), "split rows beyond J written"
    # every (mean, M2) slot, against float64 statistics of the same float32 rows
    st = p["stat"].cpu().numpy()
    m, m2 = slot_stats(x32)
    asum = np.abs(x32.astype(np.float64)).reshape(J, 16, 32).sum(-1)
    dm = 8 * U24 * asum / 32                                     # (a 5-level summation tree, then the scale)
    np.testing.assert_array_less(np.abs(st[:J, :, 0] - m), dm + 1e-30)
    np.testing.assert_array_less(np.abs(st[:J, :, 1] - m2), 16 * U24 * m2 + 64 * dm ** 2 + 1e-30)
    assert np.isnan(st[J:]).all(), "statistics beyond J written"


# ---- the fold's consumers: EpiLn<EpiF32>, EpiLn<EpiSplit> + GELU ------------------------------------------------------------------------
EPS = 1e-5
OFFSETS = (0, 25, 100, 1000)


def fold_rows(rng, J):
    """Rows [J][512] whose mean / deviation ratios cycle through OFFSETS, with the hard cases in front: an exactly constant row, two halves
    far apart, one massive feature (column 40: inside the product from K = 64 on)."""
    sig = rng.uniform(0.5, 4, J)
    off = np.array([OFFSETS[j % len(OFFSETS)] for j in range(J)], np.float64) * rng.choice([-1, 1], J)
    x = rng.standard_normal((J, ROWS)) * sig[:, None] + (off * sig)[:, None]
    if J >= 4:
        x[0] = 1.5
        x[1] = rng.standard_normal(ROWS)
        x[1, :256] -= 1000.0
        x[1, 256:] += 1000.0
        x[2] = rng.standard_normal(ROWS)
        x[2, 40] = 1000.0
        x[3] = rng.standard_normal(ROWS) * 0.5 - 2.0
    return x.astype(np.float32)


def ln_ref(x, gamma, beta, K):
    x = x.astype(np.float64)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    z = (x - mu) / np.sqrt(var + EPS)
    return z[:, :K] * gamma + beta, z[:, :K], (np.abs(mu) / np.sqrt(var + EPS))[:, 0]


def _fold_weights(rng, I, K):
    W = (rng.standard_normal((I, K)) / np.sqrt(K)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, K).astype(np.float32)
    beta = (rng.standard_normal(K) * 0.2).astype(np.float32)
    b = (rng.standard_normal(I) * 0.1).astype(np.float32)
    return W, gamma, beta, b


def fold_scale(z, W, gamma, beta, b, K):
    """|got - want| is measured in units of ||LN(x)_j|| ||W'_i|| + |d_i + b_i| (||LN(x)_j|| at least its typical sqrt(K): an exactly
    constant row has none)."""
    Wf = W.astype(np.float64) * gamma
    zn = np.maximum(np.sqrt((z ** 2).sum(1)), np.sqrt(K))
    return zn[:, None] * np.sqrt((Wf ** 2).sum(1))[None, :] + np.abs(W.astype(np.float64) @ beta + b)[None, :]


def midsize_class(I_groups, J):
    t64 = sum(-(-I // 64) for I in I_groups) * -(-J // 64)
    return 24 if t64 > 768 and max(I_groups) >= 128 else 19


def _report(tag, err_n, off, const_row=False):
    """Per-row worst normalized error in units of 2^-22 against |mu| / sigma; prints the fitted slope, asserts the model."""
    e = err_n.max(1) / U22
    A = np.stack([np.ones_like(off), off], 1)
    c0, slope = np.linalg.lstsq(A, e, rcond=None)[0]
    worst = (e / (1 + off)).max()
    groups = "  ".join(f"{o:g}:{e[np.isclose(off, o, rtol=0.05)].max():.3g}" for o in OFFSETS if np.isclose(off, o, rtol=0.05).any())
    print(f"\n{tag}: err/2^-22 = {c0:.3g} + {slope:.3g} |mu|/sigma (fit); worst err/(2^-22 (1 + |mu|/sigma)) = {worst:.3g} "
          f"(model C = {C_FOLD}); per offset {groups}" + (f"; constant row (|mu|/sigma = {off[0]:.3g}): {e[0]:.3g}" if const_row else ""))
    bad = e > C_FOLD * (1 + off)
    assert not bad.any(), (tag, np.argwhere(bad)[:5, 0].tolist(), e[bad][:5].tolist(), off[bad][:5].tolist())


def _poison(ops, kind, I, J, out_dev, **kw):
    """A K = 64 fold launch of the same class on other rows (mean 50, deviation 0.01): leaves (mu, r_sigma) of those rows behind in LDS, so
    that a K = 32 launch that did not write its own reads wrong ones."""
    from convofusion_amd import _lib
    rng = np.random.default_rng(99)
    xp = (50 + 0.01 * rng.standard_normal((J, ROWS))).astype(np.float32)
    m, m2 = slot_stats(xp)
    st = _dev(np.stack([m, m2], -1).astype(np.float32))
    Wp = _dev((rng.standard_normal((I, 64)) / 8).astype(np.float32))
    g = _dev(np.ones(64, np.float32))
    _ok(ops, kind, I, J, 64, X=Wp, Y=_dev(xp[:, :64]), gamma=g, beta=g, ln_stat=st, out=out_dev, **kw)


@pytest.mark.parametrize("kind,I,J", [("f32", 128, 1), ("f32", 128, 17), ("f32", 128, 1120), ("split", 1024, 65), ("split", 1024, 1120),
                                      ("split", 1024, 3584)])
@pytest.mark.parametrize("K", [32, 64, 512])
def test_ln_fold_consumer_fed_statistics(ops, kind, I, J, K):
    """EpiLn<EpiF32> / EpiLn<EpiSplit> + GELU with statistics made in numpy, against LayerNorm(x) @ W^T + b in float64."""
    import torch
    from convofusion_amd import _lib
    rng = np.random.default_rng(I + J + K)
    x = fold_rows(rng, J)
    W, gamma, beta, b = _fold_weights(rng, I, K)
    m, m2 = slot_stats(x)
    st = _dev(np.stack([m, m2], -1).astype(np.float32))
    ekind = _lib.EPI_LN_F32 if kind == "f32" else _lib.EPI_LN_SPLIT
    kw = dict(gelu=1) if kind == "split" else {}
    mk = (lambda: torch.full((J, I), float("nan"), dtype=torch.float32, device="cuda")) if kind == "f32" else (lambda: _sp_buf(J, I))
    _poison(ops, ekind, I, J, mk(), **kw)
    out = mk()
    used = _ok(ops, ekind, I, J, K, X=_dev(W), Y=_dev(x[:, :K]), bias=_dev(b), gamma=_dev(gamma), beta=_dev(beta), ln_stat=st, out=out, **kw)
    assert used == midsize_class([I], J), used
    print(f"\nfold {kind} I={I} J={J} K={K}: class {used}")
    y, z, off = ln_ref(x, gamma, beta, K)
    pre = y @ W.astype(np.float64).T + b
    scale = fold_scale(z, W, gamma, beta, b, K)
    if kind == "f32":
        got, want, extra = out.cpu().numpy().astype(np.float64), pre, U24 * np.abs(pre)
    else:
        got, want = sp_decode(out.cpu().numpy(), I)[0], gelu64(pre)
        extra = 0.75e-7 * np.abs(pre) + U22 * np.abs(want) + 2.0 ** -25
    assert np.isfinite(got).all()
    _report(f"fold {kind} I={I} J={J} K={K} class {used}", np.maximum(np.abs(got - want) - extra, 0) / scale, off, const_row=J >= 4)


@pytest.mark.parametrize("J", [1120, 3584])
def test_ln_fold_chained_producer_consumer(ops, J):
    """As the product runs it: EpiResidStat (K = 2048, the second FFN product) leaves raw rows, their split copy and the slot statistics;
    EpiLn<EpiSplit> + GELU (FFN1, I = 1024) consumes them."""
    from convofusion_amd import _lib
    rng = np.random.default_rng(J)
    x0 = fold_rows(rng, J)
    x0[0] = rng.standard_normal(ROWS)            # (the producer adds to every row: no constant row survives it)
    p = _producer(ops, rng, J, 2048, x0)
    I, K = 1024, ROWS
    W, gamma, beta, b = _fold_weights(rng, I, K)
    out = _sp_buf(J, I)
    used = _ok(ops, _lib.EPI_LN_SPLIT, I, J, K, gelu=1, X=_dev(W), y_sp=p["xs"], bias=_dev(b), gamma=_dev(gamma), beta=_dev(beta),
               ln_stat=p["stat"], out=out)
    assert used == midsize_class([I], J), used
    xn = p["x"].cpu().numpy()[:J]
    y, z, off = ln_ref(xn, gamma, beta, K)
    pre = y @ W.astype(np.float64).T + b
    got, want = sp_decode(out.cpu().numpy(), I)[0], gelu64(pre)
    assert np.isfinite(got).all()
    extra = 0.75e-7 * np.abs(pre) + U22 * np.abs(want) + 2.0 ** -25
    _report(f"chained fold J={J} class {used}", np.maximum(np.abs(got - want) - extra, 0) / fold_scale(z, W, gamma, beta, b, K), off)


# ---- EpiQkvT: q | k and the transposed value store, plain and under the fold ------------------------------------------------------------
def vts_positions(natural):
    """Key position of token t of a 16-token row in the 32-key block."""
    t = np.arange(16)
    return t if natural else 8 * (t // 4) + t % 4


def _check_qkvt(qk_raw, vts_raw, J, want_qk, want_v, scale_qk, scale_v, natural, tag, off=None, const_row=False):
    got_qk = sp_decode(qk_raw, 1024)[0]
    assert np.isfinite(got_qk).all(), tag
    e_qk = np.maximum(np.abs(got_qk - want_qk) - U22 * np.abs(want_qk), 0) / scale_qk
    v, hi, lo = sp_decode(vts_raw.reshape(J // 16, ROWS, 128), 32)      # [J/16][512 features][32 keys]
    assert np.isfinite(v).all(), tag
    pos = vts_positions(natural)
    pad = np.setdiff1d(np.arange(32), pos)
    assert (hi[..., pad].view(np.uint16) == 0).all() and (lo[..., pad].view(np.uint16) == 0).all(), "padding keys not exactly zero"
    got_v = v[..., pos].transpose(0, 2, 1).reshape(J, ROWS)           # back to [token][feature]
    e_v = np.maximum(np.abs(got_v - want_v) - U22 * np.abs(want_v), 0) / scale_v
    if off is None:
        assert e_qk.max() < 1e-5 and e_v.max() < 1e-5, (tag, float(e_qk.max()), float(e_v.max()))
    else:
        _report(tag + " q|k", e_qk, off, const_row)
        _report(tag + " v^T", e_v, off, const_row)


@pytest.mark.parametrize("cfg", [0, 1, 19, 24])
@pytest.mark.parametrize("J,K", [(16, 32), (64, 64), (1120, 512)])
@pytest.mark.parametrize("natural", [1, 0])
def test_qkvt(ops, cfg, J, K, natural):
    from convofusion_amd import _lib
    rng = np.random.default_rng(J + K + cfg + natural)
    X, Y, _ = _operands(rng, 3 * ROWS, J, K)
    b = rng.standard_normal(2 * ROWS).astype(np.float32)
    qk, vts = _sp_buf(J, 2 * ROWS), _sp_buf(J // 16 * ROWS, 32)
    _ok(ops, _lib.EPI_QKVT, 3 * ROWS, J, K, cfg=cfg, natural=natural, X=_dev(X), Y=_dev(Y), bias=_dev(b), out=qk, out2=vts)
    D = Y.astype(np.float64) @ X.astype(np.float64).T
    ny, nx = _norms(Y, X)
    sc = ny[:, None] * nx[None, :]
    _check_qkvt(qk.cpu().numpy(), vts.cpu().numpy(), J, D[:, :1024] + b, D[:, 1024:], sc[:, :1024] + np.abs(b), sc[:, 1024:], natural,
                f"qkvt cfg {cfg}")


@pytest.mark.parametrize("J,K", [(64, 32), (1120, 512), (3584, 512)])
@pytest.mark.parametrize("natural", [1, 0])
def test_ln_fold_qkvt(ops, J, K, natural):
    """EpiLn<EpiQkvT> (grouped: I = 1024 and 512, each group with its own c / d); K = 512 chained from an EpiResidStat producer as in the
    product, K = 32 with fed statistics."""
    from convofusion_amd import _lib
    rng = np.random.default_rng(J + K + natural)
    I = 3 * ROWS
    W, gamma, beta, _ = _fold_weights(rng, I, K)
    b = (rng.standard_normal(2 * ROWS) * 0.1).astype(np.float32)
    qk, vts = _sp_buf(J, 2 * ROWS), _sp_buf(J // 16 * ROWS, 32)
    args = dict(natural=natural, X=_dev(W), bias=_dev(b), gamma=_dev(gamma), beta=_dev(beta), out=qk, out2=vts)
    if K == ROWS:
        x0 = fold_rows(rng, J)
        x0[0] = rng.standard_normal(ROWS)
        p = _producer(ops, rng, J, 2048, x0)
        x = p["x"].cpu().numpy()[:J]
        args.update(y_sp=p["xs"], ln_stat=p["stat"])
    else:
        x = fold_rows(rng, J)
        m, m2 = slot_stats(x)
        _poison(ops, _lib.EPI_LN_QKVT, I, J, _sp_buf(J, 2 * ROWS), natural=natural, bias=_dev(b),
                out2=_sp_buf(J // 16 * ROWS, 32))
        args.update(Y=_dev(x[:, :K]), ln_stat=_dev(np.stack([m, m2], -1).astype(np.float32)))
    used = _ok(ops, _lib.EPI_LN_QKVT, I, J, K, **args)
    assert used == midsize_class([1024, 512], J), used
    y, z, off = ln_ref(x, gamma, beta, K)
    D = y @ W.astype(np.float64).T
    bb = np.concatenate([b, np.zeros(ROWS, np.float32)])
    sc = fold_scale(z, W, gamma, beta, bb, K)
    _check_qkvt(qk.cpu().numpy(), vts.cpu().numpy(), J, D[:, :1024] + b, D[:, 1024:], sc[:, :1024], sc[:, 1024:], natural,
                f"fold qkvt J={J} K={K} class {used}", off=off, const_row=K != ROWS)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(ops):
    """CFD_E_ARG before any launch: the output is left as it was."""
    import torch
    from convofusion_amd import _lib
    rng = np.random.default_rng(0)
    dX, dY = _dev(rng.standard_normal((1536, 64)).astype(np.float32)), _dev(rng.standard_normal((64, 64)).astype(np.float32))
    bias = _dev(np.zeros(1536, np.float32))
    x = torch.full((64, ROWS), float("nan"), device="cuda")
    out = _sp_buf(64, 1536)
    st = torch.full((64, 16, 2), float("nan"), device="cuda")
    g = _dev(np.ones(64, np.float32))
    cases = [
        ("resid I != 512", _lib.EPI_RESID, 256, 64, 64, dict(x=x)),
        ("resid-stat I != 512", _lib.EPI_RESID_STAT, 1024, 64, 64, dict(x=x, out=out, stat=st)),
        ("qkvt J % 16", _lib.EPI_QKVT, 1536, 60, 64, dict(out=out, out2=out, bias=bias)),
        ("ln-qkvt J % 16", _lib.EPI_LN_QKVT, 1536, 17, 64, dict(out=out, out2=out, bias=bias, gamma=g, beta=g, ln_stat=st)),
        ("K % 32", _lib.EPI_F32, 64, 64, 48, dict(out=out)),
        ("K = 0", _lib.EPI_SPLIT, 64, 64, 0, dict(out=out)),
        ("split I % 32", _lib.EPI_SPLIT, 48, 64, 64, dict(out=out)),
        ("ln-split I % 32", _lib.EPI_LN_SPLIT, 80, 64, 64, dict(out=out, gamma=g, beta=g, ln_stat=st)),
        ("f32 I % 4", _lib.EPI_F32, 66, 64, 64, dict(out=out)),
        ("ln-f32 I % 4", _lib.EPI_LN_F32, 130, 64, 64, dict(out=out, gamma=g, beta=g, ln_stat=st)),
    ]
    for what, kind, I, J, K, kw in cases:
        r, _ = _launch(ops, kind, I, J, K, X=dX, Y=dY, **kw)
        assert r == E_ARG, (what, r)
    assert torch.isnan(x).all() and bool((out == 0xFF).all()) and torch.isnan(st).all(), "a refused call wrote"
