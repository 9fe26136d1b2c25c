"""GPU tests: every launch of a T5 encoder block (cfd_t5_encode, csrc/t5_enc.hpp) against the float64 restatement of the SAME operation
(tests/t5_ref.py's stage functions) on the device's own inputs, at the edges of the kernels' tiles.

Method.  After a call the taps cfd_debug_read "t5.x" / "t5.h" / "t5.qkv" / "t5.ctx" / "t5.f" hold what the last block's launches wrote.  In a
one-block encoder the block's input is exactly embed[ids] (the gather path a_ids / r_ids), so each launch's inputs are known bit for bit:
the stage function is applied to the upcast device tensors the kernel read and compared with what it wrote.  A two-block encoder covers
the path without the gather: block 1's input is the "t5.x" of a one-block encoder built from block 0's weights alone (the bits are
deterministic, which is asserted).  The final launch is checked from "t5.x", as t5_final_rows and as the projection.

Measure: t5_ref.rel_err, max-abs over the reference's RMS, every row counted (padded rows too).  Gate per stage: FACTOR = 4 (the factor of
test_gpu_t5.py and of the metrics tests) x the distance of the same stage function run in float32 numpy from float64 on the same inputs,
computed here on the CPU -- what the formula itself loses in single precision.  Every stage prints measured value, base and gate.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import t5_ref

pytestmark = pytest.mark.gpu

FACTOR = 4.0
WIDTHS = {"x": 768, "h": 768, "qkv": 2304, "ctx": 768, "f": 3072}
F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def state(num_layers, seed, proj_dim=512):
    return t5_ref.make_state(num_layers, seed, t5_ref.VOCAB, proj_dim)


def first_block_only(sd):
    """the one-block state of ``sd``'s block 0 (same embedding, final norm and projection)"""
    return {k: v for k, v in sd.items() if not k.startswith("encoder.block.") or k.startswith("encoder.block.0.")}


def make_encoder(sd):
    from convofusion_amd.text import T5TextEncoder
    return T5TextEncoder.from_parts(t5_ref.stub_text_model(sd), None, t5_ref.projection_module(sd)).cuda().eval()


def encode(enc, ids, mask, project=True):
    import torch
    return enc.encode_ids(torch.from_numpy(np.ascontiguousarray(ids)), torch.from_numpy(np.ascontiguousarray(mask)), project=project).cpu().numpy()


def debug_read(what, numel):
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.conditioning import _engine_handle
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros(numel, device=dev)
    _lib.check(_lib.load().cfd_debug_read(_engine_handle(dev), what.encode(), C.c_void_p(buf.data_ptr()), numel))
    return buf.cpu().numpy()


def t5_info():
    """launches of the last call, token rows, workspace bytes, launches of 128 x 128 blocks"""
    return [int(v) for v in debug_read("t5.info", 4)]


def taps(rows):
    return {k: debug_read("t5." + k, rows * w).reshape(rows, w) for k, w in WIDTHS.items()}


def gate(label, got, fn):
    """``fn(dtype)`` is the stage on the device's inputs.  Prints measured / base / gate; returns the failure text or None."""
    want = fn(F64)
    base = t5_ref.rel_err(fn(F32), want)
    err = t5_ref.rel_err(got.reshape(want.shape), want)
    print(f"  {label:>9}: measured {err:.3e}  base {base:.3e}  gate {FACTOR * base:.3e}")
    assert np.isfinite(want).all() and base > 0.0
    return None if err <= FACTOR * base else f"{label}: {err:.3e} > {FACTOR:g} x {base:.3e}"


def check_block(sd, l, x_in, tp, mask, T, only=None):
    """the five launches of block ``l``: ``x_in`` what the block read, ``tp`` the taps behind it"""
    stages = {
        "qkv": (tp["qkv"], lambda dt: t5_ref.stage_qkv(sd, l, x_in, dt)),
        "attn": (tp["ctx"], lambda dt: t5_ref.stage_attn(sd, tp["qkv"], mask, T, dt)),
        "attn_out": (tp["h"], lambda dt: t5_ref.stage_attn_out(sd, l, x_in, tp["ctx"], dt)),
        "ff_in": (tp["f"], lambda dt: t5_ref.stage_ff_in(sd, l, tp["h"], dt)),
        "ff_out": (tp["x"], lambda dt: t5_ref.stage_ff_out(sd, l, tp["h"], tp["f"], dt)),
    }
    return [gate(k, got, fn) for k, (got, fn) in stages.items() if only is None or k in only]


def check_final(sd, x, hidden=None, projected=None):
    bad = []
    if hidden is not None:
        bad.append(gate("final", hidden, lambda dt: t5_ref.stage_final(sd, x, False, dt)))
    if projected is not None:
        bad.append(gate("projected", projected, lambda dt: t5_ref.stage_final(sd, x, True, dt)))
    return bad


def check_one_block(sd, ids, mask, only=None):
    """a one-block encoder on (ids, mask): all five launches and both final launches; returns (projected output, taps)"""
    n, T = ids.shape
    enc = make_encoder(sd)
    hidden = encode(enc, ids, mask, project=False)
    x_first = debug_read("t5.x", n * T * 768)
    out = encode(enc, ids, mask, project=True)
    assert t5_info()[:2] == [6, n * T]
    tp = taps(n * T)
    assert np.array_equal(tp["x"].ravel(), x_first)                    # two calls, the same bits
    x0 = sd["shared.weight"][ids].reshape(n * T, 768)
    print(f"one block, {n} x {T}:")
    bad = check_block(sd, 0, x0, tp, mask, T, only)
    if only is None:
        bad += check_final(sd, tp["x"], hidden, out)
    bad = [b for b in bad if b]
    assert not bad, bad
    return out, tp


def test_taps_check_state_and_size():
    """The five taps: CFD_E_STATE on a handle no cfd_t5_encode ran on, CFD_E_ARG past each buffer's own rows x width, a shorter read is
    the head of the full one."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.conditioning import _engine_handle
    lib = _lib.load()
    dst = torch.zeros(64, device="cuda:0")
    fresh = _lib.create_handle(0)
    try:
        for k in WIDTHS:
            assert lib.cfd_debug_read(fresh, b"t5." + k.encode(), C.c_void_p(dst.data_ptr()), 1) == -3, k
    finally:
        lib.cfd_destroy(fresh)
    ids, mask = t5_ref.prefix_inputs(3100, (3, 2), 3)
    encode(make_encoder(state(1, 31)), ids, mask)
    h = _engine_handle(torch.device("cuda:0"))
    for k, w in WIDTHS.items():
        full = debug_read("t5." + k, 6 * w)
        assert np.isfinite(full).all() and np.abs(full).max() > 0
        assert np.array_equal(debug_read("t5." + k, w + 1), full[:w + 1])
        big = torch.zeros(6 * w + 1, device="cuda:0")
        assert lib.cfd_debug_read(h, b"t5." + k.encode(), C.c_void_p(big.data_ptr()), 6 * w + 1) == -1, k
        assert k in lib.cfd_last_error().decode()
    assert lib.cfd_debug_read(h, b"t5.g", C.c_void_p(dst.data_ptr()), 1) == -1      # no such tap


def edge_lengths(T):
    return (T, T - 63 if T > 63 else 1)


@pytest.mark.parametrize("T", [64, 65, 128, 129, 256])
def test_every_launch_at_the_attention_tile_edges(T):
    """One block, a full sequence and one of T - 63 tokens (1 at T = 64): a full last key tile (64, 128, 256), a last tile of one key and
    a query workgroup with one live lane (65, 129), T5_MAX_T (bias table index 510, distances past 128 on both sides).

    Measured on the MI355X, measured / base (gate 4 x base), worst over the five T:
    qkv 2.50e-6 / 3.87e-6, attn 9.78e-6 / 1.05e-5 (T = 256; closest to its gate at T = 129: 5.86e-6 / 3.36e-6),
    attn_out 1.24e-6 / 1.64e-6, ff_in 3.31e-6 / 4.28e-6, ff_out 9.01e-7 / 8.86e-7, final 7.99e-7 / 6.10e-7, projected 1.77e-6 / 2.09e-6."""
    ids, mask = t5_ref.prefix_inputs(3000 + T, edge_lengths(T), T)
    check_one_block(state(1, 31), ids, mask)


def test_every_launch_under_masks_with_holes():
    """T = 129, three sequences: keys 0 .. 63 masked (the running maximum starts in the second tile), keys 64 .. 127 masked (a whole inner
    tile skipped), every second key masked.  The float64 reference is finite on all three.

    Measured on the MI355X, measured / base: qkv 2.50e-6 / 3.88e-6, attn 3.90e-6 / 3.54e-6, attn_out 6.55e-7 / 9.48e-7,
    ff_in 3.62e-6 / 5.70e-6, ff_out 7.90e-7 / 1.12e-6, final 6.99e-7 / 7.05e-7, projected 1.64e-6 / 1.91e-6."""
    ids, mask = t5_ref.hole_inputs(3200)
    check_one_block(state(1, 31), ids, mask)


def test_attention_with_near_one_hot_softmax():
    """T = 65 with Wq x 64 (a power of two): scores of order 100, the softmax near one-hot, so a new maximum's rescale exp(mx - sc)
    underflows to 0 and later keys' exp(sc - mx) too.  Only the attention launch is gated here.

    Measured on the MI355X, measured / base: attn 4.27e-5 / 4.27e-5 (gate 1.71e-4): the scores' own rounding, e^x's condition at |x| ~ 100."""
    sd = dict(state(1, 31))
    key = "encoder.block.0.layer.0.SelfAttention.q.weight"
    sd[key] = sd[key] * np.float32(64.0)
    ids, mask = t5_ref.prefix_inputs(3065, edge_lengths(65), 65)
    _, tp = check_one_block(sd, ids, mask, only=("attn",))
    q, k = tp["qkv"][:65, :64].astype(F64), tp["qkv"][:65, 768:832].astype(F64)
    assert np.ptp(q @ k.T, axis=1).min() > 104.0                      # exp(-104) < 2^-149: for every query some key's weight underflows to 0


@pytest.mark.parametrize("case", ["T65", "holes"])
def test_every_launch_of_a_second_block(case):
    """Two blocks: block 1 reads the residual stream from memory (no gather).  Its input is the "t5.x" of a one-block encoder of block 0's
    weights alone; the bits are deterministic (asserted: two calls, equal reads).

    Measured on the MI355X, measured / base: T65: qkv 3.39e-6 / 3.31e-6, attn 1.36e-6 / 1.47e-6, attn_out 9.30e-7 / 1.24e-6,
    ff_in 3.14e-6 / 4.33e-6, ff_out 4.63e-7 / 7.96e-7, final 5.81e-7 / 5.81e-7, projected 1.51e-6 / 1.88e-6; holes: qkv 2.83e-6 / 3.92e-6,
    attn 2.24e-6 / 2.00e-6, attn_out 7.32e-7 / 9.63e-7, ff_in 3.31e-6 / 4.36e-6, ff_out 7.37e-7 / 7.37e-7, final 5.01e-7 / 4.77e-7,
    projected 1.65e-6 / 1.96e-6."""
    sd = state(2, 32)
    ids, mask = t5_ref.prefix_inputs(3300, edge_lengths(65), 65) if case == "T65" else t5_ref.hole_inputs(3301)
    n, T = ids.shape
    one = make_encoder(first_block_only(sd))
    encode(one, ids, mask)
    x1 = debug_read("t5.x", n * T * 768)
    encode(one, ids, mask)
    assert np.array_equal(x1, debug_read("t5.x", n * T * 768))
    x1 = x1.reshape(n * T, 768)
    two = make_encoder(sd)
    hidden = encode(two, ids, mask, project=False)
    out = encode(two, ids, mask)
    assert t5_info()[:2] == [11, n * T]
    tp = taps(n * T)
    print(f"block 1 of two, {case}:")
    bad = [b for b in check_block(sd, 1, x1, tp, mask, T) + check_final(sd, tp["x"], hidden, out) if b]
    assert not bad, bad


BIG_N, BIG_T = 247, 33          # 8151 rows: >= 8065 (the projection to 512 reaches 128 x 128 blocks on 256 CUs), 8151 % 128 = 87


def big_inputs():
    lens = tuple(int(v) for v in np.random.RandomState(3400).randint(1, BIG_T + 1, size=BIG_N))
    return lens, t5_ref.prefix_inputs(3401, lens, BIG_T)


def big_launches_by_rule(M, widths):
    """cfd_text.hip's block-shape rule restated: a product runs 128 x 128 blocks when N % 128 == 0 and ceil(M / 128) (N / 128) >= CUs"""
    import torch
    n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return sum(1 for N in widths if N % 128 == 0 and -(-M // 128) * (N // 128) >= n_cu)


def rows_alone_equal_rows_in_batch(enc, ids, mask, lens, full, picks):
    for s in picks:
        alone = encode(enc, ids[[s], :lens[s]], mask[[s], :lens[s]])
        assert t5_info()[3] == 0                                       # alone: every product in 64 x 64 blocks
        assert np.array_equal(alone[0], full[s, :lens[s]]), (s, lens[s])


def test_every_product_in_128_x_128_blocks():
    """247 sequences of 1 .. 33 tokens at T = 33 = 8151 rows, one block, projection to 512: on the device under test all five products
    run t5_gemm_kernel<2, 2> (t5.info), the two residual-epilogue products (one of them the only K = 3072 one) and the bias / ReLU-of-A
    projection among them, with a last row-block of 87 rows (wave row 1 partly valid).  All five launches and the projection against
    float64; and three sequences encoded alone (64 x 64 blocks throughout) give the bits of their rows in the batch.

    Measured on the MI355X, measured / base: qkv 2.42e-6 / 3.90e-6, attn 3.11e-6 / 1.83e-6, attn_out 1.74e-6 / 2.07e-6,
    ff_in 3.78e-6 / 5.25e-6, ff_out 9.02e-7 / 1.17e-6, projected 2.00e-6 / 2.53e-6; t5.info reads 5."""
    lens, (ids, mask) = big_inputs()
    M = BIG_N * BIG_T
    assert M >= 8065 and 64 < M % 128 < 128
    sd = state(1, 33)
    enc = make_encoder(sd)
    out = encode(enc, ids, mask)
    big = t5_info()[3]
    assert big == big_launches_by_rule(M, (2304, 768, 3072, 768, 512)) and big == 5, big
    tp = taps(M)
    print(f"all products in 128 x 128 blocks, {BIG_N} x {BIG_T}:")
    x0 = sd["shared.weight"][ids].reshape(M, 768)
    bad = [b for b in check_block(sd, 0, x0, tp, mask, BIG_T) + check_final(sd, tp["x"], None, out) if b]
    assert not bad, bad
    rows_alone_equal_rows_in_batch(enc, ids, mask, lens, out, (0, int(np.argmin(lens)), BIG_N - 1))


@pytest.mark.parametrize("rows", ["big", "small"])
@pytest.mark.parametrize("width", [64, 192, 1024])
def test_projection_widths(width, rows):
    """Projection to 64 (the smallest the call takes), 192 (N % 128 = 64: 64 x 64 blocks even at 8151 rows) and 1024, on the 8151-row
    batch and on a 40-row one, against float64 from "t5.x".  Widths 64 and 192 always run 64 x 64 blocks, so a sequence's rows in the
    batch equal its rows alone bit for bit.

    Measured on the MI355X, measured / base: 8151 rows: 64 1.80e-6 / 2.37e-6, 192 1.69e-6 / 2.44e-6, 1024 2.06e-6 / 2.95e-6;
    40 rows: 64 8.77e-7 / 1.19e-6, 192 1.28e-6 / 1.48e-6, 1024 1.56e-6 / 2.10e-6."""
    if rows == "big":
        lens, (ids, mask) = big_inputs()
    else:
        lens = (1, 7, 8, 8, 5)                                          # 5 x 8 = 40 rows
        ids, mask = t5_ref.prefix_inputs(3500, lens, 8)
    n, T = ids.shape
    sd = state(1, 33, width)
    assert sd["projection.1.weight"].shape == (width, 768) and np.array_equal(sd["shared.weight"], state(1, 33)["shared.weight"])
    enc = make_encoder(sd)
    out = encode(enc, ids, mask)
    assert out.shape == (n, T, width)
    launches, m, _, big = t5_info()
    assert (launches, m) == (6, n * T)
    assert big == big_launches_by_rule(n * T, (2304, 768, 3072, 768, width))
    assert big == ({64: 4, 192: 4, 1024: 5}[width] if rows == "big" else 0), big
    x = debug_read("t5.x", n * T * 768).reshape(n * T, 768)
    print(f"projection to {width}, {n} x {T}:")
    bad = [b for b in check_final(sd, x, None, out) if b]
    assert not bad, bad
    if width in (64, 192):
        rows_alone_equal_rows_in_batch(enc, ids, mask, lens, out, (0, int(np.argmin(lens)), n - 1))
