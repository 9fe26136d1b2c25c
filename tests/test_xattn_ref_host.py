"""CPU: the two float64 statements of the cross-attention block in tests/xattn_ref.py agree with each other, and the inputs of the cases of
tests/test_gpu_xattn_block.py are what that file says they are -- a GPU case cannot pass on inputs that do not test what it claims to.

Every case runs at B = 2 utterances here (the B = 40 cases differ from their small versions in the work list only, which has no CPU side);
the block's input is the float32 oracle's residual stream in front of the block (the GPU tests take the kernel's own)."""
import functools

import numpy as np
import pytest

from oracle import denoiser_ref
from tests import xattn_ref as X


@functools.lru_cache(maxsize=None)
def _case(name):
    c = X.make_case(name, B=2)
    sd = X.case_state_dict(name)
    taps = {}
    with np.errstate(invalid="ignore"):
        denoiser_ref.denoiser_forward(sd, c["sample"], X.T_STEP, c["memories"], c["masks"], taps=taps)
    x_in = {l: taps[f"l{l}.after_tb1"].transpose(1, 0, 2).copy() for l in X.LAYERS}
    return c, sd, X.memory_taps(sd, X.T_STEP, c["unique"]), x_in, {k: v for k, v in taps.items() if k.startswith("mem.")}


def _rel(a, b):
    ok = np.isfinite(b).all(-1)
    return float(np.linalg.norm(a[ok] - b[ok]) / np.linalg.norm(b[ok]))


def test_memory_taps_restate_the_oracles():
    c, sd, mt, _, oracle_taps = _case("one_long")
    for j, n in enumerate(X.MEM_NAMES):
        want = oracle_taps["mem." + n]
        got = mt["mem." + n][:, c["row_map"][j]]
        # (the oracle forms temb for 14 identical rows, memory_taps for one: the two products may round differently -- a few float32 ulps)
        assert got.dtype == np.float32 and np.abs(got - want).max() <= 8 * np.finfo(np.float32).eps * np.abs(want).max(), n


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_folded_equals_unfolded_in_float64(name):
    c, sd, mt, x_in, _ = _case(name)
    for l in X.LAYERS:
        u, pu = X.block_unfolded(sd, l, x_in[l], mt, c["umasks"], c["row_map"])
        f, pf = X.block_folded(sd, l, x_in[l], mt, c["umasks"], c["row_map"])
        assert np.array_equal(np.isfinite(u), np.isfinite(f))
        assert _rel(f, u) < 1e-10, (l, _rel(f, u))
        for a, b in zip(pf, pu):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b)) < 1e-10
        # the row maps are only a shorter way to write the same thing
        if name == "one_long":
            rows = {n: (None if m is None else m) for n, m in c["masks"].items()}
            per_row = {"temb": mt["temb"], **{"mem." + n: mt["mem." + n][:, c["row_map"][j]] for j, n in enumerate(X.MEM_NAMES)}}
            assert np.array_equal(X.block_unfolded(sd, l, x_in[l], per_row, rows)[0], u)
        # float32 restatements and the fp16 emulation are where they should be: around 2^-24 resp. 2^-11 per operand -- up to 4 x 2^-11 = 2e-3
        # where one key holds a row's weight, well below where a thousand near-uniform probabilities average the roundings
        for fn in (X.block_unfolded, X.block_folded):
            e32 = _rel(fn(sd, l, x_in[l], mt, c["umasks"], c["row_map"], dtype=np.float32)[0].astype(np.float64), u)
            assert 1e-8 < e32 < 3e-6, (fn.__name__, e32)
        has_long = any((s + 31) // 32 * 32 >= X.LONG_KEYS for s in X.CASES[name]["S"])
        noP = X.block_folded(sd, l, x_in[l], mt, c["umasks"], c["row_map"], round_ops=("q", "k", "v"))[0]
        emu = X.block_folded(sd, l, x_in[l], mt, c["umasks"], c["row_map"], round_ops=("q", "k", "v", "p"))[0]
        if has_long:
            assert 1e-6 < _rel(noP, u) < 2e-3 and 1e-6 < _rel(emu, noP) < 2e-3, (_rel(noP, u), _rel(emu, noP))
        else:       # no long memory: nothing is rounded, bit for bit
            assert np.array_equal(noP, f, equal_nan=True) and np.array_equal(emu, f, equal_nan=True)


def test_the_online_fp16_walk_without_rounding_is_the_softmax():
    """_online_f16 with the fp16 rounding taken out is the plain softmax form: the tile walk itself adds nothing."""
    c, sd, mt, x_in, _ = _case("two_long_mixed")
    keep = X._f16
    X._f16 = lambda z: z
    try:
        walked = X.block_folded(sd, 1, x_in[1], mt, c["umasks"], c["row_map"], round_ops=("p",))[0]
    finally:
        X._f16 = keep
    assert _rel(walked, X.block_folded(sd, 1, x_in[1], mt, c["umasks"], c["row_map"])[0]) < 1e-12


def test_a_fully_masked_memory_gives_nan_rows_in_both_forms():
    c, sd, mt, x_in, _ = _case("dead_memory")
    L = X.CASES["dead_memory"]["L"]
    assert c["umasks"]["alsn"][1].all() and not c["umasks"]["alsn"][0].all() and not c["umasks"]["alsn"][2].all()
    dead_rows = c["row_map"][1] == 1                 # the chunks that carry utterance 0's own audio memory: audio_only and full
    assert dead_rows.sum() == 2
    for l in X.LAYERS:
        for fn in (X.block_unfolded, X.block_folded):
            for kw in ({}, {"dtype": np.float32}):
                u = fn(sd, l, x_in[l], mt, c["umasks"], c["row_map"], **kw)[0]
                assert np.isnan(u[dead_rows]).all() and np.isfinite(u[~dead_rows]).all()
                assert int(np.isnan(u).all(-1).sum()) == 2 * L
        emu = X.block_folded(sd, l, x_in[l], mt, c["umasks"], c["row_map"], round_ops=("q", "k", "v", "p"))[0]
        assert np.isnan(emu[dead_rows]).all() and np.isfinite(emu[~dead_rows]).all()


def test_premises_of_the_threshold_and_mixed_cases():
    pad32 = lambda s: (s + 31) // 32 * 32
    S = X.CASES["threshold"]["S"]
    assert pad32(S[1]) == X.LONG_KEYS and pad32(S[1]) - S[1] == 31 and all(pad32(s) < X.LONG_KEYS for j, s in enumerate(S) if j != 1)
    assert all(pad32(s) < X.LONG_KEYS for s in X.CASES["threshold_96"]["S"])
    assert [pad32(s) for s in X.CASES["two_long_mixed"]["S"]] == [96, 288, 160, 64, 32]
    assert [pad32(s) for s in X.CASES["one_long"]["S"]] == [32, 160, 32, 32, 32]
    c = X.make_case("one_long", B=2)                 # the one-key memory is unmasked: the kernel adds it as a vector
    assert c["umasks"]["lsnemb"] is None and X.CASES["one_long"]["L"] % 16 == 2


def test_premises_of_the_concentrated_case():
    """In float64, from the oracle's input: the median peak probability over the audio memory is above 0.5 in both layers; the keys that hold
    more than half of a row's weight cover, over the two layers, all 32 positions of a key tile and both parities of the tile index; and
    the update is an order of magnitude larger than with the unscaled values (the attention output dominates it)."""
    c, sd, mt, x_in, _ = _case("concentrated")
    plain = X.case_state_dict("one_long")
    pos, par = set(), set()
    for l in X.LAYERS:
        u, pr = X.block_unfolded(sd, l, x_in[l], mt, c["umasks"], c["row_map"])
        pk, am = pr[1].max(-1), pr[1].argmax(-1)
        assert np.median(pk) > 0.5, (l, float(np.median(pk)))
        pos |= set((am[pk > 0.5] % 32).tolist())
        par |= set(((am[pk > 0.5] // 32) % 2).tolist())
        u0 = X.block_unfolded(plain, l, x_in[l], mt, c["umasks"], c["row_map"])[0]
        assert np.linalg.norm(u) > 10 * np.linalg.norm(u0)
    assert pos == set(range(32)) and par == {0, 1}, (sorted(set(range(32)) - pos), par)
