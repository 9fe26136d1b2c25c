"""CPU: the float64 statement of the self-attention block in tests/selfattn_ref.py is the oracle's, the cases of
tests/test_gpu_selfattn_block.py are what that file says they are, and the gate that file applies separates a subtly wrong kernel from
rounding -- a GPU case cannot mean anything on a yardstick that does not.

Every length of the case table runs here at B = 1 utterance, 7 guidance rows, timestep 417, the memories of the token-major test; the
block's input is the float32 oracle's residual stream in front of the block (`x0`, `l<i>.out`), layers 0, 4 and 8, both weight sets.
Printed per (length, weight set, layer): the float32 yardstick (worst row, E), the gate made from it, and each emulated fault's worst row
as a multiple of that gate.

Measured (this file's own print-out): the float32 restatement is at most 5.2e-6 worst row / 1.7e-6 whole with the peaked weights and
4.5e-7 / 3.9e-7 with the plain ones.  The smallest fault-to-gate ratios: p16 3.1 (peaked, L = 128, layer 0, the case with the largest
float32 worst row; the next is 4.0), k16 3.9 (plain, L = 196, layer 8), v16 6.5 (plain, L = 196, layer 8); pad_weight, key_order and
adjacent are above 1e3 everywhere.
"""
import functools

import numpy as np
import pytest

from tests import selfattn_ref as R

LENGTHS = sorted({c["L"] for c in R.CASES})
SEPARATION = 3.0
# (length, weight set, layer, fault) -> measured ratio of the pairs that do not reach SEPARATION x their gate.  Only k16 pairs may stand
# here (its error shrinks as 1 / sqrt(L) under near-uniform probabilities); none does.
NOT_SEPARATED = {}


@functools.lru_cache(maxsize=None)
def _problem(L, ws):
    sd = R.weights(ws)
    return sd, R.oracle_taps(sd, R.host_inputs(L))


@functools.lru_cache(maxsize=None)
def _figures(L, ws):
    """Per layer: the oracle's distance, the peak premise, the float32 yardstick's measures and each fault's worst row."""
    sd, taps = _problem(L, ws)
    res = {}
    for l in R.LAYERS:
        x = R.block_input(taps, l)
        assert x.dtype == np.float32
        ex, pr = R.block(sd, l, x)
        assert ex.dtype == np.float64 and np.isfinite(ex).all()
        assert pr.shape == (7, 4, L, L) and np.abs(pr.sum(-1) - 1).max() < 1e-12
        after = taps[f"l{l}.after_self"].astype(np.float64)
        w32, at, E32 = R.measures(R.yardstick32(sd, l, x), ex, L)
        faults = {}
        for f in R.FAULTS:
            if f == "key_order" and L < 32:
                continue
            faults[f] = R.measures(R.block(sd, l, x, **{f: True})[0], ex, L)[0]
        res[l] = dict(oracle=float(np.linalg.norm(x + ex - after) / np.linalg.norm(after)), peak=R.peak_median(pr), w32=w32, at=at, E32=E32,
                      faults=faults, share=float(np.linalg.norm(ex) / np.linalg.norm(x)))
        g = R.gate(w32)
        print(f"L {L} {ws} layer {l}: float32 worst row {w32:.3e} at {at}, E {E32:.3e}; gate {g:.3e} / {R.gate(E32):.3e}; update / stream "
              f"{res[l]['share']:.2f}; median peak {res[l]['peak']:.3f}; fault / gate: " + " ".join(f"{f} {v / g:.1f}" for f, v in faults.items()))
    return res


CASES = [(L, ws) for L in LENGTHS for ws in R.WEIGHT_SETS]


@pytest.mark.parametrize("L,ws", CASES)
def test_float64_block_is_the_oracles(L, ws):
    for l, r in _figures(L, ws).items():
        assert r["oracle"] < 1e-5, (l, r["oracle"])
        assert 0.05 < r["share"] < 1.0, (l, r["share"])          # the update is a visible part of the stream, not all of it


@pytest.mark.parametrize("L", LENGTHS)
def test_peaked_weights_concentrate_the_rows(L):
    """The premise of every case that uses the peaked set: one key holds most of a typical row's weight (factor 4 suffices up to L = 196);
    the plain set at L >= 16 is the opposite regime."""
    for l, r in _figures(L, "peaked").items():
        assert r["peak"] > 0.5, (l, r["peak"])
    if L >= 16:
        for l, r in _figures(L, "plain").items():
            assert r["peak"] < 0.25, (l, r["peak"])


@pytest.mark.parametrize("L,ws", CASES)
def test_float32_restatement_stays_small(L, ws):
    for l, r in _figures(L, ws).items():
        assert 1e-8 < r["E32"] < 3e-6 and r["w32"] < 1e-5, (l, r["w32"], r["E32"])


@pytest.mark.parametrize("L,ws", CASES)
def test_gate_separates_every_fault_from_rounding(L, ws):
    missed = []
    for l, r in _figures(L, ws).items():
        g = R.gate(r["w32"])
        assert set(r["faults"]) == set(R.FAULTS) - ({"key_order"} if L < 32 else set())
        for f, v in r["faults"].items():
            if v < SEPARATION * g and (L, ws, l, f) not in NOT_SEPARATED:
                missed.append((l, f, round(v / g, 2)))
    assert not missed, missed
    assert all(k[3] == "k16" for k in NOT_SEPARATED)


def test_faults_are_what_they_say():
    L = 34
    sd, taps = _problem(L, "plain")
    x = R.block_input(taps, 4)
    ex, pr = R.block(sd, 4, x)
    u, pp = R.block(sd, 4, x, pad_weight=True)
    assert pp.shape[-1] == L + 1 and np.array_equal(pp[..., L], pp[..., L - 1]) and np.abs(pp.sum(-1) - 1).max() < 1e-12
    for f in ("key_order", "adjacent", "v16"):                   # the probabilities stay
        assert np.array_equal(R.block(sd, 4, x, **{f: True})[1], pr), f
    p16 = R.block(sd, 4, x, p16=True)[1]                         # rounded relative to the row's maximum: the largest entry is exact
    top = pr.argmax(-1)[..., None]
    assert np.array_equal(np.take_along_axis(p16, top, -1), np.take_along_axis(pr, top, -1)) and not np.array_equal(p16, pr)
    assert 1e-5 < np.abs(p16 - pr).max() / pr.max() < 2.0 ** -10
    # float32: nothing in the restatement is wider than float32
    u32, p32 = R.block(sd, 4, x, np.float32)
    assert u32.dtype == np.float32 and p32.dtype == np.float32


def test_case_table():
    ids = [R.case_id(c) for c in R.CASES]
    assert len(set(ids)) == len(ids)
    for c in R.CASES:
        Be, L = c["Be"], c["L"]
        assert L % 2 == 0 and c["path"] in ("tile", "tile16", "rowtile", "saved")
        assert Be * L <= 7 * 196
        if c["path"] == "tile":
            assert L != 16 and Be % 7 == 0
        if c["path"] == "tile16":
            assert L == 16 and Be % 7 == 0
        if c["path"] in ("rowtile", "saved"):
            assert L <= 32 and Be * L <= 700                      # RT_MAX_L, the default row limit of the row-tile path
    assert sum(1 for c in R.CASES if c.get("alone")) == 4 and {c["path"] for c in R.CASES if c.get("alone")} == {"tile", "tile16", "rowtile", "saved"}
    tiles = lambda c: c["Be"] * ((c["L"] + 15) // 16)
    assert sorted(tiles(c) for c in R.cases("rowtile") if c["L"] == 16) == [13, 14]      # RT_NFB2_MIN_TILES = 14
    assert tiles(next(c for c in R.cases("rowtile") if (c["Be"], c["L"]) == (7, 32))) == 14
    # the 13 rows at L = 16 are the first 13 of the 14
    a, b = R.case_inputs("rowtile", 13, 16), R.case_inputs("rowtile", 14, 16)
    assert np.array_equal(a["sample"], b["sample"][:13]) and all(np.array_equal(p, q[:13]) for p, q in zip(a["memories"], b["memories"]))
    for k, v in a["masks"].items():
        assert (v is None and b["masks"][k] is None) or np.array_equal(v, b["masks"][k][:13])
    c = R.case_inputs("tile", 14, 18)
    assert c["sample"].shape == (14, 18, 128) and np.array_equal(c["sample"][:2], c["sample"][12:])
    assert [m.shape[1] for m in c["memories"]] == list(R.S)
