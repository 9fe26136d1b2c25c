"""The float64 restatement of the reference's motion evaluation (tests/metrics_ref.py) against the reference's own outputs, recorded by
tests/golden/make_golden_metrics.py in tests/golden/metrics.npz: L1div, SRGR, jitter, motion beats, alignment, process_motion, diversity,
the embedding net and the Frechet distance.  Also re-asserted from the stored margins: the seeded inputs carry no knife-edge decision,
which is what lets the GPU tests demand exactly equal beat masks and SRGR counts.  No GPU needed."""
import os

import numpy as np
import pytest

from tests import metrics_ref as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics.npz"))
CASES = (128, 40)


def seeds(T):
    return [int(s) for s in G[f"T{T}_seeds"]]


@pytest.mark.parametrize("T", CASES)
def test_inputs_are_the_recorded_ones_and_carry_no_knife_edge(T):
    for i, s in enumerate(seeds(T)):
        assert np.array_equal(R.motion(s, T)[::13, ::29], G[f"T{T}_spot"][i])
        assert np.array_equal(R.target_of(s, T)[::13, ::29], G[f"T{T}_spot_target"][i])
        mb = min(R.beats(R.motion(s, T), o)[1] for o in R.ORDERS)
        ms = R.srgr_partial(R.motion(s, T), R.target_of(s, T), R.semantic_of(s, T))[2]
        assert mb == G[f"T{T}_margins"][i, 0] and ms == G[f"T{T}_margins"][i, 1]
        assert mb >= R.MARGIN and ms >= R.MARGIN, (s, mb, ms)


@pytest.mark.parametrize("T", CASES)
def test_per_sequence_metrics_against_the_reference(T):
    for i, s in enumerate(seeds(T)):
        x, t, sem = R.motion(s, T), R.target_of(s, T), R.semantic_of(s, T)
        # the reference computes these in float32: its own rounding is what separates it from the float64 restatement
        assert R.rel(R.l1div_partial(x), G[f"T{T}_ref_l1div"][i]) < 1e-5
        total, count, _ = R.srgr_partial(x, t, sem)
        assert R.rel(total / (T * 63), G[f"T{T}_ref_srgr_rate"][i]) < 1e-6
        assert count == G[f"T{T}_srgr_count"][i] and 0 < count < T * 63
        assert R.srgr_partial(x, t, sem, dtype=np.float32)[1] == count
        assert R.rel(R.jitter_sum(x, t) / ((T - 1) * 189), G[f"T{T}_ref_jitter"][i]) < 1e-5
        p = R.process_motion(x)
        assert R.rel(p[::5, ::7], G[f"T{T}_ref_processed_spot"][i]) < 1e-5
        if i == 0:
            assert R.rel(p, G[f"T{T}_ref_processed0"]) < 1e-5


@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("T", CASES)
def test_beats_and_alignment_against_the_reference(T, order):
    ref_beats, ref_align = G[f"T{T}_o{order}_ref_beats"], G[f"T{T}_o{order}_ref_align"]
    for i, s in enumerate(seeds(T)):
        for dtype in (np.float64, np.float32):
            assert np.array_equal(R.beats(R.motion(s, T), order, dtype)[0], ref_beats[i])
        assert not ref_beats[i][:, 0].any() and not ref_beats[i][:, -1].any()      # a frame compared with itself is never a beat
        on = R.onsets_of(s, R.ONSET_COUNTS[i % len(R.ONSET_COUNTS)], T)
        got = R.align_score(ref_beats[i][5], on, R.SIGMAS[order])
        if on.size == 0:
            assert got is None and np.isnan(ref_align[i])
        else:
            assert abs(got - ref_align[i]) < 1e-12
    assert ref_beats.sum() > 0
    assert R.align_score(np.zeros(T - 1, np.uint8), [0.5, 1.0], 0.3) == 0.0             # no beats: 0 per onset


def test_diversity_against_the_reference():
    rows = np.stack([R.process_motion(R.motion(int(s))).astype(np.float32) for s in G["div7_seeds"]])
    assert R.rel(R.avg_distance(rows), G["div7_ref"]) < 1e-5
    # the pair form against the definition
    want = np.mean([np.linalg.norm(rows[i].astype(np.float64) - rows[j]) for i in range(7) for j in range(i + 1, 7)])
    assert abs(R.avg_distance(rows) - want) < 1e-9 * want


def test_embedding_and_frechet_distance_against_the_reference():
    state = R.make_fgd_state(12, 41)
    assert np.array_equal(state["pose_encoder.out_net.0.weight"][::97, ::211], G["net12_spot"])
    x3 = np.stack([R.process_motion(R.motion(s)) for s in seeds(128)[:3]]).astype(np.float32)
    assert R.rel(R.embed(state, x3), G["emb12_ref"]) < 1e-5
    e = [R.embed(state, np.stack([R.process_motion(R.motion(first + i) * np.float32(1.0 if first == 200 else 1.1)) for i in range(48)]).astype(np.float32))
         for first in (200, 300)]
    assert abs(R.frechet(*e) - G["fgd_ref"]) <= 2 * float(G["fgd_ref_dist"]) * G["fgd_ref"] + 1e-9
    assert float(G["fgd_ref_dist"]) < 1e-3


def test_recorded_float32_distances_are_real():
    """Every gate of the GPU tests is FACTOR x one of these: none may be zero or absurd."""
    names = [k for k in G.files if "base" in k]
    assert len(names) >= 12
    for k in names:
        assert 1e-9 < float(G[k]) < 1e-5, (k, float(G[k]))
