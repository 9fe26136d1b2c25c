#!/usr/bin/env python
"""Generate tests/golden/onsets.npz from tests/onset_ref.py (numpy + scipy only).

Cases: the burst waveforms a b c d and the audible constant-level noise ``flat`` at the product configuration (n_fft 2048, hop 512, 128
bands, windows from 22050) with peak normalisation; ``faint`` (constant-level noise far below amin) without it; ``swell`` at the small
configuration (n_fft 256, hop 64, 20 bands, windows from 16000: 7 / 1 / 25 / 26, wait 7).  ``silent`` is all zeros and needs no entry.

Stored per case:

    <case>_wave                         the seeded float32 waveform (tests regenerate and compare)
    <case>_env, <case>_rms              the float64 restatement's envelope and frame energies [T]
    <case>_raw, <case>_frames           its accepted frames and the backtracked ones, int32
    <case>_times                        frames * hop / 22050 (the small configuration: / 16000), float64
    <case>_candidates                   the frames peak_pick's three conditions pass, before the greedy pass
    <case>_base_env, <case>_base_rms    the float32 restatement's distance from float64 (onset_ref.env_dist): the base of the GPU gates
    <case>_margin_<avg|max|rms>         (margin, float32 error) pairs of onset_ref.margins -- asserted here to exceed MARGIN = 100, so that
                                        every decision is made by the input and not by rounding, and asserted again by the host test

The generator also asserts that the float32 restatement makes the same decisions as the float64 one, that some onset is moved back to
frame 0, and that the greedy pass suppresses at least two candidates of ``swell``.  Usage:  python tests/golden/make_golden_onsets.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import onset_ref as R  # noqa: E402


def case(out, name, y, cfg, norm=True, check=True):
    time_sr = cfg["detect_sr"]
    d64 = R.detect(y, **cfg, time_sr=time_sr, norm=norm)
    d32 = R.detect(y, **cfg, time_sr=time_sr, norm=norm, dtype=np.float32)
    out[name + "_wave"] = y
    for k in ("env", "rms", "raw", "frames", "times", "candidates"):
        out[f"{name}_{k}"] = d64[k]
    out[name + "_base_env"] = R.env_dist(d32["env"], d64["env"])
    out[name + "_base_rms"] = R.env_dist(d32["rms"], d64["rms"])
    for k in ("raw", "frames", "candidates"):
        assert np.array_equal(d32[k], d64[k]), (name, k, d32[k], d64[k])
    if check:
        for k, (margin, err) in R.margins(y, **cfg).items():
            assert margin > R.MARGIN * err, (name, k, margin, err)
            out[f"{name}_margin_{k}"] = np.array([margin, err])
    print(f"{name}: T {len(d64['env'])}, candidates {d64['candidates'].tolist()}, raw {d64['raw'].tolist()}, frames {d64['frames'].tolist()}, "
          f"base env {out[name + '_base_env']:.3e} rms {out[name + '_base_rms']:.3e}")
    return d64


def main():
    out = {}
    zero_backtrack = False
    for name in ("a", "b", "c", "d", "flat"):
        d = case(out, name, R.wave(name), R.PRODUCT)
        assert len(d["raw"]) >= 2
        zero_backtrack |= bool((d["frames"] == 0).any())
    assert zero_backtrack, "no onset is moved back to frame 0"
    d = case(out, "faint", R.wave("faint"), R.PRODUCT, norm=False, check=False)
    assert len(d["raw"]) == 0 and not d["env"].any() and np.isfinite(d["env"]).all()
    d = case(out, "swell", R.swell_wave(), R.SMALL)
    assert R.windows(R.SMALL["detect_sr"], R.SMALL["hop"]) == (7, 1, 25, 26, 7)
    assert len(d["candidates"]) - len(d["raw"]) >= 2, "the greedy pass suppresses fewer than two candidates"
    path = os.path.join(HERE, "onsets.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
