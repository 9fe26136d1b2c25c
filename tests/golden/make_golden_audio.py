#!/usr/bin/env python
"""Generate tests/golden/audio_frontend.npz from tests/audio_ref.py (numpy only).

Stored:

    fb_<sr>_<n_fft>_<n_mels>, hann_<n_fft>    the Slaney filterbank and the periodic Hann window, float64 (host tests compare
                                              convofusion_amd.audio's tables with them)
    fft<n_fft>_wave                           the seeded waveforms of the FFT-stage cases [2, 5 hop + 37] (tests regenerate and compare)
    fft<n_fft>_base                           the float32 restatement's max distance from float64 in power, relative to each frame's
                                              largest power
    <case>_wave                               the seeded waveform of every whole-call case (small, short, window)
    <case>_base_db                            the float32 restatement's max-abs distance from float64 in dB, every entry counted
    <case>_base_mem                           the float32 MLP of the float32 Mel against the float64 MLP of the float64 Mel: max-abs over
                                              the float64 output's RMS
    <case>_clip_share                         the share of the float64 entries that sit at the -80 dB clip

The bases are what the reference formulation itself loses in float32: the base of the GPU tests' gates (FACTOR x base), never measured
on the code under test.  Usage:  python tests/golden/make_golden_audio.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import audio_ref as R  # noqa: E402

TABLES = [(16000, 2048, 80), (16000, 512, 40), (16000, 256, 20)]
MLP_SEED = 31


def main():
    out = {}
    for sr, n_fft, n_mels in TABLES:
        out[f"fb_{sr}_{n_fft}_{n_mels}"] = R.mel_filterbank(sr, n_fft, n_mels)
        out[f"hann_{n_fft}"] = R.hann_periodic(n_fft)
    for n_fft, (_, hop, _) in R.FFT_CASES.items():
        w = R.fft_wave(n_fft)
        out[f"fft{n_fft}_wave"] = w
        base = max(R.frame_power_dist(R.power_spectrum(y, n_fft, hop, np.float32), R.power_spectrum(y, n_fft, hop, np.float64)) for y in w)
        out[f"fft{n_fft}_base"] = np.float64(base)
        print(f"fft {n_fft}: base {base:.3e}")
    for name, (n_fft, hop, n_mels, _, hidden, latent) in R.CALL_CASES.items():
        y = R.call_wave(name)
        sd = R.make_mlp(n_mels, hidden, latent, MLP_SEED)
        d64, d32 = (R.mel_db(y, R.SR, n_fft, hop, n_mels, dt) for dt in (np.float64, np.float32))
        assert d32.dtype == np.float32
        out[name + "_wave"] = y
        out[name + "_base_db"] = np.float64(R.db_dist(d32, d64))
        out[name + "_base_mem"] = np.float64(R.rms_dist(R.mlp(d32, sd, np.float32), R.mlp(d64, sd, np.float64)))
        out[name + "_clip_share"] = np.float64((d64 == -R.TOP_DB).mean())
        print(f"{name}: base {out[name + '_base_db']:.3e} dB, memory {out[name + '_base_mem']:.3e} of RMS, at the clip {out[name + '_clip_share']:.3f}")
    path = os.path.join(HERE, "audio_frontend.npz")
    np.savez_compressed(path, **out)
    print("wrote audio_frontend.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
