"""CPU (-m "not gpu"): the host side of the audio onset detection -- the restatement tests/onset_ref.py against itself (librosa's
scipy-filter statement of peak_pick against the clipped-window statement the device computes, the backtrack against a brute-force one),
the window integers, the mirror's and the wav reader's refusals, and the decision margins of the golden waveforms."""
import os
import wave

import numpy as np
import pytest

from tests import onset_ref as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "onsets.npz"))
WINDOW_SETS = [(1, 1, 4, 5, 1), (7, 1, 25, 26, 7), (0, 1, 3, 4, 0), (3, 2, 2, 6, 4), (0, 3, 0, 1, 2)]


def envelopes():
    """A few hundred seeded envelopes in [0, 1]: smooth + noise, spiky, quantised (ties), constant; lengths from 1 on, many shorter than
    pre_avg + post_avg."""
    rng = np.random.default_rng(5)
    out = []
    for i in range(320):
        T = int(rng.integers(1, 12)) if i % 4 == 0 else int(rng.integers(12, 90))
        kind = i % 5
        if kind == 0:
            e = rng.random(T)
        elif kind == 1:
            e = np.abs(np.sin(np.arange(T) * rng.uniform(0.2, 1.5))) + 0.1 * rng.random(T)
        elif kind == 2:
            e = np.round(rng.random(T) * 4) / 4                      # ties: five levels
        elif kind == 3:
            e = np.full(T, rng.uniform(0.0, 2.0))                    # constant (one of them may be 0)
        else:
            e = (rng.random(T) < 0.15) * rng.random(T)               # sparse spikes on zeros
        out.append(e)
    out.append(np.zeros(9))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_clipped_windows_equal_scipy_filters(dtype):
    n_env = n_onsets = 0
    for e in envelopes():
        e = e.astype(dtype)
        x = R.normalise(e) if e.any() else e
        for win in WINDOW_SETS:
            fmax, favg = R.moving_filters(x, *win[:4])
            dmax, davg = R.moving_direct(x, *win[:4])
            assert np.array_equal(fmax, dmax), (win, len(x))
            # the filter's running sum and np.mean round differently: the two means agree to a few ulp, and the picks must agree wherever
            # the comparison is not inside that rounding
            np.testing.assert_allclose(favg, davg, rtol=0, atol=8 * np.finfo(dtype).eps)
            a = R.peak_pick_filters(x, *win[:4], R.DELTA, win[4])
            b = R.peak_pick_direct(x, *win[:4], R.DELTA, win[4])
            decided = np.abs(x - (davg + dtype(R.DELTA))).min() > 16 * np.finfo(dtype).eps if len(x) else True
            if decided:
                assert np.array_equal(a, b), (win, x)
                n_onsets += len(a)
            n_env += 1
    assert n_env > 1000 and n_onsets > 1000


def test_constant_and_zero_envelopes_have_no_onset_or_one_rule():
    win = R.windows(22050, 512)
    assert len(R.onset_detect(np.zeros(20), win)[0]) == 0
    assert len(R.onset_detect(np.full(20, np.nan), win)[0]) == 0
    # a constant non-zero envelope normalises to all zeros: x[n] != 0 fails everywhere
    assert len(R.onset_detect(np.full(20, 0.7), win)[0]) == 0


def test_greedy_pass_general_wait():
    assert R.greedy([3, 4, 5, 9, 10, 30], 0).tolist() == [3, 4, 5, 9, 10, 30]
    assert R.greedy([3, 4, 5, 9, 10, 30], 1).tolist() == [3, 5, 9, 30]
    assert R.greedy([3, 4, 5, 9, 10, 30], 7).tolist() == [3, 30]
    assert R.greedy([], 3).tolist() == []


def test_backtrack_against_brute_force():
    rng = np.random.default_rng(6)
    for i in range(200):
        T = int(rng.integers(1, 60))
        r = np.round(rng.random(T) * 6) / 6 if i % 2 else rng.random(T)         # (every other one with ties)
        ev = np.sort(rng.integers(0, T, size=int(rng.integers(0, 8))))
        got, want = R.backtrack(ev, r), R.backtrack_brute(ev, r)
        assert np.array_equal(got, want), (r, ev)
        assert (got <= ev).all()
    assert R.backtrack([5, 5, 6], np.array([3.0, 2, 1, 2, 3, 4, 5, 6])).tolist() == [2, 2, 2]     # duplicates stay


def test_window_integers():
    from convofusion_amd import audio
    for sr, hop, want in ((22050, 512, (1, 1, 4, 5, 1)), (16000, 512, (0, 1, 3, 4, 0)), (16000, 64, (7, 1, 25, 26, 7))):
        assert R.windows(sr, hop) == want
        assert audio.onset_windows(sr, hop) == want
    d = audio.OnsetDetector()
    assert d.windows == (1, 1, 4, 5, 1) and d.pad_frames == 3 and d.time_sr == 22050.0 and d.n_mels == 128
    assert audio.OnsetDetector(detect_sr=16000, hop_length=64, n_fft=256, n_mels=20).windows == (7, 1, 25, 26, 7)


def test_mirror_refusals():
    import torch
    from convofusion_amd import audio, metrics
    for kw in (dict(n_fft=1000), dict(hop_length=0), dict(n_mels=0), dict(n_mels=2000), dict(detect_sr=0), dict(time_sr=-1.0), dict(delta=-0.1),
               dict(lag=0), dict(amin=0.0), dict(top_db=-1.0), dict(detect_sr=-22050)):
        with pytest.raises(ValueError):
            audio.OnsetDetector(**kw)
    d = audio.OnsetDetector()
    with pytest.raises(ValueError):
        d.forward(torch.zeros(2, 3, 100))
    with pytest.raises(ValueError):
        d.forward(torch.zeros(2, 100, dtype=torch.int16))
    with pytest.raises(ValueError, match="frames per waveform"):                     # T over the workgroup's plan, before any device work
        d.forward(torch.zeros(1, audio.ONSET_MAX_FRAMES * 512))
    assert audio.frame_count(audio.ONSET_MAX_FRAMES * 512 - 1, 512) == audio.ONSET_MAX_FRAMES
    with pytest.raises(RuntimeError):                                                   # the product never computes on the CPU
        d.forward(torch.zeros(1, 16384))
    pred = torch.zeros(2, 128, 189)
    with pytest.raises(ValueError, match="not both"):
        metrics.motion_eval(pred, onsets=[[0.1], []], audio=torch.zeros(2, 16384))
    with pytest.raises(ValueError, match="not both"):
        metrics.MotionEvaluator().update(pred, onsets=[[0.1], []], audio=torch.zeros(2, 16384))
    for bad in (torch.zeros(3, 16384), torch.zeros(16384), torch.zeros(2, 16384, dtype=torch.int32)):
        with pytest.raises(ValueError):
            metrics.detect_onsets(bad, 2, torch.device("cpu"))


def _write_wav(path, samples, rate=16000, channels=1, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(samples.tobytes())


def test_wav_reader(tmp_path):
    from convofusion_amd import metrics
    pcm = (np.random.default_rng(3).integers(-32768, 32768, size=4000)).astype("<i2")
    _write_wav(tmp_path / "ok.wav", pcm)
    y = metrics.read_wav_pcm16(str(tmp_path / "ok.wav"))
    assert y.dtype == np.float32 and np.array_equal(y, pcm.astype(np.float32) / 32768.0)
    _write_wav(tmp_path / "rate.wav", pcm, rate=22050)
    _write_wav(tmp_path / "stereo.wav", pcm, channels=2)
    _write_wav(tmp_path / "byte.wav", pcm.astype(np.int8).view(np.uint8), width=1)
    _write_wav(tmp_path / "wide.wav", pcm.astype("<i4"), width=4)
    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    for name in ("rate", "stereo", "byte", "wide", "junk"):
        with pytest.raises(ValueError, match="stay with the caller"):
            metrics.read_wav_pcm16(str(tmp_path / f"{name}.wav"))
    # the directory reader: equal lengths only, and a missing file is an error
    for i, n in enumerate((4000, 3000)):
        d = tmp_path / "res" / "spk" / f"clip{i}"
        d.mkdir(parents=True)
        np.save(d / "gt.npy", np.zeros((24, 189), np.float32))
        _write_wav(d / "lsn_audio.wav", pcm[:n])
    with pytest.raises(ValueError, match="same"):
        metrics.read_result_audio(str(tmp_path / "res"))
    _write_wav(tmp_path / "res" / "spk" / "clip1" / "lsn_audio.wav", pcm)
    assert metrics.read_result_audio(str(tmp_path / "res")).shape == (2, 4000)
    os.remove(tmp_path / "res" / "spk" / "clip1" / "lsn_audio.wav")
    with pytest.raises(FileNotFoundError):
        metrics.read_result_audio(str(tmp_path / "res"))


def test_golden_waveforms_and_margins():
    """The stored waveforms are the seeded ones; every decision of the float64 restatement is made by the input: its margin exceeds
    MARGIN = 100 x the float32 restatement's error on the same quantity (re-asserted from the stored pairs), an onset is moved back to
    frame 0, and the greedy pass suppresses at least two candidates of the small configuration's case."""
    for name in ("a", "b", "c", "d", "flat", "faint"):
        assert np.array_equal(R.wave(name), G[name + "_wave"])
    assert np.array_equal(R.swell_wave(), G["swell_wave"])
    for name in ("a", "b", "c", "d", "flat", "swell"):
        for k in ("avg", "max", "rms"):
            margin, err = G[f"{name}_margin_{k}"]
            assert margin > R.MARGIN * err, (name, k, margin, err)
        assert len(G[name + "_raw"]) >= 2 and len(G[name + "_raw"]) == len(G[name + "_frames"])
    assert any((G[n + "_frames"] == 0).any() for n in ("a", "b", "c", "d"))
    assert len(G["swell_candidates"]) - len(G["swell_raw"]) >= 2
    assert len(G["faint_raw"]) == 0 and not G["faint_env"].any()
    # one case recomputed end to end (the others are the generator's): results and times as stored, times = frames * 512 / 22050
    d = R.detect(R.wave("a"), **R.PRODUCT)
    assert np.array_equal(d["raw"], G["a_raw"]) and np.array_equal(d["frames"], G["a_frames"]) and np.array_equal(d["times"], G["a_times"])
    assert np.array_equal(G["a_times"], G["a_frames"].astype(np.int64) * 512 / 22050.0)
