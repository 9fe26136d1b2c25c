"""Host tests of the log-Mel front end's Python side (convofusion_amd/audio.py, longform.audio_windows) and of the restatement the GPU
tests are gated by (tests/audio_ref.py).  No device."""
import os

import numpy as np
import pytest
import torch

from convofusion_amd import audio, longform
from tests import audio_ref as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "audio_frontend.npz"))
TABLES = [(16000, 2048, 80), (16000, 512, 40), (16000, 256, 20)]


@pytest.mark.parametrize("sr,n_fft,n_mels", TABLES)
def test_filterbank_and_window_match_golden(sr, n_fft, n_mels):
    fb = audio.mel_filterbank(sr, n_fft, n_mels)
    assert fb.dtype == np.float64 and fb.shape == (n_mels, n_fft // 2 + 1)
    np.testing.assert_allclose(fb, G[f"fb_{sr}_{n_fft}_{n_mels}"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(audio.hann_periodic(n_fft), G[f"hann_{n_fft}"], rtol=0, atol=1e-15)
    # the shape the kernel's band ranges rest on: at most two bands per bin, no empty band, every band one run of bins
    nz = fb != 0
    assert nz.sum(axis=0).max() <= 2 and nz.sum(axis=1).min() >= 1
    rng = audio.mel_ranges(fb)
    for m in range(n_mels):
        assert nz[m, rng[m, 0]:rng[m, 1]].all() and nz[m].sum() == rng[m, 1] - rng[m, 0]


def test_filterbank_properties():
    fb = audio.mel_filterbank(16000, 2048, 80)
    f = np.linspace(0, 8000, 1025)
    # Slaney normalisation: every triangle has unit area in Hz (up to the sampling of its slopes)
    area = (fb * (f[1] - f[0])).sum(axis=1)
    assert np.abs(area - 1.0).max() < 0.05
    assert fb[:, 0].max() == 0.0 and fb.min() >= 0.0
    w = audio.hann_periodic(8)
    np.testing.assert_allclose(w, [0, 0.14644661, 0.5, 0.85355339, 1, 0.85355339, 0.5, 0.14644661], atol=1e-8)
    tw = audio.twiddle_table(8)
    np.testing.assert_allclose(tw[2], [0, -1], atol=1e-15)
    np.testing.assert_allclose(tw[1], [np.sqrt(0.5), -np.sqrt(0.5)], atol=1e-15)


def test_frame_count():
    assert audio.frame_count(81920, 512) == 161
    assert audio.frame_count(655360, 512) == 1281
    assert audio.frame_count(4396, 512) == 9
    assert audio.frame_count(1, 512) == 1
    assert audio.frame_count(511, 512) == 1 and audio.frame_count(512, 512) == 2


@pytest.mark.parametrize("n_parts", [1, 2, 3, 8])
def test_window_and_activity_slices(n_parts):
    n_frames, n_bits = 160 * n_parts + 1, 8 * n_parts
    mel = audio.window_slices(n_frames, n_parts)
    bits = audio.activity_slices(n_bits, n_parts)
    assert len(mel) == len(bits) == 2 * n_parts - 1
    x = np.arange(n_frames)
    b = np.arange(n_bits)
    for i in range(2 * n_parts - 1):
        ln, bl = n_frames // n_parts, n_bits // n_parts
        assert mel[i] == (int(i / 2 * ln), min(int((i / 2 + 1) * ln) + 1, n_frames))      # (n_parts = 1: the + 1 runs past the end)
        assert bits[i] == (int(i / 2 * bl), int((i / 2 + 1) * bl))
        # ... and they cut what a slice with those bounds cuts
        assert np.array_equal(x[mel[i][0]:mel[i][1]], x[int(i / 2 * ln):int((i / 2 + 1) * ln) + 1])
        assert np.array_equal(b[bits[i][0]:bits[i][1]], b[int(i / 2 * bl):int((i / 2 + 1) * bl)])
        assert mel[i][1] - mel[i][0] == 161 and bits[i][1] - bits[i][0] == 8
    assert mel == R.window_slices(n_frames, n_parts) and bits == R.activity_slices(n_bits, n_parts)


def test_window_slices_example_and_odd_lengths():
    assert audio.window_slices(1281, 8)[14] == (1120, 1281)
    assert audio.window_slices(1281, 8)[1] == (80, 241)
    # a length without the spare frame: the last window is cut at the end, as the slice would be
    assert audio.window_slices(1280, 8)[14] == (1120, 1280)
    # an odd part length: int() floors the half steps
    assert audio.window_slices(3 * 161 + 1, 3) == [(0, 162), (80, 242), (161, 323), (241, 403), (322, 484)]
    with pytest.raises(ValueError):
        audio.window_slices(3, 4)
    with pytest.raises(ValueError):
        audio.activity_slices(8, 0)


def test_uncond_mel():
    m = audio.uncond_mel(161, 80)
    assert m.shape == (161, 80) and m.dtype == torch.float32
    assert bool((m[:, 40:45] == 0).all()) and bool((m[:, :40] == -90).all()) and bool((m[:, 45:] == -90).all())


def _encoder(n_mels=80, hidden=16, latent=8):
    from convofusion_amd.conditioning import AudioConvEncoder
    return AudioConvEncoder(n_mels, hidden, latent).eval()


def test_front_end_refusals_without_device():
    for kw in (dict(n_fft=1000), dict(n_fft=4096), dict(hop_length=0), dict(n_mels=0), dict(n_fft=256, n_mels=130), dict(fps=0),
               dict(activity_frames=0), dict(sample_rate=0)):
        with pytest.raises(ValueError):
            audio.AudioFrontEnd(**kw)
    with pytest.raises(ValueError, match="Mel bands"):
        audio.AudioFrontEnd(_encoder(n_mels=40))
    fe = audio.AudioFrontEnd()
    assert fe.act_chunk == 10240
    with pytest.raises(ValueError):
        fe.forward(np.zeros(100, np.float32))
    with pytest.raises(ValueError):
        fe.forward(torch.zeros(2, 3, 100))
    with pytest.raises(ValueError):
        fe.forward(torch.zeros(2, 0))
    with pytest.raises(ValueError):
        fe.forward(torch.zeros(100, dtype=torch.int32))
    for windows in (([0, 2], 9), ([-1], 3), ([], 3), ([0], 0), (list(range(65)), 1), 5):      # 4396 samples: 9 frames
        with pytest.raises(ValueError):
            fe.forward(torch.zeros(1, 4396), windows=windows)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fe.forward(torch.zeros(1, 4396))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fe.forward(torch.zeros(1, 4396), windows=([0, 1], 8))
    with pytest.raises(ValueError):
        fe.encode_mel(torch.zeros(1, 9, 80))


def test_from_model_shares_the_encoder():
    from types import SimpleNamespace
    enc = _encoder()
    enc.sample_rate, enc.hop_length, enc.fps = 16000, 256, 25
    model = SimpleNamespace(text_audio_encoder=SimpleNamespace(audio_encoder=enc))
    fe = audio.AudioFrontEnd.from_model(model, n_fft=1024)
    assert fe.audio_encoder is enc and fe.hop_length == 256 and fe.n_fft == 1024 and fe.n_mels == 80
    enc.sample_rate = enc.hop_length = enc.fps = None
    model.cfg = SimpleNamespace(DATASET=SimpleNamespace(BEATDND=SimpleNamespace(SR=16000, HOP_LEN=512, N_MELS=80)))
    fe = audio.AudioFrontEnd.from_model(model)
    assert (fe.sample_rate, fe.hop_length, fe.fps) == (16000, 512, 25)


def test_audio_windows_refusals_without_device():
    fe = audio.AudioFrontEnd(_encoder())
    good = torch.zeros(2, 2 * 81920)
    with pytest.raises(ValueError, match="audio_encoder"):
        longform.audio_windows(audio.AudioFrontEnd(), good, 3)
    with pytest.raises(ValueError, match="audio_encoder"):
        longform.audio_windows(None, good, 3)
    for n_windows in (0, 2, 4, -1):
        with pytest.raises(ValueError, match="odd"):
            longform.audio_windows(fe, good, n_windows)
    with pytest.raises(ValueError, match="n_parts"):
        longform.audio_windows(fe, torch.zeros(2, 2 * 81920 + 1), 3)
    with pytest.raises(ValueError, match="n_parts"):
        longform.audio_windows(fe, torch.zeros(2 * 81920), 3)
    with pytest.raises(ValueError, match="activity chunks"):
        longform.audio_windows(fe, torch.zeros(1, 2 * 5000), 3)
    with pytest.raises(ValueError, match="do not all have"):      # 2 x 81664 samples: 319 frames, windows of 160, 160 and 159 + the cut
        longform.audio_windows(fe, torch.zeros(1, 2 * 81664), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        longform.audio_windows(fe, good, 3)


@pytest.mark.parametrize("name", list(R.CALL_CASES))
def test_float32_switch_within_stored_base(name):
    """The all-float32 run of the restatement sits where the fixture says it does (the base of the GPU gates is reproducible), stays
    float32 to the output, and the fixture's waveform is the seeded one."""
    n_fft, hop, n_mels, n, hidden, latent = R.CALL_CASES[name]
    y = R.call_wave(name)
    assert np.array_equal(y, G[name + "_wave"]) and len(y) == n
    d64, d32 = (R.mel_db(y, R.SR, n_fft, hop, n_mels, dt) for dt in (np.float64, np.float32))
    assert d32.dtype == np.float32 and d64.dtype == np.float64 and d64.shape == (audio.frame_count(n, hop), n_mels)
    assert d64.max() == 0.0 and d64.min() >= -80.0
    base = float(G[name + "_base_db"])
    assert 0 < base < 1e-3
    assert R.db_dist(d32, d64) <= base * 1.0000001
    assert abs(float((d64 == -80.0).mean()) - float(G[name + "_clip_share"])) < 1e-12
    if name == "small":
        assert float(G[name + "_clip_share"]) == 0.125
    sd = R.make_mlp(n_mels, hidden, latent, 31)
    assert R.rms_dist(R.mlp(d32, sd, np.float32), R.mlp(d64, sd)) <= float(G[name + "_base_mem"]) * 1.0000001


@pytest.mark.parametrize("n_fft", list(R.FFT_CASES))
def test_fft_stage_base_and_framing(n_fft):
    _, hop, n = R.FFT_CASES[n_fft]
    w = R.fft_wave(n_fft)
    assert np.array_equal(w, G[f"fft{n_fft}_wave"]) and w.shape == (2, n)
    fr = R.frames(w[0], n_fft, hop)
    assert fr.shape == (6, n_fft)
    assert (fr[0, :n_fft // 2] == 0).all() and fr[0, n_fft // 2] == w[0, 0]                 # the first frame straddles the left padding
    assert (fr[5, n_fft // 2 + 37:] == 0).all() and fr[5, n_fft // 2 + 36] == w[0, -1]      # ... the last the right
    base = max(R.frame_power_dist(R.power_spectrum(y, n_fft, hop, np.float32), R.power_spectrum(y, n_fft, hop)) for y in w)
    assert base <= float(G[f"fft{n_fft}_base"]) * 1.0000001


def test_ref_normalize_and_activity():
    y = np.zeros((2, 4 * 100 + 30), np.float32)
    y[0, 99] = 0.5
    y[0, 100] = -0.25
    y[1, 415] = 3.0          # in the trailing partial chunk: it sets the peak, no bit
    yn, peak = R.normalize(y, np.float32)
    assert yn.dtype == np.float32 and np.array_equal(peak, np.float32([0.5, 3.0])) and yn[0, 99] == 1.0 and yn[0, 100] == -0.5
    assert R.activity_bits(yn[0], 100).tolist() == [1, 1, 0, 0] and R.activity_bits(yn[1], 100).tolist() == [0, 0, 0, 0]
    z, pz = R.normalize(np.zeros((1, 8), np.float32), np.float32)
    assert not np.isnan(z).any() and pz[0] == 0
    assert abs(R.act_thresh_power() - 10 ** -4.5) < 1e-20
