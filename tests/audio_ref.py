"""numpy restatement of the log-Mel front end (cfd_audio_encode, convofusion_amd/audio.py), written from librosa 0.10's documented
behaviour: ``feature.melspectrogram`` with its defaults (``center=True``, ``pad_mode="constant"``, ``win_length = n_fft``, periodic Hann,
``power=2.0``, Slaney filterbank ``fmin=0, fmax=sr/2, htk=False, norm="slaney"``), ``power_to_db(ref=np.max, amin=1e-10, top_db=80)``,
``util.normalize`` (inf-norm), ``amplitude_to_db(chunk, ref=1).max() > threshold`` per chunk, and the three Linear layers of
``AudioConvEncoder`` (LeakyReLU 0.1 behind the first two).

Every function takes ``dtype``: ``np.float64`` (the reference of the tests) or ``np.float32``, which runs every array in float32 -- the
window product, numpy's FFT (pocketfft computes in the input's precision), the power, the filterbank product, log10 and the output --
as librosa does on a float32 waveform.  The float32 run's distance from the float64 run is the base of the tests' gates
(tests/golden/make_golden_audio.py).
"""
import numpy as np

AMIN, TOP_DB = 1e-10, 80.0
ACT_AMIN, ACT_DB = 1e-5, -45.0
FACTOR = 4.0            # the gate: FACTOR x the float32 restatement's own distance from float64 (as tests/test_gpu_t5.py)


# ---------------------------------------------------------------- tables (float64)
def hz_to_mel(f):
    """Slaney's scale: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)."""
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)


def mel_filterbank(sr, n_fft, n_mels):
    """[n_mels, n_fft / 2 + 1] float64: triangles between n_mels + 2 points equally spaced in mel from 0 to sr / 2, each divided by half
    its width in Hz (norm="slaney")."""
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def hann_periodic(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def frame_count(n_samples, hop):
    return 1 + n_samples // hop


# ---------------------------------------------------------------- the transform
def normalize(y, dtype=np.float64):
    """y / max|y| per waveform (rows of a 2-D array); a peak below float32 tiny leaves the waveform as it is.  Returns (y, peak)."""
    y = np.atleast_2d(np.asarray(y)).astype(dtype)
    peak = np.abs(y).max(axis=1)
    div = np.where(peak < np.finfo(np.float32).tiny, 1.0, peak).astype(dtype)
    return (y / div[:, None]).astype(dtype), peak


def frames(y, n_fft, hop, dtype=np.float64):
    """[T, n_fft] frames of one waveform, centred, zero padded by n_fft / 2 on both sides."""
    y = np.asarray(y).astype(dtype)
    pad = np.concatenate([np.zeros(n_fft // 2, dtype), y, np.zeros(n_fft // 2, dtype)])
    T = frame_count(len(y), hop)
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return pad[idx]


def power_spectrum(y, n_fft, hop, dtype=np.float64):
    """[T, n_fft / 2 + 1] |rfft(window * frame)|^2 of one waveform."""
    win = hann_periodic(n_fft).astype(dtype)
    spec = np.fft.rfft(frames(y, n_fft, hop, dtype) * win, axis=1)
    assert spec.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    return (np.abs(spec) ** 2).astype(dtype)


def mel_power(y, sr, n_fft, hop, n_mels, dtype=np.float64):
    fb = mel_filterbank(sr, n_fft, n_mels).astype(dtype)
    return (power_spectrum(y, n_fft, hop, dtype) @ fb.T).astype(dtype)


def power_to_db(S, dtype=np.float64, amin=AMIN, top_db=TOP_DB):
    """ref = the largest entry of S (one waveform's whole spectrogram)."""
    S = np.asarray(S).astype(dtype)
    amin = dtype(amin)
    db = dtype(10.0) * np.log10(np.maximum(amin, S))
    db = db - dtype(10.0) * np.log10(np.maximum(amin, S.max()))
    return np.maximum(db, db.max() - dtype(top_db)).astype(dtype)


def mel_db(y, sr, n_fft, hop, n_mels, dtype=np.float64):
    """[T, n_mels]: what ``get_melspecs`` returns for one waveform (transposed, as it does)."""
    return power_to_db(mel_power(y, sr, n_fft, hop, n_mels, dtype), dtype)


def activity_bits(y, chunk, dtype=np.float64, threshold_db=ACT_DB, amin=ACT_AMIN):
    """One bit per whole chunk of ``chunk`` samples: amplitude_to_db(chunk, ref=1).max() > threshold_db."""
    y = np.asarray(y).astype(dtype)
    n = len(y) // chunk
    p = (np.abs(y[:n * chunk]).reshape(n, chunk) ** 2).astype(dtype)
    db = dtype(10.0) * np.log10(np.maximum(dtype(amin) ** 2, p))
    return (db.max(axis=1) > threshold_db).astype(np.int32)


def act_thresh_power(threshold_db=ACT_DB):
    return 10.0 ** (threshold_db / 10.0)


# ---------------------------------------------------------------- the encoder
def make_mlp(n_mels, hidden, latent, seed):
    """Seeded AudioConvEncoder weights (state-dict keys), float32."""
    rng = np.random.default_rng(seed)

    def lin(n, k):
        return (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)
    sd = {}
    sd["main.0.weight"], sd["main.0.bias"] = lin(hidden, n_mels)
    sd["main.3.weight"], sd["main.3.bias"] = lin(latent, hidden)
    sd["out_net.weight"], sd["out_net.bias"] = lin(latent, latent)
    return sd


def mlp(x, sd, dtype=np.float64):
    def leaky(v):
        return np.where(v > 0, v, dtype(0.1) * v)
    w = {k: v.astype(dtype) for k, v in sd.items()}
    h = leaky(np.asarray(x).astype(dtype) @ w["main.0.weight"].T + w["main.0.bias"])
    h = leaky(h @ w["main.3.weight"].T + w["main.3.bias"])
    return (h @ w["out_net.weight"].T + w["out_net.bias"]).astype(dtype)


# ---------------------------------------------------------------- slicing (unbounded_synthesis.py:279-308, restated)
def window_slices(n_frames, n_parts):
    ln = n_frames // n_parts
    return [(int(i / 2 * ln), min(int((i / 2 + 1) * ln) + 1, n_frames)) for i in range(2 * n_parts - 1)]


def activity_slices(n_bits, n_parts):
    ln = n_bits // n_parts
    return [(int(i / 2 * ln), min(int((i / 2 + 1) * ln), n_bits)) for i in range(2 * n_parts - 1)]


# ---------------------------------------------------------------- distances
def db_dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def rms_dist(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.sqrt((ref ** 2).mean()))


def frame_power_dist(p, ref):
    """max over frames of max|p - ref| / the frame's largest reference power (frames of all-zero power: counted absolute)."""
    ref = np.asarray(ref, np.float64)
    scale = ref.max(axis=-1, keepdims=True)
    scale = np.where(scale > 0, scale, 1.0)
    return float((np.abs(np.asarray(p, np.float64) - ref) / scale).max())


# ---------------------------------------------------------------- the tests' seeded cases
SR = 16000
FFT_CASES = {n: (n, n // 4, 5 * (n // 4) + 37) for n in (256, 512, 1024, 2048)}      # n_fft, hop, n_samples: 6 frames
# name: (n_fft, hop, n_mels, n_samples, hidden, latent)
CALL_CASES = {"small": (256, 64, 20, 1000, 24, 16), "short": (2048, 512, 80, 4396, 128, 512), "window": (2048, 512, 80, 81920, 128, 512)}


def fft_wave(n_fft):
    _, _, n = FFT_CASES[n_fft]
    rng = np.random.default_rng(100 + n_fft)
    t = np.arange(n) / SR
    tone = 0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.25 * np.sin(2 * np.pi * 3000.0 * t)
    return np.stack([tone + 0.1 * rng.standard_normal(n), 0.3 * rng.standard_normal(n)]).astype(np.float32)


def call_wave(name):
    """One float32 waveform per case.  small: noise + tone, last quarter silent.  short: noise + tone.  window: a 100 Hz - 6 kHz chirp
    plus noise, silent after 4.2 s."""
    n = CALL_CASES[name][3]
    rng = np.random.default_rng({"small": 7, "short": 8, "window": 9}[name])
    t = np.arange(n) / SR
    if name == "window":
        y = 0.6 * np.sin(2 * np.pi * (100.0 * t + 0.5 * (5900.0 / t[-1]) * t * t)) + 0.05 * rng.standard_normal(n)
        y[int(4.2 * SR):] = 0.0
    else:
        y = 0.4 * np.sin(2 * np.pi * 700.0 * t) + 0.2 * rng.standard_normal(n)
        if name == "small":
            y[3 * n // 4:] = 0.0
    return y.astype(np.float32)
