"""numpy restatement of the audio onset detection (cfd_audio_onsets, convofusion_amd/audio.py ``OnsetDetector``), written from librosa
0.10's documented behaviour with the arguments the reference's ``Alignment.load_audio`` passes (quant_eval/metric_eval.py:102-122):
``onset.onset_strength(y=y, sr=16000)`` (Mel power of 128 Slaney bands, ``power_to_db`` with ref = 1, positive first differences
averaged over the bands, shifted right by ``lag + n_fft // (2 hop)`` frames and cut to the spectrogram's length),
``onset.onset_detect(onset_envelope=e, backtrack=False)`` (normalisation, ``util.peak_pick`` with windows derived from librosa's default
``sr = 22050`` because none is passed), ``feature.rms(S=|stft(y)|)``, ``onset.onset_backtrack`` and ``frames_to_time`` (again at 22050).

``peak_pick_filters`` is librosa's own statement with scipy's ``maximum_filter1d`` / ``uniform_filter1d``; ``peak_pick_direct`` is the
clipped-window statement the device computes; tests/test_onsets_host.py holds the two equal.  Every function takes ``dtype``:
``np.float64`` (the yardstick) or ``np.float32`` (librosa's own float32 path, whose distance from float64 is the base of the gates,
tests/golden/make_golden_onsets.py).  **librosa itself is not installed where this was written; agreement with it is not verified.**
"""
import numpy as np

from tests import audio_ref as A

AMIN, TOP_DB, DELTA, LAG = 1e-10, 80.0, 0.07, 1
FACTOR = A.FACTOR
MARGIN = 100.0          # a decision's float64 margin must exceed MARGIN x the float32 restatement's error on the same quantity


def windows(detect_sr, hop):
    """(pre_max, post_max, pre_avg, post_avg, wait) as onset_detect hands them to peak_pick."""
    sr = detect_sr
    return (int(0.03 * sr // hop), int(0.00 * sr // hop + 1), int(0.10 * sr // hop), int(0.10 * sr // hop + 1), int(0.03 * sr // hop))


# ---------------------------------------------------------------- envelope and energy
def onset_strength(y, sr, n_fft, hop, n_mels, dtype=np.float64, lag=LAG, amin=AMIN, top_db=TOP_DB):
    """[T] of one waveform."""
    M = A.mel_power(y, sr, n_fft, hop, n_mels, dtype)                       # [T, n_mels]
    D = dtype(10.0) * np.log10(np.maximum(dtype(amin), M))                  # (ref = 1: 10 log10(max(amin, 1)) = 0)
    D = np.maximum(D, D.max() - dtype(top_db)).astype(dtype)
    T = M.shape[0]
    pad = lag + n_fft // (2 * hop)
    if T <= lag:
        return np.zeros(T, dtype)
    diff = np.maximum(dtype(0.0), D[lag:] - D[:-lag]).mean(axis=1).astype(dtype)
    return np.concatenate([np.zeros(pad, dtype), diff])[:T]


def rms(y, n_fft, hop, dtype=np.float64):
    """[T]: feature.rms(S=|stft(y)|, frame_length=n_fft) of one waveform."""
    x = A.power_spectrum(y, n_fft, hop, dtype).copy()
    x[:, 0] *= dtype(0.5)
    x[:, -1] *= dtype(0.5)
    return np.sqrt(dtype(2.0) * x.sum(axis=1) / dtype(n_fft) ** 2).astype(dtype)


def normalise(env):
    """onset_detect's normalisation, in env's dtype."""
    x = env - env.min()
    return (x / (x.max() + np.finfo(env.dtype).tiny)).astype(env.dtype)


# ---------------------------------------------------------------- peak picking
def moving_filters(x, pre_max, post_max, pre_avg, post_avg):
    """(mov_max, mov_avg) as util.peak_pick computes them with scipy's filters and its two border corrections."""
    from scipy.ndimage import maximum_filter1d, uniform_filter1d
    mov_max = maximum_filter1d(x, int(pre_max + post_max), mode="constant", origin=int(np.ceil(0.5 * (pre_max - post_max))), cval=x.min())
    mov_avg = uniform_filter1d(x, int(pre_avg + post_avg), mode="nearest", origin=int(np.ceil(0.5 * (pre_avg - post_avg))))
    n = 0
    while n - pre_avg < 0 and n < x.shape[0]:
        mov_avg[n] = np.mean(x[max(n - pre_avg, 0):n + post_avg])
        n += 1
    n = max(x.shape[0] - post_avg, 0)
    while n < x.shape[0]:
        mov_avg[n] = np.mean(x[max(n - pre_avg, 0):n + post_avg])
        n += 1
    return mov_max, mov_avg


def moving_direct(x, pre_max, post_max, pre_avg, post_avg):
    """The same two arrays from the windows [n - pre, n + post) clipped to [0, T)."""
    T = len(x)
    mov_max = np.array([x[max(n - pre_max, 0):min(n + post_max, T)].max() for n in range(T)], x.dtype)
    mov_avg = np.array([x[max(n - pre_avg, 0):min(n + post_avg, T)].mean() for n in range(T)], x.dtype)
    return mov_max, mov_avg


def greedy(candidates, wait):
    peaks, last = [], -np.inf
    for i in candidates:
        if i > last + wait:
            peaks.append(int(i))
            last = i
    return np.array(peaks, np.int32)


def _pick(x, mov_max, mov_avg, delta, wait):
    det = x * (x == mov_max)
    det = det * (det >= mov_avg + x.dtype.type(delta))
    cand = np.nonzero(det)[0]
    return greedy(cand, wait), cand


def peak_pick_filters(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    return _pick(x, *moving_filters(x, pre_max, post_max, pre_avg, post_avg), delta, wait)[0]


def peak_pick_direct(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    return _pick(x, *moving_direct(x, pre_max, post_max, pre_avg, post_avg), delta, wait)[0]


def onset_detect(env, win, delta=DELTA):
    """(accepted frames, candidates) of one envelope; an all-zero or non-finite envelope has none."""
    if not env.any() or not np.all(np.isfinite(env)):
        return np.zeros(0, np.int32), np.zeros(0, np.int64)
    x = normalise(env)
    return _pick(x, *moving_filters(x, *win[:4]), delta, win[4])


# ---------------------------------------------------------------- backtrack
def energy_minima(r):
    m = np.flatnonzero((r[1:-1] <= r[:-2]) & (r[1:-1] < r[2:])) + 1
    return np.unique(np.concatenate([[0], m])).astype(np.int64)


def backtrack(events, r):
    """onset_backtrack: every event moves to the largest energy minimum at or in front of it (frame 0 counts as one); duplicates stay."""
    minima = energy_minima(r)
    return minima[np.searchsorted(minima, np.asarray(events, np.int64), side="right") - 1].astype(np.int32)


def backtrack_brute(events, r):
    out = []
    for e in events:
        i = int(e)
        while i > 0 and not (1 <= i <= len(r) - 2 and r[i] <= r[i - 1] and r[i] < r[i + 1]):
            i -= 1
        out.append(i)
    return np.array(out, np.int32)


# ---------------------------------------------------------------- the whole chain
def detect(y, sr, n_fft, hop, n_mels, detect_sr=22050, time_sr=22050, delta=DELTA, dtype=np.float64, norm=True):
    """One waveform -> dict(env, rms, x, raw, frames, times, candidates)."""
    y = np.asarray(y)
    if norm:
        y = A.normalize(y, dtype)[0][0]
    env = onset_strength(y, sr, n_fft, hop, n_mels, dtype)
    r = rms(y, n_fft, hop, dtype)
    win = windows(detect_sr, hop)
    raw, cand = onset_detect(env, win, delta)
    frames = backtrack(raw, r) if len(raw) else np.zeros(0, np.int32)
    times = (frames.astype(np.int64) * hop) / float(time_sr)
    return dict(env=env, rms=r, x=normalise(env) if env.any() else env, raw=raw, frames=frames, times=times, candidates=cand)


def margins(y, sr, n_fft, hop, n_mels, detect_sr=22050, delta=DELTA, with_energy=True):
    """The decision margins of one waveform, each as (margin in float64, error of the float32 restatement on the same quantity):
    ``avg``  every frame's |x[n] - (mean x[window] + delta)|;
    ``max``  every gap |x[n] - x[j]|, j another entry of n's max window -- except pairs that are exactly 0 in BOTH restatements (the
             shift's leading zeros and frames whose bands all sit at the dB floor: zero by construction in any precision, and decided by
             x[n] != 0);
    ``rms``  every |r[i] - r[i + 1]| (both comparisons of every possible minimum)."""
    pre_max, post_max, pre_avg, post_avg, _ = windows(detect_sr, hop)
    d64 = detect(y, sr, n_fft, hop, n_mels, detect_sr, dtype=np.float64)
    d32 = detect(y, sr, n_fft, hop, n_mels, detect_sr, dtype=np.float32)
    x64, x32 = d64["x"], d32["x"].astype(np.float64)
    T = len(x64)
    out = {}
    q = lambda x: x - (moving_direct(x, pre_max, post_max, pre_avg, post_avg)[1] + delta)
    out["avg"] = (float(np.abs(q(x64)).min()), float(np.abs(q(x64) - q(x32)).max()))
    gaps, errs = [], [0.0]
    for n in range(T):
        for j in range(max(n - pre_max, 0), min(n + post_max, T)):
            if j == n or (x64[n] == 0 and x64[j] == 0 and x32[n] == 0 and x32[j] == 0):
                continue
            gaps.append(abs(x64[n] - x64[j]))
            errs.append(abs((x64[n] - x64[j]) - (x32[n] - x32[j])))
    out["max"] = (float(min(gaps)), float(max(errs)))
    if with_energy:
        g64, g32 = np.diff(d64["rms"]), np.diff(d32["rms"].astype(np.float64))
        out["rms"] = (float(np.abs(g64).min()), float(np.abs(g64 - g32).max()))
    return out


def env_dist(a, ref):
    """max |a - ref| / max |ref| (absolute where the reference is all zero)."""
    ref = np.asarray(ref, np.float64)
    s = np.abs(ref).max()
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / (s if s > 0 else 1.0))


# ---------------------------------------------------------------- the tests' seeded cases
SR = 16000
PRODUCT = dict(sr=SR, n_fft=2048, hop=512, n_mels=128, detect_sr=22050)
SMALL = dict(sr=SR, n_fft=256, hop=64, n_mels=20, detect_sr=16000)            # windows 7 / 1 / 25 / 26, wait 7
# name: (n_samples, seed, floor level, [(start sample, length, level)])
BURSTS = {
    "a": (16384, 21, 0.004, [(1500, 2500, 0.5), (7200, 2000, 0.25), (12000, 2200, 0.8)]),
    "b": (20480, 22, 0.006, [(900, 1800, 0.3), (6000, 2600, 0.7), (11500, 1500, 0.2), (16000, 2400, 0.55)]),
    "c": (24576, 113, 0.003, [(2600, 3000, 0.6), (9000, 2000, 0.15), (13500, 2500, 0.9), (19500, 2500, 0.4)]),
    "d": (24576, 54, 0.005, [(0, 2000, 0.45), (6500, 3000, 0.3), (14000, 1800, 0.75), (21000, 2000, 0.5)]),
}
BATCH = ("c", "d", "silent", "flat")           # equal lengths: one call of four against four calls of one


def burst_wave(name):
    """Seeded noise bursts of differing level on a quiet noise floor, float32."""
    n, seed, floor, bursts = BURSTS[name]
    rng = np.random.default_rng(seed)
    y = floor * rng.standard_normal(n)
    for start, length, level in bursts:
        y[start:start + length] += level * rng.standard_normal(min(length, n - start))
    return y.astype(np.float32)


FLAT_SEED = 21


def special_wave(name, n=24576):
    """silent: zeros.  flat: constant-level noise at an audible level.  faint: constant-level noise at 3e-8, for a call WITHOUT peak
    normalisation: every Mel power is orders below amin, every band sits at one dB value, the envelope is all zero and there is no onset.
    (An audible constant-level noise always has onsets: the centred transform's first frames are half padding, so the envelope is not
    flat, and after onset_detect's normalisation its largest entry is 1 whatever the level -- ``flat`` has two, and is checked like
    the burst cases.)"""
    if name == "silent":
        return np.zeros(n, np.float32)
    level = {"flat": 0.3, "faint": 3e-8}[name]
    return (level * np.random.default_rng(FLAT_SEED).standard_normal(n)).astype(np.float32)


def wave(name):
    return burst_wave(name) if name in BURSTS else special_wave(name)


def swell_wave(n=4096, seed=33):
    """The SMALL configuration's case: noise whose level swells ever faster (its dB curve is convex, so the envelope rises frame after
    frame and consecutive frames are candidates -- the greedy pass has something to suppress), twice, on a quiet floor."""
    rng = np.random.default_rng(seed)
    y = 0.002 * rng.standard_normal(n)
    for start in (500, 2300):
        t = np.arange(1400) / 1400.0
        y[start:start + 1400] += 0.002 * 10.0 ** (2.4 * t * t) * rng.standard_normal(1400)
    return y.astype(np.float32)
