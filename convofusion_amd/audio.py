"""The log-Mel front end on the HIP path: waveforms to Mel frames in dB, audio memories and activity bits in one library call
(cfd_audio_encode, csrc/audio_fe.hpp), and the audio onsets of the beat alignment in another (``OnsetDetector``: cfd_audio_onsets,
csrc/onset_fe.hpp).

The reference makes these in its data loader on the CPU with librosa 0.10 (convofusion/data/beat_dnd/dataset.py: ``get_melspecs``
:506-520 -- ``feature.melspectrogram`` + ``power_to_db(ref=np.max)`` --, ``check_audio`` :477-492 for the activity bits,
``util.normalize`` per BEAT chunk :473) and slices one utterance-long spectrogram per window for long-form runs
(unbounded_synthesis.py:279-308).  ``AudioFrontEnd`` takes the waveform on the device instead; resampling and file decoding other than
plain PCM stay with the caller.  The tables (Slaney filterbank, periodic Hann window, twiddles) are built here in float64 and rounded once.

librosa is not a dependency and was not available where this was written: the semantics follow its documentation and are held to a
float64 numpy restatement (tests/audio_ref.py); agreement with librosa itself is not verified (INTEGRATION.md section 3 has the
three-line comparison for someone who has it).  Inference only, CUDA tensors only, no CPU fallback.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

N_FFT_SUPPORTED = (256, 512, 1024, 2048)
MAX_SAMPLES = 1 << 26
MAX_WINDOWS = 64
AMIN, TOP_DB = 1e-10, 80.0
ACT_AMIN = 1e-5              # amplitude_to_db's amin


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3))


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)


def mel_filterbank(sr, n_fft, n_mels):
    """The Slaney Mel filterbank [n_mels, n_fft / 2 + 1], float64 (librosa.filters.mel with fmin 0, fmax sr / 2, htk=False, norm="slaney"):
    triangles between n_mels + 2 points equally spaced on Slaney's scale, each scaled by 2 / (its width in Hz)."""
    sr, n_fft, n_mels = float(sr), int(n_fft), int(n_mels)
    if n_fft < 2 or n_fft % 2 or n_mels < 1 or not sr > 0:
        raise ValueError(f"mel_filterbank: need sr > 0, an even n_fft >= 2 and n_mels >= 1 (got {sr}, {n_fft}, {n_mels})")
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.maximum(0.0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
    return w * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def mel_ranges(fb):
    """int32 [n_mels, 2]: first and one-past-last non-zero bin of every band (an empty band: 0, 0)."""
    nz = np.asarray(fb) != 0
    first = np.where(nz.any(axis=1), nz.argmax(axis=1), 0)
    last = np.where(nz.any(axis=1), nz.shape[1] - nz[:, ::-1].argmax(axis=1), 0)
    return np.stack([first, last], axis=1).astype(np.int32)


def hann_periodic(n_fft):
    """scipy.signal.get_window("hann", n_fft, fftbins=True), float64."""
    n = int(n_fft)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def twiddle_table(n_fft):
    """float64 [n_fft, 2]: (cos, -sin)(2 pi k / n_fft)."""
    ang = 2.0 * np.pi * np.arange(int(n_fft)) / int(n_fft)
    return np.stack([np.cos(ang), -np.sin(ang)], axis=1)


def frame_count(n_samples, hop):
    """Frames of a centred STFT: 1 + n_samples // hop."""
    return 1 + int(n_samples) // int(hop)


def uncond_mel(frames, n_mels):
    """The unconditional audio input (convofusion.py:914-915): -90 dB everywhere, columns 40:45 set to 0.  float32 [frames, n_mels]."""
    m = torch.full((int(frames), int(n_mels)), -90.0, dtype=torch.float32)
    m[:, 40:45] = 0.0
    return m


def window_slices(n_frames, n_parts):
    """The Mel frame ranges [start, stop) of the 2 n_parts - 1 half-overlapping windows of an utterance of n_frames frames
    (unbounded_synthesis.py:279,302, restated): with len = n_frames // n_parts, window i is [int(i / 2 * len), int((i / 2 + 1) * len) + 1),
    cut at n_frames as a slice is."""
    n, p = int(n_frames), int(n_parts)
    if p < 1 or n < p:
        raise ValueError(f"window_slices: need n_parts >= 1 and n_frames >= n_parts (got {n}, {p})")
    ln = n // p
    return [(int(i / 2 * ln), min(int((i / 2 + 1) * ln) + 1, n)) for i in range(2 * p - 1)]


def activity_slices(n_bits, n_parts):
    """The activity-bit ranges of the same windows (unbounded_synthesis.py:280,308): as ``window_slices`` without the + 1."""
    n, p = int(n_bits), int(n_parts)
    if p < 1 or n < p:
        raise ValueError(f"activity_slices: need n_parts >= 1 and n_bits >= n_parts (got {n}, {p})")
    ln = n // p
    return [(int(i / 2 * ln), min(int((i / 2 + 1) * ln), n)) for i in range(2 * p - 1)]


class AudioFrontEnd:
    """Waveform [U, n_samples] (float32, CUDA, mono, at ``sample_rate``) -> Mel frames in dB, the audio memory of ``audio_encoder`` (an
    ``AudioConvEncoder``-shaped module with ``main.0 / main.3 / out_net``; None: no memory), one activity bit per ``activity_frames`` motion
    frames (``int(activity_frames / fps * sample_rate)`` samples: amplitude_to_db(chunk, ref=1).max() > ``activity_db``) and the peaks."""

    def __init__(self, audio_encoder=None, sample_rate=16000, n_fft=2048, hop_length=512, n_mels=80, fps=25, activity_frames=16,
                 activity_db=-45.0):
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = int(sample_rate), int(n_fft), int(hop_length), int(n_mels)
        self.fps, self.activity_frames, self.activity_db = fps, int(activity_frames), float(activity_db)
        if self.n_fft not in N_FFT_SUPPORTED:
            raise ValueError(f"AudioFrontEnd: n_fft must be one of {N_FFT_SUPPORTED} (got {n_fft})")
        if self.hop_length < 1:
            raise ValueError(f"AudioFrontEnd: hop_length must be at least 1 (got {hop_length})")
        if not 1 <= self.n_mels <= self.n_fft // 2 + 1:
            raise ValueError(f"AudioFrontEnd: 1 <= n_mels <= n_fft / 2 + 1 = {self.n_fft // 2 + 1} (got {n_mels})")
        if self.sample_rate < 1 or not fps > 0 or self.activity_frames < 1:
            raise ValueError("AudioFrontEnd: sample_rate, fps and activity_frames must be positive")
        self.act_chunk = int(self.activity_frames / fps * self.sample_rate)          # dataset.py:481
        if self.act_chunk < 1:
            raise ValueError("AudioFrontEnd: an activity chunk is shorter than one sample")
        self.audio_encoder = audio_encoder
        if audio_encoder is not None:
            k = audio_encoder.main[0].weight.shape[1]
            if k != self.n_mels:
                raise ValueError(f"AudioFrontEnd: the encoder takes {k} Mel bands, the front end makes {self.n_mels}")
        self._tables = {}

    @classmethod
    def from_model(cls, model, **kwargs):
        """The front end of a Convofusion-like ``model``: its ``text_audio_encoder.audio_encoder`` (the parameters are shared, not copied)
        with the sample rate, hop length and fps that encoder was configured with, else ``cfg.DATASET.BEATDND``'s SR / HOP_LEN / N_MELS."""
        enc = model.text_audio_encoder.audio_encoder
        ds = getattr(getattr(getattr(model, "cfg", None), "DATASET", None), "BEATDND", None)
        kw = dict(n_mels=enc.main[0].weight.shape[1])
        for name, attr, key in (("sample_rate", "sample_rate", "SR"), ("hop_length", "hop_length", "HOP_LEN"), ("fps", "fps", None)):
            v = getattr(enc, attr, None)
            if v is None and ds is not None and key is not None:
                v = getattr(ds, key, None)
            if v is not None:
                kw[name] = v
        kw.update(kwargs)
        return cls(enc, **kw)

    def tables(self, device):
        """(twiddle, window, melfb, mel_range) on ``device``, built once per device in float64 and rounded to float32."""
        device = torch.device(device)
        t = self._tables.get(device)
        if t is None:
            fb = mel_filterbank(self.sample_rate, self.n_fft, self.n_mels).astype(np.float32)
            t = SimpleNamespace(
                twiddle=torch.from_numpy(twiddle_table(self.n_fft).astype(np.float32)).to(device),
                window=torch.from_numpy(hann_periodic(self.n_fft).astype(np.float32)).to(device),
                melfb=torch.from_numpy(fb).to(device), mel_range=torch.from_numpy(mel_ranges(fb)).to(device))
            self._tables[device] = t
        return t

    def check_windows(self, windows, n_samples):
        """``windows``: None, or (starts, frames) -- frame ranges [start, start + frames) taken from every waveform.  Returns (starts, frames)
        as ints, frames = the whole spectrogram's for None."""
        T = frame_count(n_samples, self.hop_length)
        if windows is None:
            return [], T
        try:
            starts, frames = windows
            starts, frames = [int(s) for s in starts], int(frames)
        except (TypeError, ValueError):
            raise ValueError("windows must be (starts, frames): a list of first frames and one frame count") from None
        if not 1 <= len(starts) <= MAX_WINDOWS:
            raise ValueError(f"windows: 1 to {MAX_WINDOWS} windows per call (got {len(starts)})")
        if frames < 1 or any(s < 0 or s + frames > T for s in starts):
            raise ValueError(f"windows: every window must lie inside the {T} frames of a waveform (starts {starts}, {frames} frames)")
        return starts, frames

    def _weights(self, device):
        enc = self.audio_encoder
        if getattr(enc, "training", False):
            raise NotImplementedError("the HIP audio front end is inference-only (call .eval() on the encoder)")
        return [p.detach().to(device=device, dtype=torch.float32).contiguous()
                for p in (enc.main[0].weight, enc.main[0].bias, enc.main[3].weight, enc.main[3].bias, enc.out_net.weight, enc.out_net.bias)]

    def forward(self, wave, *, normalize=False, windows=None):
        """wave [U, n_samples] (or [n_samples]) float32 on the device.  normalize: divide every waveform by its own max|y| first
        (``librosa.util.normalize``, as the reference does for BEAT chunks).  windows: None or (starts, frames).
        Returns a namespace: ``mel`` [U * max(W, 1), frames, n_mels] in dB (row u * W + w), ``memory`` [same rows, frames, latent] or None,
        ``activity`` int32 [U, n_samples // act_chunk] (on the waveform after normalisation), ``peak`` [U] (before it)."""
        if not isinstance(wave, torch.Tensor) or wave.dim() not in (1, 2) or not wave.is_floating_point():
            raise ValueError("AudioFrontEnd: wave must be a float tensor [U, n_samples] or [n_samples]")
        if wave.dim() == 1:
            wave = wave[None]
        U, n = (int(v) for v in wave.shape)
        if U < 1 or not 1 <= n <= MAX_SAMPLES:
            raise ValueError(f"AudioFrontEnd: 1 <= n_samples <= {MAX_SAMPLES} and at least one waveform (got {U} x {n})")
        starts, frames = self.check_windows(windows, n)
        if wave.device.type != "cuda":
            raise RuntimeError("convofusion_amd.audio runs on an MI355X only (tensors must be on 'cuda'); no CPU fallback")
        dev = wave.device
        y = wave.detach().to(torch.float32).contiguous()
        t = self.tables(dev)
        rows = U * max(len(starts), 1)
        a = _lib.AudioArgs()
        a.wave, a.n_wave, a.n_samples, a.normalize = y.data_ptr(), U, n, int(bool(normalize))
        a.n_fft, a.hop, a.n_mels = self.n_fft, self.hop_length, self.n_mels
        a.twiddle, a.window, a.melfb, a.mel_range = t.twiddle.data_ptr(), t.window.data_ptr(), t.melfb.data_ptr(), t.mel_range.data_ptr()
        a.amin, a.top_db = AMIN, TOP_DB
        win = (C.c_int32 * max(len(starts), 1))(*starts)
        a.n_win, a.win_start, a.win_frames = len(starts), C.cast(win, C.c_void_p), frames if starts else 0
        a.act_chunk, a.act_amin_power, a.act_thresh_power = self.act_chunk, ACT_AMIN ** 2, 10.0 ** (self.activity_db / 10.0)
        mel = torch.empty(rows, frames, self.n_mels, device=dev, dtype=torch.float32)
        memory = keep = None
        if self.audio_encoder is not None:
            keep = self._weights(dev)
            a.w0, a.b0, a.w1, a.b1, a.w2, a.b2 = (p.data_ptr() for p in keep)
            a.hidden, a.latent = keep[0].shape[0], keep[2].shape[0]
            memory = torch.empty(rows, frames, a.latent, device=dev, dtype=torch.float32)
        activity = torch.empty(U, n // self.act_chunk, device=dev, dtype=torch.int32)
        peak = torch.empty(U, device=dev, dtype=torch.float32)
        from .conditioning import _engine_handle
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.load().cfd_audio_encode(_engine_handle(dev), C.byref(a), C.c_void_p(mel.data_ptr()),
                                                    C.c_void_p(memory.data_ptr()) if memory is not None else None,
                                                    C.c_void_p(activity.data_ptr()), C.c_void_p(peak.data_ptr()), C.c_void_p(stream)))
        return SimpleNamespace(mel=mel, memory=memory, activity=activity, peak=peak)

    __call__ = forward

    def encode_mel(self, mel):
        """Mel frames [..., n_mels] through the same encoder (the mirror ``AudioConvEncoder``'s three ``cfd_linear_act`` launches)."""
        if self.audio_encoder is None:
            raise ValueError("AudioFrontEnd: no audio_encoder to encode with")
        from .conditioning import ACT_LEAKY01, ACT_NONE, linear_act
        w0, b0, w1, b1, w2, b2 = self._weights(mel.device)
        return linear_act(linear_act(linear_act(mel, w0, b0, ACT_LEAKY01), w1, b1, ACT_LEAKY01), w2, b2, ACT_NONE)


# ---------------------------------------------------------------- onset detection (cfd_audio_onsets, csrc/onset_fe.hpp)
ONSET_MAX_FRAMES = 2048          # what the detection workgroup's LDS plan holds (ONS_MAX_T)


def onset_windows(detect_sr, hop_length):
    """(pre_max, post_max, pre_avg, post_avg, wait) as ``librosa.onset.onset_detect`` derives them for ``peak_pick``: 0.03 s, 0.00 s + 1,
    0.10 s, 0.10 s + 1 and 0.03 s in frames of ``hop_length`` at ``detect_sr``, floor-divided as floats.  The reference passes no ``sr``,
    so its windows are those of librosa's default 22050: (1, 1, 4, 5, 1) at hop 512."""
    sr, hop = detect_sr, hop_length
    return (int(0.03 * sr // hop), int(0.00 * sr // hop + 1), int(0.10 * sr // hop), int(0.10 * sr // hop + 1), int(0.03 * sr // hop))


class OnsetResult:
    """What ``OnsetDetector.forward`` returns, all on the device: ``csr`` = (offsets int32 [U + 1], times float64 [capacity]) -- the pair
    ``metrics.motion_eval`` takes; waveform u owns entries offsets[u] .. offsets[u + 1] --, ``frames_raw`` / ``frames`` int32 [capacity]
    (the accepted frames and the backtracked ones, same segments), ``envelope`` / ``rms`` float32 [U, T], ``n_total`` int32 [1]."""

    def __init__(self, csr, frames_raw, frames, envelope, rms, n_total):
        self.csr, self.frames_raw, self.frames, self.envelope, self.rms, self.n_total = csr, frames_raw, frames, envelope, rms, n_total

    def host(self):
        """Host lists, one numpy array per waveform: (times float64, frames_raw int32, frames int32).  This is the one place that waits for
        the device and reads the total."""
        off = self.csr[0].cpu().numpy()
        n = int(self.n_total.item())
        t, fr, fb = self.csr[1][:n].cpu().numpy(), self.frames_raw[:n].cpu().numpy(), self.frames[:n].cpu().numpy()
        cut = lambda x: [x[off[u]:off[u + 1]] for u in range(len(off) - 1)]
        return cut(t), cut(fr), cut(fb)


class OnsetDetector:
    """Waveform [U, n_samples] (float32, CUDA, mono, equal lengths, at ``sample_rate``) -> audio onsets, as the reference's
    ``Alignment.load_audio`` (quant_eval/metric_eval.py:102-122) gets them from librosa 0.10: ``onset_strength(y, sr)``,
    ``onset_detect(onset_envelope, backtrack=False)``, ``feature.rms(S=|stft(y)|)``, ``onset_backtrack``, ``frames_to_time``.

    ``detect_sr`` sets the five window integers and ``time_sr`` the times (frame * hop_length / time_sr).  **Both default to 22050, not to
    the audio's 16000**: the reference passes no ``sr`` to ``onset_detect`` and ``frames_to_time``, so librosa's default rate applies;
    that is the reference's number, and 16000 can be chosen knowingly.  **librosa is not a dependency and agreement with librosa itself is
    not verified**: the formulas are librosa 0.10's as documented, held to the float64 restatement tests/onset_ref.py."""

    def __init__(self, sample_rate=16000, n_fft=2048, hop_length=512, n_mels=128, detect_sr=22050, time_sr=22050, delta=0.07, lag=1,
                 amin=AMIN, top_db=TOP_DB):
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = int(sample_rate), int(n_fft), int(hop_length), int(n_mels)
        self.detect_sr, self.time_sr, self.delta, self.lag = detect_sr, float(time_sr), float(delta), int(lag)
        self.amin, self.top_db = float(amin), float(top_db)
        if self.n_fft not in N_FFT_SUPPORTED:
            raise ValueError(f"OnsetDetector: n_fft must be one of {N_FFT_SUPPORTED} (got {n_fft})")
        if self.hop_length < 1 or self.sample_rate < 1:
            raise ValueError(f"OnsetDetector: hop_length and sample_rate must be at least 1 (got {hop_length}, {sample_rate})")
        if not 1 <= self.n_mels <= self.n_fft // 2 + 1:
            raise ValueError(f"OnsetDetector: 1 <= n_mels <= n_fft / 2 + 1 = {self.n_fft // 2 + 1} (got {n_mels})")
        if not detect_sr > 0 or not self.time_sr > 0:
            raise ValueError(f"OnsetDetector: detect_sr and time_sr must be positive (got {detect_sr}, {time_sr})")
        if not self.delta >= 0 or self.lag < 1 or not self.amin > 0 or not self.top_db >= 0:
            raise ValueError(f"OnsetDetector: delta >= 0, lag >= 1, amin > 0 and top_db >= 0 (got {delta}, {lag}, {amin}, {top_db})")
        self.windows = onset_windows(detect_sr, self.hop_length)
        pre_max, post_max, pre_avg, post_avg, wait = self.windows
        if min(pre_max, pre_avg, wait) < 0 or post_max < 1 or post_avg < 1:
            raise ValueError(f"OnsetDetector: the windows (pre_max, post_max, pre_avg, post_avg, wait) = {self.windows} are negative or empty")
        self.pad_frames = self.lag + self.n_fft // (2 * self.hop_length)
        self._tables = {}

    tables = AudioFrontEnd.tables           # (twiddle, window, melfb, mel_range) per device, built once

    def forward(self, wave, *, normalize=True):
        """wave [U, n_samples] (or [n_samples]) float32 on the device.  normalize: divide every waveform by its own max|y| first
        (``librosa.util.normalize``, as the reference does).  Returns an ``OnsetResult``; nothing visits the host."""
        if not isinstance(wave, torch.Tensor) or wave.dim() not in (1, 2) or not wave.is_floating_point():
            raise ValueError("OnsetDetector: wave must be a float tensor [U, n_samples] or [n_samples]")
        if wave.dim() == 1:
            wave = wave[None]
        U, n = (int(v) for v in wave.shape)
        if not 1 <= U <= 65535 or not 1 <= n <= MAX_SAMPLES:
            raise ValueError(f"OnsetDetector: 1 <= n_samples <= {MAX_SAMPLES} and 1 to 65535 waveforms (got {U} x {n})")
        T = frame_count(n, self.hop_length)
        if T > ONSET_MAX_FRAMES:
            raise ValueError(f"OnsetDetector: {T} frames per waveform, one call holds {ONSET_MAX_FRAMES} "
                             f"(fewer than {ONSET_MAX_FRAMES * self.hop_length} samples at hop {self.hop_length}); split the clip")
        if wave.device.type != "cuda":
            raise RuntimeError("convofusion_amd.audio runs on an MI355X only (tensors must be on 'cuda'); no CPU fallback")
        dev = wave.device
        y = wave.detach().to(torch.float32).contiguous()
        t = self.tables(dev)
        cap = U * T
        a = _lib.OnsetArgs()
        a.wave, a.n_wave, a.n_samples, a.normalize = y.data_ptr(), U, n, int(bool(normalize))
        a.n_fft, a.hop, a.n_mels = self.n_fft, self.hop_length, self.n_mels
        a.twiddle, a.window, a.melfb, a.mel_range = t.twiddle.data_ptr(), t.window.data_ptr(), t.melfb.data_ptr(), t.mel_range.data_ptr()
        a.amin, a.top_db, a.lag, a.pad_frames = self.amin, self.top_db, self.lag, self.pad_frames
        a.pre_max, a.post_max, a.pre_avg, a.post_avg, a.wait = self.windows
        a.delta, a.time_hop, a.time_sr, a.capacity = self.delta, self.hop_length, self.time_sr, cap
        off = torch.empty(U + 1, device=dev, dtype=torch.int32)
        times = torch.empty(cap, device=dev, dtype=torch.float64)
        raw = torch.empty(cap, device=dev, dtype=torch.int32)
        bt = torch.empty(cap, device=dev, dtype=torch.int32)
        env = torch.empty(U, T, device=dev, dtype=torch.float32)
        rms = torch.empty(U, T, device=dev, dtype=torch.float32)
        n_total = torch.empty(1, device=dev, dtype=torch.int32)
        a.envelope, a.rms, a.frames_raw, a.frames = env.data_ptr(), rms.data_ptr(), raw.data_ptr(), bt.data_ptr()
        from .conditioning import _engine_handle
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.load().cfd_audio_onsets(_engine_handle(dev), C.byref(a), C.c_void_p(off.data_ptr()), C.c_void_p(times.data_ptr()),
                                                    C.c_void_p(n_total.data_ptr()), C.c_void_p(stream)))
        return OnsetResult((off, times), raw, bt, env, rms, n_total)

    __call__ = forward
