"""GPU tests: audio onset detection in HIP (cfd_audio_onsets, convofusion_amd/audio.py ``OnsetDetector``, and ``audio=`` of
convofusion_amd/metrics.py) against the float64 restatement tests/onset_ref.py.  No librosa import.  The envelope and the frame energies
may lie at most FACTOR = 4 x as far from float64 as the float32 restatement does on the same input (tests/golden/onsets.npz); the raw
frames, the backtracked frames, the offsets and the times must be EQUAL -- the golden waveforms are chosen so that every decision has
100 x the float32 error to spare (tests/test_onsets_host.py).  No frame and no waveform is left out.  Measured distances are printed.

Measured on an MI355X (distance from float64 as a share of the largest entry; gate): envelope a 2.7e-8 (3.3e-7), b 5.4e-8 (1.4e-7),
c 4.9e-8 (5.6e-7), d 3.8e-8 (4.0e-7), flat 6.5e-8 (1.6e-7), swell 1.5e-7 (1.6e-6); energy 4.1e-8 - 9.9e-8 (9.5e-8 for swell's 6.2e-8,
1.5e-7 - 3.2e-7 otherwise)."""
import ctypes as C
import functools
import os
import wave

import numpy as np
import pytest

from tests import metrics_ref as M
from tests import onset_ref as R

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "onsets.npz"))
FACTOR = R.FACTOR
E_ARG, E_SHAPE = -1, -2


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _handle():
    import torch
    from convofusion_amd.conditioning import _engine_handle
    return _engine_handle(torch.device("cuda", torch.cuda.current_device()))


def audio_info():
    import torch
    from convofusion_amd import _lib
    info = torch.zeros(4, device="cuda")
    _lib.check(_lib.load().cfd_debug_read(_handle(), b"audio.info", C.c_void_p(info.data_ptr()), 4))
    return [int(v) for v in info.tolist()]


@functools.lru_cache(maxsize=None)
def detector(small=False):
    from convofusion_amd.audio import OnsetDetector
    if small:
        return OnsetDetector(detect_sr=16000, time_sr=16000, hop_length=64, n_fft=256, n_mels=20)
    return OnsetDetector()


def wave_of(name):
    y = R.swell_wave() if name == "swell" else R.wave(name)
    if name != "silent":
        assert np.array_equal(y, G[name + "_wave"])
    return y


def check_case(name, res, u, off_lo, off_hi, times, raw, frames):
    """Waveform u of a result against the stored float64 restatement of ``name``; the segment's contents are passed in as host arrays."""
    env, rms = res.envelope[u].cpu().numpy(), res.rms[u].cpu().numpy()
    for what, got, want, base in (("envelope", env, G[name + "_env"], float(G[name + "_base_env"])),
                                  ("energy", rms, G[name + "_rms"], float(G[name + "_base_rms"]))):
        d, gate = R.env_dist(got, want), FACTOR * base
        print(f"  {name} {what}: {d:.3e} of the largest entry (gate {gate:.3e})")
        assert got.shape == want.shape and np.isfinite(got).all()
        assert d <= gate, (name, what, d, gate)
    assert off_hi - off_lo == len(G[name + "_raw"])
    assert np.array_equal(raw, G[name + "_raw"]), (name, raw, G[name + "_raw"])
    assert np.array_equal(frames, G[name + "_frames"]), (name, frames, G[name + "_frames"])
    assert times.dtype == np.float64 and np.array_equal(times, G[name + "_times"])


# ---------------------------------------------------------------- 1., 2. the product configuration, one waveform per call
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "flat"])
def test_product_configuration_against_float64(name):
    import torch
    y = wave_of(name)
    res = detector().forward(dev(y))
    torch.cuda.synchronize()
    T = 1 + len(y) // 512
    assert audio_info()[:3] == [4, T, 1]                    # peak, frames, detection, CSR
    assert res.envelope.shape == (1, T) and res.csr[1].numel() == T
    times, raw, frames = res.host()
    off = res.csr[0].cpu().numpy()
    assert off.tolist() == [0, len(G[name + "_raw"])] and int(res.n_total.item()) == off[1]
    check_case(name, res, 0, off[0], off[1], times[0], raw[0], frames[0])
    assert np.array_equal(times[0], frames[0].astype(np.int64) * 512 / 22050.0)
    again = detector().forward(dev(y))                      # the same bits on every call
    for p, q in zip((res.csr[0], res.csr[1][:off[1]], res.frames_raw[:off[1]], res.frames[:off[1]], res.envelope, res.rms, res.n_total),
                    (again.csr[0], again.csr[1][:off[1]], again.frames_raw[:off[1]], again.frames[:off[1]], again.envelope, again.rms, again.n_total)):
        assert torch.equal(p, q)


# ---------------------------------------------------------------- 3. the small configuration: the greedy pass suppresses candidates
def test_small_configuration_greedy_pass():
    import torch
    y = wave_of("swell")
    det = detector(small=True)
    assert det.windows == (7, 1, 25, 26, 7)
    assert len(G["swell_candidates"]) - len(G["swell_raw"]) >= 2
    res = det.forward(dev(y))
    torch.cuda.synchronize()
    times, raw, frames = res.host()
    off = res.csr[0].cpu().numpy()
    check_case("swell", res, 0, off[0], off[1], times[0], raw[0], frames[0])
    assert np.array_equal(times[0], frames[0].astype(np.int64) * 64 / 16000.0)


# ---------------------------------------------------------------- 4. no onsets
def test_silent_and_faint_waveforms_have_empty_segments():
    import torch
    for name, normalize in (("silent", True), ("silent", False), ("faint", False)):
        y = wave_of(name)
        res = detector().forward(dev(y), normalize=normalize)
        torch.cuda.synchronize()
        env, rms = res.envelope.cpu().numpy(), res.rms.cpu().numpy()
        assert np.isfinite(env).all() and not env.any() and np.isfinite(rms).all()
        assert res.csr[0].cpu().tolist() == [0, 0] and int(res.n_total.item()) == 0
        if name == "silent":
            assert not rms.any()
        else:
            d, gate = R.env_dist(rms[0], G["faint_rms"]), FACTOR * float(G["faint_base_rms"])
            print(f"  faint energy: {d:.3e} (gate {gate:.3e})")
            assert d <= gate and len(G["faint_raw"]) == 0


# ---------------------------------------------------------------- 5. batches, capacity, the frame limit
def test_batch_equals_single_calls_bit_for_bit():
    import torch
    det = detector()
    ys = np.stack([wave_of(n) for n in R.BATCH])
    res = det.forward(dev(ys))
    torch.cuda.synchronize()
    assert audio_info()[:3] == [4, 49, 4]
    off = res.csr[0].cpu().numpy()
    times, raw, frames = res.host()
    assert off.tolist() == np.concatenate([[0], np.cumsum([0 if n == "silent" else len(G[n + "_raw"]) for n in R.BATCH])]).tolist()
    for u, name in enumerate(R.BATCH):
        one = det.forward(dev(ys[u]))
        n = int(one.n_total.item())
        assert n == off[u + 1] - off[u]
        assert torch.equal(one.envelope[0], res.envelope[u]) and torch.equal(one.rms[0], res.rms[u])
        assert torch.equal(one.csr[1][:n], res.csr[1][off[u]:off[u + 1]])
        assert torch.equal(one.frames_raw[:n], res.frames_raw[off[u]:off[u + 1]]) and torch.equal(one.frames[:n], res.frames[off[u]:off[u + 1]])
        if name != "silent":
            check_case(name, res, u, off[u], off[u + 1], times[u], raw[u], frames[u])
    assert off[3] == off[2]                                 # the silent waveform's segment is empty, the one behind it is not
    assert off[4] > off[3]


def _raw_call(det, y, capacity, n_fft=None):
    """cfd_audio_onsets with a capacity (or n_fft) of the caller's; returns the error code."""
    import torch
    from convofusion_amd import _lib
    U, n = y.shape
    t = det.tables(y.device)
    a = _lib.OnsetArgs()
    a.wave, a.n_wave, a.n_samples, a.normalize = y.data_ptr(), U, n, 1
    a.n_fft, a.hop, a.n_mels = n_fft or det.n_fft, det.hop_length, det.n_mels
    a.twiddle, a.window, a.melfb, a.mel_range = t.twiddle.data_ptr(), t.window.data_ptr(), t.melfb.data_ptr(), t.mel_range.data_ptr()
    a.amin, a.top_db, a.lag, a.pad_frames = det.amin, det.top_db, det.lag, det.pad_frames
    a.pre_max, a.post_max, a.pre_avg, a.post_avg, a.wait = det.windows
    a.delta, a.time_hop, a.time_sr, a.capacity = det.delta, det.hop_length, det.time_sr, capacity
    off = torch.full((U + 1,), -7, device="cuda", dtype=torch.int32)
    times = torch.zeros(max(capacity, 1), device="cuda", dtype=torch.float64)
    code = _lib.load().cfd_audio_onsets(_handle(), C.byref(a), C.c_void_p(off.data_ptr()), C.c_void_p(times.data_ptr()), None, None)
    torch.cuda.synchronize()
    return code, off, _lib.load().cfd_last_error().decode()


def test_refusals_come_before_any_launch():
    import torch
    det = detector()
    y = dev(np.stack([wave_of("c"), wave_of("d")]))
    T, wait = 49, det.windows[4]
    need = 2 * ((T + wait) // (wait + 1))
    code, off, msg = _raw_call(det, y, need - 1)            # an undersized capacity
    assert code == E_SHAPE and "capacity" in msg and audio_info()[0] == 0 and (off == -7).all()
    code, off, _ = _raw_call(det, y, need)                  # the bound itself is admitted
    assert code == 0 and off.cpu().tolist() == [0, len(G["c_raw"]), len(G["c_raw"]) + len(G["d_raw"])]
    code, off, msg = _raw_call(det, y, 2 * T, n_fft=1000)   # n_fft outside the supported four
    assert code == E_ARG and "n_fft" in msg and audio_info()[0] == 0
    # T over the limit: the mirror refuses it, and so does the library
    long = torch.zeros(1, 2048 * 512, device="cuda")
    with pytest.raises(ValueError, match="frames per waveform"):
        det.forward(long)
    code, off, msg = _raw_call(det, long, 4096)
    assert code == E_SHAPE and "frames" in msg and audio_info()[0] == 0 and (off == -7).all()


def test_the_frame_limit_itself_is_admitted():
    """2048 frames, the most one workgroup's plan holds: bursts at both ends of the clip are found, with every scan slot in use."""
    import torch
    n = 2048 * 512 - 1
    rng = np.random.default_rng(17)
    y = (0.002 * rng.standard_normal(n)).astype(np.float32)
    for start in (40000, n - 60000):
        y[start:start + 8000] += (0.5 * rng.standard_normal(8000)).astype(np.float32)
    res = detector().forward(dev(y))
    torch.cuda.synchronize()
    assert audio_info()[:3] == [4, 2048, 1]
    times, raw, frames = res.host()
    assert np.isfinite(res.envelope.cpu().numpy()).all()
    assert (np.diff(raw[0]) > 1).all() and (frames[0] <= raw[0]).all() and raw[0].max() < 2048
    assert any(abs(int(f) - (40000 // 512 + 2)) <= 3 for f in raw[0]) and any(abs(int(f) - ((n - 60000) // 512 + 2)) <= 3 for f in raw[0])
    assert np.array_equal(times[0], frames[0].astype(np.int64) * 512 / 22050.0)


# ---------------------------------------------------------------- 6. the evaluator
@functools.lru_cache(maxsize=None)
def motions(n):
    return np.stack([M.motion(100 + i, 128) for i in range(n)])


@pytest.mark.parametrize("names", [("c", "d", "flat"), ("c", "silent", "d", "flat")])
def test_evaluator_with_audio_equals_evaluator_with_the_restatements_times(names):
    import torch
    from convofusion_amd.metrics import MotionEvaluator, motion_eval
    pred = dev(motions(len(names)))
    ys = dev(np.stack([wave_of(n) for n in names]))
    lists = [np.zeros(0) if n == "silent" else G[n + "_times"] for n in names]
    a, b = MotionEvaluator(), MotionEvaluator()
    a.update(pred, audio=ys)
    b.update(pred, onsets=lists)
    ra, rb = a.compute(), b.compute()
    torch.cuda.synchronize()
    assert ra["align"] is not None and ra["align"] == rb["align"]            # the same bits
    assert ra["align_counted"] == rb["align_counted"] == len(names) - ("silent" in names)
    per_a = motion_eval(pred, audio=ys, want={"align"})["align"]
    per_b = motion_eval(pred, onsets=lists, want={"align"})["align"]
    assert torch.equal(per_a, per_b)
    with pytest.raises(ValueError, match="not both"):
        a.update(pred, onsets=lists, audio=ys)


# ---------------------------------------------------------------- 7. a result directory
def pcm_of(name):
    y = wave_of(name)
    return np.clip(np.round(y / np.abs(y).max() * 30000), -32768, 32767).astype("<i2")


def test_result_directory_with_detected_onsets(tmp_path):
    import torch
    from convofusion_amd.metrics import evaluate_result_dir
    rng = np.random.default_rng(9)
    clips = []
    for i, name in enumerate(("c", "d")):
        # 16-bit PCM holds the waveform rounded to 1 / 32768: the restatement runs on what the file holds, and its decisions keep
        # the same room from rounding as the golden ones'
        pcm = pcm_of(name)
        y = pcm.astype(np.float32) / np.float32(32768.0)
        for k, (margin, err) in R.margins(y, **R.PRODUCT).items():
            assert margin > R.MARGIN * err, (name, k, margin, err)
        mo = motions(2)[i]
        clips.append((pcm, R.detect(y, **R.PRODUCT), mo, mo + 0.01 * rng.standard_normal(mo.shape).astype(np.float32)))
    for root, with_onsets in ((tmp_path / "wav", False), (tmp_path / "npy", True)):
        for i, (pcm, d, mo, gt) in enumerate(clips):
            p = root / "spk" / f"clip{i}"
            p.mkdir(parents=True)
            np.save(p / "pred.npy", mo)
            np.save(p / "gt.npy", gt)
            np.save(p / "sem_lsn.npy", np.ones(128, np.float32))
            if with_onsets:
                np.save(p / "onsets.npy", d["times"])
            else:
                with wave.open(str(p / "lsn_audio.wav"), "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(16000)
                    w.writeframes(pcm.tobytes())
    assert all(len(c[1]["raw"]) >= 2 for c in clips)
    got = evaluate_result_dir(str(tmp_path / "wav"), detect_onsets=True)
    torch.cuda.synchronize()
    want = evaluate_result_dir(str(tmp_path / "npy"))
    assert got["align"] is not None and got["align_counted"] == 2
    assert got == want                                      # every figure, the alignment's bits among them
    with pytest.raises(FileNotFoundError):
        evaluate_result_dir(str(tmp_path / "npy"), detect_onsets=True)          # no lsn_audio.wav there
