"""GPU tests: the log-Mel front end in one HIP call (cfd_audio_encode, convofusion_amd/audio.py, longform.audio_windows) against the float64
restatement tests/audio_ref.py.  No librosa import; weights are seeded.  The gate of every comparison is FACTOR = 4 x what the float32
restatement of the same formulas loses against float64 on the same input (tests/golden/audio_frontend.npz): the device's float32 FFT has
another butterfly order than pocketfft's.  No entry is excluded anywhere.  Measured distances are printed."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import audio_ref as R

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "audio_frontend.npz"))
FACTOR = R.FACTOR
MLP_SEED = 31
E_ARG, E_SHAPE = -1, -2


def _handle():
    import torch
    from convofusion_amd.conditioning import _engine_handle
    return _engine_handle(torch.device("cuda", torch.cuda.current_device()))


def audio_info():
    """cfd_debug_read "audio.info": launches of the last call (0: refused), frames per waveform, output rows, workspace bytes"""
    import torch
    from convofusion_amd import _lib
    info = torch.zeros(4, device="cuda")
    _lib.check(_lib.load().cfd_debug_read(_handle(), b"audio.info", C.c_void_p(info.data_ptr()), 4))
    return [int(v) for v in info.tolist()]


def _encoder(n_mels, hidden, latent):
    import torch
    from convofusion_amd.conditioning import AudioConvEncoder
    enc = AudioConvEncoder(n_mels, hidden, latent)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in R.make_mlp(n_mels, hidden, latent, MLP_SEED).items()}, strict=True)
    return enc.cuda().eval()


@functools.lru_cache(maxsize=None)
def front_end(name, with_encoder=True):
    from convofusion_amd.audio import AudioFrontEnd
    n_fft, hop, n_mels, _, hidden, latent = R.CALL_CASES[name]
    return AudioFrontEnd(_encoder(n_mels, hidden, latent) if with_encoder else None, sample_rate=R.SR, n_fft=n_fft, hop_length=hop, n_mels=n_mels)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(mel_db float64 [T, n_mels], memory float64 [T, latent]) of the case's waveform, computed once and shared (callers do not write)"""
    n_fft, hop, n_mels, _, hidden, latent = R.CALL_CASES[name]
    y = R.call_wave(name)
    assert np.array_equal(y, G[name + "_wave"])
    d = R.mel_db(y, R.SR, n_fft, hop, n_mels)
    return d, R.mlp(d, R.make_mlp(n_mels, hidden, latent, MLP_SEED))


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------- 1. the FFT stage alone
@pytest.mark.parametrize("n_fft", [256, 512, 1024, 2048])
def test_fft_stage_power(n_fft):
    import torch
    from convofusion_amd import _lib, audio
    _, hop, n = R.FFT_CASES[n_fft]
    w = R.fft_wave(n_fft)
    assert np.array_equal(w, G[f"fft{n_fft}_wave"])
    tw = dev(audio.twiddle_table(n_fft).astype(np.float32))
    win = dev(audio.hann_periodic(n_fft).astype(np.float32))
    y = dev(w)
    T = audio.frame_count(n, hop)
    assert T == 6
    out = torch.full((2, T, n_fft // 2 + 1), float("nan"), device="cuda")
    _lib.check(_lib.load().cfd_audio_power(_handle(), C.c_void_p(y.data_ptr()), 2, n, n_fft, hop, C.c_void_p(tw.data_ptr()),
                                           C.c_void_p(win.data_ptr()), C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert audio_info()[:3] == [1, T, 2]
    gate = FACTOR * float(G[f"fft{n_fft}_base"])
    for u in range(2):
        e = R.frame_power_dist(got[u], R.power_spectrum(w[u], n_fft, hop))
        print(f"fft {n_fft} waveform {u}: {e:.3e} of the frame's largest power (gate {gate:.3e})")
        assert e <= gate, (e, gate)


# ---------------------------------------------------------------- 2., 3., 7. the whole call
@pytest.mark.parametrize("name", ["small", "short", "window"])
def test_whole_call_against_float64(name):
    import torch
    want_db, want_mem = reference(name)
    fe = front_end(name)
    r = fe.forward(dev(R.call_wave(name))[None])
    torch.cuda.synchronize()
    T = want_db.shape[0]
    assert r.mel.shape == (1, T, want_db.shape[1]) and r.memory.shape == (1, T, want_mem.shape[1])
    assert audio_info()[:3] == [7, T, 1]
    got = r.mel[0].cpu().numpy()
    e_db, g_db = R.db_dist(got, want_db), FACTOR * float(G[name + "_base_db"])
    e_m, g_m = R.rms_dist(r.memory[0].cpu().numpy(), want_mem), FACTOR * float(G[name + "_base_mem"])
    clip = float((want_db == -80.0).mean())
    print(f"case {name}: mel_db {e_db:.3e} dB (gate {g_db:.3e}), memory {e_m:.3e} of RMS (gate {g_m:.3e}); {clip:.3f} of the entries at the clip")
    assert got.max() == 0.0 and got.min() >= -80.0
    if name == "small":
        assert clip == 0.125
    assert e_db <= g_db, (e_db, g_db)
    assert e_m <= g_m, (e_m, g_m)
    # the same bits on every call
    again = fe.forward(dev(R.call_wave(name))[None])
    assert torch.equal(again.mel, r.mel) and torch.equal(again.memory, r.memory)


# ---------------------------------------------------------------- 4. silence
@pytest.mark.parametrize("normalize", [False, True])
def test_all_zero_waveform(normalize):
    import torch
    fe = front_end("short")
    r = fe.forward(torch.zeros(2, 20480 + 100, device="cuda"), normalize=normalize)
    assert not torch.isnan(r.mel).any() and not torch.isnan(r.memory).any()
    assert bool((r.mel == 0.0).all())
    assert r.activity.shape == (2, 2) and bool((r.activity == 0).all()) and bool((r.peak == 0.0).all())


# ---------------------------------------------------------------- 5. a waveform's bits do not depend on the batch
def test_batch_independence():
    import torch
    fe = front_end("short")
    y = R.call_wave("short")
    rng = np.random.default_rng(5)
    batch = np.stack([100.0 * rng.standard_normal(len(y)), y, 0.01 * rng.standard_normal(len(y))]).astype(np.float32)
    alone = fe.forward(dev(y)[None])
    three = fe.forward(dev(batch))
    assert torch.equal(three.mel[1], alone.mel[0]) and torch.equal(three.memory[1], alone.memory[0])
    assert torch.equal(three.peak[1:2], alone.peak) and torch.equal(three.activity[1], alone.activity[0])
    # ref is per waveform: every row of the batch reaches 0 dB
    assert [float(three.mel[u].max()) for u in range(3)] == [0.0, 0.0, 0.0]


# ---------------------------------------------------------------- 6., 7. windows
def test_windows_are_slices_of_the_whole():
    import torch
    fe = front_end("small")
    y = R.call_wave("small")
    rng = np.random.default_rng(6)
    two = np.stack([y, (0.3 * rng.standard_normal(len(y))).astype(np.float32)])
    whole = fe.forward(dev(two))
    T = whole.mel.shape[1]
    assert T == 16
    starts, frames = [0, 4, 8], 8
    win = fe.forward(dev(two), windows=(starts, frames))
    assert audio_info()[:3] == [7, T, 6]
    assert win.mel.shape == (6, 8, 20) and win.memory.shape == (6, 8, 16)
    for u in range(2):
        for w, s in enumerate(starts):
            assert torch.equal(win.mel[u * 3 + w], whole.mel[u, s:s + frames]), (u, w)
            assert torch.equal(win.memory[u * 3 + w], whole.memory[u, s:s + frames]), (u, w)
    assert torch.equal(win.activity, whole.activity) and torch.equal(win.peak, whole.peak)
    # the last frame is reachable, one past it is not (refused on the host side of the module, and by the library: test_refusals)
    last = fe.forward(dev(two), windows=([T - 1], 1))
    assert torch.equal(last.mel[:, 0], whole.mel[:, T - 1])


# ---------------------------------------------------------------- 8. normalize and the activity bits
def test_normalize_and_activity_bits():
    import torch
    from convofusion_amd.audio import AudioFrontEnd
    fe = AudioFrontEnd(None, sample_rate=16000, n_fft=256, hop_length=64, n_mels=20, fps=25, activity_frames=1)      # chunks of 640 samples
    assert fe.act_chunk == 640
    thr = np.sqrt(10.0 ** -4.5)                  # the threshold as an amplitude: 5.6e-3
    n = 5 * 640 + 300
    y = np.zeros((2, n), np.float32)
    # waveform 0: chunk 0 peaks 2 x above the threshold at its LAST sample, chunk 1 at its FIRST, chunk 2 is 2 x below, chunk 3 silent,
    # chunk 4 2 x above in the middle; the trailing partial chunk holds the largest sample of all and gives no bit
    y[0, 639], y[0, 640], y[0, 1280 + 17], y[0, 4 * 640 + 320], y[0, 5 * 640 + 10] = 2 * thr, -2 * thr, 0.5 * thr, 2 * thr, -0.5
    # waveform 1: quiet everywhere (2 x below the threshold) but for its peak: after normalisation every chunk with a sample is active
    y[1, 100], y[1, 700], y[1, 2000] = 0.5 * thr, -0.5 * thr, 0.5 * thr
    plain = fe.forward(dev(y))
    assert plain.activity.shape == (2, 5) and plain.activity.dtype == torch.int32
    assert plain.activity.cpu().tolist() == [[1, 1, 0, 0, 1], [0, 0, 0, 0, 0]]
    assert plain.activity.cpu().tolist() == [R.activity_bits(y[u], 640, np.float32).tolist() for u in range(2)]
    peak = np.abs(y).max(axis=1)
    assert peak.dtype == np.float32 and np.array_equal(plain.peak.cpu().numpy(), peak)
    # normalised: waveform 0 is divided by its peak 0.5, so chunks 0, 1 and 4 end 4 x above the threshold; chunk 2 is given 0.25 thr to end
    # 2 x below it.  Waveform 1 is divided by 0.5 thr: its three samples become +-1, and their chunks 0, 1 and 3 turn active
    y[0, 1280 + 17] = 0.25 * thr
    yn, pk = R.normalize(y, np.float32)
    norm = fe.forward(dev(y), normalize=True)
    want = [R.activity_bits(yn[u], 640, np.float32).tolist() for u in range(2)]
    assert want == [[1, 1, 0, 0, 1], [1, 1, 0, 1, 0]]
    assert norm.activity.cpu().tolist() == want
    assert np.array_equal(norm.peak.cpu().numpy(), pk.astype(np.float32))
    # ... and the Mel frames are those of the normalised waveform
    for u in range(2):
        ref = R.mel_db(yn[u], 16000, 256, 64, 20)
        base = R.db_dist(R.mel_db(yn[u], 16000, 256, 64, 20, np.float32), ref)
        e = R.db_dist(norm.mel[u].cpu().numpy(), ref)
        print(f"normalised waveform {u}: mel_db {e:.3e} dB (gate {FACTOR * base:.3e})")
        assert e <= FACTOR * base, (e, FACTOR * base)


# ---------------------------------------------------------------- 9. refusals
def test_refusals_happen_before_any_launch():
    import torch
    from convofusion_amd import _lib, audio
    lib = _lib.load()
    fe = front_end("small")
    t = fe.tables(torch.device("cuda", torch.cuda.current_device()))
    y = dev(R.call_wave("small"))[None]
    enc = [p.detach().contiguous() for p in (fe.audio_encoder.main[0].weight, fe.audio_encoder.main[0].bias, fe.audio_encoder.main[3].weight,
                                             fe.audio_encoder.main[3].bias, fe.audio_encoder.out_net.weight, fe.audio_encoder.out_net.bias)]
    mel = torch.zeros(3, 16, 20, device="cuda")
    mem = torch.zeros(3, 16, 16, device="cuda")
    act = torch.zeros(8, dtype=torch.int32, device="cuda")
    keep = []

    def call(weights=True, memory=True, activity=False, **over):
        a = _lib.AudioArgs()
        a.wave, a.n_wave, a.n_samples, a.normalize = y.data_ptr(), 1, 1000, 0
        a.n_fft, a.hop, a.n_mels = 256, 64, 20
        a.twiddle, a.window, a.melfb, a.mel_range = t.twiddle.data_ptr(), t.window.data_ptr(), t.melfb.data_ptr(), t.mel_range.data_ptr()
        a.amin, a.top_db, a.act_chunk, a.act_amin_power, a.act_thresh_power = 1e-10, 80.0, 640, 1e-10, 10.0 ** -4.5
        if weights:
            a.w0, a.b0, a.w1, a.b1, a.w2, a.b2 = (p.data_ptr() for p in enc)
            a.hidden, a.latent = 24, 16
        for k, v in over.items():
            if k == "win_start":
                arr = (C.c_int32 * len(v))(*v)
                keep.append(arr)
                v = C.cast(arr, C.c_void_p)
            setattr(a, k, v)
        code = lib.cfd_audio_encode(_handle(), C.byref(a), C.c_void_p(mel.data_ptr()), C.c_void_p(mem.data_ptr()) if memory else None,
                                    C.c_void_p(act.data_ptr()) if activity else None, None, None)
        return code, lib.cfd_last_error().decode()

    code, _ = call()
    assert code == 0 and audio_info()[:3] == [6, 16, 1]        # (no peak, bits or normalisation asked for: no front launch)
    cases = [("n_fft", E_ARG, dict(n_fft=300)), ("n_fft", E_ARG, dict(n_fft=4096)), ("n_fft", E_ARG, dict(n_fft=128)),
             ("hop", E_ARG, dict(hop=0)), ("n_mels", E_ARG, dict(n_mels=130)), ("n_mels", E_ARG, dict(n_mels=0)),
             ("n_samples", E_SHAPE, dict(n_samples=0)), ("n_samples", E_SHAPE, dict(n_samples=audio.MAX_SAMPLES + 1)),
             ("n_wave", E_SHAPE, dict(n_wave=0)), ("window", E_SHAPE, dict(n_win=2, win_start=[0, 9], win_frames=8)),
             ("window", E_SHAPE, dict(n_win=1, win_start=[-1], win_frames=8)), ("n_win", E_SHAPE, dict(n_win=65, win_start=[0] * 65, win_frames=1)),
             ("win_frames", E_SHAPE, dict(n_win=1, win_start=[0], win_frames=0)), ("win_start", E_ARG, dict(n_win=1, win_frames=4)),
             ("weights", E_ARG, dict(weights=False)), ("encoder", E_ARG, dict(w1=None)), ("act_chunk", E_ARG, dict(activity=True, act_chunk=0)),
             ("NULL", E_ARG, dict(twiddle=None)), ("normalize", E_ARG, dict(normalize=2)), ("amin", E_ARG, dict(amin=0.0))]
    for word, want, kw in cases:
        code, text = call(**kw)
        assert code == want, (kw, code, text)
        assert word in text or word == "NULL", (kw, text)
        assert audio_info()[0] == 0, kw
    # the boundary cases are taken: the window that ends at the last frame, and a call without the encoder when no memory is asked for
    assert call(n_win=2, win_start=[0, 8], win_frames=8)[0] == 0 and audio_info()[:3] == [6, 16, 2]
    assert call(weights=False, memory=False)[0] == 0 and audio_info()[0] == 3
    assert call(activity=True)[0] == 0 and audio_info()[0] == 7
    # the developer hook refuses the same transform arguments
    code = lib.cfd_audio_power(_handle(), C.c_void_p(y.data_ptr()), 1, 1000, 384, 64, C.c_void_p(t.twiddle.data_ptr()),
                               C.c_void_p(t.window.data_ptr()), C.c_void_p(mel.data_ptr()), None)
    assert code == E_ARG and audio_info()[0] == 0
    torch.cuda.synchronize()


def test_workspace_only_grows():
    import torch
    fe = front_end("small", with_encoder=False)
    fe.forward(torch.zeros(4, 4000, device="cuda"))
    big = audio_info()[3]
    fe.forward(torch.zeros(1, 500, device="cuda"))
    assert audio_info()[3] == big
    fe.forward(torch.zeros(4, 4000, device="cuda"))
    assert audio_info()[3] == big


# ---------------------------------------------------------------- 10. long-form: waveform to the rows synthesize_latents takes
def test_longform_audio_windows():
    import torch
    from convofusion_amd import longform
    from convofusion_amd.audio import uncond_mel
    from convofusion_amd.conditioning import default_fuser
    from convofusion_amd.sampler import CFG_CHUNKS, build_guidance_batch
    from convofusion_amd.scheduler import DDIMScheduler
    from tests.gpu_helpers import SCHED_KW, hip_denoiser
    fe = front_end("window")
    U, n_parts = 2, 2
    W = 2 * n_parts - 1
    rng = np.random.default_rng(10)
    t = np.arange(n_parts * 81920) / R.SR
    wave = np.stack([0.3 * np.sin(2 * np.pi * 300.0 * t) + 0.05 * rng.standard_normal(len(t)), 0.2 * rng.standard_normal(len(t))]).astype(np.float32)
    wave[0, 81920 + 20480:] = 0.0                  # utterance 0 falls silent in its second part: bits 10 .. 15 are 0
    memory, activity, mel, uncond = longform.audio_windows(fe, dev(wave), W)
    assert memory.shape == (U * W, 161, 512) and activity.shape == (U * W, 8) and mel.shape == (U * W, 161, 80) and uncond.shape == (1, 161, 512)
    whole = fe.forward(dev(wave))
    assert whole.mel.shape == (U, 321, 80) and whole.activity.shape == (U, 16)
    for u in range(U):
        for w in range(W):
            assert torch.equal(mel[u * W + w], whole.mel[u, 80 * w:80 * w + 161]), (u, w)
            assert torch.equal(memory[u * W + w], whole.memory[u, 80 * w:80 * w + 161]), (u, w)
            assert torch.equal(activity[u * W + w], whole.activity[u, 4 * w:4 * w + 8]), (u, w)
    assert whole.activity.cpu().tolist() == [[1] * 10 + [0] * 6, [1] * 16]
    # the unconditional memory: uncond_mel through the same weights, against float64 with the gate of the product case's memory
    n_mels, hidden, latent = 80, 128, 512
    want = R.mlp(uncond_mel(161, 80).numpy(), R.make_mlp(n_mels, hidden, latent, MLP_SEED))
    e, gate = R.rms_dist(uncond[0].cpu().numpy(), want), FACTOR * float(G["window_base_mem"])
    mirror = fe.audio_encoder(uncond_mel(161, 80).cuda()[None])
    print(f"unconditional audio memory: {e:.3e} of RMS (gate {gate:.3e})")
    assert torch.equal(uncond, mirror)
    assert e <= gate, (e, gate)
    # ... and the rows go where the loop takes them: the 7-way guidance batch over U * W rows, one tied run of 3 DDIM iterations
    B = U * W
    torch.manual_seed(3)
    fuser = default_fuser().cuda().eval()
    _, _, _, apb, lsnemb = fuser(memory, memory, memory, activity, [1] * B)
    _, _, _, apb0, lsnemb0 = fuser(uncond, uncond, uncond, torch.full((1, 8), 2, device="cuda"), [0])
    cond = [torch.randn(B, 24, 512, device="cuda"), memory, torch.randn(B, 24, 512, device="cuda"), apb.float(), lsnemb.float()]
    unc = [torch.randn(1, 24, 512, device="cuda"), uncond, torch.randn(1, 24, 512, device="cuda"), apb0.float(), lsnemb0.float()]
    uniq, maps, _ = build_guidance_batch(cond, unc)
    assert uniq[1].shape == (B + 1, 161, 512) and all(m.numel() == CFG_CHUNKS * B for m in maps)
    mems = [m[i.long()].contiguous() for m, i in zip(uniq, maps)]
    win, seq = longform.synthesize_latents(hip_denoiser(1234, 1.0), DDIMScheduler(**SCHED_KW), mems, None, n_utterances=U, n_windows=W,
                                           num_inference_steps=3, seed=4)
    assert win.shape == (U, W, 16, 128) and seq.shape == (U, (W + 1) * 8, 128) and bool(torch.isfinite(win).all())
