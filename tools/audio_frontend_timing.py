"""Developer tool (GPU box): the log-Mel front end -- cfd_audio_encode (csrc/audio_fe.hpp) against two statements of the same work in one
session:

  torch   on the device: ``torch.stft`` (centred, zero padded, periodic Hann) -> ``abs() ** 2`` -> matmul with the filterbank ->
          ``log10`` / ``amax`` / ``clamp`` -> window slicing -> the mirror ``AudioConvEncoder.forward`` (three cfd_linear_act launches),
          peaks and activity bits with ``amax``
  numpy   on the CPU threads the process gets: the float32 run of tests/audio_ref.py per waveform (framing, pocketfft, filterbank, dB,
          slicing, the MLP, bits), the input already in host memory; no host-to-device copy of the result is counted

Inputs at the product configuration (16 kHz, n_fft 2048, hop 512, 80 bands, encoder 80 -> 128 -> 512 -> 512): one window (81 920
samples, 161 frames), one 8-part utterance (655 360 samples, 15 windows of 161 frames), 32 one-window utterances.  The HIP path is
timed twice: the library call alone (tables, weights and the argument struct made beforehand, outputs allocated) and
``AudioFrontEnd.forward`` as a caller gets it (its Python and its four allocations included).

Per input and path: WINDOWS timed windows of INNER back-to-back calls between two device events behind WARM untimed calls (numpy:
``perf_counter`` around each of WINDOWS calls); reported are the median, minimum and maximum.  The HIP Mel frames are compared with the
torch ones at every input (max-abs dB).  librosa itself is not timed: it is not a dependency.

Usage:  python tools/audio_frontend_timing.py [OUT.json]      (default profiles/audio_frontend_timing.json)
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from convofusion_amd import _lib, audio  # noqa: E402
from convofusion_amd.conditioning import AudioConvEncoder, _engine_handle  # noqa: E402
from tests import audio_ref as R  # noqa: E402

SR, N_FFT, HOP, N_MELS, HIDDEN, LATENT = 16000, 2048, 512, 80, 128, 512
WINDOW = 81920
INPUTS = [("one window", 1, 1), ("one 8-part utterance, 15 windows", 1, 8), ("32 one-window utterances", 32, 1)]
WARM, WINDOWS, INNER = 5, 9, 20


def summary(per_call, inner):
    return {"median_ms": statistics.median(per_call), "min_ms": min(per_call), "max_ms": max(per_call), "calls_per_window": inner, "windows": len(per_call)}


def timed(fn, inner=INNER):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) / inner)
    return summary(per_call, inner)


def timed_host(fn):
    fn()
    per_call = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        fn()
        per_call.append((time.perf_counter() - t0) * 1e3)
    return summary(per_call, 1)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "audio_frontend_timing.json")
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    sd = R.make_mlp(N_MELS, HIDDEN, LATENT, 31)
    enc = AudioConvEncoder(N_MELS, HIDDEN, LATENT)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    enc = enc.to(dev).eval()
    fe = audio.AudioFrontEnd(enc, sample_rate=SR, n_fft=N_FFT, hop_length=HOP, n_mels=N_MELS)
    t = fe.tables(dev)
    weights = fe._weights(dev)
    lib, handle = _lib.load(), _engine_handle(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fb_t = t.melfb.t().contiguous()
    thr = 10.0 ** (fe.activity_db / 10.0)
    results = {"device": torch.cuda.get_device_name(0), "config": [SR, N_FFT, HOP, N_MELS, HIDDEN, LATENT], "cpu_threads": torch.get_num_threads(),
               "inputs": []}
    for label, U, parts in INPUTS:
        n = parts * WINDOW
        rng = np.random.default_rng(U * 100 + parts)
        y_np = (0.3 * rng.standard_normal((U, n))).astype(np.float32)
        y = torch.from_numpy(y_np).to(dev)
        T = audio.frame_count(n, HOP)
        slices = audio.window_slices(T, parts) if parts > 1 else None
        starts, frames = ([a for a, _ in slices], slices[0][1] - slices[0][0]) if slices else ([], T)
        windows = (starts, frames) if slices else None
        rows = U * max(len(starts), 1)
        n_bits = n // fe.act_chunk

        mel = torch.empty(rows, frames, N_MELS, device=dev)
        mem = torch.empty(rows, frames, LATENT, device=dev)
        act = torch.empty(U, n_bits, dtype=torch.int32, device=dev)
        peak = torch.empty(U, device=dev)
        win = (C.c_int32 * max(len(starts), 1))(*starts)
        a = _lib.AudioArgs(wave=y.data_ptr(), n_wave=U, n_samples=n, normalize=0, n_fft=N_FFT, hop=HOP, n_mels=N_MELS, twiddle=t.twiddle.data_ptr(),
                           window=t.window.data_ptr(), melfb=t.melfb.data_ptr(), mel_range=t.mel_range.data_ptr(), amin=1e-10, top_db=80.0,
                           n_win=len(starts), win_start=C.cast(win, C.c_void_p), win_frames=frames if starts else 0, hidden=HIDDEN, latent=LATENT,
                           act_chunk=fe.act_chunk, act_amin_power=1e-10, act_thresh_power=thr)
        a.w0, a.b0, a.w1, a.b1, a.w2, a.b2 = (p.data_ptr() for p in weights)

        def hip_call():
            _lib.check(lib.cfd_audio_encode(handle, C.byref(a), C.c_void_p(mel.data_ptr()), C.c_void_p(mem.data_ptr()), C.c_void_p(act.data_ptr()),
                                            C.c_void_p(peak.data_ptr()), C.c_void_p(stream)))

        def hip_module():
            return fe.forward(y, windows=windows)

        def torch_path():
            spec = torch.stft(y, N_FFT, hop_length=HOP, window=t.window, center=True, pad_mode="constant", return_complex=True)     # [U, bins, T]
            S = (spec.abs() ** 2).transpose(1, 2) @ fb_t                                                                          # [U, T, mels]
            db = 10.0 * torch.log10(S.clamp(min=1e-10)) - 10.0 * torch.log10(S.amax(dim=(1, 2), keepdim=True).clamp(min=1e-10))
            db = db.clamp(min=-80.0)
            if starts:
                db = torch.stack([db[:, s:s + frames] for s in starts], dim=1).reshape(rows, frames, N_MELS)
            pk = y.abs().amax(dim=1)
            bits = ((y[:, :n_bits * fe.act_chunk].reshape(U, n_bits, fe.act_chunk).abs().amax(dim=2) ** 2).clamp(min=1e-10) > thr).to(torch.int32)
            return db, enc(db), bits, pk

        def numpy_path():
            out = []
            for u in range(U):
                db = R.mel_db(y_np[u], SR, N_FFT, HOP, N_MELS, np.float32)
                if starts:
                    db = np.stack([db[s:s + frames] for s in starts])
                out.append((db, R.mlp(db, sd, np.float32), R.activity_bits(y_np[u], fe.act_chunk, np.float32), np.abs(y_np[u]).max()))
            return out

        hip = timed(hip_call)
        info = torch.zeros(4, device=dev)
        _lib.check(lib.cfd_debug_read(handle, b"audio.info", C.c_void_p(info.data_ptr()), 4))
        module = timed(hip_module)
        tor = timed(torch_path)
        cpu = timed_host(numpy_path)
        hip_call()
        want_db, want_mem, want_bits, want_pk = torch_path()
        row = {"input": label, "n_wave": U, "n_samples": n, "frames": T, "rows": rows, "launches": int(info[0].item()), "workspace_bytes": int(info[3].item()),
               "hip_call": hip, "hip_module": module, "torch_device": tor, "numpy_cpu": cpu,
               "torch_over_hip_call": tor["median_ms"] / hip["median_ms"], "numpy_over_hip_call": cpu["median_ms"] / hip["median_ms"],
               "hip_vs_torch_mel_max_abs_db": float((mel - want_db).abs().max()),
               "hip_vs_torch_memory_max_abs_over_rms": float((mem - want_mem).abs().max() / want_mem.pow(2).mean().sqrt()),
               "bits_equal": bool(torch.equal(act, want_bits)), "peak_equal": bool(torch.equal(peak, want_pk))}
        results["inputs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
