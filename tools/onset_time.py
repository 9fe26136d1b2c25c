"""Developer tool (GPU box): audio onset detection -- ``OnsetDetector.forward`` (cfd_audio_onsets, csrc/onset_fe.hpp) and
``MotionEvaluator.update(pred, audio=)`` against the host statement of the same work in one session:

  numpy   the float32 run of tests/onset_ref.py per clip (peak normalisation, framing, pocketfft, filterbank, dB, envelope, scipy's two
          filters, the greedy pass, the energies, the backtrack, the times) on a pool of 16 processes, the clips already in host memory;
          the pool is started beforehand and no copy of the result to the device is counted

Inputs at the product configuration (16 kHz, n_fft 2048, hop 512, 128 bands, windows from 22050): 1, 32 and 1 024 clips of 5.12 s
(81 920 samples, 161 frames), seeded noise bursts on a quiet floor.  Timed per input:

  forward        ``OnsetDetector.forward`` and a device synchronise behind it (blocking, as a caller who wants the result waits)
  update_audio   ``MotionEvaluator.update(pred, audio=wave)`` and a synchronise: detection and motion evaluation on one stream
  update_lists   ``MotionEvaluator.update(pred, onsets=lists)`` and a synchronise: the onsets as host lists, made beforehand (what a caller
                 with ``onsets.npy`` files pays; the difference to update_audio is what detection on the device adds)
  numpy          one pass over all clips on the pool (``perf_counter``)

WINDOWS timed windows of INNER back-to-back blocking calls behind WARM untimed ones, host clock around work that ends in a synchronise;
reported are the median, minimum and maximum per call.  The device's frames are compared with the float32 restatement's at every input.
librosa itself is not timed: it is not a dependency.

Usage:  python tools/onset_time.py [OUT.json]      (default profiles/onset_timing.json)
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
from convofusion_amd import _lib  # noqa: E402
from convofusion_amd.audio import OnsetDetector  # noqa: E402
from convofusion_amd.conditioning import _engine_handle  # noqa: E402
from convofusion_amd.metrics import MotionEvaluator  # noqa: E402
from tests import metrics_ref as M  # noqa: E402
from tests import onset_ref as R  # noqa: E402

N_SAMPLES, CLIPS, THREADS = 81920, (1, 32, 1024), 16
WARM, WINDOWS = 3, 7


def clip(seed):
    rng = np.random.default_rng(1000 + seed)
    y = 0.004 * rng.standard_normal(N_SAMPLES)
    for _ in range(6):
        s, n, lv = int(rng.integers(0, N_SAMPLES - 6000)), int(rng.integers(1500, 6000)), float(rng.uniform(0.1, 0.9))
        y[s:s + n] += lv * rng.standard_normal(n)
    return y.astype(np.float32)


def host_detect(y):
    d = R.detect(y, **R.PRODUCT, dtype=np.float32)
    return d["raw"], d["times"]


def summary(per_call, inner):
    return {"median_ms": statistics.median(per_call), "min_ms": min(per_call), "max_ms": max(per_call), "calls_per_window": inner, "windows": len(per_call)}


def timed_blocking(fn, inner):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
            torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) * 1e3 / inner)
    return summary(per_call, inner)


def audio_info():
    info = torch.zeros(4, device="cuda")
    _lib.check(_lib.load().cfd_debug_read(_engine_handle(torch.device("cuda", torch.cuda.current_device())), b"audio.info", C.c_void_p(info.data_ptr()), 4))
    return [int(v) for v in info.tolist()]


def main():
    from multiprocessing import get_context
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "onset_timing.json")
    os.environ["OMP_NUM_THREADS"] = "1"          # (one process per clip: the pool is the parallelism)
    pool = get_context("spawn").Pool(THREADS)
    pool.map(host_detect, [clip(0)] * THREADS)   # started and warm
    det = OnsetDetector()
    base = np.stack([M.motion(200 + i, 128) for i in range(8)])
    result = {"device": torch.cuda.get_device_name(0), "config": [16000, 2048, 512, 128, 22050], "cpu_processes": THREADS, "inputs": []}
    for n in CLIPS:
        waves = [clip(i) for i in range(n)]
        y = torch.from_numpy(np.stack(waves)).cuda()
        pred = torch.from_numpy(base[np.arange(n) % len(base)]).cuda()
        inner = 20 if n <= 32 else 5
        host = pool.map(host_detect, waves, chunksize=max(1, n // (4 * THREADS)))
        res = det.forward(y)
        times, raw, _ = res.host()
        launches, frames, _, ws_bytes = audio_info()
        same = sum(int(np.array_equal(raw[u], host[u][0])) for u in range(n))
        lists = [h[1] for h in host]
        ev = MotionEvaluator()

        def update_audio():
            ev.reset()
            ev.update(pred, audio=y)

        def update_lists():
            ev.reset()
            ev.update(pred, onsets=lists)
        entry = {"clips": n, "n_samples": N_SAMPLES, "frames": frames, "launches": launches, "workspace_bytes": ws_bytes,
                 "onsets_total": int(res.n_total.item()), "clips_with_frames_equal_to_float32_restatement": same,
                 "forward": timed_blocking(lambda: det.forward(y), inner), "update_audio": timed_blocking(update_audio, inner),
                 "update_lists": timed_blocking(update_lists, inner)}
        per = []
        for _ in range(3 if n >= 1024 else WINDOWS):
            t0 = time.perf_counter()
            pool.map(host_detect, waves, chunksize=max(1, n // (4 * THREADS)))
            per.append((time.perf_counter() - t0) * 1e3)
        entry["numpy"] = summary(per, 1)
        entry["numpy_over_forward"] = entry["numpy"]["median_ms"] / entry["forward"]["median_ms"]
        entry["update_audio_minus_lists_ms"] = entry["update_audio"]["median_ms"] - entry["update_lists"]["median_ms"]
        print(json.dumps(entry), flush=True)
        result["inputs"].append(entry)
    pool.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
