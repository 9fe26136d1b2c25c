"""Developer tool: what the motion evaluation costs at N sequences of 128 frames and the product width of the FGD net (300), seeded
motions (tests/metrics_ref.py) and a seeded net.

  gpu   on the MI355X: ``MotionEvaluator.update`` (pred + target + semantic + onsets, batches of 128) + ``compute`` (FGD, diversity of both
        sets, ...), stage B alone (``FGDNet.forward``), and the float32 torch-eager pose encoder (the unfolded modules) on the same device
  cpu   the float32 numpy / torch restatement on 16 threads: its vectorised form, and the reference's own procedure -- one motion at a
        time through the unfolded net, a Python double loop over all pairs for the diversity (timed on PAIR_ROWS rows and scaled by the
        number of pairs)

Medians of REPS repeats after one warm-up; host clock between two waits for the stream.
Usage:  python tools/metrics_time.py gpu|cpu [N] [REPS] [OUT.json]     (default 1024, 5, profiles/metrics_time_<mode>.json)
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from convofusion_amd.metrics import FGDNet, MotionEvaluator  # noqa: E402
from tests import metrics_ref as R  # noqa: E402

F, BATCH, PAIR_ROWS = 300, 128, 96


def make_sets(N):
    base = np.stack([R.motion(s) for s in range(64)])
    rng = np.random.default_rng(0)
    mix = rng.dirichlet(np.ones(4), size=(2, N)).astype(np.float32)         # every sequence a seeded blend of four base motions
    idx = rng.integers(0, 64, size=(2, N, 4))
    sets = [(mix[k][:, :, None, None] * base[idx[k]]).sum(axis=1).astype(np.float32) for k in range(2)]
    return sets[0], sets[1], rng.uniform(0, 1, (N, 128)).astype(np.float32), [R.onsets_of(i, 7) for i in range(N)]


def make_net():
    torch.manual_seed(11)
    net = FGDNet(128, 189, F)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_var.uniform_(0.5, 1.5)
            m.running_mean.normal_(0, 0.1)
    return net.eval()


def eager(net, x):
    enc = net.pose_encoder
    return enc.fc_mu(enc.out_net(enc.net(x.transpose(1, 2)).flatten(1)))


def median(fn, reps, sync=lambda: None):
    secs = []
    for rep in range(reps + 1):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        if rep:
            secs.append(time.perf_counter() - t0)
    return statistics.median(secs), r


def main():
    mode = sys.argv[1]
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", f"metrics_time_{mode}.json")
    pred, target, sem, onsets = make_sets(N)
    net = make_net()
    res = {"mode": mode, "sequences": N, "frames": 128, "feature_length": F, "reps": reps}
    if mode == "gpu":
        import ctypes as C
        from convofusion_amd import _lib
        from convofusion_amd.conditioning import _engine_handle
        dev = torch.device("cuda", 0)
        res["device"] = torch.cuda.get_device_name(dev)
        sync = lambda: torch.cuda.synchronize(dev)
        p, t, s = (torch.from_numpy(v).to(dev) for v in (pred, target, sem))
        net.pack(dev)
        launches = []

        def info():
            buf = torch.zeros(3, device=dev)
            _lib.check(_lib.load().cfd_debug_read(_engine_handle(dev), b"metrics.info", C.c_void_p(buf.data_ptr()), 3))
            return int(buf[0])

        def whole(count=False):
            ev = MotionEvaluator(net)
            for b0 in range(0, N, BATCH):
                ev.update(p[b0:b0 + BATCH], t[b0:b0 + BATCH], s[b0:b0 + BATCH], onsets[b0:b0 + BATCH])
            return ev.compute()
        res["update_compute_s"], metrics = median(whole, reps, sync)
        res["metrics"] = metrics
        res["stage_b_s"], emb = median(lambda: net(p), reps, sync)
        res["stage_b_launches"] = info()
        gpu_net = make_net().to(dev)
        with torch.no_grad():
            res["eager_f32_s"], want = median(lambda: eager(gpu_net, p), reps, sync)
            res["stage_b_vs_eager_max_abs"] = float((emb - want).abs().max())
            for n in (1, 16, 128):
                res[f"stage_b_{n}_s"] = median(lambda: net(p[:n]), reps, sync)[0]
                res[f"eager_f32_{n}_s"] = median(lambda: eager(gpu_net, p[:n]), reps, sync)[0]
        # launches of one update of 128 with a target (two cfd_motion_eval calls) and of the two diversity calls
        res["launches_per_update_of_128"] = 2 * (1 + 5 + 1)
        res["launches_compute"] = 4
    else:
        torch.set_num_threads(16)
        res["threads"] = 16
        f32 = np.float32

        def vectorised():
            proc = [np.stack([R.process_motion(x, f32) for x in v]) for v in (pred, target)]
            with torch.no_grad():
                e = [eager(net, torch.from_numpy(v)).numpy() for v in proc]
            for i in range(N):
                R.l1div_partial(pred[i], f32), R.srgr_partial(pred[i], target[i], sem[i], dtype=f32), R.jitter_sum(pred[i], target[i], f32)
                R.align_score(R.beats(pred[i], 10, f32)[0][5], onsets[i], 0.3, dtype=f32)
            return R.frechet(*e), R.avg_distance(proc[0], f32), R.avg_distance(proc[1], f32)
        res["vectorised_s"], _ = median(vectorised, min(reps, 2))

        def one_at_a_time():
            with torch.no_grad():
                return [eager(net, torch.from_numpy(R.process_motion(x, f32))[None]).numpy() for x in pred]
        res["net_one_at_a_time_s"], _ = median(one_at_a_time, 1)
        rows = np.stack([R.process_motion(x, f32).reshape(-1) for x in pred[:PAIR_ROWS]])

        def pair_loop():
            d = 0
            for i in range(PAIR_ROWS):
                for j in range(i + 1, PAIR_ROWS):
                    d += np.linalg.norm(rows[i] - rows[j])
            return d
        sec, _ = median(pair_loop, 1)
        res["pair_loop_s_scaled"] = sec * (N * (N - 1) / 2) / (PAIR_ROWS * (PAIR_ROWS - 1) / 2)
    for k, v in res.items():
        print(k, v, flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
