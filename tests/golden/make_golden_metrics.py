#!/usr/bin/env python
"""Hold tests/metrics_ref.py to the REFERENCE's own evaluation code and record the reference's outputs: tests/golden/metrics.npz.

quant_eval/motion_autoencoder.py, quaternion.py and jitter_metric.py are imported (torch and numpy only).  metric_eval.py imports librosa
at its top, which is not installed, so the class and function nodes needed (FIDCalculator, Alignment, SRGR, L1div,
calculate_avg_distance, process_motion) are taken out of its syntax tree and executed as they stand.  ``Alignment.calculate_align`` is
two lines around ``librosa.frames_to_time``; the onset times are given in seconds here, so its other two calls are made directly:
``GAHR(motion_frames2time(beat_right_wrist, 0, fps), onsets, sigma)``.

The inputs are regenerated from seeds by metrics_ref.py; this script PICKS the seeds: a sequence is taken only if, in float64, every beat
decision (orders 10 and 12) is at least 1e-4 max(v) from a tie and every SRGR comparison at least 1e-4 from the threshold.  Only numbers
are stored: the seeds, spot values of the inputs, the margins, the reference's outputs, and for every real-valued output the distance of
the float32 restatement from the float64 one (the GPU tests' gates are FACTOR x that).
Build container only (needs /root/reference).  Usage: python tests/golden/make_golden_metrics.py
"""
import ast
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference/quant_eval"
sys.path.insert(0, REF)

from tests import metrics_ref as R  # noqa: E402

F_SMALL, F_WIDE = 12, 300
NET_SEED, PACK_SEED = 41, 43


def reference_nodes():
    from scipy import linalg
    from scipy.signal import argrelextrema
    if not hasattr(np, "float"):
        np.float = float            # quaternion.py:13 reads np.finfo(np.float).eps at import; the alias left numpy in 1.24
    from quaternion import qbetween_np, qrot_np
    want = {"FIDCalculator", "Alignment", "SRGR", "L1div", "calculate_avg_distance", "process_motion"}
    path = os.path.join(REF, "metric_eval.py")
    tree = ast.parse(open(path).read())
    env = {"np": np, "math": math, "linalg": linalg, "argrelextrema": argrelextrema, "qbetween_np": qbetween_np, "qrot_np": qrot_np, "torch": torch}
    for node in tree.body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in want:
            exec(compile(ast.Module([node], []), path, "exec"), env)
            want.discard(node.name)
    assert not want, want
    return env


def pick_seeds(T, count, first):
    seeds, margins, seed = [], [], first
    while len(seeds) < count:
        x, t = R.motion(seed, T), R.target_of(seed, T)
        mb = min(R.beats(x, o)[1] for o in R.ORDERS)
        ms = R.srgr_partial(x, t, R.semantic_of(seed, T))[2]
        if mb >= R.MARGIN and ms >= R.MARGIN:
            seeds.append(seed)
            margins.append((mb, ms))
        else:
            print(f"  T = {T}: seed {seed} left out (beat margin {mb:.2e}, SRGR margin {ms:.2e})")
        seed += 1
    return seeds, np.array(margins)


def main():
    E = reference_nodes()
    from jitter_metric import calculate_jitter
    from motion_autoencoder import HalfEmbeddingNet
    out = {}
    f32, f64 = np.float32, np.float64

    # ---- stage A
    for T, count, first in ((128, 5, 0), (40, 2, 100)):
        seeds, margins = pick_seeds(T, count, first)
        print(f"T = {T}: seeds {seeds}, smallest beat margin {margins[:, 0].min():.2e}, smallest SRGR margin {margins[:, 1].min():.2e}")
        tag = f"T{T}_"
        out[tag + "seeds"], out[tag + "margins"] = np.array(seeds), margins
        out[tag + "spot"] = np.stack([R.motion(s, T)[::13, ::29] for s in seeds])
        out[tag + "spot_target"] = np.stack([R.target_of(s, T)[::13, ::29] for s in seeds])
        base = dict.fromkeys(("l1div", "srgr", "jitter", "processed"), 0.0)
        l1, sr, cnt, jit, proc = [], [], [], [], []
        for s in seeds:
            x, t, sem = R.motion(s, T), R.target_of(s, T), R.semantic_of(s, T)
            c = E["L1div"]()
            c.run(x.copy())
            l1.append(c.sum)
            g = E["SRGR"](R.THRESHOLD, 63)
            sr.append(g.run(x.copy(), t.copy(), sem.copy()))
            cnt.append(R.srgr_partial(x, t, sem)[1])
            jit.append(calculate_jitter(x.reshape(T, 63, 3), t.reshape(T, 63, 3)))
            proc.append(np.asarray(E["process_motion"](x.reshape(T, 63, 3).copy())).reshape(T, 189))
            # the restatement against the reference (the reference works in float32)
            assert R.rel(R.l1div_partial(x), l1[-1]) < 1e-5
            assert R.rel(R.srgr_partial(x, t, sem)[0] / (T * 63), sr[-1]) < 1e-6
            assert R.rel(R.jitter_sum(x, t) / ((T - 1) * 189), jit[-1]) < 1e-5
            assert R.rel(R.process_motion(x), proc[-1]) < 1e-5, R.rel(R.process_motion(x), proc[-1])
            base["l1div"] = max(base["l1div"], R.rel(R.l1div_partial(x, f32), R.l1div_partial(x)))
            base["srgr"] = max(base["srgr"], R.rel(R.srgr_partial(x, t, sem, dtype=f32)[0], R.srgr_partial(x, t, sem)[0]))
            base["jitter"] = max(base["jitter"], R.rel(R.jitter_sum(x, t, f32), R.jitter_sum(x, t)))
            base["processed"] = max(base["processed"], R.rel(R.process_motion(x, f32), R.process_motion(x)))
        out[tag + "ref_l1div"], out[tag + "ref_srgr_rate"], out[tag + "srgr_count"] = np.array(l1, f64), np.array(sr, f64), np.array(cnt)
        out[tag + "ref_jitter"] = np.array(jit, f64)
        out[tag + "ref_processed0"] = proc[0].astype(f32)
        out[tag + "ref_processed_spot"] = np.stack(proc)[:, ::5, ::7].astype(f32)
        for order in R.ORDERS:
            al = E["Alignment"](R.SIGMAS[order], order)
            masks, scores, b_align = [], [], 0.0
            for i, s in enumerate(seeds):
                x = R.motion(s, T)
                tracks = al.load_pose(x.copy(), 0, T / R.FPS, R.FPS, True)    # right arm 10, shoulder 9, wrist 11, left arm 6, shoulder 5, wrist 7
                m = np.zeros((6, T - 1), np.uint8)
                for joint, tr in zip((10, 9, 11, 6, 5, 7), tracks):
                    m[R.TRACK_JOINTS.index(joint), tr[0]] = 1
                mine, _ = R.beats(x, order)
                assert np.array_equal(mine, m), (s, order)
                assert np.array_equal(R.beats(x, order, f32)[0], m), (s, order)
                masks.append(m)
                on = R.onsets_of(s, R.ONSET_COUNTS[i % len(R.ONSET_COUNTS)], T)
                if on.size:
                    ref = al.GAHR(al.motion_frames2time(tracks[2], 0, R.FPS), on, al.sigma)
                    assert abs(R.align_score(m[5], on, al.sigma) - ref) < 1e-12
                    if ref > 0:
                        b_align = max(b_align, R.rel(R.align_score(m[5], on.astype(f32), al.sigma, dtype=f32), ref))
                    scores.append(ref)
                else:
                    scores.append(np.nan)
            out[f"{tag}o{order}_ref_beats"], out[f"{tag}o{order}_ref_align"] = np.stack(masks), np.array(scores)
            out[f"{tag}o{order}_base_align"] = b_align
            print(f"  order {order}: beats per track {np.stack(masks).sum(axis=2).min()} - {np.stack(masks).sum(axis=2).max()}, align {scores}")
        for k, v in base.items():
            out[tag + "base_" + k] = v
        print("  float32 restatement against float64:", {k: f"{v:.2e}" for k, v in base.items()})
        if T == 128:
            seeds128, proc128 = seeds, proc

    # ---- diversity: the reference's pairwise loop on processed motions
    seeds7 = seeds128 + [20, 21]
    p7 = [np.asarray(E["process_motion"](R.motion(s).reshape(128, 63, 3).copy())).reshape(-1).astype(f32) for s in seeds7]
    out["div7_seeds"], out["div7_ref"] = np.array(seeds7), E["calculate_avg_distance"](p7)
    mine7 = np.stack([R.process_motion(R.motion(s)).astype(f32) for s in seeds7])
    assert R.rel(R.avg_distance(mine7), out["div7_ref"]) < 1e-5
    out["div7_base"] = R.rel(R.avg_distance(mine7, f32), R.avg_distance(mine7))
    near = np.stack([mine7[0], (mine7[0].astype(f64) * (1 + 1e-4)).astype(f32)])
    out["div2_base"] = R.rel(R.avg_distance(near, f32), R.avg_distance(near))
    print(f"diversity of 7: reference {out['div7_ref']:.6f}; float32 restatement {out['div7_base']:.2e}, nearly equal pair {out['div2_base']:.2e}")

    # ---- the embedding net at feature_length 12
    state = R.make_fgd_state(F_SMALL, NET_SEED)
    net = HalfEmbeddingNet(128, 189, F_SMALL)
    slopes = [m.negative_slope for m in net.pose_encoder.out_net if isinstance(m, torch.nn.LeakyReLU)]
    assert len(slopes) == 3 and all(float(s) == 1.0 for s in slopes), slopes
    print(f"HalfEmbeddingNet.pose_encoder.out_net: {len(slopes)} LeakyReLU with negative_slope == 1.0 (nn.LeakyReLU(True)): the identity")
    missing = net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("decoder.") for k in missing.missing_keys)
    net.eval()
    x3 = np.stack(proc128[:3]).astype(f32)
    with torch.no_grad():
        e3 = net(torch.from_numpy(x3)).numpy()
    assert R.rel(R.embed(state, x3), e3) < 1e-4, R.rel(R.embed(state, x3), e3)
    out["emb12_ref"], out["emb12_base"] = e3, R.rel(R.embed(state, x3, f32), R.embed(state, x3))
    out["net12_spot"] = state["pose_encoder.out_net.0.weight"][::97, ::211]
    print(f"embedding, F = {F_SMALL}: restatement against the reference {R.rel(R.embed(state, x3), e3):.2e}, float32 restatement {out['emb12_base']:.2e}")

    # ---- FGD between two 48-sequence sets, through the reference's process_motion, net and FIDCalculator
    sets = []
    for first in (200, 300):
        xs = np.stack([np.asarray(E["process_motion"]((R.motion(first + i) * (1.0 if first == 200 else 1.1)).reshape(128, 63, 3).copy())).reshape(128, 189)
                       for i in range(48)]).astype(f32)
        with torch.no_grad():
            sets.append(net(torch.from_numpy(xs)).numpy())
    out["fgd_ref"] = E["FIDCalculator"].frechet_distance(sets[0], sets[1])
    mine = []
    for dt in (f64, f32):
        mine.append([R.embed(state, np.stack([R.process_motion(R.motion(first + i) * f32(1.0 if first == 200 else 1.1), dt) for i in range(48)]).astype(f32), dt)
                     for first in (200, 300)])
    fgd64, fgd32 = R.frechet(*mine[0]), R.frechet(*mine[1])
    out["fgd_base"], out["fgd_ref_dist"] = abs(fgd32 - fgd64) / abs(fgd64), abs(out["fgd_ref"] - fgd64) / abs(fgd64)
    print(f"FGD: reference {out['fgd_ref']:.6f}, float64 restatement {fgd64:.6f}, float32 restatement {fgd32:.6f}")
    assert out["fgd_ref_dist"] < 1e-3

    # ---- the product width, from a seeded folded pack
    parts = R.make_folded_parts(F_WIDE, PACK_SEED)
    x2 = np.stack(proc128[:2]).astype(f32)
    out["emb300_base"] = R.rel(R.embed_folded(parts, x2, f32), R.embed_folded(parts, x2))
    out["pack300_spot"] = parts[4][0][::37, ::1009]
    print(f"embedding, F = {F_WIDE} (folded pack): float32 restatement {out['emb300_base']:.2e}")

    np.savez_compressed(os.path.join(HERE, "metrics.npz"), **out)
    print("wrote metrics.npz:", os.path.getsize(os.path.join(HERE, "metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
