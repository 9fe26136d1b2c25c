"""Developer tool (GPU box): what a guided iteration with frame-accurate key poses costs as a device call, next to the torch loop it
stands beside.  Modelled on tools/guide_time.py, whose timer, loop case and statistics it uses.

At the product shape (B = 1, L = 16, 128 frames, DDIM-50, the default combine: 6 evaluated chunks over B + 1 distinct memories,
S = (24, 161, 24, 8, 1); seeded weights; key pose: frame 73, one hand's 60 columns), whole loop calls / 50:
  pose_keyframes_iteration  one guided iteration of ``sampler.sample_with_pose_keyframes`` (every iteration guided)
  torch_loop_iteration      one guided iteration of ``sampler.sample_with_loss_guidance(edit.pose_keyframe_loss(fused=True))`` -- and, with
                            ``--parent-root DIR`` (a checkout of the parent commit with its library built), the same loop there, in a
                            child process of this run: same box, same session (twice, with this tree's own loop in a child between)
  plain_iteration           one iteration of ``sampler.sample``
The call alone (``Denoiser.guide_pose``, x_new only) with ``reuse_memory_side`` 0 and 2 and its launches ("weg.info" + "vae.info"); the
3-window tied run (``longform.window_ties(1, 3)``) as a loop, next to the tied ``sample``; and the 15-window x 6-chunk call (1 440 token
rows, 15 decoded windows), neither of which has a predecessor.

Timer: hipEvents (torch.cuda.Event); calls alone: medians of 50 with the spread; loops: medians of 5 whole calls.  Every variant is
warmed up first.  The call blocks (it returns with its results complete), so its figure is a host round trip.

Usage:  python tools/pose_guide_time.py [--parent-root DIR] [--out OUT.json]      (default profiles/r33_pose_guide_time.json)
        python tools/pose_guide_time.py --torch-loop-only --root DIR              (the child: prints one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_time as G  # noqa: E402

FRAMES, NF = 128, 189


def pose_targets(B):
    import numpy as np
    from tests.gpu_helpers import to_dev
    rng = np.random.Generator(np.random.PCG64(49))
    target = to_dev((rng.standard_normal((B, FRAMES, NF), dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    fm = np.zeros((B, FRAMES), dtype=np.float32)
    fm[:, 73] = 1
    cm = np.zeros(NF, dtype=np.float32)
    cm[69:129] = 1
    return target, to_dev(fm), to_dev(cm)


def vae_model(root):
    sys.path.insert(0, root)
    from tests.test_gpu_vae_vjp import _model
    return _model()


def torch_loop(root):
    """The loops that exist on the parent commit too: the torch-autograd guided loop over the fused decode and the plain loop."""
    import torch
    sys.path.insert(0, root)
    from convofusion_amd import edit, sampler
    m, sch, mems, masks, _, _, kw, _ = G.loop_case(root)
    target, fm, cm = pose_targets(1)
    loss = edit.pose_keyframe_loss(vae_model(root), target, fm, cm, fused=True)
    return {"torch_loop_iteration": G.per_iteration(G.timed(torch, lambda: sampler.sample_with_loss_guidance(m, sch(), mems, masks, loss, 0.5, **kw),
                                                            n=5, warm=2)),
            "plain_iteration": G.per_iteration(G.timed(torch, lambda: sampler.sample(m, sch(), mems, masks, **kw), n=5, warm=2))}


def pose_call(torch, m, vae, cb, chunks, B, reuse, tie=None):
    """One ``Denoiser.guide_pose`` at timesteps that alternate (a loop never repeats one), x_new only."""
    import numpy as np
    from convofusion_amd.denoiser import tie_csr
    from convofusion_amd.sampler import default_guidance_weights
    from oracle import inputs
    from tests.gpu_helpers import read_debug, to_dev
    rows = np.concatenate([np.arange(c * B, (c + 1) * B) for c in chunks])
    maps = [to_dev(np.ascontiguousarray(cb["row_map"][j][rows])) for j in range(5)]
    umasks = {}
    for j, k in enumerate(inputs.MEM_NAMES):
        mk = cb["masks"][k]
        umasks[k] = None if mk is None else to_dev(np.stack([mk[list(cb["row_map"][j]).index(u)] for u in range(B + 1)]))
    mems = [to_dev(v) for v in cb["unique"]]
    x = to_dev(cb["init"])
    w = to_dev(np.tile(np.asarray(default_guidance_weights(7, 7.5), dtype=np.float32)[list(chunks)], (B, 1)))
    target, fm, cm = pose_targets(B)
    csr = None if tie is None else tie_csr(tie)
    t = [433]

    def call():
        t[0] = 865 - t[0]          # 433, 432, 433, ...
        m.guide_pose(x, t[0], mems, umasks, w, vae, target, fm, feature_mask=cm, sqrt_acp=0.8, sqrt_1m_acp=0.6, step=0.1, inv_n=1.0 / (B * 60), tie=tie,
                     csr=csr, row_maps=maps, reuse_memory_side=reuse, want=("x_new",))
    r = G.timed(torch, call)
    r["launches"] = int(read_debug(m, "weg.info", (5,))[0])
    r["vae_launches"] = int(read_debug(m, "vae.info", (2,))[0])
    r["token_rows"] = len(chunks) * B * 16
    r["decoded_frames"] = B * FRAMES
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--torch-loop-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.torch_loop_only:
        print(json.dumps(torch_loop(os.path.abspath(a.root))))
        return
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    res = {"what": "hipEvent times on one MI355X, seeded weights (1234; VAE: oracle.vae_weights); ms.  Loops: B = 1, L = 16, 128 frames, DDIM-50, 6 "
                   "evaluated chunks over 2 distinct memories, S = (24, 161, 24, 8, 1), key pose = frame 73, one hand's 60 columns; whole calls / "
                   "50, medians of 5.  pose_keyframes_iteration: sample_with_pose_keyframes, every iteration guided; torch_loop_iteration: "
                   "sample_with_loss_guidance(pose_keyframe_loss(fused=True)); plain_iteration: sample; parent / parent_again: the latter two on the "
                   "parent commit's tree and library in a child process of this run, tree_child: on this tree in a child process between "
                   "them (the top-level figures of the two are this process's own).  pose_call_*: Denoiser.guide_pose alone (x_new only), medians of "
                   "50, with reuse_memory_side 0 / 2 and the launches (row-tile engine + VAE).  tied_*: one utterance of 3 windows "
                   "(window_ties(1, 3)), 18 forward rows, 3 decoded windows.  rows1440_*: 15 windows x 6 chunks in one call.",
           "device": torch.cuda.get_device_name(0)}
    def child(root):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-loop-only", "--root", root], capture_output=True, text=True,
                           cwd=root, timeout=500)
        if p.returncode != 0:
            raise SystemExit(f"the run in {root} failed ({p.returncode}):\n{p.stderr[-2000:]}")
        return json.loads(p.stdout.strip().splitlines()[-1])
    if a.parent_root:
        # the parent's loops and, under the same conditions, this tree's: a child process each, the parent's first and last
        res["parent"] = child(os.path.abspath(a.parent_root))
        res["tree_child"] = child(os.path.abspath(a.root))
        res["parent_again"] = child(os.path.abspath(a.parent_root))
    res.update(torch_loop(a.root))
    from convofusion_amd import longform, sampler
    from oracle import inputs
    vae = vae_model(a.root)
    m, sch, mems, masks, _, _, kw, cb = G.loop_case(a.root)
    target, fm, cm = pose_targets(1)
    res["pose_keyframes_iteration"] = G.per_iteration(G.timed(
        torch, lambda: sampler.sample_with_pose_keyframes(m, sch(), mems, masks, vae, target, fm, 0.5, feature_mask=cm, **kw), n=5, warm=2))
    chunks = (0, 1, 2, 3, 4, 5)
    for reuse in (0, 2):
        res[f"pose_call_reuse{reuse}"] = pose_call(torch, m, vae, cb, chunks, 1, reuse)
    # the 3-window tied run
    m3, sch3, mems3, masks3, _, _, kw3, cb3 = G.loop_case(a.root, B=3)
    target3, fm3, _ = pose_targets(3)
    tie = longform.window_ties(1, 3).cuda()
    res["tied_pose_keyframes_iteration"] = G.per_iteration(G.timed(
        torch, lambda: sampler.sample_with_pose_keyframes(m3, sch3(), mems3, masks3, vae, target3, fm3, 0.5, feature_mask=cm, tie=tie, **kw3), n=5, warm=2))
    res["tied_plain_iteration"] = G.per_iteration(G.timed(torch, lambda: sampler.sample(m3, sch3(), mems3, masks3, tie=tie, **kw3), n=5, warm=2))
    for reuse in (0, 2):
        res[f"tied_pose_call_reuse{reuse}"] = pose_call(torch, m3, vae, cb3, chunks, 3, reuse, tie=tie)
    # 15 windows x 6 chunks = 1 440 token rows and 15 decoded windows in one call
    cb15 = inputs.make_cfg_batch(seed=48, B=15, L=16, S=G.S_PRODUCT, pad_tail=(5, 0, 7, 0, 0))
    tie15 = longform.window_ties(1, 15).cuda()
    for reuse in (0, 2):
        res[f"rows1440_pose_call_reuse{reuse}"] = pose_call(torch, m, vae, cb15, chunks, 15, reuse, tie=tie15)
    out = a.out or os.path.join(a.root, "profiles", "r33_pose_guide_time.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
