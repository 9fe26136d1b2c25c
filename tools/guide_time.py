"""Developer tool (GPU box): what a key-pose guided iteration costs as a device call, next to the torch loop it stands beside.

At the product shape (B = 1, L = 16, DDIM-50, the default combine: 6 evaluated chunks over B + 1 distinct memories,
S = (24, 161, 24, 8, 1); seeded weights), whole loop calls / 50:
  keyframes_iteration     one guided iteration of ``sampler.sample_with_keyframes`` (every iteration guided)
  torch_loop_iteration    one guided iteration of ``sampler.sample_with_loss_guidance(edit.keyframe_loss)`` -- and, with
                          ``--parent-root DIR`` (a checkout of the parent commit with its library built), the same loop there, in a
                          child process of this run: same box, same session
  plain_iteration         one iteration of ``sampler.sample``
The guide call alone (``Denoiser.guide``, x_new only) with ``reuse_memory_side`` 0 and 2 and its launches ("weg.info"); the 3-window
tied run (``longform.window_ties(1, 3)``) as a loop, next to the tied ``sample``; and the 15-window x 6-chunk call (1 440 token rows),
which has no predecessor.

Timer: hipEvents (torch.cuda.Event); calls alone: medians of 50 with the spread; loops: medians of 5 whole calls.  Every variant is
warmed up first.  The guide call blocks (it returns with its results complete), so its figure is a host round trip.

Usage:  python tools/guide_time.py [--parent-root DIR] [--out OUT.json]      (default profiles/r31_guide_time.json)
        python tools/guide_time.py --torch-loop-only --root DIR              (the child: prints one JSON line)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

N = 50
S_PRODUCT = (24, 161, 24, 8, 1)
STEPS = 50


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def timed(torch, fn, n=N, warm=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def per_iteration(s):
    return {k: (v / STEPS if k.endswith("_ms") else v) for k, v in s.items()}


def loop_case(root, B=1):
    import numpy as np
    sys.path.insert(0, root)
    from convofusion_amd import scheduler
    from oracle import inputs
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    cb = inputs.make_cfg_batch(seed=43, B=B, L=16, S=S_PRODUCT, pad_tail=(5, 0, 7, 0, 0))
    rng = np.random.Generator(np.random.PCG64(47))
    target = to_dev((rng.standard_normal((B, 16, 128), dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    mask = np.zeros((B, 16), dtype=bool)
    mask[:, 3::5] = True
    umasks = {}
    for j, k in enumerate(inputs.MEM_NAMES):
        mk = cb["masks"][k]
        umasks[k] = None if mk is None else to_dev(np.stack([mk[list(cb["row_map"][j]).index(u)] for u in range(B + 1)]))
    kw = dict(B=B, L=16, num_inference_steps=STEPS, guidance_scale=7.5, eta=0.0, init_latents=to_dev(cb["init"]), dedup=False,
              row_maps=[to_dev(r) for r in cb["row_map"]], skip_zero_weight_chunks=True)
    return (hip_denoiser(1234, 1.0), lambda: scheduler.DDIMScheduler(**SCHED_KW), [to_dev(v) for v in cb["unique"]], umasks, target, to_dev(mask), kw, cb)


def torch_loop(root):
    """The loops that exist on the parent commit too: the torch-autograd guided loop and the plain loop."""
    import torch
    sys.path.insert(0, root)
    from convofusion_amd import edit, sampler
    m, sch, mems, masks, target, mask, kw, _ = loop_case(root)
    loss = edit.keyframe_loss(target, mask)
    return {"torch_loop_iteration": per_iteration(timed(torch, lambda: sampler.sample_with_loss_guidance(m, sch(), mems, masks, loss, 0.5, **kw), n=5, warm=2)),
            "plain_iteration": per_iteration(timed(torch, lambda: sampler.sample(m, sch(), mems, masks, **kw), n=5, warm=2))}


def guide_call(torch, m, cb, chunks, B, reuse, tie=None):
    """One ``Denoiser.guide`` at timesteps that alternate (a loop never repeats one), x_new only."""
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
    target, mask = torch.zeros_like(x), torch.ones(B, 16, device="cuda")
    csr = None if tie is None else tie_csr(tie)
    t = [433]

    def call():
        t[0] = 865 - t[0]          # 433, 432, 433, ...
        m.guide(x, t[0], mems, umasks, w, target, mask, sqrt_acp=0.8, sqrt_1m_acp=0.6, step=0.1, inv_n=1.0 / (B * 16 * 128), tie=tie, csr=csr,
                row_maps=maps, reuse_memory_side=reuse, want=("x_new",))
    r = timed(torch, call)
    r["launches"] = int(read_debug(m, "weg.info", (5,))[0])
    r["token_rows"] = len(chunks) * B * 16
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
    res = {"what": "hipEvent times on one MI355X, seeded weights (1234); ms.  Loops: B = 1, L = 16, DDIM-50, 6 evaluated chunks over 2 distinct "
                   "memories, S = (24, 161, 24, 8, 1), whole calls / 50, medians of 5.  keyframes_iteration: sample_with_keyframes, every "
                   "iteration guided; torch_loop_iteration: sample_with_loss_guidance(keyframe_loss); plain_iteration: sample; parent: the "
                   "latter two on the parent commit's tree and library in a child process of this run.  guide_call_*: Denoiser.guide alone "
                   "(x_new only), medians of 50, with reuse_memory_side 0 / 2 and the launches.  tied_*: one utterance of 3 windows "
                   "(window_ties(1, 3)), 18 forward rows.  rows1440_*: 15 windows x 6 chunks in one guide call.",
           "device": torch.cuda.get_device_name(0)}
    if a.parent_root:
        parent = os.path.abspath(a.parent_root)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-loop-only", "--root", parent], capture_output=True, text=True,
                           cwd=parent, timeout=500)
        if p.returncode != 0:
            raise SystemExit(f"the parent's run failed ({p.returncode}):\n{p.stderr[-2000:]}")
        res["parent"] = json.loads(p.stdout.strip().splitlines()[-1])
    res.update(torch_loop(a.root))
    from convofusion_amd import longform, sampler
    from oracle import inputs
    m, sch, mems, masks, target, mask, kw, cb = loop_case(a.root)
    res["keyframes_iteration"] = per_iteration(timed(torch, lambda: sampler.sample_with_keyframes(m, sch(), mems, masks, target, mask, 0.5, **kw), n=5, warm=2))
    chunks = (0, 1, 2, 3, 4, 5)
    for reuse in (0, 2):
        res[f"guide_call_reuse{reuse}"] = guide_call(torch, m, cb, chunks, 1, reuse)
    # the 3-window tied run
    m3, sch3, mems3, masks3, target3, mask3, kw3, cb3 = loop_case(a.root, B=3)
    tie = longform.window_ties(1, 3).cuda()
    res["tied_keyframes_iteration"] = per_iteration(timed(torch, lambda: sampler.sample_with_keyframes(m3, sch3(), mems3, masks3, target3, mask3, 0.5, tie=tie, **kw3),
                                                          n=5, warm=2))
    res["tied_plain_iteration"] = per_iteration(timed(torch, lambda: sampler.sample(m3, sch3(), mems3, masks3, tie=tie, **kw3), n=5, warm=2))
    for reuse in (0, 2):
        res[f"tied_guide_call_reuse{reuse}"] = guide_call(torch, m3, cb3, chunks, 3, reuse, tie=tie)
    # 15 windows x 6 chunks = 1 440 token rows in one call
    cb15 = inputs.make_cfg_batch(seed=48, B=15, L=16, S=S_PRODUCT, pad_tail=(5, 0, 7, 0, 0))
    tie15 = longform.window_ties(1, 15).cuda()
    for reuse in (0, 2):
        res[f"rows1440_guide_call_reuse{reuse}"] = guide_call(torch, m, cb15, chunks, 15, reuse, tie=tie15)
    out = a.out or os.path.join(a.root, "profiles", "r31_guide_time.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
