"""Developer tool (GPU box): what the memory gradient costs, next to the latent VJP it extends.

At the product shape (Be = 7 rows of L = 16 over B + 1 = 2 distinct memories with row maps, S = (24, 161, 24, 8, 1); seeded weights):
  vjp                 one ``cfd_denoise_vjp`` (``Denoiser.vjp``, no ``out``) -- and, with ``--parent-root DIR`` (a checkout of the parent
                      commit with its library built), the same call there, in a child process of this run: same box, same session.
                      No code on its path changes; the pair documents that.
  vjp_mem_all         one ``cfd_denoise_vjp_mem`` with all five memories (``Denoiser.vjp_memories``)
  vjp_mem_lsnemb      the same with ``wrt=("lsnemb",)`` and no sample gradient
  fit_identity_step   one step of ``fit.fit_identity`` at B = 8 examples (forward + memory gradient + Adam), whole call of STEPS steps / STEPS
and the launches of each ("weg.info").

Timer: hipEvents (torch.cuda.Event) around one call, medians of 50 with the spread; every variant is warmed up first.  The calls block
(they return with their results complete), so a figure is a host round trip, not the cost of an enqueue.

Usage:  python tools/mem_vjp_time.py [--parent-root DIR] [--out OUT.json]      (default profiles/r29_mem_vjp_time.json)
        python tools/mem_vjp_time.py --plain-only --root DIR                   (the child: prints one JSON line)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

N = 50
S_PRODUCT = (24, 161, 24, 8, 1)


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


def product_case(root):
    import numpy as np
    sys.path.insert(0, root)
    from oracle import inputs
    from tests.gpu_helpers import hip_denoiser, to_dev
    cb = inputs.make_cfg_batch(seed=43, B=1, L=16, S=S_PRODUCT, pad_tail=(5, 0, 7, 0, 0))
    sample = np.random.Generator(np.random.PCG64(44)).standard_normal((7, 16, 128), dtype=np.float32)
    umasks = {}
    for j, k in enumerate(inputs.MEM_NAMES):
        mk = cb["masks"][k]
        umasks[k] = None if mk is None else to_dev(np.stack([mk[list(cb["row_map"][j]).index(u)] for u in range(2)]))
    return hip_denoiser(1234, 1.0), to_dev(sample), [to_dev(v) for v in cb["unique"]], umasks, [to_dev(r) for r in cb["row_map"]]


def plain(root):
    import torch
    m, x, mems, masks, maps = product_case(root)
    from tests.gpu_helpers import read_debug
    c = torch.ones_like(x)
    r = timed(torch, lambda: m.vjp(x, 433, mems, masks, c, row_maps=maps, want_out=False))
    r["launches"] = int(read_debug(m, "weg.info", (5,))[0])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.plain_only:
        print(json.dumps(plain(os.path.abspath(a.root))))
        return
    import numpy as np
    import torch
    res = {"what": "hipEvent times on one MI355X, seeded weights (1234); ms, medians of 50.  Product shape: Be = 7 rows of L = 16 over 2 distinct "
                   "memories with row maps, S = (24, 161, 24, 8, 1), timestep 433.  vjp: cfd_denoise_vjp (no out); vjp_parent: the same call on "
                   "the parent commit's tree and library in a child process of this run; vjp_mem_all: cfd_denoise_vjp_mem, all five memories "
                   "and the sample's gradient; vjp_mem_lsnemb: lsnemb only, no sample gradient; fit_identity_step: fit.fit_identity at B = 8, "
                   "L = 16, the same memory lengths, whole call of 10 Adam steps / 10.",
           "device": torch.cuda.get_device_name(0)}
    if a.parent_root:
        parent = os.path.abspath(a.parent_root)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--root", parent], capture_output=True, text=True, cwd=parent,
                           timeout=300)
        if p.returncode != 0:
            raise SystemExit(f"the parent's run failed ({p.returncode}):\n{p.stderr[-2000:]}")
        res["vjp_parent"] = json.loads(p.stdout.strip().splitlines()[-1])
    res["vjp"] = plain(a.root)
    m, x, mems, masks, maps = product_case(a.root)
    from convofusion_amd import fit, scheduler
    from oracle import inputs
    from tests.gpu_helpers import SCHED_KW, read_debug, to_dev
    c = torch.ones_like(x)
    res["vjp_mem_all"] = timed(torch, lambda: m.vjp_memories(x, 433, mems, masks, c, row_maps=maps, want_out=False))
    res["vjp_mem_all"]["launches"] = int(read_debug(m, "weg.info", (5,))[0])
    res["vjp_mem_lsnemb"] = timed(torch, lambda: m.vjp_memories(x, 433, mems, masks, c, wrt=("lsnemb",), row_maps=maps, want_out=False, want_grad=False))
    res["vjp_mem_lsnemb"]["launches"] = int(read_debug(m, "weg.info", (5,))[0])
    B, steps = 8, 10
    inp = inputs.make_plain_batch(seed=45, Be=B, L=16, S=S_PRODUCT, pad_tail=(5, 0, 7, 0, 0))
    lat = to_dev(np.random.Generator(np.random.PCG64(46)).standard_normal((B, 16, 128), dtype=np.float32))
    fm, fk = [to_dev(v) for v in inp["memories"]], {k: to_dev(v) for k, v in inp["masks"].items()}
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    one = timed(torch, lambda: fit.fit_identity(m, sch, lat, fm, fk, steps=steps, lr=0.01, seed=1), n=N, warm=2)
    res["fit_identity_step"] = {k: (v / steps if k.endswith("_ms") else v) for k, v in one.items()}
    res["fit_identity_step"]["launches_of_its_vjp_mem"] = int(read_debug(m, "weg.info", (5,))[0])
    out = a.out or os.path.join(a.root, "profiles", "r29_mem_vjp_time.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
