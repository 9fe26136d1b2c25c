"""-m gpu: every instance of xattn_fused_kernel, block by block against float64 (csrc/xattn_fused.hpp; the references: tests/xattn_ref.py).

One case = one guidance batch (7 chunks of B utterances, distinct memories + row maps, as a sampling run passes them) through cfd_forward
on a handle created with CFD_ROWTILE=0, stopped in front of and behind the cross-attention block of layers 1 and 8 (stop stages 3 + 4 l and
4 + 4 l; one timestep, 417).  d = out - in is the kernel's update of its OWN input; ex = block_unfolded(in) in float64.  Measures, per query
row r = (batch row, token):  e_r = |d_r - ex_r|_2 / rms_r |ex_r|_2, its worst row, and E = |d - ex|_F / |ex|_F.

  pairs  <false, false>: the plain forward.                                  worst <= 5 worst_f32 + 1e-6 and E <= 5 E_f32 + 1e-6, where *_f32 is
  ATT    <true, false>:  the same forward with attention maps requested.     the float32 restatement formed the same way, fl32(in + update) - in
                         (factor and floor: the ill-conditioned-chunk test of test_gpu_forward.py -- 22-bit operands against 24)
  F16    <false, true>:  cfd_debug_forward_operands(15).  emu = block_folded(round q, k, v, p), emu_noP = block_folded(round q, k, v):
                         what the emulation does not explain, |d - emu| (worst row and whole, in the units above), must be
                         <= 2 |emu - emu_noP| + the pairs allowance.  The kernel's q, K and V roundings are the emulation's; its P' roundings
                         fall at other points of the same size -- two independent roundings of equal size differ by sqrt 2, 2 leaves margin.
                         The bound is worst row against worst row: one row's own P' rounding may be small by chance.
                         |emu - ex|, the policy's own rounding, is printed and no gate.

Every (case, instance) asserts through "xa.info" that the instance and the work-list form the case is about really ran, that the update is
finite exactly where the float64 reference is, and that a second call is bit-identical.  The cases and their premises: tests/xattn_ref.py
(CASES), tests/test_xattn_ref_host.py.  Measured values of the first green run: profiles/r21_xattn_block_gates.log.

What the first run of these gates found: pairs and ATT sat AT their gate in every case and over it in two tests --
four_tiles layer 1, worst row 3.907e-6 against 3.793e-6 allowed; the attention maps in 5 of 36 (layer, memory) pairs, e.g. 1.626e-6 against
1.539e-6 -- with no row, tile or memory standing out.  The cause was on the memory side: the folded weights A and VV (elements ~2e-3) were
stored as fp16 split pairs whose `lo` halves are subnormal, 16 - 17 significant bits instead of 22.  They are now stored x CFD_MEMW_SCALE
(csrc/cfd_common.hpp) and the products' epilogues scale back, both exact: E 2.5e-6 -> 1.3e-6, worst row 3.9e-6 -> 1.4e-6, the maps' max abs
1.6e-6 -> 1.7e-7, which is float32's.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import xattn_ref as X

pytestmark = pytest.mark.gpu
INSTANCES = {"pairs": 0, "att": 1, "f16": 2}
# what "xa.info" must say per case: query tiles per workgroup, single-fp16 segments of a workgroup under the F16 instance, whether some
# workgroup walks a memory in passes (more segments than the four memories of the list), flush between online memories
FORM = {
    "one_long":       dict(tpw=1, n16=1, passes=False, flush=0),
    "threshold":      dict(tpw=1, n16=1, passes=False, flush=0),
    "two_long_mixed": dict(tpw=1, n16=2, passes=False, flush=1),
    "two_tiles":      dict(tpw=2, n16=1, passes=True, flush=0),
    "four_tiles":     dict(tpw=4, n16=1, passes=True, flush=0),
    "concentrated":   dict(tpw=1, n16=2, passes=False, flush=1),
    "dead_memory":    dict(tpw=1, n16=1, passes=False, flush=0),
}


@functools.lru_cache(maxsize=2)
def _engine(concentrated):
    from tests.test_gpu_selfattn_token_major import _denoiser      # a Denoiser whose handle has the row-tile path off
    return _denoiser(X.case_state_dict("concentrated" if concentrated else "one_long"))


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's inputs on the host and on the device, and its memory taps (shared by every test of the case; never written)."""
    import torch
    from tests.gpu_helpers import to_dev
    c = X.make_case(name)
    sd = X.case_state_dict(name)
    dev = dict(x=to_dev(c["sample"]), unique=[to_dev(u) for u in c["unique"]], umasks={n: to_dev(v) for n, v in c["umasks"].items()},
               row_map=[torch.from_numpy(r).cuda() for r in c["row_map"]])
    return c, sd, X.memory_taps(sd, X.T_STEP, c["unique"]), dev


def _set_operands(m, policy):
    from convofusion_amd import _lib
    _lib.check(_lib.load().cfd_debug_forward_operands(m._handle, policy))


def _forward(m, dev, stage=0, want_att=False):
    """cfd_forward on the case's distinct memories and row maps, stopped at `stage`: (the residual stream [Be][L][512] -- the output
    [Be][L][128] with stage 0 --, the maps or None, "xa.info")."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.denoiser import Denoiser
    from tests.gpu_helpers import read_debug
    lib, h, x = _lib.load(), m._handle, dev["x"]
    Be, L = int(x.shape[0]), int(x.shape[1])
    mems, keep = Denoiser.pack_memories(dev["unique"], dev["umasks"], dev["row_map"])
    out = torch.empty_like(x)
    att, att_ptrs = None, None
    if want_att:
        att = [torch.full((Be, 9, L, int(u.shape[1])), float("nan"), dtype=torch.float32, device="cuda") for u in dev["unique"]]
        att_ptrs = (C.c_void_p * _lib.NUM_MEM)(*[a.data_ptr() for a in att])
    ts = (C.c_int32 * 1)(X.T_STEP)
    _lib.check(lib.cfd_debug_stop_stage(h, stage))
    try:
        _lib.check(lib.cfd_forward(h, C.c_void_p(x.data_ptr()), Be, L, ts, 1, mems, C.c_void_p(out.data_ptr()), att_ptrs,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.cfd_debug_stop_stage(h, 0))
    del keep
    info = read_debug(m, "xa.info", (7,))
    res = read_debug(m, "x", (Be, L, 512)) if stage else out.cpu().numpy()
    return res, (None if att is None else [a.cpu().numpy() for a in att]), info


def _check_info(info, name, inst):
    form = FORM[name]
    got = dict(inst=int(info[0]), nwg=int(info[1]), tpw=int(info[2]), n16=int(info[3]), nseg=int(info[4]), flush=int(info[5]), one=int(info[6]))
    assert got["inst"] == INSTANCES[inst] and got["nwg"] > 0, (name, inst, got)          # (-1 / 0: the call fell back to another path)
    assert got["tpw"] == form["tpw"] and got["flush"] == form["flush"] and got["one"] == 4, (name, inst, got)
    assert got["n16"] == (form["n16"] if inst == "f16" else 0), (name, inst, got)
    assert (got["nseg"] > 4) if form["passes"] else (got["nseg"] == 4), (name, inst, got)
    return got


def _block(m, dev, layer, inst):
    """(in, out, info) of layer `layer`'s block under instance `inst`; the second call of the stopped forward is bit-identical."""
    _set_operands(m, 15 if inst == "f16" else 0)
    try:
        x_in, _, _ = _forward(m, dev, 3 + 4 * layer, want_att=inst == "att")
        x_out, _, info = _forward(m, dev, 4 + 4 * layer, want_att=inst == "att")
        again, _, _ = _forward(m, dev, 4 + 4 * layer, want_att=inst == "att")
    finally:
        _set_operands(m, 0)
    assert np.array_equal(x_out, again, equal_nan=True), "a second call differs"
    return x_in, x_out, info


def _worst(e, L):
    r = int(np.nanargmax(e))
    return float(e[r]), (r // L, r % L)


@pytest.mark.parametrize("inst", sorted(INSTANCES))
@pytest.mark.parametrize("name", sorted(FORM))
def test_block_against_float64(name, inst):
    c, sd, taps, dev = _case(name)
    m = _engine(name == "concentrated")
    L = X.CASES[name]["L"]
    args = (taps, c["umasks"], c["row_map"])
    pos, par, missed = set(), set(), []
    for layer in X.LAYERS:
        x_in, x_out, info = _block(m, dev, layer, inst)
        got = _check_info(info, name, inst)
        d = x_out.astype(np.float64) - x_in.astype(np.float64)
        ex, pr = X.block_unfolded(sd, layer, x_in, *args)
        # finite exactly where the reference is
        ref_nan = np.isnan(ex).all(-1)
        assert np.array_equal(np.isfinite(ex).all(-1), ~ref_nan)
        assert np.array_equal(np.isfinite(d).all(-1), ~ref_nan), (name, inst, layer, int(ref_nan.sum()), int((~np.isfinite(d).all(-1)).sum()))
        assert int(ref_nan.sum()) == (2 * L if name == "dead_memory" else 0)
        if name == "dead_memory":
            assert np.array_equal(ref_nan.all(-1), c["row_map"][1] == 1) and np.isnan(d[ref_nan]).all()
        u32 = X.block_unfolded(sd, layer, x_in, *args, dtype=np.float32)[0]
        d32 = (x_in + u32).astype(np.float64) - x_in.astype(np.float64)
        e32, E32, rms = X.row_errors(d32, ex)
        w32, _ = _worst(e32, L)
        e, E, _ = X.row_errors(d, ex)
        w, at = _worst(e, L)
        tag = f"{name} {inst} layer {layer} [tpw {got['tpw']} n16 {got['n16']} nseg {got['nseg']} nwg {got['nwg']}]:"
        if name == "concentrated":      # the premise once more, on the kernel's own input
            pk, am = pr[1].max(-1), pr[1].argmax(-1)
            assert np.median(pk) > 0.5, (layer, float(np.median(pk)))
            pos |= set((am[pk > 0.5] % 32).tolist())
            par |= set(((am[pk > 0.5] // 32) % 2).tolist())
        if inst != "f16":
            print(f"{tag} worst row {w:.3e} at {at} (float32 {w32:.3e}), E {E:.3e} (float32 {E32:.3e})")
            if not (w <= 5 * w32 + 1e-6 and E <= 5 * E32 + 1e-6):
                missed.append(f"layer {layer}: worst row {w:.4e} at {at} against {5 * w32 + 1e-6:.4e}, E {E:.4e} against {5 * E32 + 1e-6:.4e}")
            continue
        emu = X.block_folded(sd, layer, x_in, *args, round_ops=("q", "k", "v", "p"))[0]
        noP = X.block_folded(sd, layer, x_in, *args, round_ops=("q", "k", "v"))[0]
        ok = ~ref_nan.reshape(-1)
        row = lambda a, b: np.where(ok, np.sqrt((np.where(np.isfinite(a - b), a - b, 0.0) ** 2).sum(-1)).reshape(-1) / rms, np.nan)
        nex = float(np.linalg.norm(ex[~ref_nan]))
        g, gp, own = row(d, emu), row(emu, noP), row(emu, ex)
        wg, at = _worst(g, L)
        G = float(np.linalg.norm((d - emu)[~ref_nan]) / nex)
        GP = float(np.linalg.norm((emu - noP)[~ref_nan]) / nex)
        print(f"{tag} unexplained worst row {wg:.3e} at {at}, whole {G:.3e}; P' rounding worst row {np.nanmax(gp):.3e}, whole {GP:.3e}; "
              f"the policy's own rounding worst row {np.nanmax(own):.3e}, whole {float(np.linalg.norm((emu - ex)[~ref_nan]) / nex):.3e}; "
              f"against float64 worst row {w:.3e}, E {E:.3e} (float32 {w32:.3e}, {E32:.3e})")
        if not (wg <= 2 * np.nanmax(gp) + 5 * w32 + 1e-6 and G <= 2 * GP + 5 * E32 + 1e-6):
            missed.append(f"layer {layer}: unexplained worst row {wg:.4e} at {at} against {2 * np.nanmax(gp) + 5 * w32 + 1e-6:.4e}, "
                          f"whole {G:.4e} against {2 * GP + 5 * E32 + 1e-6:.4e}")
    assert not missed, (name, inst, missed)
    if name == "concentrated":
        assert pos == set(range(32)) and par == {0, 1}, (sorted(set(range(32)) - pos), par)


def test_below_the_threshold_the_hook_changes_nothing():
    """96 audio keys (the threshold case has 97 = 128 padded): no memory is long, so under cfd_debug_forward_operands(15) the forward runs
    the pair instance, bit for bit what it computes without the hook."""
    c, sd, taps, dev = _case("threshold_96")
    m = _engine(False)
    res = {}
    for policy in (0, 15):
        _set_operands(m, policy)
        try:
            res[policy] = [_forward(m, dev, stage) for stage in (4 + 4 * 1, 4 + 4 * 8, 0)]
        finally:
            _set_operands(m, 0)
    for (a, _, ia), (b, _, ib) in zip(res[0], res[15]):
        assert int(ia[0]) == 0 and int(ib[0]) == 0 and int(ib[3]) == 0 and int(ib[1]) > 0, (ia, ib)
        assert np.isfinite(a).all() and np.array_equal(a, b)


def test_the_hook_refuses_what_it_cannot_mean():
    import torch
    from convofusion_amd import _lib, scheduler
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import SCHED_KW
    c, sd, taps, dev = _case("one_long")
    m = _engine(False)
    lib = _lib.load()
    assert lib.cfd_debug_forward_operands(m._handle, 7) == -1                 # CFD_E_ARG
    assert lib.cfd_debug_forward_operands(None, 15) == -1
    mems = [torch.from_numpy(np.ascontiguousarray(q)).cuda() for q in c["memories"]]
    masks = {k: (None if v is None else torch.from_numpy(v).cuda()) for k, v in c["masks"].items()}
    run = SamplingRun(m, scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW), mems, masks, 2, X.CASES["one_long"]["L"], 2, guidance_scale=7.5, seed=3)
    try:
        assert lib.cfd_debug_forward_operands(m._handle, 15) == -3            # CFD_E_STATE: a sampling run is open
    finally:
        run.steps(2)
        assert torch.isfinite(run.read(close=True)).all()
    # attention maps wanted: split-pair tiles whatever the hook says (the ATT instance), as a run with an attention ring
    _set_operands(m, 15)
    try:
        _, _, info = _forward(m, dev, 4 + 4 * 1, want_att=True)
    finally:
        _set_operands(m, 0)
    assert int(info[0]) == 1 and int(info[3]) == 0, info


def test_attention_maps_of_the_att_instance_against_float64():
    """One full forward with maps on the two-long-memories case; every layer's maps against the float64 probabilities of that layer's tapped
    input (nine stopped calls of the same deterministic forward): max abs <= 5 x the float32 restatement's + 1e-6, masked keys exactly 0,
    rows sum to 1 within 1e-5."""
    name = "two_long_mixed"
    c, sd, taps, dev = _case(name)
    m = _engine(False)
    _, att, info = _forward(m, dev, 0, want_att=True)
    assert int(info[0]) == 1 and int(info[1]) > 0, info
    args = (taps, c["umasks"], c["row_map"])
    missed = []
    for layer in range(9):
        x_in, _, info = _forward(m, dev, 3 + 4 * layer, want_att=True)
        assert int(info[0]) == (1 if layer else -1), (layer, info)          # (layer 0's tap is in front of the first block: nothing launched yet)
        p64 = X.block_unfolded(sd, layer, x_in, *args)[1]
        p32 = X.block_unfolded(sd, layer, x_in, *args, dtype=np.float32)[1]
        for j, n in enumerate(X.MEM_NAMES):
            got = att[j][:, layer]
            assert np.isfinite(got).all(), (layer, n)
            err, err32 = float(np.abs(got - p64[j]).max()), float(np.abs(p32[j].astype(np.float64) - p64[j]).max())
            print(f"maps layer {layer} {n}: max abs {err:.3e} (float32 {err32:.3e}), row sums within {float(np.abs(got.sum(-1) - 1).max()):.2e}")
            if not err <= 5 * err32 + 1e-6:
                missed.append(f"layer {layer} {n}: max abs {err:.4e} against {5 * err32 + 1e-6:.4e}")
            assert np.abs(got.astype(np.float64).sum(-1) - 1).max() <= 1e-5, (layer, n)
            if c["umasks"][n] is not None:
                dead = c["umasks"][n][c["row_map"][j]]                       # [Be][S]
                assert (got[np.broadcast_to(dead[:, None, :], got.shape)] == 0).all(), (layer, n)

    assert not missed, missed
