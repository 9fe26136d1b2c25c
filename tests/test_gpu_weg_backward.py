"""-m gpu: the reverse sweep of the row-tile word-excitation-guidance evaluation (csrc/rowtile_bwd.hpp, launched from csrc/weg_rt.hpp),
LAUNCH BY LAUNCH against the float64 restatement tests/weg_bwd_ref.py.

``cfd_debug_weg_stop`` leaves the sweep behind one named launch; the buffers that launch wrote are read with ``cfd_debug_read`` and
compared with the float64 tap of the same meaning.  Before every stopped evaluation the gradient buffers are filled with NaN: what
the launches up to the stop have not written must still hold it, and what they have written must be finite in every one of the B * L
rows (the tiles are ragged, the buffers dense).

Two measures per tap: relative L2 over the tap, and the worst token row (the row's error norm over the tap's RMS row norm), so that
one wrong row of a ragged tile fails.  GATES are 4 x the largest error measured on the MI355X per tap class over the three cases
(the kernels reduce in a fixed order: the margin is for other seeds and shapes, not for run-to-run noise; profiles/
r17_weg_backward_taps.txt has the per-tap figures next to plain numpy float32 at the same tap), and never above 2e-4 / 2e-3 -- a gate
above that no longer separates a dropped term from rounding (tests/test_oracle_weg.py checks that float32 itself stays under those
caps at every tap of these cases).

The one buffer that is no reference quantity as it stands is dP: in the folded formulation the value bias (and the memory LayerNorm's
beta) lives in the cross-attention's constant bias, so dP lacks, per (token row, memory), one constant that the softmax backward
removes anyway.  It is compared after that removal (dP - sum_s p_s dP_s per memory, over the unmasked keys), and B4 is covered a
second time through its running-gradient tap and B5's dy."""
import ctypes as C

import numpy as np
import pytest

from tests import weg_bwd_ref
from tests.weg_bwd_ref import BWD_CASES, bwd_case, rows, tap_errors

pytestmark = pytest.mark.gpu

NL = 9
CAP = (2e-4, 2e-3)
# class -> the largest (relative L2, worst row) measured on the MI355X over the three cases (profiles/r17_weg_backward_taps.txt).  Almost
# all of it is inherited: the sweep starts from the split-pair forward's probabilities (1.5e-5 at the top layer's B5 already); plain
# numpy float32 in the unfolded formulation sits at 1e-6.
MEASURED = {
    "gx": (1.48e-5, 5.97e-5), "dpre": (1.43e-5, 5.74e-5), "dn3": (1.40e-5, 5.44e-5), "dz2": (1.53e-5, 6.13e-5), "dP": (2.63e-6, 6.00e-6),
    "dn2": (1.49e-5, 6.29e-5), "dz1": (1.44e-5, 5.81e-5), "dO": (1.54e-5, 6.37e-5), "dqkv": (1.59e-5, 3.21e-5), "dn1": (1.62e-5, 3.34e-5),
}
GATES = {c: (4 * a, 4 * b) for c, (a, b) in MEASURED.items()}
assert all(g[0] <= CAP[0] and g[1] <= CAP[1] for g in GATES.values())

# the sweep, top down: (stop, layer, launch); what a launch writes
SWEEP = [(16 * l + k, l, k) for l in reversed(range(NL)) for k in range(1, 10) if not (l == NL - 1 and k < 5)] + [(10, 0, 10)]
WRITES = {1: ("g", "dh"), 2: ("dy",), 3: ("g", "dz"), 4: ("g", "dP"), 5: ("dy",), 6: ("g", "dz"), 7: ("g", "dO"), 8: ("dqkv",), 9: ("dy",), 10: ("g",)}
WIDTH = {"dh": 1024, "dy": 512, "dz": 512, "dO": 512, "dqkv": 1536, "g0": 512, "g1": 512, "g2": 512}


def _dp_centred(dp_by_mem, p_by_mem, masks_by_mem):
    """[rows, sum S_j]: per memory dP - sum_s p_s dP_s over its unmasked keys (masked keys: 0)."""
    out = []
    for dp, p, mk in zip(dp_by_mem, p_by_mem, masks_by_mem):
        dp = np.where(mk, 0.0, np.asarray(dp, dtype=np.float64))
        out.append(np.where(mk, 0.0, dp - (dp * p).sum(axis=-1, keepdims=True)))
    return np.concatenate(out, axis=-1)


def _expected(name, dtype):
    """stop -> list of (class, tap name, buffer, reference rows) for the launches of the sweep."""
    B, L, S, _, _, _ = BWD_CASES[name]
    inp, _, _, res = bwd_case(name, dtype)
    taps = res[4]
    p64 = bwd_case(name)[3][4]
    mk = [np.zeros((B * L, S[j]), dtype=bool) if inp["masks"][weg_bwd_ref.MEM_NAMES[j]] is None
          else np.repeat(inp["masks"][weg_bwd_ref.MEM_NAMES[j]], L, axis=0) for j in range(5)]
    exp = {}
    for stop, l, k in SWEEP:
        e = []
        if k == 1:
            e += [("gx", f"gx.{l + 1}.0", "g", rows(taps[f"gx.{l + 1}.0"])), ("dpre", f"dpre.{l}", "dh", rows(taps[f"dpre.{l}"]))]
        elif k == 2:
            e += [("dn3", f"dn3.{l}", "dy", rows(taps[f"dn3.{l}"]))]
        elif k == 3:
            e += [("gx", f"gx.{l}.4", "g", rows(taps[f"gx.{l}.4"])), ("dz2", f"dz2.{l}", "dz", rows(taps[f"dz2.{l}"]))]
        elif k == 4:
            cen = _dp_centred([taps[f"dP.{l}.{j}"].reshape(B * L, -1) for j in range(5)], [p64[f"p.{l}.{j}"].reshape(B * L, -1) for j in range(5)], mk)
            e += [("gx", f"gx.{l}.3", "g", rows(taps[f"gx.{l}.3"])), ("dP", f"dP.{l}", "dP", cen)]
        elif k == 5:
            e += [("dn2", f"dn2.{l}", "dy", rows(taps[f"dn2.{l}"]))]
        elif k == 6:
            e += [("gx", f"gx.{l}.2", "g", rows(taps[f"gx.{l}.2"])), ("dz1", f"dz1.{l}", "dz", rows(taps[f"dz1.{l}"]))]
        elif k == 7:
            e += [("gx", f"gx.{l}.1", "g", rows(taps[f"gx.{l}.1"])), ("dO", f"dO.{l}", "dO", rows(taps[f"dO.{l}"]))]
        elif k == 8:
            e += [("dqkv", f"dqkv.{l}", "dqkv", rows(taps[f"dqkv.{l}"]))]
        elif k == 9:
            e += [("dn1", f"dn1.{l}", "dy", rows(taps[f"dn1.{l}"]))]
        else:
            e += [("gx", "gx.0.0", "g", rows(taps["gx.0.0"]))]
        exp[stop] = e
    return exp, mk, p64


@pytest.mark.parametrize("name", list(BWD_CASES))
def test_reverse_sweep_launch_by_launch(name):
    import torch
    from convofusion_amd import _lib, weg
    from tests.gpu_helpers import dev_inputs, hip_denoiser, read_debug, to_dev
    B, L, S, _, t, focus = BWD_CASES[name]
    M, Sp = B * L, [(s + 31) // 32 * 32 for s in S]
    off = np.concatenate([[0], np.cumsum(Sp)]).astype(int)
    inp, _, _, r64 = bwd_case(name)
    exp64, mk, p64 = _expected(name, np.float64)
    exp32, _, _ = _expected(name, np.float32)
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    masks = {k: (v.to(torch.uint8).contiguous() if v is not None else None) for k, v in masks.items()}   # (as the library takes them: no copy, one address per call)
    lat, eot = to_dev(inp["sample"]), torch.zeros(1, dtype=torch.long)
    ev = lambda: weg.loss_and_grad(m, lat, t, mems, masks, focus, False, eot)
    lib = _lib.load()
    loss0, _, _, grad0 = ev()                                    # a complete evaluation: the workspace exists from here on
    info = read_debug(m, "weg.info", (5,))
    print(f"{name}: {int(info[0])} launches, Sp_tot {int(info[1])}, rt_xbwd_dy_kernel<{int(info[2])}>, objective kernel {'large' if info[3] else 'small'}")
    assert int(info[1]) == off[-1] and int(info[2]) == (1024 if off[-1] > 512 else 512)
    assert abs(float(loss0) - float(r64[0])) < 2e-6
    WIDTH["dP"] = int(off[-1])
    worst, bad, n_g, written = {}, [], 0, set()
    try:
        for stop, l, k in SWEEP:
            _lib.check(lib.cfd_debug_weg_fill(m._handle, C.c_float(float("nan"))))
            _lib.check(lib.cfd_debug_weg_stop(m._handle, stop))
            ev()
            for buf in WRITES[k]:
                if buf == "g":
                    n_g += 1
                    written.add(f"g{n_g % 3}")
                else:
                    written.add(buf)
            gi = int(read_debug(m, "weg.info", (5,))[4])
            assert gi == (n_g % 3 if n_g else -1), (stop, gi, n_g)
            # sentinels: what the sweep has not reached is untouched, what it has written is written in every row
            got = {}
            for buf, w in WIDTH.items():
                a = read_debug(m, "weg." + buf, (M, w))
                if buf in written:
                    assert np.isfinite(a).all(), f"stop {stop} (layer {l}, B{k}): {buf} has unwritten or non-finite entries"
                else:
                    assert np.isnan(a).all(), f"stop {stop} (layer {l}, B{k}): {buf} was written before its launch"
                got[buf] = a
            got["g"] = got[f"g{gi}"] if gi >= 0 else None
            if gi >= 0:
                assert np.array_equal(got["g"], read_debug(m, "weg.g", (M, 512)))
            for (cls, tap, buf, want), (_, _, _, want32) in zip(exp64[stop], exp32[stop]):
                a = got[buf]
                if buf == "dP":
                    a = _dp_centred([a[:, off[j]:off[j] + S[j]] for j in range(5)], [p64[f"p.{l}.{j}"].reshape(M, -1) for j in range(5)], mk)
                e, er = tap_errors(a, want)
                e32, er32 = tap_errors(want32, want)
                print(f"{name} layer {l} B{k:<2d} {tap:9s} HIP rel L2 {e:.2e} worst row {er:.2e} | numpy float32 {e32:.2e} {er32:.2e}")
                worst[cls] = max(worst.get(cls, (0, 0))[0], e), max(worst.get(cls, (0, 0))[1], er)
                if not (e <= GATES[cls][0] and er <= GATES[cls][1]):
                    bad.append((tap, f"B{k}", e, er))
    finally:
        _lib.check(lib.cfd_debug_weg_stop(m._handle, 0))
    print(name, "largest per class:", {c: (f"{a:.2e}", f"{b:.2e}") for c, (a, b) in worst.items()})
    assert not bad, f"first tap outside its gate: {bad[0]}; all: {bad}"
    # the stopped evaluations were no uses of the graph key and left the product path as it was
    for _ in range(3):
        loss1, _, _, grad1 = ev()
        assert float(loss1) == float(loss0) and torch.equal(grad1, grad0)
    # the saved residual stream is readable too (the forward has its own tests: finite and the reference's to forward precision)
    for l, k in ((0, 0), (4, 3), (NL - 1, 3)):           # (NL - 1, 3): the last point the saved forward reaches
        x = read_debug(m, f"weg.x.{l}.{k}", (M, 512))
        assert tap_errors(x, rows(r64[4][f"x.{l}.{k}"]))[0] < 1e-3


def test_stop_hook_refuses_what_it_cannot_serve():
    import torch
    from convofusion_amd import _lib, weg
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    lib = _lib.load()
    h = m.engine(torch.device("cuda", 0))
    for stop in (-1, 11, 16 * 8 + 4, 16 * 9 + 5, 16 * 3 + 10, 16 * 3):      # the top layer has no B1 .. B4; 10 belongs to layer 0 only
        assert lib.cfd_debug_weg_stop(h, stop) == -1, stop                     # CFD_E_ARG
    enc = [torch.zeros(1, s, 512, device="cuda") for s in (4, 6, 12, 8, 1)]
    lat = torch.zeros(1, 64, 128, device="cuda")                               # 64 tokens per row: not a row-tile evaluation
    try:
        _lib.check(lib.cfd_debug_weg_stop(h, 16 * 2 + 5))
        with pytest.raises(_lib.CfdError) as err:
            weg.loss_and_grad(m, lat, 5, enc, {}, [[2]], False, torch.zeros(1, dtype=torch.long))
        assert err.value.code == -3                                            # CFD_E_STATE
    finally:
        _lib.check(lib.cfd_debug_weg_stop(h, 0))
    loss, _, _, grad = weg.loss_and_grad(m, lat, 5, enc, {}, [[2]], False, torch.zeros(1, dtype=torch.long))   # ... and runs with the hook off
    assert torch.isfinite(grad).all()
