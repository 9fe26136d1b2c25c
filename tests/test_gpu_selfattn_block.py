"""-m gpu: every self-attention path, block by block against float64 (the reference, the measures, the weight sets and the case table:
tests/selfattn_ref.py; their premises and the gate's separation of emulated faults from rounding: tests/test_selfattn_ref_host.py).

  tile      self_attn_fused_kernel (csrc/attn_fused.hpp) behind the one q | k | v launch: a handle created with CFD_ROWTILE=0
  tile16    the tile kernels at L = 16: the grouped q | k + V^T launch and rt_selfattn_kernel at tpr = 1 (same handle)
  rowtile   RT_EPI_QKV, rt_selfattn_kernel and the row-tile out-projection (csrc/rowtile.hpp): the default handle
  saved     the same launches as the row-tile gradient engine's saved forward runs them (Denoiser.vjp): "weg.x.<l>.0" and "weg.x.<l>.1"
            of all nine layers from ONE call with no stop stage -- the production launch sequence, every layer; plain weights only

One test = one (path, case, weight set); layers 0, 4 and 8 inside it.  The block's input is the residual stream at debug stop stage 1
(layer 0) or 5 + 4 (l - 1), its output the stream at stage 2 + 4 l, both read with cfd_debug_read "x" at timestep 417.  d = out - in in
float64 from the two float32 reads is the kernels' update of their OWN input, ex = block(in) in float64: nothing upstream enters.  Per
query row r = (batch row, token) e_r = |d_r - ex_r|_2 / rms_r |ex_r|_2, its worst row, and E = |d - ex|_F / |ex|_F.  Each test asserts,
in this order: the intended path ran (the launches per class of an un-stopped forward of the same problem: 18 cross-attention launches
on the row-tile path, 9 on the tile kernels, 9 attention-class launches; the saved forward: "weg.info" counts launches); the wiring (in
and out within the forward tolerance 1e-4 of the oracle's taps: the stages mean what this file thinks); d and ex finite in every row;
THE GATE, worst row and E each <= 5 x the float32 restatement's + 1e-6, the restatement formed as the device forms its result,
fl32(in + block_f32(in)) - in (the cross-attention block's rule: 22-bit split-pair operands against float32's 24, a floor for rows
whose float32 error is small by chance); bits -- a second call is bit-identical, and in one case per path batch row 0 run alone (Be = 1)
has the bits it has inside the batch.  No row, layer or case is left out of any comparison.

Not reachable under a stop stage, and left with the tests that cover them end to end (test_layernorm_fold_*, the headline-shape sampler
tests): the LayerNorm fold and layer 0 on shared rows -- decide_forward_path switches both off when a stop stage is set.

Measured values of the first green run, per (path, case, weight set, layer): profiles/selfattn_block_gates.log.  The largest per path
(worst row / E, next to the gates they met):
  tile      plain  2.61e-6 (gate 2.99e-6) / 1.50e-6 (2.78e-6)      peaked 9.86e-6 (1.46e-5) / 2.79e-6 (8.52e-6)
  tile16    plain  2.72e-6 (3.00e-6) / 1.76e-6 (2.80e-6)           peaked 5.99e-6 (1.44e-5) / 2.53e-6 (6.15e-6)
  rowtile   plain  3.66e-7 (2.90e-6) / 3.05e-7 (2.15e-6)           peaked 2.93e-6 (2.34e-5) / 7.11e-7 (6.60e-6)
  saved     plain  3.49e-7 (2.94e-6) / 3.05e-7 (2.15e-6)
-- the row-tile paths at no more than 0.17 of a gate, the tile kernels at up to 0.91 of one; every bit comparison exact.

The row-tile figures are behind the change the first run of these gates led to, the tile kernels' are what leaving it out there costs: the
account, with before and after, is in DESIGN.md section 5.1 ("The self-attention block has the same defect in its weights").

If a tile-kernel case turns red with no change to the kernels, look at the host first: the gate is made from numpy's float32 matmul, whose
worst row (about 4e-7 with the plain weights) follows the host BLAS's summation order, and at 0.91 of a gate another numpy / BLAS build can
move the gate past the device's figure.  The printed float32 values against those in the log tell.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import selfattn_ref as R
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-4            # tests/test_gpu_forward.py
BIT_LAYERS = (0, 8)


@functools.lru_cache(maxsize=None)
def _engine(rowtile, ws):
    """A Denoiser with the weight set `ws`: on the default handle (small problems on the row-tile path) or on one with that path off."""
    import torch
    sd = R.weights(ws)
    if not rowtile:
        from tests.test_gpu_selfattn_token_major import _denoiser
        return _denoiser(sd)
    from convofusion_amd.denoiser import Denoiser
    from tests.gpu_helpers import ABL, DENOISER_KW
    m = Denoiser(ablation=ABL, **DENOISER_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    m.engine(torch.device("cuda"))
    return m


def _to_dev(inp):
    from tests.gpu_helpers import to_dev
    return dict(x=to_dev(inp["sample"]), mems=[to_dev(v) for v in inp["memories"]], masks={k: to_dev(v) for k, v in inp["masks"].items()})


@functools.lru_cache(maxsize=None)
def _problem(path, Be, L, ws):
    """The case's inputs on the host and on the device and the oracle's taps (shared by every test of the case; never written)."""
    inp = R.case_inputs(path, Be, L)
    return inp, _to_dev(inp), R.oracle_taps(R.weights(ws), inp)


def _forward(m, dev, stage=0):
    """cfd_forward stopped at `stage`: the residual stream [Be][L][512] (stage 0: the output [Be][L][128])."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.denoiser import Denoiser
    from tests.gpu_helpers import read_debug
    lib, h, x = _lib.load(), m._handle, dev["x"]
    Be, L = int(x.shape[0]), int(x.shape[1])
    mems, keep = Denoiser.pack_memories(dev["mems"], dev["masks"])
    out = torch.empty_like(x)
    ts = (C.c_int32 * 1)(R.T_STEP)
    _lib.check(lib.cfd_debug_stop_stage(h, stage))
    try:
        _lib.check(lib.cfd_forward(h, C.c_void_p(x.data_ptr()), Be, L, ts, 1, mems, C.c_void_p(out.data_ptr()), None,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        res = read_debug(m, "x", (Be, L, 512)) if stage else out.cpu().numpy()
    finally:
        _lib.check(lib.cfd_debug_stop_stage(h, 0))
    del keep
    return res


def _in_stage(layer):
    return 1 if layer == 0 else 5 + 4 * (layer - 1)


def _out_stage(layer):
    return 2 + 4 * layer


def _launches(m, dev):
    """(cross-attention launches, attention-class launches) of one un-stopped forward of the problem."""
    from tests.test_gpu_forward_path import _profile_handle
    out = _forward(m, dev, 0)
    assert np.isfinite(out).all()
    prof = _profile_handle(m)
    return prof["xattn"][1], prof["gemm_attn"][1]


def _saved_taps(m, dev):
    """One Denoiser.vjp call: ({(l, k): "weg.x.<l>.<k>" [Be][L][512]} for k = 0 (layer l's input) and 1 (behind its self-attention), all
    nine layers; "weg.info"'s launch count)."""
    import torch
    from tests.gpu_helpers import read_debug
    x = dev["x"]
    Be, L = int(x.shape[0]), int(x.shape[1])
    m.vjp(x, R.T_STEP, dev["mems"], dev["masks"], torch.ones_like(x))
    taps = {(l, k): read_debug(m, f"weg.x.{l}.{k}", (Be * L, 512)).reshape(Be, L, 512) for l in range(9) for k in (0, 1)}
    return taps, int(read_debug(m, "weg.info", (5,))[0])


def _judge(tag, ws, L, blocks, taps):
    """Wiring, finiteness and the gate over `blocks` = {layer: (in, out)}; prints every measure next to its gate."""
    sd = R.weights(ws)
    for l, (x_in, x_out) in blocks.items():
        w_in, w_out = rel_l2(x_in, R.block_input(taps, l)), rel_l2(x_out, taps[f"l{l}.after_self"])
        assert w_in < FWD_TOL and w_out < FWD_TOL, (tag, l, w_in, w_out)
    missed = []
    for l, (x_in, x_out) in blocks.items():
        d = x_out.astype(np.float64) - x_in.astype(np.float64)
        ex, pr = R.block(sd, l, x_in)
        assert np.isfinite(d).all(-1).all() and np.isfinite(ex).all(-1).all(), (tag, l)
        if ws == "peaked":      # the premise once more, on the kernels' own input
            assert R.peak_median(pr) > 0.5, (tag, l, R.peak_median(pr))
        w32, _, E32 = R.measures(R.yardstick32(sd, l, x_in), ex, L)
        w, at, E = R.measures(d, ex, L)
        gw, gE = R.gate(w32), R.gate(E32)
        print(f"{tag} {ws} layer {l}: worst row {w:.3e} at {at} (float32 {w32:.3e}, gate {gw:.3e}), E {E:.3e} (float32 {E32:.3e}, gate {gE:.3e})")
        if not (w <= gw and E <= gE):
            missed.append(f"layer {l}: worst row {w:.4e} at {at} against {gw:.4e}, E {E:.4e} against {gE:.4e}")
    assert not missed, (tag, ws, missed)


def _params(*paths):
    return [pytest.param(c, id=R.case_id(c)) for c in R.cases(*paths)]


@pytest.mark.parametrize("ws", R.WEIGHT_SETS)
@pytest.mark.parametrize("case", _params("tile", "tile16", "rowtile"))
def test_block_against_float64(case, ws):
    path, Be, L = case["path"], case["Be"], case["L"]
    rowtile = path == "rowtile"
    m = _engine(rowtile, ws)
    inp, dev, taps = _problem(path, Be, L, ws)
    tag = f"{path} {Be}x{L}"
    got = _launches(m, dev)
    assert got == ((18, 9) if rowtile else (9, 9)), (tag, got)
    blocks, differs = {}, []
    for l in R.LAYERS:
        x_in, x_out = _forward(m, dev, _in_stage(l)), _forward(m, dev, _out_stage(l))
        if not np.array_equal(x_out, _forward(m, dev, _out_stage(l))):
            differs.append(f"layer {l}: a second call differs")
        blocks[l] = (x_in, x_out)
    _judge(tag, ws, L, blocks, taps)
    if case.get("alone"):      # rows are independent: batch row 0 by itself
        one = _to_dev(R.first_rows(inp, 1))
        for l in BIT_LAYERS:
            if not np.array_equal(_forward(m, one, _out_stage(l))[0], blocks[l][1][0]):
                differs.append(f"layer {l}: batch row 0 alone differs from batch row 0 of {Be}")
    assert not differs, (tag, ws, differs)


@pytest.mark.parametrize("case", _params("saved"))
def test_saved_forward_against_float64(case):
    Be, L = case["Be"], case["L"]
    m = _engine(True, "plain")
    inp, dev, taps = _problem("saved", Be, L, "plain")
    tag = f"saved {Be}x{L}"
    saved, launches = _saved_taps(m, dev)
    assert launches > 0, (tag, launches)
    _judge(tag, "plain", L, {l: (saved[(l, 0)], saved[(l, 1)]) for l in range(9)}, taps)
    again, _ = _saved_taps(m, dev)
    differs = [f"weg.x.{l}.{k}: a second call differs" for (l, k) in saved if not np.array_equal(saved[(l, k)], again[(l, k)])]
    # the saved forward is the plain forward where a difference would start: behind the self-attention of layers 0 and 8
    for l in BIT_LAYERS:
        if not np.array_equal(saved[(l, 1)], _forward(m, dev, _out_stage(l))):
            differs.append(f"weg.x.{l}.1 differs from the stopped plain forward")
    if case.get("alone"):
        one, _ = _saved_taps(m, _to_dev(R.first_rows(inp, 1)))
        differs += [f"weg.x.{l}.1: batch row 0 alone differs" for l in BIT_LAYERS if not np.array_equal(one[(l, 1)][0], saved[(l, 1)][0])]
    assert not differs, (tag, differs)


@pytest.mark.parametrize("ws", R.WEIGHT_SETS)
def test_two_block_out_projection_is_bit_identical(ws):
    """enqueue_rows_rt runs the 512 x 512 residual products with two 16-feature blocks per workgroup from 14 token tiles on and calls that
    bit-identical (same sums in the same order): the first 13 rows of the (14, 16) case against the (13, 16) case, behind the
    out-projection of layers 0 and 8."""
    m = _engine(True, ws)
    dev13, dev14 = _problem("rowtile", 13, 16, ws)[1], _problem("rowtile", 14, 16, ws)[1]
    for l in BIT_LAYERS:
        a, b = _forward(m, dev13, _out_stage(l)), _forward(m, dev14, _out_stage(l))
        assert np.isfinite(b).all() and np.array_equal(a, b[:13]), (ws, l, float(np.abs(a - b[:13]).max()))
