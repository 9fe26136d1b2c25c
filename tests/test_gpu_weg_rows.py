"""-m gpu: word-excitation guidance with every row its own utterance (cfd_weg_step, ``weg.step_rows`` / ``weg_update_rows``,
``sample_with_weg(per_row=True)``, ``longform.synthesize_latents(focus_indices=)``) against the restatement tests/weg_rows_ref.py,
which composes ``oracle.weg_ref`` at B = 1 row by row: the per-row focus kernels at launch level, the gradient against float64 per
row, the tied fold bit for bit, the loop with per-row refinement rounds, and the tied long-form run.  Errors are printed.
Seeded weights: whether guided motions look right under a trained checkpoint is not measured here."""
import ctypes as C

import numpy as np
import pytest

from oracle import denoiser_ref, inputs, scheduler_ref
from tests import weg_rows_ref as R
from tests.helpers import load_golden, rel_l2, state_dict

pytestmark = pytest.mark.gpu
SHAPE = dict(L=16, S=(6, 20, 12, 8, 1), pad=(2, 0, 3, 0, 0))      # tlsn masks 3 + b % 4 trailing keys: EOTs 8, 7, 6


# ----------------------------------------------------------------------------- 1. the objective, at launch level
def _focus_rows(m, att, focus, lasts, last, per_row, small, nt_max=None):
    """One cfd_test_weg_focus_rows launch: (rc, losses, max_att, d_att) as device tensors."""
    import torch
    from convofusion_amd import _lib, weg
    B, NL, L, S = att.shape
    off = np.cumsum([0] + [len(s) for s in focus]).astype(np.int32)
    flat = np.array([i for s in focus for i in s] or [0], dtype=np.int32)
    nt_max = max(1, max(len(s) for s in focus)) if nt_max is None else nt_max
    lr = None if lasts is None else np.asarray(lasts, dtype=np.int32)
    ws = torch.empty(B * (3 * L * (last - 1) + 3 * nt_max), dtype=torch.float32, device="cuda")
    losses = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    mx = torch.full((max(1, int(off[-1])),), float("nan"), dtype=torch.float32, device="cuda")
    d = torch.full_like(att, float("nan"))
    k3 = (C.c_float * 3)(*weg.gaussian_kernel3())
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.load().cfd_test_weg_focus_rows(m.engine(att.device), ptr(att), B, NL, L, S, off.ctypes.data, flat.ctypes.data,
                                             lr.ctypes.data if lr is not None else None, last, nt_max, k3, per_row, small, ptr(ws), ptr(losses),
                                             ptr(mx), ptr(d), None)
    torch.cuda.synchronize()
    return rc, losses, mx, d


FOCUS_CASES = {
    # the narrowest legal slice (row 2: two columns), focus on the first and the last column, a repeated token, one empty row
    "small": ((3, 9, 16, 24), (22, 9, 3), [[1, 21, 7, 7], [], [1, 2]]),
    "general": ((2, 9, 196, 32), (22, 30), [[1, 5, 21], [29, 3]]),
}


@pytest.mark.parametrize("case", list(FOCUS_CASES))
def test_per_row_focus_kernels_match_the_oracle_per_row(case):
    import torch
    from convofusion_amd import weg
    from tests.gpu_helpers import hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    (B, NL, L, S), lasts, focus = FOCUS_CASES[case]
    rng = np.random.Generator(np.random.PCG64(5))
    att = rng.random((B, NL, L, S)).astype(np.float32) ** 4
    att /= att.sum(-1, keepdims=True)
    want_l, want_mx, want_d = R.focus_loss_rows(att, focus, lasts)
    att_d = to_dev(att)
    results = {}
    for small in ((1, 0) if case == "small" else (0,)):
        rc, losses, mx, d = _focus_rows(m, att_d, focus, lasts, max(lasts), 1, small)
        assert rc == 0
        results[small] = (losses, mx, d)
        d_host = d.cpu().numpy()
        e = rel_l2(d_host, want_d)
        print(f"{case} kernel small={small}: losses {losses.cpu().numpy()} (oracle {want_l}), d_att rel L2 {e:.2e}")
        np.testing.assert_allclose(losses.cpu().numpy(), want_l, atol=2e-6)
        np.testing.assert_allclose(mx.cpu().numpy()[:sum(len(s) for s in focus)], [float(v) for s in want_mx for v in s], rtol=1e-5)
        assert e < 1e-5
        for b in range(B):       # keys outside the row's slice: exact zeros; a row without focus tokens: loss 0, gradient 0
            assert not d_host[b, ..., 0].any() and not d_host[b, ..., lasts[b]:].any()
            if not focus[b]:
                assert float(losses[b]) == 0.0 and not d_host[b].any()
    if case == "small":          # the two kernels are one arithmetic
        assert all(torch.equal(a, b) for a, b in zip(results[0], results[1]))
    else:
        assert _focus_rows(m, att_d, focus, lasts, max(lasts), 1, 1)[0] == -1      # CFD_E_ARG: the shape does not fit the small kernel
    # a null table and the batch-mean scale: cfd_weg_focus's bits from both kernels
    _, ref_l, ref_mx, ref_d = weg.attention_focus_loss(m, att_d, focus, False, ())
    for small in ((1, 0) if case == "small" else (0,)):
        rc, losses, mx, d = _focus_rows(m, att_d, focus, None, S - 1, 0, small)
        assert rc == 0 and torch.equal(losses, ref_l) and torch.equal(d, ref_d)
        assert [float(v) for v in mx[:sum(len(s) for s in focus)]] == [float(v) for s in ref_mx for v in s]
    # the hook refuses a focus index outside its row's slice and a slice shorter than 2, naming the row, before any launch
    from convofusion_amd import _lib
    assert _focus_rows(m, att_d, [[lasts[0]]] + [[]] * (B - 1), lasts, max(lasts), 1, 0)[0] == -1
    assert "row 0" in _lib.load().cfd_last_error().decode()
    assert _focus_rows(m, att_d, focus, (2,) + tuple(lasts[1:]), max(lasts), 1, 0)[0] == -2
    assert "row 0" in _lib.load().cfd_last_error().decode()


# ----------------------------------------------------------------------------- 2. the gradient
_f64 = {}


def _grad_case(S_tlsn):
    S = (6, 20, S_tlsn, 8, 1)
    inp = inputs.make_plain_batch(seed=77 + S_tlsn, Be=3, L=16, S=S, pad_tail=SHAPE["pad"])
    eots = R.row_eots(inp["masks"])
    focus = [[2, 5], [3], [1, 4]] if S_tlsn == 12 else [[2, 70, 75], [33], [1, 73]]
    return inp, 500, eots, focus


def _float64_rows(S_tlsn):
    from tests import weg_bwd_ref
    if S_tlsn not in _f64:
        inp, t, eots, focus = _grad_case(S_tlsn)
        out = []
        for b in range(3):
            st, mk = R.one_row(inp["memories"], inp["masks"], b)
            r = weg_bwd_ref.loss_and_grad_taps(state_dict(1234, 1.0), inp["sample"][b:b + 1], t, st, mk, [focus[b]], True, [eots[b]])
            out.append((float(r[0]), [float(v) for v in r[2][0]], r[3][0]))
        _f64[S_tlsn] = out
    return _f64[S_tlsn]


@pytest.mark.parametrize("S_tlsn", [12, 80])
def test_step_gradient_matches_float64_per_row(S_tlsn):
    """cfd_weg_step at B = 3 with EOTs that differ (S_tlsn = 80: the general focus kernel on the engine) against float64 per row under
    the existing F64_GRAD_GATE; row b of the batched call against the B = 1 call on row b alone; two identical calls and
    reuse_memory_side 1 / 2 against a fresh call, bit for bit."""
    import torch
    from convofusion_amd import weg
    from tests import weg_bwd_ref
    from tests.gpu_helpers import dev_inputs, hip_denoiser, read_debug, to_dev
    from tests.test_gpu_weg import F64_GRAD_GATE
    m = hip_denoiser(1234, 1.0)
    inp, t, eots, focus = _grad_case(S_tlsn)
    assert len(set(eots)) == 3
    mems, masks = dev_inputs(inp)
    x = to_dev(inp["sample"])
    losses, mx, grad = weg.loss_and_grad_rows(m, x, t, mems, masks, focus)
    info = read_debug(m, "weg.info", (5,))
    assert int(info[3]) == (1 if S_tlsn == 80 else 0)
    St = inp["memories"][2].shape[1]
    datt = read_debug(m, "weg.d_att", (3, 9, 16, St))
    g = grad.cpu().numpy()
    for b, (l64, mx64, g64) in enumerate(_float64_rows(S_tlsn)):
        e, er = weg_bwd_ref.tap_errors(g[b], g64)
        print(f"S_tlsn {S_tlsn} row {b} (EOT {eots[b]}): loss {losses[b]:.6f} (float64 {l64:.6f}); grad vs float64 rel L2 {e:.2e} worst row {er:.2e}")
        assert abs(float(losses[b]) - l64) < 2e-6
        np.testing.assert_allclose([float(v) for v in mx[b]], mx64, rtol=2e-5)
        assert e <= F64_GRAD_GATE[0] and er <= F64_GRAD_GATE[1]
        assert not datt[b, ..., 0].any() and not datt[b, ..., eots[b]:].any()
    # rows are row-local on this path: the batched call's row b is the B = 1 call's
    for b in range(3):
        mb, kb = [v[b:b + 1].contiguous() for v in mems], {k: (v[b:b + 1].contiguous() if v is not None else None) for k, v in masks.items()}
        l1, _, g1 = weg.loss_and_grad_rows(m, x[b:b + 1].contiguous(), t, mb, kb, [focus[b]])
        same = torch.equal(g1[0], grad[b]) and float(l1[0]) == float(losses[b])
        print(f"row {b}: batched vs alone equal bits: {same}; distance {rel_l2(g1[0].cpu().numpy(), g[b]):.2e}")
        assert same
    again = weg.loss_and_grad_rows(m, x, t, mems, masks, focus)
    assert np.array_equal(again[0], losses) and torch.equal(again[2], grad)
    for mode in (True, "memories"):
        weg.loss_and_grad_rows(m, x, t, mems, masks, focus)
        reused = weg.loss_and_grad_rows(m, x, t, mems, masks, focus, same_conditioning=mode)
        assert np.array_equal(reused[0], losses) and torch.equal(reused[2], grad), mode


def test_step_refusals_name_the_row():
    import torch
    from convofusion_amd import _lib, weg
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    inp, t, eots, focus = _grad_case(12)
    mems, masks = dev_inputs(inp)
    x = to_dev(inp["sample"])
    with pytest.raises(IndexError, match="row 2"):
        weg.step_rows(m, x, t, mems, masks, [[2], [3], [6]])
    a = _lib.WegRowsArgs()
    from convofusion_amd.denoiser import Denoiser
    marr, keep = Denoiser.pack_memories(mems, masks)
    off, idx = np.array([0, 1, 2, 3], dtype=np.int32), np.array([2, 3, 6], dtype=np.int32)
    lasts = np.array(eots, dtype=np.int32)
    a.B, a.L, a.timestep, a.latents, a.mem = 3, 16, t, x.data_ptr(), marr
    a.tok_off, a.tok_idx, a.last_rows, a.kernel3 = off.ctypes.data, idx.ctypes.data, lasts.ctypes.data, (C.c_float * 3)(*weg.gaussian_kernel3())
    out = torch.zeros(3 + 3, device="cuda")
    call = lambda: _lib.load().cfd_weg_step(m.engine(x.device), C.byref(a), C.c_void_p(out.data_ptr()), C.c_void_p(out[3:].data_ptr()), None, None, None,
                                            None)
    assert call() == -1 and "row 2" in _lib.load().cfd_last_error().decode()          # CFD_E_ARG: focus index 6 outside [1, 6)
    idx[2] = 1
    lasts[1] = 2
    assert call() == -2 and "row 1" in _lib.load().cfd_last_error().decode()          # CFD_E_SHAPE: a slice shorter than 2
    lasts[1] = eots[1]
    a.tie = x.data_ptr()
    assert call() == -1 and "tie_csr" in _lib.load().cfd_last_error().decode()
    a.tie = None
    assert call() == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 3. the tie
def test_tied_step_is_the_fold_of_the_untied_gradient_bit_for_bit():
    import torch
    from convofusion_amd import weg
    from convofusion_amd.longform import window_ties
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    inp, t, eots, focus = _grad_case(12)
    mems, masks = dev_inputs(inp)
    tie = window_ties(1, 3, 16)
    x = inp["sample"]
    x_tilde = R.tie_copy(x, tie.numpy())
    _, _, g_tilde = weg.loss_and_grad_rows(m, to_dev(x_tilde), t, mems, masks, focus)
    flat = tie.reshape(-1)
    tied = torch.nonzero(flat >= 0).reshape(-1)
    for steps in ((0.7, 0.0, 1.3), (0.7, 0.0, 0.0)):
        want_g, want_x = R.fold(x_tilde, g_tilde.cpu().numpy(), tie.numpy(), steps)
        losses, _, grad, x_new = weg.step_rows(m, to_dev(x), t, mems, masks, focus, steps, tie=tie.cuda())
        assert np.array_equal(grad.cpu().numpy(), want_g) and np.array_equal(x_new.cpu().numpy(), want_x)
        new = x_new.reshape(-1, 128)
        assert torch.equal(new[tied.cuda()], new[flat[tied].long().cuda()])            # every tied token has its source's bits
        assert not grad.reshape(-1, 128)[tied.cuda()].any()
        moved = (x_new.cpu().numpy() != x_tilde)
        if steps[2] == 0.0:      # row 1 has step 0 and nothing stepped is tied into it: its free tokens keep their bits
            assert not moved[1, 8:].any() and moved[0].any() and moved[1, :8].any()
        else:                    # ... and with row 2 stepping it moves through the tokens tied into it, by exactly their folded term
            assert moved[1, 8:].any()
            np.testing.assert_array_equal(x_new.cpu().numpy()[1, 8:],
                                          x_tilde[1, 8:] - (np.float32(0.0) * g_tilde.cpu().numpy()[1, 8:] + np.float32(1.3) * g_tilde.cpu().numpy()[2, :8]))
    # in place: x_new may be the latents themselves
    xd = to_dev(x)
    weg.step_rows(m, xd, t, mems, masks, focus, (0.7, 0.0, 1.3), tie=tie.cuda(), want_grad=False, x_new=xd)
    assert np.array_equal(xd.cpu().numpy(), R.fold(x_tilde, g_tilde.cpu().numpy(), tie.numpy(), (0.7, 0.0, 1.3))[1])


# ----------------------------------------------------------------------------- 4. the loop
def _loop_device_inputs():
    from tests.gpu_helpers import to_dev
    cb, init, noise, _, _ = R.loop_inputs()
    return [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}, to_dev(init), to_dev(noise)


def test_loop_with_per_row_weg_matches_the_oracle_row_by_row():
    """Five DDPM iterations at B = 3 with one threshold iteration (tests/weg_rows_ref.py, LOOP) against ``sampler_ref.diffusion_reverse``
    with its ``pre_step`` composed per row from ``weg_ref.weg_update``; the device run's refinement rounds are the oracle's recorded
    ones; each row equals the B = 1 per-row run on that row, and at B = 1 per_row=True equals the reference's loop."""
    import torch
    from convofusion_amd import scheduler
    from convofusion_amd.distributed import shard_cfg_batch
    from convofusion_amd.sampler import sample, sample_with_weg
    from tests.gpu_helpers import SCHED_KW, hip_denoiser
    c = R.LOOP
    B, L, n = c["B"], c["L"], c["n_steps"]
    ref, plain, log = R.loop_oracle()
    g = load_golden("weg_rows_loop")
    assert [e["rounds"] for e in log] == g["rounds"].tolist() and len({tuple(r) for r in g["rounds"].tolist()}) > 1
    np.testing.assert_allclose([e["losses"] for e in log], g["losses"], atol=1e-6)
    assert len(set(g["rounds"][1].tolist())) == 3                                       # the rows need different numbers of rounds
    m = hip_denoiser(1234, 1.0)
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    mems, masks, init, noise = _loop_device_inputs()
    stats = []
    kw = dict(L=L, num_inference_steps=n, guidance_scale=7.5, carry_scale_range=True)
    lat = sample_with_weg(m, sch, mems, masks, c["focus"], c["params"], B=B, init_latents=init, step_noise=noise, per_row=True, weg_stats=stats, **kw)
    err, moved = rel_l2(lat.permute(1, 0, 2).cpu().numpy(), ref), rel_l2(plain, ref)
    print(f"per-row loop: vs oracle {err:.2e}; WEG moved the result by {moved:.2e}; rounds {[s['rounds'] for s in stats]}; "
          f"calls {[s['calls'] for s in stats]}; losses {[[round(v, 5) for v in s['losses']] for s in stats]}")
    # (past max_iter_to_alter, with no threshold iteration left, the oracle still evaluates the objective and acts on nothing; the
    #  device loop does not evaluate there)
    it = [s["i"] for s in stats]
    assert it == [0, 1, 2] and not g["rounds"][3:].any()
    assert [s["rounds"] for s in stats] == g["rounds"][it].tolist()
    np.testing.assert_allclose([s["losses"] for s in stats], g["losses"][it], atol=1e-4)
    assert moved > 10 * err and err < 1e-3
    # each row alone: the same loop at B = 1 on the row's own memories and noise
    for b in range(B):
        enc = [shard_cfg_batch(x, b, b + 1, B) for x in mems]
        mk = {k: shard_cfg_batch(v, b, b + 1, B) for k, v in masks.items()}
        one = sample_with_weg(m, sch, enc, mk, [c["focus"][b]], c["params"], B=1, init_latents=init[b:b + 1].contiguous(),
                              step_noise=noise[:, b:b + 1].contiguous(), per_row=True, **kw)
        e = rel_l2(one[0].cpu().numpy(), lat[b].cpu().numpy())
        print(f"row {b}: batched vs B = 1 per-row run {e:.2e}")
        assert e < 1e-5
        if b == 0:               # ... and at B = 1 the per-row loop is the reference's loop
            old = sample_with_weg(m, sch, enc, mk, [c["focus"][b]], c["params"], B=1, init_latents=init[b:b + 1].contiguous(),
                                  step_noise=noise[:, b:b + 1].contiguous(), **kw)
            e = rel_l2(one.cpu().numpy(), old.cpu().numpy())
            print(f"B = 1: per_row=True vs per_row=False {e:.2e}")
            assert e < 1e-5
    # no focus word anywhere: ``sample``'s bits
    none = sample_with_weg(m, sch, mems, masks, [[], [], []], c["params"], B=B, init_latents=init, step_noise=noise, per_row=True, **kw)
    base = sample(m, sch, mems, masks, B=B, L=L, num_inference_steps=n, guidance_scale=7.5, init_latents=init, step_noise=noise)
    assert torch.equal(none, base)


# ----------------------------------------------------------------------------- 5. long form
def test_longform_focus_words_on_a_tied_run():
    """1 utterance x 3 windows as one tied run with focus words in windows 0 and 2 (DDIM, 5 iterations, one threshold iteration) against
    the tied numpy loop with the restatement's lock-step ``pre_step``; the overlapping halves are equal bit for bit; without focus words
    the call returns today's bits."""
    import torch
    from convofusion_amd import scheduler
    from convofusion_amd.longform import synthesize_latents, window_ties
    from oracle import philox_ref
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    c = R.LOOP
    U, W, L, n, seed = 1, 3, 16, 5, c["seed"]
    focus = [[2, 5], [], [1, 4]]
    cb = inputs.make_cfg_batch(seed=seed, B=W, L=L, S=c["S"], pad_tail=c["pad"])
    init = philox_ref.normal_tensor(seed, 0, range(W), 1, L)
    ts = [np.split(x, 7, axis=0)[1] for x in cb["memories"]]
    tm = {k: (np.split(v, 7, axis=0)[1] if v is not None else None) for k, v in cb["masks"].items()}
    tie = window_ties(U, W, L).numpy()
    sd = state_dict(1234, 1.0)
    fwd = lambda x, t, enc, masks: denoiser_ref.denoiser_forward(sd, x, t, enc, masks)
    log = []
    ref = R.tied_reverse(fwd, scheduler_ref.DDIMSchedulerRef(), cb["memories"], cb["masks"], init, tie, num_inference_steps=n,
                         pre_step=lambda i, t, lat: R.weg_update_rows_tied(sd, lat, i, t, ts, tm, focus, c["params"], n, tie, log=log))
    plain = R.tied_reverse(fwd, scheduler_ref.DDIMSchedulerRef(), cb["memories"], cb["masks"], init, tie, num_inference_steps=n)
    target = 1.0 - c["params"]["thresholds"][1]
    margin = min(abs(v - target) for e in log if e["i"] == 1 for call in e["evaluated"] for v, f in zip(call, focus) if f)
    print("oracle rounds", [e["rounds"] for e in log], "closest compared loss to the target", margin)
    assert margin >= 1e-3 and any(r for e in log for r in e["rounds"])
    m = hip_denoiser(1234, 1.0)
    sch = scheduler.DDIMScheduler(**SCHED_KW)
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    kw = dict(n_utterances=U, n_windows=W, L=L, num_inference_steps=n, guidance_scale=7.5, seed=seed, skip_zero_weight_chunks=False)
    win, seq = synthesize_latents(m, sch, mems, masks, focus_indices=focus, weg_parameters=c["params"], **kw)
    lat = win.reshape(W, L, 128)
    err, moved = rel_l2(lat.cpu().numpy(), ref), rel_l2(plain, ref)
    print(f"long form with focus words: vs tied oracle {err:.2e}; WEG moved the result by {moved:.2e}")
    for w in range(1, W):
        assert torch.equal(win[0, w, :L // 2], win[0, w - 1, L // 2:])
    assert tuple(seq.shape) == (U, (W + 1) * L // 2, 128)
    assert moved > 10 * err and err < 1e-3
    today, _ = synthesize_latents(m, sch, mems, masks, **kw)
    for f in (None, [[], [], []]):
        same, _ = synthesize_latents(m, sch, mems, masks, focus_indices=f, weg_parameters=c["params"], **kw)
        assert torch.equal(same, today)
    assert rel_l2(today.reshape(W, L, 128).cpu().numpy(), plain) < 1e-3
