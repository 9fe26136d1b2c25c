"""CPU (-m "not gpu"): the host side of per-row word-excitation guidance -- the gate of a refinement round (``weg.row_steps``) and the
round protocol (``weg.refine_rows``) against the restatement's per-row control flow on recorded loss sequences, the restatement at
B = 1 against ``weg_ref.weg_update``, the fold of the restatement, the struct layout, and every refusal before device work."""
import ctypes as C

import numpy as np
import pytest

from tests import weg_rows_ref as R


class _RecordedRows:
    """A stand-in for the device behind ``step_call``: row b's loss after k effective steps is seq[b][k]; a call evaluates every row
    and then steps the rows whose step is not 0 -- at loss 0 the gradient is 0 and the step moves nothing."""

    def __init__(self, seqs):
        self.seqs, self.taken, self.calls = seqs, [0] * len(seqs), []

    def __call__(self, row_step):
        losses = [s[k] for s, k in zip(self.seqs, self.taken)]
        self.calls.append(list(row_step))
        self.taken = [k + int(st != 0 and l != 0) for k, st, l in zip(self.taken, row_step, losses)]
        return losses


# row 0 leaves early, row 1 runs into max_refinement_steps, row 2 sits at loss 0, row 3 has no focus token (loss 0 throughout), row 4
# never enters, row 5 enters and drops to exactly 0 inside the rounds
SEQS = [[0.90, 0.86, 0.70, 0.60, 0.50, 0.40], [0.95, 0.94, 0.93, 0.92, 0.91, 0.90, 0.89], [0.0] * 6, [0.0] * 6,
        [0.50, 0.45, 0.40, 0.30, 0.2, 0.1], [0.99, 0.0, 0.0, 0.0, 0.0, 0.0]]


@pytest.mark.parametrize("threshold,max_steps,closing", [(0.2, 3, 2.5), (0.2, 3, 0.0), (0.2, 1, 2.5), (0.05, 4, 2.5), (1.5, 3, 2.5), (0.6, 2, 0.0)])
def test_round_protocol_matches_the_reference_control_flow_per_row(threshold, max_steps, closing):
    from convofusion_amd import weg
    dev = _RecordedRows(SEQS)
    first = dev([0.0] * len(SEQS))                       # the threshold iteration's first evaluation
    losses, rounds = weg.refine_rows(dev, first, threshold, 1.25, max_steps, closing)
    for b, seq in enumerate(SEQS):
        k, r, loss, _ = R.reference_row(seq, threshold, max_steps, closing != 0)
        assert (dev.taken[b], rounds[b], losses[b]) == (k, r, loss), (b, dev.calls)
    # every call but the last carries the round step or 0; the last one the closing step for every row
    assert all(st in (0.0, 1.25) for call in dev.calls[1:-1] for st in call)
    if any(l > 1.0 - threshold for l in first) or closing:
        assert dev.calls[-1] == [closing] * len(SEQS)
    else:
        assert len(dev.calls) == 1


def test_row_steps_gate():
    from convofusion_amd import weg
    steps, active = weg.row_steps([0.9, 0.9, 0.9, 0.3, 0.0], [True, True, False, True, True], [0, 3, 0, 0, 0], 0.8, 3, 2.0)
    assert steps == [2.0, 0.0, 0.0, 0.0, 0.0] and active == [True, False, False, False, False]
    assert weg.row_steps([0.8], [True], [0], 0.8, 3, 2.0) == ([0.0], [False])        # at the target: the row leaves


def test_restated_fold_and_lists():
    from convofusion_amd.longform import window_ties
    tie = window_ties(1, 3, 4).numpy()
    assert R.tied_lists(tie) == {2: [4], 3: [5], 6: [8], 7: [9]}
    rng = np.random.Generator(np.random.PCG64(3))
    x, g = rng.standard_normal((3, 4, 128), dtype=np.float32), rng.standard_normal((3, 4, 128), dtype=np.float32)
    xt = R.tie_copy(x, tie)
    grad, new = R.fold(xt, g, tie, (0.5, 0.0, 2.0))
    assert not grad[1, :2].any() and not grad[2, :2].any()
    np.testing.assert_array_equal(grad[0, 2], g[0, 2] + g[1, 0])
    np.testing.assert_array_equal(new[0, 2], xt[0, 2] - (np.float32(0.5) * g[0, 2] + np.float32(0.0) * g[1, 0]))
    np.testing.assert_array_equal(new[1, 2], xt[1, 2] - (np.float32(0.0) * g[1, 2] + np.float32(2.0) * g[2, 0]))
    np.testing.assert_array_equal(new[1, :2], new[0, 2:])
    np.testing.assert_array_equal(new[2, 2:], xt[2, 2:] - np.float32(2.0) * g[2, 2:])
    g0, n0 = R.fold(x, g, None, (1.0, 1.0, 1.0))
    np.testing.assert_array_equal(g0, g)
    np.testing.assert_array_equal(n0, x - g)


def test_restatement_at_one_row_is_the_oracle_branch():
    """At B = 1 ``weg_rows_ref.weg_update_rows`` is ``weg_ref.weg_update`` bit for bit, carry included; the lock-step form with an
    all -1 tie table gives the same latents."""
    from oracle import weg_ref
    from tests.helpers import state_dict
    c = R.LOOP
    sd = state_dict(1234, 1.0)
    _, init, _, ts, tm = R.loop_inputs()
    st, mk = R.one_row(ts, tm, 0)
    x = init[:1]
    for i, t in ((0, 800), (1, 600)):
        ca, cb, cc = ([1.0, 0.5] for _ in range(3))
        want, loss = weg_ref.weg_update(sd, x, i, t, st, mk, [c["focus"][0]], c["params"], 5, scale_carry=ca)
        log = []
        got = R.weg_update_rows(sd, x, i, t, st, mk, [c["focus"][0]], c["params"], 5, scale_carry=cb, log=log)
        np.testing.assert_array_equal(got, want)
        assert ca == cb and log[0]["losses"] == [loss]
        tied = R.weg_update_rows_tied(sd, x, i, t, st, mk, [c["focus"][0]], c["params"], 5, np.full((1, 16), -1), scale_carry=cc)
        np.testing.assert_array_equal(tied, want)
        assert ca == cc


def test_struct_layout_matches_the_header():
    from convofusion_amd import _lib
    A = _lib.WegRowsArgs
    assert [getattr(A, f).offset for f in ("B", "L", "timestep", "latents", "mem", "tok_off", "tok_idx", "last_rows", "kernel3", "row_step", "tie",
                                           "tie_csr", "reuse_memory_side")] == [0, 4, 8, 16, 24, 184, 192, 200, 208, 224, 232, 240, 248]
    assert C.sizeof(A) == 256
    assert "cfd_weg_step" in _lib.SYMBOLS and "cfd_test_weg_focus_rows" in _lib.SYMBOLS


def _cpu_batch(B, S=(6, 20, 12, 8, 1), G=7):
    import torch
    return [torch.zeros((G * B, s, 512)) for s in S]


def test_refusals_come_before_device_work():
    """Everything here runs on CPU tensors and objects that cannot reach a device: a refusal that came late would fail differently."""
    import torch
    from convofusion_amd import weg
    from convofusion_amd.denoiser import Denoiser
    from convofusion_amd.longform import synthesize_latents
    from convofusion_amd.run_kind import check_weg_rows
    from convofusion_amd.sampler import sample_with_weg
    S = (6, 20, 12, 8, 1)
    assert weg.step_refusal(3, 16, S) is None and weg.step_refusal(43, 16, S) is None
    assert "700" in weg.step_refusal(44, 16, S) and "32" in weg.step_refusal(1, 34, S) and "1024" in weg.step_refusal(1, 16, (6, 900, 200, 8, 1))
    # tie without per_row: the message names the keyword
    tie = torch.full((3, 16), -1, dtype=torch.int32)
    with pytest.raises(ValueError, match="per_row=True"):
        check_weg_rows(False, tie, 3, 16, S)
    with pytest.raises(ValueError, match="per_row=True"):
        sample_with_weg(None, None, _cpu_batch(3), None, [[1], [], []], {}, B=3, tie=tie)
    with pytest.raises(NotImplementedError, match="700"):
        sample_with_weg(None, None, _cpu_batch(44), None, [[1]] * 44, {}, B=44, per_row=True)
    check_weg_rows(True, tie, 3, 16, S)
    check_weg_rows(False, None, 3, 16, S)
    # the call's own tables
    with pytest.raises(IndexError, match="row 1"):
        weg._row_tables(2, 12, [[1, 7], [7]], [8, 7])
    with pytest.raises(ValueError, match="row 1"):
        weg._row_tables(2, 12, [[1], []], [8, 2])
    lasts, off, flat = weg._row_tables(3, 12, [[2, 5], [], [1]], [8, 7, -6])
    assert lasts.tolist() == [8, 7, 6] and off.tolist() == [0, 2, 2, 3] and flat.tolist() == [2, 5, 1]
    m = Denoiser.__new__(Denoiser)      # (never initialised: a refusal that came late would trip over it)
    with pytest.raises(NotImplementedError, match="row-tile"):
        weg.step_rows(m, torch.zeros((44, 16, 128)), 5, [x[:44] for x in _cpu_batch(44, G=1)], {}, [[1]] * 44, eot_indices=[8] * 44)
    # long form
    params = dict(scale_factor=1, scale_range=(1.0, 0.5), max_iter_to_alter=1, thresholds={}, max_refinement_steps=1)
    kw = dict(n_utterances=1, n_windows=3, num_inference_steps=5)
    with pytest.raises(ValueError, match="cannot be combined"):
        synthesize_latents(None, None, _cpu_batch(3), None, focus_indices=[[1], [], []], weg_parameters=params,
                           keyframes=(torch.zeros(3, 16, 128), torch.ones(3, 16), 1.0, None), **kw)
    with pytest.raises(ValueError, match="cannot be combined"):
        synthesize_latents(None, None, _cpu_batch(3), None, focus_indices=[[1], [], []], weg_parameters=params,
                           pose_keyframes=(torch.zeros(3, 128, 189), torch.ones(3, 128), None, 1.0, None), vae=object(), **kw)
    with pytest.raises(ValueError, match="U \\* W = 3 lists"):
        synthesize_latents(None, None, _cpu_batch(3), None, focus_indices=[[1]], weg_parameters=params, **kw)
    with pytest.raises(ValueError, match="weg_parameters"):
        synthesize_latents(None, None, _cpu_batch(3), None, focus_indices=[[1], [], []], **kw)
    with pytest.raises(NotImplementedError, match="max_rows"):
        synthesize_latents(None, None, _cpu_batch(45), None, focus_indices=[[1]] + [[]] * 44, weg_parameters=params, n_utterances=1, n_windows=45,
                           num_inference_steps=5)
