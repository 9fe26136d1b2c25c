"""CPU: the host half of key-pose guidance on the device -- ``run_kind.check_keyframe_guidance`` next to ``check_loss_guidance``, the calls
``sampler.sample_with_keyframes`` makes on a stand-in run and a stand-in denoiser (in the manner of tests/test_sampler_loops_host.py),
``denoiser.guide_refusal`` at its row limit, and the tie fold of tests/guide_ref.py against torch autograd through an index gather."""
import re

import numpy as np
import pytest
import torch

from convofusion_amd import denoiser as denoiser_mod, longform, run_kind, sampler
from tests import guide_ref
from tests.test_sampler_loops_host import CH, FakeRun, RC, St, batch, ddpm, stage  # noqa: F401  (stage: the fixture)
from tests.test_vjp_host import LOSS_GUIDANCE_REFUSALS, _sched


# ---- the run kinds

@pytest.mark.parametrize("name", [k for k in LOSS_GUIDANCE_REFUSALS if k != "tied"])
def test_keyframe_loop_shares_the_loss_guided_loop_s_refusals(name):
    text, kind, sched_kw, kw = LOSS_GUIDANCE_REFUSALS[name]
    sch = _sched(kind, **sched_kw)
    with pytest.raises(NotImplementedError, match=re.escape(text)) as e:
        run_kind.check_keyframe_guidance(sch, **kw)
    assert "sample_with_keyframes" in str(e.value)
    # the loop itself: no denoiser, CPU memories -- the refusal comes first
    with pytest.raises(NotImplementedError, match=re.escape(text)):
        sampler.sample_with_keyframes(None, sch, [torch.zeros(7, s, 512) for s in (3, 5, 6, 2, 1)], None, torch.zeros(1, 16, 128),
                                      torch.ones(1, 16), 0.1, B=1, L=16, num_inference_steps=5, **kw)


def test_keyframe_loop_accepts_a_tie_and_the_loss_guided_loop_still_refuses_it():
    tie = longform.window_ties(1, 3)
    for kind in ("ddpm", "ddim"):
        run_kind.check_keyframe_guidance(_sched(kind), tie=tie)
        run_kind.check_keyframe_guidance(_sched(kind))
        with pytest.raises(NotImplementedError, match=re.escape("a tied run (tie) takes no loss guidance")) as e:
            run_kind.check_loss_guidance(_sched(kind), tie=tie)
        assert "sample_with_keyframes" in str(e.value)      # ... and says where key poses on a tied run go


def test_guide_refusal_has_a_row_limit_of_its_own():
    S = (24, 161, 24, 8, 1)
    assert denoiser_mod.guide_refusal(256, 16, S) is None                       # 4096 token rows
    assert denoiser_mod.guide_refusal(6 * 8, 16, S) is None                     # 768: the differentiable forward refuses these
    assert "768 token rows exceed the row-tile path's 700" in denoiser_mod.vjp_refusal(6 * 8, 16, S, max_rows=700)
    assert "Be * L = 4112 token rows exceed the guide call's 4096" in denoiser_mod.guide_refusal(257, 16, S)
    assert "L = 34 tokens per batch row exceed the row-tile path's 32" in denoiser_mod.guide_refusal(1, 34, S)
    assert "1056 padded keys" in denoiser_mod.guide_refusal(1, 16, (24, 897, 24, 8, 1))
    assert denoiser_mod.guide_refusal(10, 16, S, max_rows=100) is not None
    # the loop checks its shape before any device work: 6 evaluated chunks x 43 utterances x 16 tokens = 4128 rows
    enc = [torch.zeros(7 * 43, s, 512) for s in (3, 5, 6, 2, 1)]
    with pytest.raises(NotImplementedError, match=re.escape("the 6 evaluated guidance chunks: Be * L = 4128 token rows exceed the guide call's 4096")):
        sampler.sample_with_keyframes(None, _sched("ddim"), enc, None, torch.zeros(43, 16, 128), torch.ones(43, 16), 0.1, B=43, L=16,
                                      num_inference_steps=5)
    with pytest.raises(NotImplementedError, match="operands='auto'"):
        sampler.sample_with_keyframes(None, _sched("ddim"), enc, None, torch.zeros(43, 16, 128), torch.ones(43, 16), 0.1, B=43, L=16,
                                      num_inference_steps=5, operands="auto")
    with pytest.raises(ValueError, match="mask keeps no token"):
        sampler.sample_with_keyframes(None, _sched("ddim"), enc, None, torch.zeros(43, 16, 128), torch.zeros(43, 16), 0.1, B=43, L=16,
                                      num_inference_steps=5)


# ---- the calls of the loop

class TiedRun(FakeRun):
    """A stand-in run whose ``write`` takes the statement that the latents satisfy the tie, as ``SamplingRun.write`` does."""

    def write(self, latents, satisfies_tie=False):
        assert satisfies_tie
        assert torch.is_inference_mode_enabled()
        super().write(latents)


class GuideDenoiser:
    """Records every ``guide`` call; the update it returns is x * 2 written into the tensor it was handed (exact)."""

    def __init__(self):
        self.return_attention = "kept"
        self.calls = []

    def guide(self, x, timestep, states, masks, w, target, mask, **kw):
        assert torch.is_inference_mode_enabled() and not torch.is_grad_enabled()
        assert kw["x_new"] is x and kw["want"] == ("x_new",)
        self.calls.append(dict(timestep=timestep, x=x.clone(), memory_rows=[int(s.shape[0]) for s in states], w=w.clone(), target=target, mask=mask.clone(),
                               return_attention=self.return_attention, **{k: v for k, v in kw.items() if k not in ("x_new", "want")}))
        x.mul_(2.0)
        return None, None, x, None


KEYFRAME_SEQUENCES = {
    None: (CH + [St(1)]) * 4 + [RC],
    (): [St(4), RC],
    (1, 3): [St(1)] + CH + [St(1), St(1)] + CH + [St(1), RC],
}


@pytest.mark.parametrize("tied", (False, True))
@pytest.mark.parametrize("guided", (None, (), (1, 3)))
def test_sample_with_keyframes_call_sequence(stage, monkeypatch, guided, tied):
    sch, den = ddpm(), GuideDenoiser()
    B, L = 2, 4
    run = stage.open(TiedRun(sch.timestep_table(4)[1], 0, False, B=B))
    T = run.timesteps
    base = run.latents.clone()
    enc, masks = batch(B)
    target = torch.arange(B * L * 128, dtype=torch.float64).reshape(B, L, 128) / 7.0
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[0, 1] = mask[1, 0] = mask[1, 3] = True
    tie = csr = None
    if tied:
        tie = torch.full((B, L), -1, dtype=torch.int64)
        tie[1, 0] = 2
        csr = torch.arange(2 * B * L + 1, dtype=torch.int32)
        monkeypatch.setattr(denoiser_mod, "tie_csr", lambda t: csr if torch.equal(t, tie.to(torch.int32)) else None)
    steps = [0.5, 0.25, 0.125, 0.0625]
    out = sampler.sample_with_keyframes(den, sch, enc, masks, target, mask, steps, B=B, L=L, num_inference_steps=4, guided_iterations=guided,
                                        tie=tie, seed=11)
    assert run.calls == KEYFRAME_SEQUENCES[guided]
    its = list(range(4)) if guided is None else list(guided)
    assert len(den.calls) == len(its) == len(run.written)
    acp = sch.alphas_cumprod.to(torch.float64)
    for n, (i, c) in enumerate(zip(its, den.calls)):
        a = float(acp[T[i]])
        assert c["timestep"] == T[i] and c["step"] == steps[i] and c["side_engine"] is True and c["return_attention"] is False
        assert c["sqrt_acp"] == a ** 0.5 and c["sqrt_1m_acp"] == (1.0 - a) ** 0.5 and c["inv_n"] == 1.0 / (3 * 128)
        assert c["reuse_memory_side"] == (2 if n else 0)                        # the memory side is kept from the second guided iteration on
        assert c["memory_rows"] == [6 * B] * 5                                  # the six chunks of non-zero weight
        assert torch.equal(c["w"], torch.tensor([[0.0, 7.5, 7.5, 7.5, 7.5, 7.5]] * B))
        assert c["target"].dtype == torch.float32 and torch.equal(c["target"], target.to(torch.float32))
        assert torch.equal(c["mask"], mask.to(torch.float32))
        assert torch.equal(c["x"], base * 2.0 ** n) and torch.equal(run.written[n], base * 2.0 ** (n + 1))
        if tied:
            assert c["tie"].dtype == torch.int32 and torch.equal(c["tie"], tie.to(torch.int32)) and c["csr"] is csr
        else:
            assert c["tie"] is None and c["csr"] is None
    assert torch.equal(out, base * 2.0 ** len(its)) and not out.is_inference()
    assert den.return_attention == "kept"
    opened = stage.opened[0]
    assert opened["want_ring"] is False and opened["kw"]["seed"] == 11 and (opened["kw"]["tie"] is tie)


def test_sample_with_keyframes_takes_the_weight_table_s_columns(stage):
    sch, den = ddpm(), GuideDenoiser()
    B, L = 2, 4
    stage.open(TiedRun(sch.timestep_table(4)[1], 0, False, B=B))
    enc, masks = batch(B)
    mw = np.zeros((4, B, 6))
    mw[:, :, 1] = [[1.0, 2.0]] * 4          # audio
    mw[2, :, 4] = 0.5                       # lsnid in iteration 2 only
    sampler.sample_with_keyframes(den, sch, enc, masks, torch.zeros(B, L, 128), torch.ones(B, L), 0.1, B=B, L=L, num_inference_steps=4,
                                  guidance_scale=2.0, modality_weights=mw)
    assert [c["memory_rows"] for c in den.calls] == [[3 * B] * 5] * 4           # chunks 0, 2 (audio) and 5 (lsnid)
    assert torch.equal(den.calls[0]["w"], torch.tensor([[0.0, 2.0, 0.0], [0.0, 4.0, 0.0]]))
    assert torch.equal(den.calls[2]["w"], torch.tensor([[0.0, 2.0, 1.0], [0.0, 4.0, 1.0]]))


def test_exception_in_guide_closes_the_run_and_restores_return_attention(stage):
    sch, den = ddpm(), GuideDenoiser()
    run = stage.open(TiedRun(sch.timestep_table(4)[1], B=2))

    def guide(*a, **kw):
        raise RuntimeError("guide")
    den.guide = guide
    with pytest.raises(RuntimeError, match="guide"):
        sampler.sample_with_keyframes(den, sch, *batch(2), torch.zeros(2, 4, 128), torch.ones(2, 4), 0.1, B=2, L=4, num_inference_steps=4,
                                      guided_iterations=(2,))
    assert run.calls[-1] == ("close",) and not run.open and den.return_attention == "kept"


# ---- the reference's tie fold against autograd

@pytest.mark.parametrize("table", ("windows", "shared"))
def test_guide_ref_fold_is_the_gradient_through_an_index_gather(table):
    B, L, C = 3, 16, 8
    if table == "windows":
        tie = longform.window_ties(1, B, L).numpy()
    else:
        tie = np.full((B, L), -1, dtype=np.int32)
        tie[1, 0] = tie[2, 5] = 9
        tie[2, 0] = L + 3
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.standard_normal((B, L, C))
    a = rng.standard_normal((B, L, C))
    idx = np.where(tie.reshape(-1) >= 0, tie.reshape(-1), np.arange(B * L))
    xt = torch.from_numpy(x).requires_grad_(True)
    gathered = xt.reshape(B * L, C)[torch.from_numpy(idx)].reshape(B, L, C)
    assert np.array_equal(gathered.detach().numpy(), guide_ref.gather_tie(x, tie))
    f = (torch.from_numpy(a) * gathered ** 3).sum()                # any function of x~
    (g,) = torch.autograd.grad(f, xt)
    g_tilde = 3.0 * a * guide_ref.gather_tie(x, tie) ** 2          # its gradient at x~
    got = guide_ref.fold(g_tilde, tie)
    # (float64 on both sides; the two write 3 a x^2 in another order and a source sums up to three such terms: a few 1e-16 of O(10) values)
    assert np.allclose(got, g.numpy(), rtol=1e-12, atol=1e-12) and not got.reshape(-1, C)[tie.reshape(-1) >= 0].any()
    # the update: free tokens move by the folded gradient, tied tokens take their source's new value
    new = guide_ref.update(guide_ref.gather_tie(x, tie), got, tie, 0.25)
    flat = new.reshape(-1, C)
    assert np.array_equal(flat[tie.reshape(-1) >= 0], flat[tie.reshape(-1)[tie.reshape(-1) >= 0]])
    assert np.array_equal(flat[tie.reshape(-1) < 0], (x - 0.25 * got).reshape(-1, C)[tie.reshape(-1) < 0])
    assert guide_ref.fold(g_tilde, None) is g_tilde and guide_ref.gather_tie(x, None) is x
