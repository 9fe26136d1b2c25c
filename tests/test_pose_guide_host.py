"""CPU: the host half of frame-accurate key poses on the device -- the pieces of tests/pose_guide_ref.py against torch autograd (the
layout map, the pose-space loss and its cotangent), its composed float64 gradient against central differences of its own forward, the
calls ``sampler.sample_with_pose_keyframes`` makes on a stand-in run and a stand-in denoiser, ``longform.pose_keyframes_for_windows``
and ``denoiser.guide_pose_refusal``."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from convofusion_amd import denoiser as denoiser_mod, edit, longform, run_kind, sampler
from tests import pose_guide_ref as R
from tests.test_keyframes_host import TiedRun
from tests.test_sampler_loops_host import CH, RC, St, batch, ddpm, stage  # noqa: F401  (stage: the fixture)
from tests.test_vjp_host import LOSS_GUIDANCE_REFUSALS, _sched

VAE = SimpleNamespace(latent_dim=128, num_heads=2, ff_size=1024, num_layers=5, latent_size=1, body_nfeats=69, hands_nfeats=120)


# ---- the restatement's pieces against torch

def test_layout_map_is_loop_to_vae_and_its_transpose_is_vae_to_loop():
    rng = np.random.Generator(np.random.PCG64(3))
    x = rng.standard_normal((3, 6, 8))
    z = R.loop_to_vae(x)
    assert z.shape == (2, 3, 3, 8)
    assert np.array_equal(z, edit.loop_to_vae(torch.from_numpy(x)).numpy())
    assert np.array_equal(R.vae_to_loop(z), x) and np.array_equal(R.vae_to_loop(z), edit.vae_to_loop(torch.from_numpy(z)).numpy())
    for b, l in ((0, 0), (1, 3), (2, 4), (2, 5)):
        assert np.array_equal(z[l % 2, b, l // 2], x[b, l])                  # token l = 2 p + part
    # the cotangent travels back through the transpose of the map: torch autograd through edit.loop_to_vae
    a = rng.standard_normal(z.shape)
    xt = torch.from_numpy(x).requires_grad_(True)
    (g,) = torch.autograd.grad((torch.from_numpy(a) * edit.loop_to_vae(xt) ** 2).sum(), xt)
    assert np.array_equal(R.vae_to_loop(2.0 * a * z), g.numpy())


def test_loss_and_cotangent_are_pose_keyframe_loss_s_formula():
    """The formula of ``edit.pose_keyframe_loss`` on given feats (a stand-in decoder that returns them, zeroed beyond the lengths as decode
    does), with a selected frame beyond a length: it counts target^2 and its cotangent is 2 inv_n (0 - target)."""
    rng = np.random.Generator(np.random.PCG64(4))
    B, F, nf = 2, 9, 189
    lens = [9, 5]
    feats = rng.standard_normal((B, F, nf))
    feats[1, 5:] = 0
    target = rng.standard_normal((B, F, nf))
    fm = np.zeros((B, F))
    fm[0, 2] = fm[1, 4] = fm[1, 7] = 1                                       # (1, 7) lies beyond lens[1]
    cm = np.zeros(nf)
    cm[69:129] = 1
    inv_n = 1.0 / (3 * 60)
    ft = torch.from_numpy(feats).requires_grad_(True)
    stand_in = SimpleNamespace(decode=lambda z, lengths: ft)
    fn = edit.pose_keyframe_loss(stand_in, torch.from_numpy(target), torch.from_numpy(fm), torch.from_numpy(cm), lens)
    loss = fn(torch.zeros(B, 2, 128, dtype=torch.float64))
    (g,) = torch.autograd.grad(loss, ft)
    got_loss, got_d = R.loss_and_cotangent(feats, target, fm, cm, inv_n)
    assert abs(got_loss - float(loss.detach())) <= 1e-14 * abs(float(loss.detach()))
    assert np.allclose(got_d, g.numpy(), rtol=1e-14, atol=0)
    assert np.array_equal(got_d[1, 7, 69:129], 2.0 * inv_n * (0.0 - target[1, 7, 69:129])) and not got_d[0, 3].any()


def test_composed_float64_gradient_matches_central_differences():
    """B = 1, L = 2, n = 2, 16 frames.  The restatement is exact in real arithmetic and float64 central differences at h = 1e-5 carry
    about 1e-8 of rounding (eps / h relative to the loss's own size) against a truncation of h^2: relative 1e-6 is derived, not measured."""
    from oracle import inputs, vae_weights
    from tests.helpers import state_dict
    sd, vsd = state_dict(1234, 1.0), vae_weights.make_state_dict()
    inp = inputs.make_plain_batch(seed=605, Be=2, L=2, S=(6, 20, 12, 8, 1), pad_tail=(2, 0, 3, 0, 0))
    rng = np.random.Generator(np.random.PCG64(41))
    x = inp["sample"][:1].astype(np.float64)
    w = np.array([[0.0, 7.5]])
    F = 16
    target = 0.5 * rng.standard_normal((1, F, 189))
    fm = np.zeros((1, F))
    fm[0, 3] = fm[0, 11] = 1
    cm = np.ones(189)
    a = 0.9
    kw = dict(lengths=[F], target=target, frame_mask=fm, feature_mask=cm, s0=a ** 0.5, s1=(1 - a) ** 0.5, inv_n=1.0 / (2 * 189))
    ref = R.guide_pose(sd, vsd, x, 5, inp["memories"], inp["masks"], w, step=0.5, round_input=False, **kw)
    assert np.linalg.norm(ref["grad"]) > 0
    h = 1e-5
    for k in range(3):
        v = rng.standard_normal(x.shape)
        v /= np.linalg.norm(v)
        up = R.forward(sd, vsd, x + h * v, 5, inp["memories"], inp["masks"], w, **kw)
        dn = R.forward(sd, vsd, x - h * v, 5, inp["memories"], inp["masks"], w, **kw)
        fd, an = (up - dn) / (2 * h), float((ref["grad"] * v).sum())
        print(f"direction {k}: central difference {fd:.10e} analytic {an:.10e} relative {abs(fd - an) / abs(an):.2e}")
        assert abs(fd - an) <= 1e-6 * abs(an)
    assert abs(R.forward(sd, vsd, x, 5, inp["memories"], inp["masks"], w, **kw) - ref["loss"]) <= 1e-14 * ref["loss"]


# ---- the loop

@pytest.mark.parametrize("name", [k for k in LOSS_GUIDANCE_REFUSALS if k != "tied"])
def test_pose_keyframe_loop_shares_the_loss_guided_loop_s_refusals(name):
    text, kind, sched_kw, kw = LOSS_GUIDANCE_REFUSALS[name]
    with pytest.raises(NotImplementedError, match=re.escape(text)):
        sampler.sample_with_pose_keyframes(None, _sched(kind, **sched_kw), [torch.zeros(7, s, 512) for s in (3, 5, 6, 2, 1)], None, VAE,
                                           torch.zeros(1, 128, 189), torch.ones(1, 128), 0.1, B=1, L=16, num_inference_steps=5, **kw)


def test_pose_keyframe_loop_accepts_a_tie_and_validates_like_pose_keyframe_loss():
    tie = longform.window_ties(1, 3)
    run_kind.check_keyframe_guidance(_sched("ddim"), tie=tie)
    with pytest.raises(NotImplementedError, match=re.escape("a tied run (tie) takes no loss guidance")):
        run_kind.check_loss_guidance(_sched("ddim"), tie=tie)
    enc = [torch.zeros(7, s, 512) for s in (3, 5, 6, 2, 1)]
    go = lambda *a, **kw: sampler.sample_with_pose_keyframes(None, _sched("ddim"), enc, None, VAE, *a, B=1, L=16, num_inference_steps=5, **kw)
    for args, kw, text in (((torch.zeros(1, 128), torch.ones(1, 128), 0.1), {}, "target must be [B, F, nfeats]"),
                           ((torch.zeros(1, 128, 189), torch.ones(1, 64), 0.1), {}, "frame_mask must be [B, F] = [1, 128]"),
                           ((torch.zeros(1, 128, 189), torch.ones(1, 128), 0.1), dict(feature_mask=torch.ones(5)), "feature_mask must be [189]"),
                           ((torch.zeros(1, 128, 189), torch.ones(1, 128), 0.1), dict(lengths=[100]), "whose largest is 128"),
                           ((torch.zeros(1, 128, 189), torch.zeros(1, 128), 0.1), {}, "the masks select no frame or no feature"),
                           ((torch.zeros(2, 128, 189), torch.ones(2, 128), 0.1), {}, "with B = 1")):
        with pytest.raises(ValueError, match=re.escape(text)) as e:
            go(*args, **kw)
        assert "sample_with_pose_keyframes" in str(e.value)
        # ... the same check words pose_keyframe_loss's refusal (shared, not copied)
        if "B = 1" not in text:
            with pytest.raises(ValueError, match=re.escape(text)) as e:
                edit.pose_keyframe_loss(VAE, args[0], args[1], kw.get("feature_mask"), kw.get("lengths"))
            assert "pose_keyframe_loss" in str(e.value)
    with pytest.raises(NotImplementedError, match=re.escape("nframes = 136 is not in [1, 16 * (L / 2)] = [1, 128]")):
        go(torch.zeros(1, 136, 189), torch.ones(1, 136), 0.1)
    with pytest.raises(NotImplementedError, match="operands='auto'"):
        go(torch.zeros(1, 128, 189), torch.ones(1, 128), 0.1, operands="auto")


class PoseDenoiser:
    """Records every ``guide_pose`` call; the update it returns is x * 2 written into the tensor it was handed (exact)."""

    def __init__(self):
        self.return_attention = "kept"
        self.calls = []

    def guide_pose(self, x, timestep, states, masks, w, vae, target, frame_mask, **kw):
        assert torch.is_inference_mode_enabled() and not torch.is_grad_enabled()
        assert kw["x_new"] is x and kw["want"] == ("x_new",)
        self.calls.append(dict(timestep=timestep, x=x.clone(), memory_rows=[int(s.shape[0]) for s in states], w=w.clone(), vae=vae, target=target,
                               frame_mask=frame_mask.clone(), return_attention=self.return_attention,
                               **{k: v for k, v in kw.items() if k not in ("x_new", "want")}))
        x.mul_(2.0)
        return None, None, x, None, None


SEQUENCES = {None: (CH + [St(1)]) * 4 + [RC], (): [St(4), RC], (1, 3): [St(1)] + CH + [St(1), St(1)] + CH + [St(1), RC]}


@pytest.mark.parametrize("tied", (False, True))
@pytest.mark.parametrize("guided", (None, (), (1, 3)))
def test_sample_with_pose_keyframes_call_sequence(stage, monkeypatch, guided, tied):
    sch, den = ddpm(), PoseDenoiser()
    B, L, F = 2, 4, 32
    run = stage.open(TiedRun(sch.timestep_table(4)[1], 0, False, B=B))
    T = run.timesteps
    base = run.latents.clone()
    enc, masks = batch(B)
    target = torch.arange(B * F * 189, dtype=torch.float64).reshape(B, F, 189) / 7.0
    fm = torch.zeros(B, F, dtype=torch.bool)
    fm[0, 5] = fm[1, 0] = fm[1, 29] = True
    cols = torch.zeros(189, dtype=torch.bool)
    cols[69:129] = True
    tie = csr = None
    if tied:
        tie = torch.full((B, L), -1, dtype=torch.int64)
        tie[1, 0] = 2
        csr = torch.arange(2 * B * L + 1, dtype=torch.int32)
        monkeypatch.setattr(denoiser_mod, "tie_csr", lambda t: csr if torch.equal(t, tie.to(torch.int32)) else None)
    steps = [0.5, 0.25, 0.125, 0.0625]
    out = sampler.sample_with_pose_keyframes(den, sch, enc, masks, VAE, target, fm, steps, feature_mask=cols, lengths=[32, 30], B=B, L=L,
                                             num_inference_steps=4, guided_iterations=guided, tie=tie, seed=11)
    assert run.calls == SEQUENCES[guided]
    its = list(range(4)) if guided is None else list(guided)
    assert len(den.calls) == len(its) == len(run.written)
    acp = sch.alphas_cumprod.to(torch.float64)
    for n, (i, c) in enumerate(zip(its, den.calls)):
        a = float(acp[T[i]])
        assert c["timestep"] == T[i] and c["step"] == steps[i] and c["side_engine"] is True and c["return_attention"] is False
        assert c["sqrt_acp"] == a ** 0.5 and c["sqrt_1m_acp"] == (1.0 - a) ** 0.5 and c["inv_n"] == 1.0 / (3 * 60)
        assert c["reuse_memory_side"] == (2 if n else 0)                        # the memory side is kept from the second guided iteration on
        assert c["memory_rows"] == [6 * B] * 5 and c["vae"] is VAE
        assert torch.equal(c["w"], torch.tensor([[0.0, 7.5, 7.5, 7.5, 7.5, 7.5]] * B))
        assert c["target"].dtype == torch.float32 and torch.equal(c["target"], target.to(torch.float32))
        assert torch.equal(c["frame_mask"], fm.to(torch.float32)) and torch.equal(c["feature_mask"], cols.to(torch.float32))
        assert c["lengths"].tolist() == [32, 30]
        assert torch.equal(c["x"], base * 2.0 ** n) and torch.equal(run.written[n], base * 2.0 ** (n + 1))
        if tied:
            assert c["tie"].dtype == torch.int32 and torch.equal(c["tie"], tie.to(torch.int32)) and c["csr"] is csr
        else:
            assert c["tie"] is None and c["csr"] is None
    assert torch.equal(out, base * 2.0 ** len(its)) and not out.is_inference()
    assert den.return_attention == "kept"
    opened = stage.opened[0]
    assert opened["want_ring"] is False and opened["kw"]["seed"] == 11 and (opened["kw"]["tie"] is tie)


# ---- long-form

def test_pose_keyframes_for_windows_follows_stitch_frames():
    U, W, nf = 2, 3, 189
    target = torch.arange(U * 256 * nf, dtype=torch.float32).reshape(U, 256, nf)
    fm = torch.zeros(U, 256)
    frames = (0, 127, 128, 191, 192)
    fm[1, list(frames)] = 1
    cols = torch.zeros(nf)
    cols[69:129] = 1
    t_rows, m_rows = longform.pose_keyframes_for_windows(target, fm, W, feature_mask=cols)
    assert tuple(t_rows.shape) == (U * W, 128, nf) and tuple(m_rows.shape) == (U * W, 128)
    where = {0: (0, 0), 127: (0, 127), 128: (1, 64), 191: (1, 127), 192: (2, 64)}
    assert not m_rows[:W].any() and int(m_rows.sum()) == len(frames)
    for f, (w, g) in where.items():
        assert m_rows[W + w, g] == 1 and torch.equal(t_rows[W + w, g], target[1, f])
    # the map is where stitch_frames takes each frame from: stitching the rows' hand columns gives the stitched target back
    back = longform.stitch_frames(t_rows.reshape(U, W, 128, nf))
    assert torch.equal(back[:, :, 69:129], target[:, :, 69:129])
    assert torch.equal(longform.stitch_frames(m_rows.reshape(U, W, 128, 1).repeat(1, 1, 1, 4))[..., 3], fm)
    # root x / z translation: refused with W > 1 (all features included), fine with one window
    for bad in (None, torch.ones(nf), torch.eye(nf)[0], torch.eye(nf)[2]):
        with pytest.raises(ValueError, match="window's own space"):
            longform.pose_keyframes_for_windows(target, fm, W, feature_mask=bad)
    longform.pose_keyframes_for_windows(target, fm, W, feature_mask=torch.eye(nf)[1])
    longform.pose_keyframes_for_windows(target[:, :128], fm[:, :128], 1)
    with pytest.raises(ValueError, match=re.escape("[U, (W + 1) * 64, nfeats]")):
        longform.pose_keyframes_for_windows(target, fm, 2)


def test_long_form_refuses_both_kinds_of_key_poses_and_a_missing_vae():
    enc = [torch.zeros(7 * 3, s, 512) for s in (3, 5, 6, 2, 1)]
    pk = (torch.zeros(3, 128, 189), torch.ones(3, 128), None, 0.1, None)
    kf = (torch.zeros(3, 16, 128), torch.ones(3, 16), 0.1, None)
    go = lambda **kw: longform.synthesize_latents(None, _sched("ddim"), enc, n_utterances=1, n_windows=3, num_inference_steps=5, **kw)
    with pytest.raises(ValueError, match="cannot be combined"):
        go(keyframes=kf, pose_keyframes=pk, vae=VAE)
    with pytest.raises(ValueError, match="needs vae="):
        go(pose_keyframes=pk)
    with pytest.raises(ValueError, match=re.escape("target must be [U * W, 8 L, nfeats] = [3, 128, nfeats]")):
        go(pose_keyframes=(torch.zeros(3, 64, 189),) + pk[1:], vae=VAE)
    with pytest.raises(ValueError, match="pose_keyframes must be"):
        go(pose_keyframes=pk[:3], vae=VAE)


# ---- the limits

def test_guide_pose_refusal_names_each_limit():
    S = (24, 161, 24, 8, 1)
    ok = dict(latent_dim=128, num_heads=2, ff_size=1024, num_layers=5, latent_size=1)
    f = denoiser_mod.guide_pose_refusal
    assert f(6, 16, S, 1, 128, **ok) is None and f(256, 16, S, 256, 1, **ok) is None and f(2, 2, S, 1, 16, **ok) is None
    assert "Be * L = 4112 token rows exceed the guide call's 4096" in f(257, 16, S, 257, 128, **ok)       # guide_refusal's, in its words
    assert "L = 34 tokens per batch row exceed the row-tile path's 32" in f(1, 34, S, 1, 128, **ok)
    assert "1056 padded keys" in f(1, 16, (24, 897, 24, 8, 1), 1, 128, **ok)
    assert "L = 15 is odd" in f(1, 15, S, 1, 100, **ok)
    assert "nframes = 129 is not in [1, 16 * (L / 2)] = [1, 128]" in f(1, 16, S, 1, 129, **ok)
    assert "nframes = 0 is not in" in f(1, 16, S, 1, 0, **ok)
    assert "nframes = 300 exceeds the decoder backward's 256 frames" in f(1, 32, S, 1, 300, **ok)         # decode_vjp_refusal's, in its words
    assert "odd num_layers <= 9" in f(1, 16, S, 1, 128, **dict(ok, num_layers=4))
    assert "2 heads" in f(1, 16, S, 1, 128, **dict(ok, num_heads=4))
