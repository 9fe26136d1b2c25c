"""-m gpu: word-excitation guidance on the HIP path (convofusion_amd/weg.py + csrc/grad.hpp) against the oracle
(oracle/weg_ref.py) and against gradients from torch autograd through the REFERENCE (tests/golden/weg.npz).

Tolerances: the objective 2e-6 absolute; the gradient 1e-3 relative L2 (BASELINE.json north_star), observed ~1e-5."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import denoiser_ref, inputs, philox_ref, sampler_ref, scheduler_ref, weg_ref
from tests.helpers import max_abs, load_golden, rel_l2, state_dict
from tests.test_oracle_weg import CASES, weg_case

pytestmark = pytest.mark.gpu


def _ops():
    import torch
    from convofusion_amd import weg
    from convofusion_amd.conditioning import _engine_handle
    dev = torch.device("cuda", 0)
    return weg._Ops(_engine_handle(dev), dev)


def test_gemm_f32_strided_views():
    import torch
    from tests.gpu_helpers import to_dev
    ops = _ops()
    rng = np.random.Generator(np.random.PCG64(1))
    # plain, transposed operands, ragged sizes
    for M, N, K in [(16, 512, 512), (70, 33, 129), (1, 5, 7), (130, 64, 16), (16, 40, 1100), (300, 40, 50)]:   # > 256 rows: the tiled kernel
        a, b = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((N, K), dtype=np.float32)
        bias = rng.standard_normal(N, dtype=np.float32)
        ref = 0.5 * (a.astype(np.float64) @ b.astype(np.float64).T) + bias
        out = ops.new(M, N)
        ops.gemm(to_dev(a), to_dev(b).t(), out, to_dev(bias), alpha=0.5)
        assert rel_l2(out.cpu().numpy(), ref) < 1e-6
        out2 = ops.new(N, M).t()                     # transposed output view, accumulate
        out2.zero_()
        ops.gemm(to_dev(a), to_dev(b).t(), out2, None, 1.0, True)
        ops.gemm(to_dev(a), to_dev(b).t(), out2, None, 1.0, True)
        assert rel_l2(out2.cpu().numpy(), 2 * (a.astype(np.float64) @ b.astype(np.float64).T)) < 1e-6
    # two-level batch over head views of sequence-major tensors
    T, S, B, H, hd = 6, 9, 3, 4, 32
    q, k = rng.standard_normal((T, B, H * hd), dtype=np.float32), rng.standard_normal((S, B, H * hd), dtype=np.float32)
    sc = ops.new(B, H, T, S)
    ops.gemm(to_dev(q).view(T, B, H, hd).permute(1, 2, 0, 3), to_dev(k).view(S, B, H, hd).permute(1, 2, 3, 0), sc)
    ref = np.einsum("tbhd,sbhd->bhts", q.reshape(T, B, H, hd).astype(np.float64), k.reshape(S, B, H, hd).astype(np.float64))
    assert rel_l2(sc.cpu().numpy(), ref) < 1e-6


def test_row_kernels_match_oracle():
    import torch
    from convofusion_amd import weg
    from tests.gpu_helpers import to_dev
    ops = _ops()
    rng = np.random.Generator(np.random.PCG64(2))
    x = rng.standard_normal((37, 512), dtype=np.float32) * 2 + 0.3
    g = (1 + 0.1 * rng.standard_normal(512, dtype=np.float32)).astype(np.float32)
    dy = rng.standard_normal((37, 512), dtype=np.float32)
    dx = ops.new(37, 512)
    ops.layer_norm_bwd(to_dev(x), to_dev(g), to_dev(dy), dx, accumulate=False)
    assert rel_l2(dx.cpu().numpy(), weg_ref.layer_norm_bwd(x, g, dy)) < 1e-5
    ops.layer_norm_bwd(to_dev(x), to_dev(g), to_dev(dy), dx, accumulate=True)
    assert rel_l2(dx.cpu().numpy(), 2 * weg_ref.layer_norm_bwd(x, g, dy)) < 1e-5
    # softmax forward with a ragged key-padding mask, and its backward with a direct term
    B, H, T, S = 3, 2, 5, 70
    sc = rng.standard_normal((B, H, T, S), dtype=np.float32) * 3
    mask = np.zeros((B, S), dtype=bool)
    mask[1, 60:] = True
    mask[2, 1:] = True
    p = ops.softmax_(to_dev(sc), to_dev(mask.astype(np.uint8)), H * T).cpu().numpy()
    m = np.where(mask[:, None, None, :], -np.inf, sc.astype(np.float64))
    e = np.exp(m - m.max(-1, keepdims=True))
    pref = e / e.sum(-1, keepdims=True)
    assert np.abs(p - pref).max() < 1e-6 and (p[1, :, :, 60:] == 0).all()
    dp, ex = rng.standard_normal(p.shape, dtype=np.float32), rng.standard_normal(p.shape, dtype=np.float32)
    ds = ops.softmax_bwd_(to_dev(p), to_dev(dp), to_dev(ex)).cpu().numpy()
    d = (dp + ex).astype(np.float64)
    assert rel_l2(ds, pref * (d - (d * pref).sum(-1, keepdims=True))) < 1e-5
    # element-wise pieces
    a, b = rng.standard_normal((4, 3, 512), dtype=np.float32) * 2, rng.standard_normal((4, 3, 512), dtype=np.float32) * 2
    assert rel_l2(ops.ew(weg.EW_SILU, to_dev(a)).cpu().numpy(), denoiser_ref.silu(a)) < 1e-6
    assert rel_l2(ops.ew(weg.EW_GELU, to_dev(a)).cpu().numpy(), denoiser_ref.gelu(a)) < 1e-6
    assert rel_l2(ops.ew(weg.EW_SILU_BWD, to_dev(a), to_dev(b)).cpu().numpy(), a * weg_ref.silu_grad(b)) < 1e-6
    assert rel_l2(ops.ew(weg.EW_GELU_BWD, to_dev(a), to_dev(b)).cpu().numpy(), a * weg_ref.gelu_grad(b)) < 1e-6
    assert rel_l2(ops.ew(weg.EW_AXPY, to_dev(a), to_dev(b), alpha=-2.5).cpu().numpy(), a - np.float32(2.5) * b) < 1e-7
    e2 = rng.standard_normal((3, 1024), dtype=np.float32)
    assert rel_l2(ops.ew(weg.EW_MODULATE, to_dev(a), to_dev(e2), D=512, R1=3).cpu().numpy(), a * (1 + e2[None, :, :512]) + e2[None, :, 512:]) < 1e-6
    assert rel_l2(ops.ew(weg.EW_MODULATE_BWD, to_dev(a), to_dev(e2), D=512, R1=3).cpu().numpy(), a * (1 + e2[None, :, :512])) < 1e-6
    pe = rng.standard_normal((4, 512), dtype=np.float32)
    assert rel_l2(ops.ew(weg.EW_ADD_BCAST, to_dev(a), to_dev(pe), D=512, R1=3, s0=512, s1=0).cpu().numpy(), a + pe[:, None, :]) < 1e-7


@pytest.mark.parametrize("case", ["rand_b2", "rand_eot", "golden"])
def test_focus_objective_matches_oracle(case):
    import torch
    from convofusion_amd import weg
    from tests.gpu_helpers import hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    rng = np.random.Generator(np.random.PCG64(5))
    todo = []
    if case == "golden":
        g = load_golden("weg")
        for name in CASES:
            _, _, _, focus, neot, eot = weg_case(name)
            todo.append((g[name + ".att_tlsn"], focus, neot, eot))
    else:
        B, NL, L, S = (2, 9, 16, 24) if case == "rand_b2" else (1, 9, 196, 32)
        att = rng.random((B, NL, L, S)).astype(np.float32) ** 4
        att /= att.sum(-1, keepdims=True)
        if case == "rand_b2":
            todo.append((att, [[1, 2, 22], [7, 7]], False, ()))       # first / last column of the slice, a repeated token
            todo.append((att, [[], [3]], False, ()))
        else:
            todo.append((att, [[1, 5, 20]], True, np.array([22])))
    for att, focus, neot, eot in todo:
        loss, losses, mx, datt = weg_ref.focus_loss(att, focus, neot, eot)
        l2, ls2, mx2, d2 = weg.attention_focus_loss(m, to_dev(att), focus, neot, eot)
        assert abs(float(l2) - float(loss)) < 2e-6
        np.testing.assert_allclose(ls2.cpu().numpy(), losses, atol=2e-6)
        np.testing.assert_allclose([float(v) for s in mx2 for v in s], [float(v) for s in mx for v in s], rtol=1e-5)
        assert rel_l2(d2.cpu().numpy(), datt) < 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_matches_oracle_and_reference_autograd(name):
    import torch
    from convofusion_amd import weg
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    g = load_golden("weg")
    sd, inp, t, focus, neot, eot = weg_case(name)
    m = hip_denoiser(CASES[name][0], CASES[name][1])
    mems, masks = dev_inputs(inp)
    loss, losses, mx, grad = weg.loss_and_grad(m, to_dev(inp["sample"]), t, mems, masks, focus, neot, to_dev(eot))
    lo, _, _, go = weg_ref.loss_and_grad(sd, inp["sample"], t, inp["memories"], inp["masks"], focus, neot, eot)
    grad = grad.cpu().numpy()
    e_or, e_ref = rel_l2(grad, go), rel_l2(grad, g[name + ".grad"])
    print(name, f"loss {float(loss):.6f} (oracle {float(lo):.6f}, reference {float(g[name + '.loss']):.6f})  grad vs oracle {e_or:.2e}  vs reference autograd {e_ref:.2e}")
    assert abs(float(loss) - float(g[name + ".loss"])) < 2e-6
    np.testing.assert_allclose([float(v) for s in mx for v in s], g[name + ".max_att"], rtol=2e-5)
    assert e_or < 1e-3 and e_ref < 1e-3
    upd = weg.update_latent(to_dev(inp["sample"]), to_dev(grad), 1000 * np.sqrt(0.9), m).cpu().numpy()
    assert rel_l2(upd, g[name + ".updated"]) < 1e-4
    # a second evaluation at moved latents that reuses the memory-side work of the first is bit-identical to a fresh one
    lat2 = to_dev(inp["sample"] + np.float32(0.01))
    fresh = weg.loss_and_grad(m, lat2, t, mems, masks, focus, neot, to_dev(eot))
    weg.loss_and_grad(m, to_dev(inp["sample"]), t, mems, masks, focus, neot, to_dev(eot))
    reused = weg.loss_and_grad(m, lat2, t, mems, masks, focus, neot, to_dev(eot), same_conditioning=True)
    assert float(fresh[0]) == float(reused[0]) and torch.equal(fresh[3], reused[3])
    # the guided loop's case: same memories, another timestep every call -- served from tables over all timesteps (built at the
    # first such call), bit-identical to fresh evaluations; a refinement call at one of them (same_conditioning=True) stays on them
    for t2 in (t, 3, 999, t):
        fresh = weg.loss_and_grad(m, lat2, t2, mems, masks, focus, neot, to_dev(eot))
        weg.loss_and_grad(m, to_dev(inp["sample"]), t, mems, masks, focus, neot, to_dev(eot), same_conditioning="memories")
        tabled = weg.loss_and_grad(m, lat2, t2, mems, masks, focus, neot, to_dev(eot), same_conditioning="memories")
        again = weg.loss_and_grad(m, lat2, t2, mems, masks, focus, neot, to_dev(eot), same_conditioning=True)
        assert float(fresh[0]) == float(tabled[0]) == float(again[0]), t2
        assert torch.equal(fresh[3], tabled[3]) and torch.equal(fresh[3], again[3]), t2
    # the launch-by-launch form of the same evaluation
    l3, _, _, g3 = weg.loss_and_grad_stepwise(m, to_dev(inp["sample"]), t, mems, masks, focus, neot, to_dev(eot))
    # (two implementations: the float32 launch sequence in the reference's unfolded formulation against the product path's
    #  row-tile kernels -- split-pair forward in the folded formulation, float32-MFMA backward; both are held to the
    #  reference's autograd gradient above)
    assert abs(float(l3) - float(loss)) < 2e-6 and rel_l2(g3.cpu().numpy(), grad) < 1e-4
    # attention maps of the saved-activation forward against the reference's
    att, _ = weg.forward_saved(m, to_dev(inp["sample"]), t, mems, masks)
    assert np.abs(att.cpu().numpy() - g[name + ".att_tlsn"]).max() < (2e-4 if ("sharp" in name or "heavy" in name) else 1e-5)   # sharp / heavy-tailed: large logits


@pytest.mark.parametrize("rollout", [False, True])
def test_loop_with_weg_matches_oracle(rollout):
    """Five iterations of the loop with its WEG branch (one threshold step that triggers the iterative refinement)
    against the oracle loop driven by the oracle denoiser; ``rollout``: the in-painting variant, where the update
    lands between the overwrite of the first 8 tokens and the replication (unbounded_synthesis.py:70-143)."""
    import torch
    from convofusion_amd import scheduler
    from convofusion_amd.sampler import sample_with_weg
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    B, L, S, pad, n_steps, seed = 1, 16, (6, 20, 12, 8, 1), (2, 0, 3, 0, 0), 5, 11
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad)
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    noise = np.stack([philox_ref.normal_tensor(seed, i, range(B), 0, L) for i in range(n_steps)])
    preseq = (0.5 * philox_ref.normal_tensor(seed, 7, range(B), 2, 8)).astype(np.float32) if rollout else None
    focus = [[2, 5]]
    params = dict(scale_factor=1000, scale_range=[1.0, 0.5], max_iter_to_alter=3, thresholds={1: 0.16}, max_refinement_steps=2)
    sd = state_dict(1234, 1.0)
    text_states = [np.split(x, 7, axis=0)[1] for x in cb["memories"]]
    text_masks = {k: (np.split(v, 7, axis=0)[1] if v is not None else None) for k, v in cb["masks"].items()}
    log = []
    # _diffusion_reverse carries its scale_range table from iteration to iteration (convofusion.py:442-444); the rollout does not
    carry = None if rollout else list(params["scale_range"])

    def pre_step(i, t, lat):
        new, loss = weg_ref.weg_update(sd, lat, i, t, text_states, text_masks, focus, params, n_steps, scale_carry=carry)
        log.append(loss)
        return new

    ref, _, ref_atts = sampler_ref.diffusion_reverse(
        lambda x, t, enc, masks: denoiser_ref.denoiser_forward(sd, x, t, enc, masks), scheduler_ref.DDPMSchedulerRef(), cb["memories"],
        cb["masks"], init, lambda i, t: noise[i], guidance_scale=7.5, num_inference_steps=n_steps, pre_step=pre_step, preseq=preseq,
        return_att=True)
    plain, _, _ = sampler_ref.diffusion_reverse(
        lambda x, t, enc, masks: denoiser_ref.denoiser_forward(sd, x, t, enc, masks), scheduler_ref.DDPMSchedulerRef(), cb["memories"],
        cb["masks"], init, lambda i, t: noise[i], guidance_scale=7.5, num_inference_steps=n_steps, preseq=preseq)
    m = hip_denoiser(1234, 1.0)
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    lat = sample_with_weg(m, sch, mems, masks, focus, params, B=B, L=L, num_inference_steps=n_steps, guidance_scale=7.5,
                          init_latents=to_dev(init), step_noise=to_dev(noise), preseq=to_dev(preseq), carry_scale_range=not rollout)
    lat = lat.permute(1, 0, 2).cpu().numpy()
    err, moved = rel_l2(lat, ref), rel_l2(plain, ref)
    print(f"loop with WEG: vs oracle {err:.2e}; WEG moved the result by {moved:.2e}; oracle objective per step {log}")
    assert moved > 10 * err and err < 1e-3
    if not rollout:
        # the same run from the structured guidance batch (B + 1 distinct memories and row maps instead of the 7x batch)
        from convofusion_amd.sampler import build_guidance_batch
        cond = [to_dev(u[1:]) for u in cb["unique"]]
        unc = [to_dev(u[:1]) for u in cb["unique"]]
        cm = {k: (to_dev(v)[B:2 * B] if v is not None else None) for k, v in cb["masks"].items()}     # placeholder rows, replaced below
        um = {k: (to_dev(v)[:1] if v is not None else None) for k, v in cb["masks"].items()}          # chunk 0 = all dropped
        for j, name in enumerate(inputs.MEM_NAMES):                                                    # the conditional rows' own masks
            if cb["masks"][name] is not None:
                c = inputs.COND_CHUNKS[j][0]
                cm[name] = to_dev(cb["masks"][name])[c * B:(c + 1) * B]
        u_mems, maps, u_masks = build_guidance_batch(cond, unc, cm, um)
        lat2 = sample_with_weg(m, sch, u_mems, u_masks, focus, params, B=B, L=L, num_inference_steps=n_steps, guidance_scale=7.5,
                               init_latents=to_dev(init), step_noise=to_dev(noise), row_maps=maps, carry_scale_range=True)
        assert rel_l2(lat2.permute(1, 0, 2).cpu().numpy(), lat) < 1e-5
        # the reference's attention dict has one entry per iteration, WEG or not (convofusion.py:517-523): return_attention="all"
        # leaves the latents untouched bit for bit and its last entry is what return_attention=True returns
        kw = dict(B=B, L=L, num_inference_steps=n_steps, guidance_scale=7.5, init_latents=to_dev(init), step_noise=to_dev(noise),
                  carry_scale_range=True)
        lat_all, att_all = sample_with_weg(m, sch, mems, masks, focus, params, return_attention="all", **kw)
        lat_last, att_last = sample_with_weg(m, sch, mems, masks, focus, params, return_attention=True, **kw)
        lat_none = sample_with_weg(m, sch, mems, masks, focus, params, **kw)
        assert torch.equal(lat_all, lat_none) and torch.equal(lat_last, lat_none)
        assert sorted(att_all) == [0, 200, 400, 600, 800] and all(len(v) == 5 for v in att_all.values())
        assert all(torch.equal(a, b) for a, b in zip(att_all[0], att_last))
        assert all(tuple(a.shape) == (B, 9, L, s) for a, s in zip(att_all[800], S))
        # ... and every entry is the oracle's: the maps of the full-conditioning chunk of the GUIDED loop's iteration t (kept by the captured
        # iteration itself at this size: cfd_sample_args.att_ring)
        worst = max(max_abs(att_all[t][j].cpu().numpy(), ref_atts[t][j]) for t in ref_atts for j in range(5))
        print("guided loop, every iteration's maps vs the oracle: worst", worst)
        assert sorted(ref_atts) == sorted(att_all) and worst < 1e-4


def test_gradient_at_the_synthetic_shape_matches_oracle():
    """BASELINE's synthetic shape (196 latent tokens, 1500 audio tokens, extended memory PE): 13 row tiles per product on
    the token side and the tiled GEMM (> 256 rows) on the audio memory."""
    from convofusion_amd import weg
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    B, L, S, pad, t, focus = 1, 196, (32, 1500, 32, 8, 1), (8, 0, 8, 0, 0), 250, [[2, 11, 20]]
    inp = inputs.make_plain_batch(seed=91, Be=B, L=L, S=S, pad_tail=pad)
    eot = np.argmax(inp["masks"]["tlsn"].astype(np.int64), axis=1) - 1
    sd = state_dict(1234, 1.0, 1536)
    lo, _, mo, go = weg_ref.loss_and_grad(sd, inp["sample"], t, inp["memories"], inp["masks"], focus, True, eot)
    mems, masks = dev_inputs(inp)
    loss, _, mx, grad = weg.loss_and_grad(hip_denoiser(1234, 1.0), to_dev(inp["sample"]), t, mems, masks, focus, True, to_dev(eot))
    e = rel_l2(grad.cpu().numpy(), go)
    print(f"synthetic shape: loss {float(loss):.6f} (oracle {float(lo):.6f}), grad vs oracle {e:.2e}")
    assert abs(float(loss) - float(lo)) < 2e-6 and e < 1e-3
    np.testing.assert_allclose([float(v) for s in mx for v in s], [float(v) for s in mo for v in s], rtol=2e-5)


def _random_small_cases():
    """Six random shapes inside the row-tile evaluation's eligibility: batch 1 .. 3, even L <= 32 including ragged tiles, memory lengths
    with padded tails, several focus tokens.  Yields (case, B, L, S, pad, t, inputs, eot, neot, focus)."""
    rng = np.random.Generator(np.random.PCG64(77))
    for case in range(6):
        B = (1, 2, 1, 3, 1, 2)[case]
        L = int(rng.choice([4, 10, 16, 20, 32]))
        St = int(rng.integers(8, 33))
        S = (int(rng.integers(2, 33)), int(rng.integers(4, 300)), St, int(rng.integers(1, 10)), 1)
        pad = (int(rng.integers(0, 2)), int(rng.integers(0, S[1] // 2)), int(rng.integers(1, St // 2)), 0, 0)
        t = int(rng.integers(0, 1000))
        inp = inputs.make_plain_batch(seed=700 + case, Be=B, L=L, S=S, pad_tail=pad)
        eot = np.argmax(inp["masks"]["tlsn"].astype(np.int64), axis=1) - 1
        neot = B == 1     # (the end-of-text normalisation needs batch 1, like the reference: word_excitation_guidance.py:25)
        top = int(eot.min()) if neot else St - 1
        focus = [sorted(set(int(v) for v in rng.integers(1, max(2, top), size=int(rng.integers(1, 4))))) for b in range(B)]
        yield case, B, L, S, pad, t, inp, eot, neot, focus


def test_gradient_on_random_small_shapes_matches_oracle():
    """The row-tile evaluation (cfd_weg_eval's path for small problems) on random shapes inside its eligibility -- batch 1 .. 3, even
    L <= 32 including ragged tiles, memory lengths with padded tails, several focus tokens -- against the numpy oracle's backward."""
    from convofusion_amd import weg
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    sd = state_dict(1234, 1.0)
    m = hip_denoiser(1234, 1.0)
    for case, B, L, S, pad, t, inp, eot, neot, focus in _random_small_cases():
        lo, _, mo, go = weg_ref.loss_and_grad(sd, inp["sample"], t, inp["memories"], inp["masks"], focus, neot, eot)
        mems, masks = dev_inputs(inp)
        loss, _, mx, grad = weg.loss_and_grad(m, to_dev(inp["sample"]), t, mems, masks, focus, neot, to_dev(eot))
        e = rel_l2(grad.cpu().numpy(), go)
        print(f"case {case}: B={B} L={L} S={S} pad={pad} t={t} focus={focus}: loss {float(loss):.6f} (oracle {float(lo):.6f}), grad {e:.2e}")
        assert abs(float(loss) - float(lo)) < 2e-6 and e < 1e-3
        np.testing.assert_allclose([float(v) for s in mx for v in s], [float(v) for s in mo for v in s], rtol=2e-5)


# ----------------------------------------------------------------------------- shapes the product path takes other kernels for, against float64
# The end gradient against tests/weg_bwd_ref.py at float64: (relative L2 over [B][L][128], worst token row over the RMS row norm).
# 4 x the largest value measured on the MI355X over the cases below, and within the caps of the tap tests (2e-4 / 2e-3:
# tests/test_gpu_weg_backward.py); figures in profiles/r17_weg_backward_taps.txt.
F64_GRAD_GATE = (4 * 1.36e-5, 4 * 8.65e-5)      # measured: 1.36e-5 (two tokens per row), 8.65e-5 (21 x 32 rows)
assert F64_GRAD_GATE[0] <= 2e-4 and F64_GRAD_GATE[1] <= 2e-3


def _holes_case():
    """B = 3, masks with holes on all five memories (the pattern of test_key_padding_masks_with_holes): the first key, isolated keys, a
    whole 32-key block, one row without masked keys."""
    B, L, S = 3, 16, (24, 161, 24, 8, 2)
    inp = inputs.make_plain_batch(seed=909, Be=B, L=L, S=S)
    rng = np.random.Generator(np.random.PCG64(13))
    for j, name in enumerate(inputs.MEM_NAMES):
        mk = rng.random((B, S[j])) < 0.3
        mk[0, 0] = True
        if S[j] > 64:
            mk[1, 32:64] = True
        mk[2, :] = False
        mk[:, S[j] - 1] = False
        inp["masks"][name] = mk
    return inp, 321, [[1, 5, 22], [2, 9], [3, 17, 20]]


def _shape_case(name):
    """(inputs, timestep, focus, weight memory length) of a product-level case; no end-of-text normalisation (last = S_tlsn - 1)."""
    if name == "big_keys":                               # 672 padded keys: rt_xbwd_dy_kernel<RT_MAX_KEYS> (and rt_xpv_kernel<RT_MAX_KEYS>)
        return inputs.make_plain_batch(seed=31, Be=1, L=16, S=(24, 530, 24, 8, 1)), 250, [[3, 9, 22]]
    if name == "large_focus":                            # 32 x 38 cells > 1024: weg_focus_kernel with the workspace inside the row-tile arena
        return inputs.make_plain_batch(seed=32, Be=1, L=32, S=(6, 20, 40, 8, 1), pad_tail=(2, 3, 0, 0, 0)), 700, [[1, 17, 30, 38]]
    if name == "tiles_b21":                              # 672 rows, 42 tiles
        return inputs.make_plain_batch(seed=33, Be=21, L=32, S=(3, 5, 6, 2, 1)), 450, [[1 + (b + k) % 4 for k in range(1 + b % 3)] for b in range(21)]
    if name == "tiles_b43":                              # 688 rows, 43 tiles
        return inputs.make_plain_batch(seed=34, Be=43, L=16, S=(3, 5, 6, 2, 1), pad_tail=(0, 1, 0, 0, 0)), 80, [[1 + b % 4, 4 - b % 3] for b in range(43)]
    if name == "len2":                                   # the lower length edge
        return inputs.make_plain_batch(seed=35, Be=2, L=2, S=(6, 20, 12, 8, 1), pad_tail=(2, 0, 0, 0, 0)), 5, [[2, 10], [1]]
    assert name == "holes"
    return _holes_case()


_f64 = {}


def _float64_result(key, inp, t, focus, neot=False, eot=()):
    from tests import weg_bwd_ref
    if key not in _f64:
        _f64[key] = weg_bwd_ref.loss_and_grad_taps(state_dict(1234, 1.0), inp["sample"], t, inp["memories"], inp["masks"], focus, neot, eot)
    return _f64[key]


def _knob_model(knob):
    """A model with the weights of hip_denoiser(1234, 1.0) whose handle was created under ``knob``=0 (the developer knobs are read when the
    handle is created); one per knob for the session."""
    import os
    import torch
    from convofusion_amd.denoiser import Denoiser
    from tests.gpu_helpers import ABL, DENOISER_KW, hip_denoiser
    if knob not in _knob_model.__dict__:
        os.environ[knob] = "0"
        try:
            m = Denoiser(ablation=ABL, **DENOISER_KW)
            m.load_state_dict(hip_denoiser(1234, 1.0).state_dict(), strict=True)
            m = m.cuda().eval()
            m.engine(torch.device("cuda"))
        finally:
            del os.environ[knob]
        _knob_model.__dict__[knob] = m
    return _knob_model.__dict__[knob]


def _f32_sequence_model():
    """A model whose handle evaluates on the float32 launch sequence (weg_eval.hpp) whatever the shape."""
    return _knob_model("CFD_WEG_ROWTILE")


def _eager_model():
    """A model whose handle never captures or replays an evaluation (CFD_WEG_GRAPH=0)."""
    return _knob_model("CFD_WEG_GRAPH")


def _check_against_float64(label, m, inp, t, focus, r64, neot=False, eot=None, row_tile=True, same_conditioning=False, dev=None, raw=None):
    """One product evaluation against the float64 restatement: losses 2e-6, max_att 2e-5, the gradient at F64_GRAD_GATE in both measures;
    the text attention exactly 0 in masked columns, the objective's gradient at the maps exactly 0 outside the text slice.
    ``dev``: the memories and masks already on the device (the library reuses memory-side work only for unchanged pointers);
    ``raw``: a list that receives what ``weg.loss_and_grad`` returned."""
    import torch
    from convofusion_amd import weg
    from tests import weg_bwd_ref
    from tests.gpu_helpers import dev_inputs, read_debug, to_dev
    mems, masks = dev if dev is not None else dev_inputs(inp)
    eot_dev = to_dev(np.asarray(eot)) if eot is not None else torch.zeros(1, dtype=torch.long)
    loss, losses, mx, grad = weg.loss_and_grad(m, to_dev(inp["sample"]), t, mems, masks, focus, neot, eot_dev, same_conditioning=same_conditioning)
    if raw is not None:
        raw.append((loss, losses, mx, grad))
    l64, ls64, mx64, g64, _, att64, datt64 = r64
    B, L, _ = inp["sample"].shape
    St = inp["memories"][2].shape[1]
    g = grad.cpu().numpy()
    e, er = weg_bwd_ref.tap_errors(g.reshape(B * L, -1), g64.reshape(B * L, -1))
    info = read_debug(m, "weg.info", (5,))
    print(f"{label}: B={B} L={L} loss {float(loss):.6f} (float64 {float(l64):.6f}); grad vs float64 rel L2 {e:.2e} worst row {er:.2e}; "
          f"row-tile launches {int(info[0])}, Sp_tot {int(info[1])}, rt_xbwd_dy_kernel<{int(info[2])}>, objective kernel {'large' if info[3] else 'small'}")
    assert abs(float(loss) - float(l64)) < 2e-6
    np.testing.assert_allclose(losses.cpu().numpy(), ls64, atol=2e-6)
    np.testing.assert_allclose([float(v) for s in mx for v in s], [float(v) for s in mx64 for v in s], rtol=2e-5)
    assert e <= F64_GRAD_GATE[0] and er <= F64_GRAD_GATE[1]
    last = int(eot[0]) if neot else St - 1
    mk = inp["masks"]["tlsn"]
    if row_tile:
        assert int(info[1]) == sum((int(x.shape[1]) + 31) // 32 * 32 for x in inp["memories"])
        att, datt = read_debug(m, "weg.att", (B, 9, L, St)), read_debug(m, "weg.d_att", (B, 9, L, St))
    else:      # the launch-by-launch form of the float32 sequence: the same kernels, its maps and their gradient in the caller's hands
        a, _ = weg.forward_saved(m, to_dev(inp["sample"]), t, mems, masks)
        _, _, _, d = weg.attention_focus_loss(m, a, focus, neot, eot_dev)
        att, datt = a.cpu().numpy(), d.cpu().numpy()
    if mk is not None:
        assert np.all(att[np.broadcast_to(mk[:, None, None, :], att.shape)] == 0)
    assert np.abs(att - att64).max() < 1e-5
    assert not datt[..., 0].any() and not datt[..., last:].any()     # (inside the slice the reference's own gradient at a masked column is not 0)
    assert rel_l2(datt, datt64) < 1e-4
    return g, info


@pytest.mark.parametrize("name", ["big_keys", "large_focus", "tiles_b21", "tiles_b43", "len2", "holes"])
def test_gradient_at_row_tile_shape_edges_matches_float64(name):
    """Shapes at which the row-tile evaluation takes a kernel instance or a grid no other WEG case reaches, end to end against float64:
    more than 512 padded keys, the large objective kernel, 42 and 43 token tiles, two tokens per row, key-padding masks with holes."""
    from tests.gpu_helpers import hip_denoiser
    inp, t, focus = _shape_case(name)
    _, info = _check_against_float64(name, hip_denoiser(1234, 1.0), inp, t, focus, _float64_result(name, inp, t, focus))
    assert int(info[2]) == (1024 if name == "big_keys" else 512)
    assert int(info[3]) == (1 if name == "large_focus" else 0)


def test_float32_launch_sequence_with_batches_matches_float64_and_the_row_tile_path():
    """The float32 launch sequence (weg_eval.hpp: every evaluation outside the row-tile path's eligibility) with more than one batch row
    -- the random shapes with B = 2 and 3 and the masks with holes, on a handle created with CFD_WEG_ROWTILE=0 -- against float64 and
    against the row-tile path's gradient for the same inputs."""
    from tests import weg_bwd_ref
    from tests.gpu_helpers import hip_denoiser
    m32, mrt = _f32_sequence_model(), hip_denoiser(1234, 1.0)
    todo = [(f"random{case}", inp, t, focus, neot, eot) for case, B, L, S, pad, t, inp, eot, neot, focus in _random_small_cases() if B > 1]
    todo.append(("holes",) + _shape_case("holes") + (False, None))
    for label, inp, t, focus, neot, eot in todo:
        r64 = _float64_result(label, inp, t, focus, neot, eot if eot is not None else ())
        g_rt, info = _check_against_float64(label + " row-tile", mrt, inp, t, focus, r64, neot, eot)
        assert info[0] > 0
        g_32, info = _check_against_float64(label + " float32 sequence", m32, inp, t, focus, r64, neot, eot, row_tile=False)
        assert info[0] == 0 and info[1] == 0          # no row-tile evaluation ever ran on this handle
        B, L, _ = inp["sample"].shape
        e, er = weg_bwd_ref.tap_errors(g_32.reshape(B * L, -1), g_rt.reshape(B * L, -1))
        print(f"{label}: float32 sequence vs row-tile rel L2 {e:.2e} worst row {er:.2e}")
        assert e <= F64_GRAD_GATE[0] and er <= F64_GRAD_GATE[1]


def test_eval_rejects_what_the_reference_cannot_run():
    import torch
    from convofusion_amd import _lib, weg
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    enc = [torch.zeros(1, s, 512, device="cuda") for s in (4, 6, 12, 8, 1)]
    mask = {"tlsn": (torch.arange(12) >= 9)[None].cuda()}
    lat = torch.zeros(1, 16, 128, device="cuda")
    with pytest.raises(_lib.CfdError):       # text slice [1, 2): F.pad(mode='reflect') needs two entries (weg.py:35)
        weg.loss_and_grad(m, lat, 5, enc, mask, [[1]], True, torch.tensor([2]))
    with pytest.raises(_lib.CfdError):       # odd latent length: the reference's SineBH position encoding cannot broadcast
        weg.loss_and_grad(m, torch.zeros(1, 15, 128, device="cuda"), 5, enc, mask, [[2]], True, torch.tensor([8]))
    with pytest.raises(_lib.CfdError):       # timestep outside the 1000-row table
        weg.loss_and_grad(m, lat, 1000, enc, mask, [[2]], True, torch.tensor([8]))
    with pytest.raises(ValueError):          # the conditioning tuple must be the text-only chunk (one row per latent row)
        weg.loss_and_grad(m, lat, 5, [e.expand(7, -1, -1) for e in enc], mask, [[2]], True, torch.tensor([8]))


def test_graph_replayed_evaluation_interleaved_with_the_sampling_graph_equals_eager():
    """cfd_weg_eval replays its launch sequence as a hipGraph from its second use on.  Round 1 found such replays "wrong when
    interleaved with the sampling graph": the captured kernels held the CALLER's latents / losses / grad pointers by value, and
    the Python side passes fresh tensors on every call.  With the inputs and outputs staged through fixed buffers the replayed
    evaluation must equal the eager one (CFD_WEG_GRAPH=0) bit for bit -- here with a new latents tensor (new address) per
    call, both graph variants (full / memory side reused), and replays of the sampling graph in between."""
    import torch
    from convofusion_amd import weg
    from convofusion_amd.sampler import SamplingRun, sample_with_weg
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    B, L, S, pad = 1, 16, (6, 20, 12, 8, 1), (2, 0, 3, 0, 0)
    cb = inputs.make_cfg_batch(seed=23, B=B, L=L, S=S, pad_tail=pad)
    mems = [to_dev(x) for x in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    text_states = [e.chunk(7)[1].contiguous() for e in mems]
    text_masks = {k: (v.chunk(7)[1].to(torch.uint8).contiguous() if v is not None else None) for k, v in masks.items()}
    eot = torch.argmax(text_masks["tlsn"].int(), dim=1) - 1
    focus = [[2, 5]]
    m_graph, m_eager = hip_denoiser(1234, 1.0), _eager_model()          # (the knob is read when the handle is created)
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    run = SamplingRun(m_graph, sch, mems, masks, B, L, 20, guidance_scale=7.5, seed=3)
    g = torch.Generator(device="cuda").manual_seed(5)
    keep = []
    for it in range(8):
        lat = torch.randn((B, L, 128), device="cuda", generator=g)     # a fresh tensor (fresh address) every call
        keep.append(torch.empty(1000 + 37 * it, device="cuda"))        # ... and shift the allocator's next address
        t, same = (500, it % 4 != 0) if it < 6 else (499, False)       # full, reused x3, full, reused, then another timestep
        a = weg.loss_and_grad(m_graph, lat, t, text_states, text_masks, focus, True, eot, same_conditioning=same)
        b = weg.loss_and_grad(m_eager, lat, t, text_states, text_masks, focus, True, eot, same_conditioning=same)
        assert float(a[0]) == float(b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3]), it
        assert torch.isfinite(a[3]).all() and float(a[3].abs().max()) > 0
        run.steps(1)                                                    # a replay of the sampling graph on the same stream
    run.close()
    # end to end: the guided loop (threshold step with refinement) through both
    params = dict(scale_factor=1000, scale_range=[1.0, 0.5], max_iter_to_alter=3, thresholds={1: 0.16}, max_refinement_steps=3)
    init = to_dev(philox_ref.normal_tensor(23, 0, range(B), 1, L))
    la = sample_with_weg(m_graph, sch, mems, masks, focus, params, B=B, L=L, num_inference_steps=5, guidance_scale=7.5, init_latents=init, seed=2)
    lb = sample_with_weg(m_eager, sch, mems, masks, focus, params, B=B, L=L, num_inference_steps=5, guidance_scale=7.5, init_latents=init, seed=2)
    assert torch.equal(la, lb)


# The state machine of cfd_weg_eval on one handle: (inputs, timestep, focus, same_conditioning) per call, in order.
#   1-2  "memories" at 500, 499: tables over all timesteps, the second call reuses the memory side at a new timestep
#   3    True at 499: the tables stay full because the handle had them
#   4    False at 500: back to one-row tables
#   5-7  True at 500: eager, the second use of that key captured, then replayed
#   8    another focus list with True: a new token-table version and graph key, the memory side still reused
#   9    L = 32 inputs with False: the arena and the problem are rebuilt
#   10   back to the L = 16 inputs with False
STATE_WALK_FOCUS = {"f1": [[2, 5]], "f2": [[3, 6, 7]]}
STATE_WALK = [("L16", 500, "f1", "memories"), ("L16", 499, "f1", "memories"), ("L16", 499, "f1", True), ("L16", 500, "f1", False),
              ("L16", 500, "f1", True), ("L16", 500, "f1", True), ("L16", 500, "f1", True), ("L16", 500, "f2", True),
              ("L32", 500, "f1", False), ("L16", 500, "f1", False)]


def state_walk_inputs():
    """{name: (inputs, device memories, device masks as uint8, eot)} of the walk: B = 1, S = (6, 20, 12, 8, 1) with pad tails
    (2, 0, 3, 0, 0) -- the graph test's shape -- at L = 16 and L = 32.  The device tensors are made once: their addresses are part of
    what the library compares."""
    import torch
    from tests.gpu_helpers import dev_inputs
    out = {}
    for name, L in (("L16", 16), ("L32", 32)):
        inp = inputs.make_plain_batch(seed=23 + L, Be=1, L=L, S=(6, 20, 12, 8, 1), pad_tail=(2, 0, 3, 0, 0))
        mems, masks = dev_inputs(inp)
        masks = {k: (v.to(torch.uint8).contiguous() if v is not None else None) for k, v in masks.items()}
        out[name] = (inp, mems, masks, np.argmax(inp["masks"]["tlsn"].astype(np.int64), axis=1) - 1)
    return out


def test_state_machine_walk_matches_float64_and_the_eager_handle():
    """One handle through cfd_weg_eval's state machine (STATE_WALK): every reuse mode, one-row and full tables, capture and replay of
    an evaluation, a new focus-token table, a shape change and back.  Every call on a freshly allocated latents tensor, against
    float64 at the gates of _check_against_float64 and bit for bit against the same call on a handle that never captures
    (CFD_WEG_GRAPH=0); then the same walk on the float32 launch sequence (CFD_WEG_ROWTILE=0) against float64."""
    import torch
    from tests.gpu_helpers import hip_denoiser
    data = state_walk_inputs()
    m_graph, m_eager, m_f32 = hip_denoiser(1234, 1.0), _eager_model(), _f32_sequence_model()
    for m, row_tile in ((m_graph, True), (m_f32, False)):
        for n, (name, t, fk, same) in enumerate(STATE_WALK, 1):
            inp, mems, masks, eot = data[name]
            focus = STATE_WALK_FOCUS[fk]
            r64 = _float64_result(("walk", name, t, fk), inp, t, focus, True, eot)
            kw = dict(neot=True, eot=eot, same_conditioning=same, dev=(mems, masks))
            a = []
            _check_against_float64(f"walk {n} {'row-tile' if row_tile else 'float32 sequence'} {name} t={t} {fk} same={same}", m, inp, t,
                                   focus, r64, row_tile=row_tile, raw=a, **kw)
            if row_tile:
                b = []
                _check_against_float64(f"walk {n} eager", m_eager, inp, t, focus, r64, raw=b, **kw)
                (la, lsa, mxa, ga), (lb, lsb, mxb, gb) = a[0], b[0]
                assert float(la) == float(lb) and torch.equal(lsa, lsb) and torch.equal(ga, gb), n
                assert all(torch.equal(x, y) for ra, rb in zip(mxa, mxb) for x, y in zip(ra, rb)), n
