"""-m gpu: Denoiser.forward parity -- HIP path vs the golden outputs of the REFERENCE and vs the oracle.

Tolerance: north_star asks for 1e-3 relative on the final latents; one forward is held to 1e-4
relative L2 (split-bf16x3 products carry ~2^-16 operand error) and attention probabilities to 1e-4 abs.
"""
import numpy as np
import pytest

from oracle import inputs
from tests.helpers import forward_case, max_abs, rel_l2, state_dict

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-4


def _run(name):
    import torch
    from tests.gpu_helpers import dev_inputs, hip_denoiser
    sd, inp, t, g = forward_case(name)
    wseed, sharp = (1234, 1.0) if name in ("tiny", "real", "synth") else (4321, 4.0)
    m = hip_denoiser(wseed, sharp)
    mems, masks = dev_inputs(inp)
    with torch.no_grad():
        out, att = m(torch.from_numpy(inp["sample"]).cuda(), torch.tensor(t), mems, mem_mask_dict=masks)
    torch.cuda.synchronize()
    return sd, inp, t, g, out.cpu().numpy(), [a.cpu().numpy() for a in att], m


def test_stagewise_taps_tiny():
    """Localises a failure: compare the residual stream after every sub-block with the oracle's taps."""
    import torch
    from convofusion_amd import _lib
    from oracle import denoiser_ref
    from tests.gpu_helpers import dev_inputs, hip_denoiser, read_debug
    sd, inp, t, g = forward_case("tiny")
    taps = {}
    denoiser_ref.denoiser_forward(sd, inp["sample"], t, inp["memories"], inp["masks"], taps=taps)
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    x = torch.from_numpy(inp["sample"]).cuda()
    Be, L = inp["sample"].shape[:2]
    lib = _lib.load()
    report = []
    stages = [(1, "x0")]
    for l in range(9):
        stages += [(2 + 4 * l, f"l{l}.after_self"), (3 + 4 * l, f"l{l}.after_tb1"), (4 + 4 * l, f"l{l}.after_cross"), (5 + 4 * l, f"l{l}.out")]
    try:
        for stage, key in stages:
            m.engine(x.device)
            _lib.check(lib.cfd_debug_stop_stage(m._handle, stage))
            with torch.no_grad():
                m(x, torch.tensor(t), mems, mem_mask_dict=masks)
            got = read_debug(m, "x", (Be, L, 512))
            want = taps[key].transpose(1, 0, 2)
            report.append((key, rel_l2(got, want)))
            if stage == 1:
                temb = read_debug(m, "temb", (1, 512))
                report.append(("temb", rel_l2(temb, taps["temb"][0, :1])))
    finally:
        _lib.check(lib.cfd_debug_stop_stage(m._handle, 0))
    print("\n".join(f"{k:18s} rel {e:.3e}" for k, e in report))
    bad = [(k, e) for k, e in report if not e < FWD_TOL]
    assert not bad, bad


@pytest.mark.parametrize("name", ["tiny", "tiny_sharp", "real", "oddlen"])
def test_forward_matches_reference_golden(name):
    sd, inp, t, g, out, att, m = _run(name)
    assert np.isfinite(out).all()
    e = rel_l2(out, g["out"])
    print(name, "out rel", e)
    assert e < FWD_TOL
    from oracle import denoiser_ref
    for j, nm in enumerate(denoiser_ref.MEM_NAMES):
        ref = g[f"att{j}"]
        assert att[j].shape[1:] == ref.shape[1:]
        assert max_abs(att[j][: ref.shape[0]], ref) < 1e-4, nm
        mk = inp["masks"][nm]
        if mk is not None:  # masked keys get exactly zero probability, like the reference
            assert np.all(att[j][np.broadcast_to(mk[:, None, None, :], att[j].shape)] == 0)
        np.testing.assert_allclose(att[j].sum(-1), 1.0, atol=1e-5)


def test_forward_long_memory_extended_pe():
    sd, inp, t, g, out, att, m = _run("synth")
    assert rel_l2(out, g["out"]) < FWD_TOL
    assert max_abs(att[1][..., :64], g["att1_head"]) < 1e-4
    assert max_abs(att[0], g["att0"]) < 1e-4


def test_forward_matches_oracle_per_row_timesteps():
    import torch
    from oracle import denoiser_ref
    from tests.gpu_helpers import dev_inputs, hip_denoiser
    sd, inp, t, g = forward_case("tiny")
    ts = np.array([0, 1, 37, 250, 500, 998, 999])
    want, _ = denoiser_ref.denoiser_forward(sd, inp["sample"], ts, inp["memories"], inp["masks"])
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    with torch.no_grad():
        out, _ = m(torch.from_numpy(inp["sample"]).cuda(), torch.from_numpy(ts).cuda(), mems, mem_mask_dict=masks)
    assert rel_l2(out.cpu().numpy(), want) < FWD_TOL


def test_forward_rejects_what_the_reference_rejects():
    import torch
    from convofusion_amd._lib import CfdError
    from tests.gpu_helpers import dev_inputs, hip_denoiser
    sd, inp, t, g = forward_case("tiny")
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    x = torch.from_numpy(inp["sample"]).cuda()
    with pytest.raises(CfdError):  # odd L
        m(x[:, :15].contiguous(), torch.tensor(t), mems, mem_mask_dict=masks)
    with pytest.raises(RuntimeError):  # no CPU fallback
        m.engine(torch.device("cpu"))


def test_forward_does_not_mutate_inputs_and_is_deterministic():
    import torch
    from tests.gpu_helpers import dev_inputs, hip_denoiser
    sd, inp, t, g = forward_case("tiny")
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    x = torch.from_numpy(inp["sample"]).cuda()
    x0, m0 = x.clone(), [a.clone() for a in mems]
    with torch.no_grad():
        a, _ = m(x, torch.tensor(t), mems, mem_mask_dict=masks)
        b, _ = m(x, torch.tensor(t), mems, mem_mask_dict=masks)
    assert torch.equal(a, b)
    assert torch.equal(x, x0) and all(torch.equal(p, q) for p, q in zip(mems, m0))


def test_headline_shape_rows_match_reference():
    """BASELINE configs[1] at FULL size (Be = 7 x 32 = 224 rows, L = 196, 1500 audio tokens): rows are independent, so the
    7 guidance rows of utterances {0, 17, 31} are held against the REFERENCE Denoiser's outputs for exactly those rows
    (tests/golden/denoiser_c2rows.npz, made by make_golden_c2rows.py) -- the hot MFMA path at the shape the metric is
    quoted on (Lp = 224: a partial last key tile, 13 row tiles per batch row), with and without attention maps
    (the two cross-attention paths)."""
    import torch
    from oracle import inputs
    from tests.gpu_helpers import hip_denoiser, to_dev
    from tests.helpers import load_golden
    g = load_golden("denoiser_c2rows")
    meta = [int(v) for v in g["meta"]]
    B, L, S, pad, t, seed, utts = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13], meta[14:]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, uncond_pad_tail=pad)
    m = hip_denoiser(1234, 1.0)
    x = to_dev(np.concatenate([cb["init"]] * 7))
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    keep = m.return_attention
    try:
        for want_att in (False, True):
            m.return_attention = want_att
            with torch.no_grad():
                out, att = m(x, torch.tensor(t), mems, mem_mask_dict=masks)
            out = out.cpu().numpy()
            assert np.isfinite(out).all()
            for u in utts:
                idx = np.array([c * B + u for c in range(7)])
                e = rel_l2(out[idx], g[f"out{u}"])
                print(f"attention maps {want_att}: utterance {u} rows rel {e:.2e}")
                assert e < FWD_TOL
            if want_att:
                a1 = att[1][2 * B + 17].cpu().numpy()       # audio attention of the audio-only chunk's row of utterance 17
                assert max_abs(a1[:, :, :96], g["att1_u17_row2_head"]) < 1e-4
                assert max_abs(a1.sum(-1), g["att1_u17_row2_rowsum"]) < 1e-4
                assert max_abs(att[2][1 * B + 17].cpu().numpy(), g["att2_u17_row1"]) < 1e-4
            del att
    finally:
        m.return_attention = keep


def test_fused_cross_attention_with_several_long_memories_and_degenerate_rows():
    """The fused cross-attention kernel on the shapes the golden cases do not have: THREE memories longer than one 32-key tile (the
    single output accumulator is flushed to the residual stream between two online memories, and the per-memory sums of the rank-one
    timestep term must survive those flushes), key lengths that are not multiples of 32, ragged key-padding masks, a memory row whose
    512 features are all equal (the static part of its LayerNorm variance is 0: the per-step variance comes from the timestep
    embedding alone) and one that is all zeros, queries in a partial last tile (L = 36).  Against the numpy oracle."""
    import torch
    from oracle import denoiser_ref
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S = 2, 36, (70, 200, 40, 33, 1)
    cb = inputs.make_cfg_batch(seed=77, B=B, L=L, S=S, pad_tail=(5, 9, 0, 2, 0))
    mems = [x.copy() for x in cb["memories"]]
    mems[1][3, 17, :] = 0.731       # constant row
    mems[0][5, 2, :] = 0.0          # zero row
    rng = np.random.Generator(np.random.PCG64(5))
    sample = rng.standard_normal((7 * B, L, 128)).astype(np.float32)
    sd = state_dict()
    m = hip_denoiser(1234, 1.0)
    for t in (3, 640):
        want, _ = denoiser_ref.denoiser_forward(sd, sample, t, mems, cb["masks"])
        with torch.no_grad():
            out, _ = m(torch.from_numpy(sample).cuda(), torch.tensor([t]).cuda(), [to_dev(x) for x in mems],
                       mem_mask_dict={k: to_dev(v) for k, v in cb["masks"].items()})
        e = rel_l2(out.cpu().numpy(), want)
        print("t =", t, "rel L2 vs oracle", e)
        assert e < FWD_TOL


def test_out_of_range_memories_are_refused_not_clamped():
    """The split-pair operands saturate at +-65504 (fp16).  The products K = A a_s, V = VV a_s of the CENTRED raw memories follow the
    caller's scale (the text encoder's projection is unbounded, t5.py:8-108).  Memories 1e3 times larger than the test inputs stay inside
    the range and must still match the oracle (the memory LayerNorm makes the reference nearly scale-free, and so must we);
    memories scaled into saturation must be REFUSED (CFD_E_RANGE) -- by Denoiser.forward and by the sampling run -- not clamped."""
    import torch
    from convofusion_amd._lib import CfdError
    from convofusion_amd.sampler import SamplingRun
    from oracle import denoiser_ref
    from tests.gpu_helpers import SCHED_KW, dev_inputs, hip_denoiser, read_debug
    from convofusion_amd import scheduler
    sd, inp, t, g = forward_case("tiny")
    m = hip_denoiser(1234, 1.0)
    x = torch.from_numpy(inp["sample"]).cuda()
    big = dict(inp, memories=[np.float32(1e3) * v for v in inp["memories"]])
    want, _ = denoiser_ref.denoiser_forward(sd, big["sample"], t, big["memories"], big["masks"])
    mems, masks = dev_inputs(big)
    with torch.no_grad():
        out, _ = m(x, torch.tensor(t), mems, mem_mask_dict=masks)
    e = rel_l2(out.cpu().numpy(), want)
    print("memories x 1e3: rel", e, "census", float(read_debug(m, "sat", (1,))[0]))
    assert e < FWD_TOL and float(read_debug(m, "sat", (1,))[0]) == 0
    huge = [np.float32(3e6) * v for v in inp["memories"]]
    hm = [torch.from_numpy(v).cuda() for v in huge]
    with pytest.raises(CfdError) as ei:
        m(x, torch.tensor(t), hm, mem_mask_dict=masks)
    assert ei.value.code == -5
    with pytest.raises(CfdError) as ei:
        SamplingRun(m, scheduler.DDPMScheduler(**SCHED_KW), hm, masks, inp["sample"].shape[0], inp["sample"].shape[1], 4, guidance_chunks=1, seed=0)
    assert ei.value.code == -5
    with torch.no_grad():   # the handle is usable afterwards
        out2, _ = m(x, torch.tensor(t), mems, mem_mask_dict=masks)
    assert torch.equal(out, out2)
    # Paths whose memory-side projections run INSIDE the forward (per-row timesteps; attention maps wanted) project the NORMALISED
    # memories (the memory LayerNorm comes first there), so the caller's scale cannot reach the split pairs: the same huge memories are
    # served, match the oracle, and leave the census -- which belongs to the handle and is read at the end of the SAME call -- clean.
    Be = inp["sample"].shape[0]
    want_huge, _ = denoiser_ref.denoiser_forward(sd, inp["sample"], t, huge, inp["masks"])
    with torch.no_grad():
        out3, _ = m(x, torch.full((Be,), t), hm, mem_mask_dict=masks)
    assert rel_l2(out3.cpu().numpy(), want_huge) < 10 * FWD_TOL and float(read_debug(m, "sat", (1,))[0]) == 0
    keep = m.return_attention
    try:
        m.return_attention = True
        try:       # served from normalised memories (tile kernels) or refused (small problems keep the once-per-call projections): never clamped
            with torch.no_grad():
                out4, _ = m(x, torch.tensor(t), hm, mem_mask_dict=masks)
            assert rel_l2(out4.cpu().numpy(), want_huge) < 10 * FWD_TOL
        except CfdError as e:
            assert e.code == -5
    finally:
        m.return_attention = keep
    # a failed call on one handle leaves the other handle (and the next call on this one) alone
    with pytest.raises(CfdError):
        m(x, torch.tensor(t), hm, mem_mask_dict=masks)
    with torch.no_grad():
        out6, _ = m(x, torch.tensor(t), mems, mem_mask_dict=masks, side_engine=True)
    assert rel_l2(out6.cpu().numpy(), want) < FWD_TOL
    # a sample outside the range is named as such
    with pytest.raises(CfdError) as ei:
        m(x * 1e6, torch.tensor(t), mems, mem_mask_dict=masks)
    assert ei.value.code == -5 and "sample" in str(ei.value)
    with torch.no_grad():
        out5, _ = m(x, torch.tensor(t), mems, mem_mask_dict=masks)
    assert torch.equal(out, out5)


def test_heavy_tailed_weights_stress_case():
    """Stand-in for the trained checkpoint that cannot be loaded here (README.md:52-57): weights with outlier LayerNorm gains, outlier and
    near-zero (fp16-subnormal ``hi``) rows in the FFN / in-projection matrices, memories with outlier tokens and features
    (oracle.weights.make_state_dict_heavy, oracle.inputs.make_outlier_batch).  Goldens from the imported reference
    (tests/golden/make_golden_heavy.py): one forward on the row-tile path, one on the tile kernels (fused cross-attention), within the
    tolerance of the uniform-weight goldens; the listener-text attention maps; the saturation census must stay clean (or the call must
    fail with CFD_E_RANGE -- never a silently clamped operand)."""
    import torch
    from convofusion_amd.denoiser import Denoiser
    from tests.gpu_helpers import ABL, DENOISER_KW, dev_inputs, read_debug, to_dev
    from tests.helpers import heavy_case, heavy_state_dict
    m = Denoiser(ablation=ABL, **DENOISER_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in heavy_state_dict().items()}, strict=True)
    m = m.cuda().eval()
    for name in ("fwd_small", "fwd_tile"):
        inp, t, want, want_att = heavy_case(name)
        mems, masks = dev_inputs(inp)
        for ra in (False, True):
            m.return_attention = ra
            with torch.no_grad():
                out, att = m(to_dev(inp["sample"]), torch.tensor(t), mems, mem_mask_dict=masks)
            e = rel_l2(out.cpu().numpy(), want)
            ea = max_abs(att[2].cpu().numpy(), want_att) if ra else 0.0
            print(f"{name} (attention maps {'on' if ra else 'off'}): rel {e:.2e}, listener-text maps max abs {ea:.2e}, census {float(read_debug(m, 'sat', (1,))[0])}")
            # (maps: the outlier gains make the logits large -- the numpy oracle and the torch reference, both float32, differ by 3e-3 there)
            assert e < FWD_TOL and ea < 1e-2 and float(read_debug(m, "sat", (1,))[0]) == 0


@pytest.mark.parametrize("shape", ["row_tile", "tile_kernels"])
def test_a_row_with_a_fully_masked_memory_is_nan_like_the_reference(shape):
    """A batch row whose key-padding mask covers EVERY key of a memory has a softmax over nothing: the reference's MultiheadAttention
    returns NaN there, the residual stream of that row becomes NaN and stays NaN through every later LayerNorm, so the row's whole output
    is NaN while the other rows are untouched.  The HIP path must do the same -- in particular the split-pair stores must not turn the
    NaN into a clamped, finite operand (split_f32's v_med3 maps NaN to -65504)."""
    import torch
    from oracle import denoiser_ref
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    Be, L, S = (5, 16, (6, 20, 6, 8, 1)) if shape == "row_tile" else (9, 100, (20, 70, 24, 8, 1))
    inp = inputs.make_plain_batch(seed=606, Be=Be, L=L, S=S, pad_tail=(2, 0, 3, 0, 0))
    inp["masks"]["tlsn"][1, :] = True
    sd = state_dict()
    want, _ = denoiser_ref.denoiser_forward(sd, inp["sample"], 300, inp["memories"], inp["masks"])
    assert np.isnan(want[1]).all() and np.isfinite(np.delete(want, 1, axis=0)).all()      # what the reference's arithmetic gives
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    keep = m.return_attention
    try:
        for ra in (False, True):
            m.return_attention = ra
            with torch.no_grad():
                out, _ = m(to_dev(inp["sample"]), torch.tensor(300), mems, mem_mask_dict=masks)
            out = out.cpu().numpy()
            assert np.isnan(out[1]).all(), f"{shape}, attention maps {ra}: the masked row came out finite"
            assert rel_l2(np.delete(out, 1, axis=0), np.delete(want, 1, axis=0)) < FWD_TOL
    finally:
        m.return_attention = keep


@pytest.mark.parametrize("shape", ["row_tile", "tile_kernels"])
@pytest.mark.parametrize("offset", ["all_features", "halves_apart"])
def test_layernorms_of_rows_far_from_zero_mean(shape, offset):
    """Residual-stream rows whose mean is far from zero, and rows whose two 256-feature halves sit far apart: every LayerNorm of the layer then
    subtracts a mean much larger than the deviations it keeps.  The fused cross-attention kernel puts LayerNorm2's statistics together from
    the two half rows its pair of waves loaded (mean and sum of squared deviations per half, Chan's pairwise update: xattn_fused.hpp prologue);
    `halves_apart` makes the between-halves term the whole variance.  The offset enters through latent_embd.bias
    (convofusion/models/architectures/denoiser.py:181: the residual stream starts as latent_embd(sample) + positional terms).  Against the numpy oracle."""
    import torch
    from convofusion_amd.denoiser import Denoiser
    from oracle import denoiser_ref
    from tests.gpu_helpers import ABL, DENOISER_KW, dev_inputs, to_dev
    Be, L, S = (5, 16, (6, 20, 6, 8, 1)) if shape == "row_tile" else (9, 100, (20, 170, 24, 8, 1))
    inp = inputs.make_plain_batch(seed=909, Be=Be, L=L, S=S, pad_tail=(2, 0, 3, 0, 0))
    sd = {k: v.copy() for k, v in state_dict().items()}
    if offset == "all_features":
        sd["latent_embd.bias"] = (sd["latent_embd.bias"] + 25.0).astype(np.float32)
    else:
        sd["latent_embd.bias"] = (sd["latent_embd.bias"] + np.where(np.arange(512) < 256, 12.0, -12.0)).astype(np.float32)
    want, _ = denoiser_ref.denoiser_forward(sd, inp["sample"], 420, inp["memories"], inp["masks"])
    m = Denoiser(ablation=ABL, **DENOISER_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    mems, masks = dev_inputs(inp)
    with torch.no_grad():
        out, _ = m(to_dev(inp["sample"]), torch.tensor(420), mems, mem_mask_dict=masks)
    e = rel_l2(out.cpu().numpy(), want)
    print(shape, offset, "rel L2 vs oracle", e)
    assert e < FWD_TOL


@pytest.mark.parametrize("shape", ["row_tile", "tile_kernels"])
def test_key_padding_masks_with_holes(shape):
    """nn.MultiheadAttention's key_padding_mask is any boolean pattern, not only a padded tail (every other fixture masks tails): masks
    with holes -- the first key, isolated keys, whole 32-key tiles, different patterns per batch row -- on all five memories, against the
    numpy oracle, with and without attention maps (the fused kernel's -inf key bias, the three-launch softmax's mask loads, the row-tile
    path's per-step tables); masked columns must come out exactly zero and the rows must sum to one."""
    import torch
    from oracle import denoiser_ref
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    Be, L, S = (6, 16, (24, 161, 24, 8, 2)) if shape == "row_tile" else (10, 100, (40, 300, 33, 8, 3))
    inp = inputs.make_plain_batch(seed=808, Be=Be, L=L, S=S)
    rng = np.random.Generator(np.random.PCG64(12))
    names = ("spkemb", "alsn", "tlsn", "apb", "lsnemb")
    for j, name in enumerate(names):
        mk = rng.random((Be, S[j])) < 0.3
        mk[0, 0] = True                                   # the first key
        if S[j] > 64:
            mk[1, 32:64] = True                           # a whole 32-key tile
            mk[2, :] = False                              # a row without any masked key next to masked ones
        mk[:, S[j] - 1] = False                           # (never everything: that case is test_a_row_with_a_fully_masked_memory_...)
        inp["masks"][name] = mk
    sd = state_dict()
    want, watt = denoiser_ref.denoiser_forward(sd, inp["sample"], 123, inp["memories"], inp["masks"])
    m = hip_denoiser(1234, 1.0)
    mems, masks = dev_inputs(inp)
    keep = m.return_attention
    try:
        for ra in (False, True):
            m.return_attention = ra
            with torch.no_grad():
                out, att = m(to_dev(inp["sample"]), torch.tensor(123), mems, mem_mask_dict=masks)
            e = rel_l2(out.cpu().numpy(), want)
            print(f"{shape}, attention maps {ra}: rel {e:.2e}")
            assert e < FWD_TOL
            if ra:
                for j, name in enumerate(names):
                    a = att[j].cpu().numpy()
                    assert max_abs(a, watt[j]) < 1e-4
                    assert np.all(a[np.broadcast_to(inp["masks"][name][:, None, None, :], a.shape)] == 0)
                    np.testing.assert_allclose(a.sum(-1), 1.0, atol=1e-5)
    finally:
        m.return_attention = keep


@pytest.mark.gpu
@pytest.mark.parametrize("Be", [14, 70])
def test_repeated_forwards_with_the_same_memories_reuse_their_projections(Be):
    """The reference's own loop calls the denoiser once per iteration with the same conditioning tensors (convofusion.py:499-513).
    Denoiser.forward recognises the same tensor objects at the same version and lets the library reuse the memories' timestep-independent
    projections (cfd_forward_same_memories) -- on the row-tile path (14 rows) and on the tile kernels (70 rows of 16 tokens).  Every call
    must equal the same call on a denoiser that has never seen the memories: a second and third timestep, after an in-place change of a
    memory (version counter: projections made again), after a change of a mask, and with a sampling run on the handle in between."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    from convofusion_amd import scheduler
    L, S = 16, (6, 40, 6, 8, 1)
    inp = inputs.make_plain_batch(seed=77, Be=Be, L=L, S=S, pad_tail=(2, 5, 1, 0, 0))
    x = to_dev(inp["sample"])
    mems = [to_dev(m) for m in inp["memories"]]
    masks = {k: to_dev(v) for k, v in inp["masks"].items()}
    m = hip_denoiser(1234, 1.0)

    other = hip_denoiser.__wrapped__(1234, 1.0)     # (a second module with its own handle: hip_denoiser itself is cached and would return m)
    other.assume_constant_memories = False

    def fresh(t):
        with torch.no_grad():
            return other(x, torch.tensor(t), [q.clone() for q in mems], mem_mask_dict={k: (None if v is None else v.clone()) for k, v in masks.items()})

    def call(t, reused):
        with torch.no_grad():
            out = m(x, torch.tensor(t), mems, mem_mask_dict=masks)
        assert m.last_forward_reused == reused, (t, m.last_forward_reused)
        return out

    def same(a, b):     # (bit-identical; NaN -- the rows whose memory the changed mask covers completely -- in the same places)
        eq = lambda p, q: torch.equal(torch.isnan(p), torch.isnan(q)) and torch.equal(p.nan_to_num(nan=0.0), q.nan_to_num(nan=0.0))
        return eq(a[0], b[0]) and all(eq(p, q) for p, q in zip(a[1], b[1]))

    m._last_forward_memories = None
    assert same(call(900, False), fresh(900))
    assert same(call(500, True), fresh(500))              # reused
    assert same(call(37, True), fresh(37))                # reused again
    mems[1].mul_(1.5)                               # in place: the version counter moves, the projections are made again
    assert same(call(36, False), fresh(36))
    assert same(call(35, True), fresh(35))
    name = [k for k, v in masks.items() if v is not None][0]
    masks[name][:, 0] = ~masks[name][:, 0] if masks[name].dtype == torch.bool else 1 - masks[name][:, 0]
    assert same(call(34, False), fresh(34))
    # something else on the handle in between: the library refuses the promise by itself
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    cb = inputs.make_cfg_batch(seed=3, B=2, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
    sample(m, sch, [to_dev(q) for q in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}, B=2, L=L, num_inference_steps=2, seed=1)
    assert same(call(33, True), fresh(33))          # (the Python side promises; the LIBRARY ignores the promise: a run was on the handle)
    assert same(call(32, True), fresh(32))


@pytest.mark.parametrize("Be", [14, 70])
def test_a_memory_rewritten_through_a_raw_pointer_is_not_served_from_the_previous_forward(Be):
    """The same-memories reuse keys on tensor identity + torch's version counter, which a write through a raw pointer does not move
    (round 5's staleness hole).  (i) the package's own raw-pointer writers bump the counter themselves: ``linear_act(..., out=mem)`` between
    two forwards gives the answer of a denoiser that has never seen the memories; (ii) ``mem.data.copy_()`` -- invisible to the counter by
    torch's own rules -- is refused with a RuntimeError when ``verify_constant_memories`` is on (a device checksum per tensor), gives the
    right answer with ``assume_constant_memories = False``, and is the documented caveat otherwise;
    (iii) a changed layer-0 shape or path between two forwards of the same memories (row-tile path first, tile kernels second: the one-key
    memory's value rows were only made by the second kind) still reuses correctly."""
    import torch
    from convofusion_amd.conditioning import ACT_GELU, linear_act
    from tests.gpu_helpers import hip_denoiser, to_dev
    L, S = 16, (6, 40, 6, 8, 1)
    inp = inputs.make_plain_batch(seed=78, Be=Be, L=L, S=S, pad_tail=(2, 5, 1, 0, 0))
    x = to_dev(inp["sample"])
    mems = [to_dev(m) for m in inp["memories"]]
    masks = {k: to_dev(v) for k, v in inp["masks"].items()}
    m = hip_denoiser(1234, 1.0)

    other = hip_denoiser.__wrapped__(1234, 1.0)     # (a second module with its own handle: hip_denoiser itself is cached and would return m)
    other.assume_constant_memories = False

    def fresh(t, xx=None):
        with torch.no_grad():
            return other(x if xx is None else xx, torch.tensor(t), [q.clone() for q in mems], mem_mask_dict={k: (None if v is None else v.clone()) for k, v in masks.items()})

    def call(t, xx=None, reused=None):
        with torch.no_grad():
            out = m(x if xx is None else xx, torch.tensor(t), mems, mem_mask_dict=masks)
        assert reused is None or m.last_forward_reused == reused, (t, m.last_forward_reused)
        return out

    def same(a, b):
        eq = lambda p, q: torch.equal(torch.isnan(p), torch.isnan(q)) and torch.equal(p.nan_to_num(nan=0.0), q.nan_to_num(nan=0.0))
        return eq(a[0], b[0]) and all(eq(p, q) for p, q in zip(a[1], b[1]))

    m._last_forward_memories = None
    assert same(call(900, reused=False), fresh(900)) and same(call(800, reused=True), fresh(800))
    # (i) a product API that writes a caller tensor through its raw pointer
    g = torch.Generator(device="cpu").manual_seed(5)
    w = (torch.randn(512, 512, generator=g) * 0.05).cuda()
    src = mems[1].clone()
    v0 = mems[1]._version
    linear_act(src, w, None, ACT_GELU, out=mems[1])
    assert mems[1]._version > v0, "linear_act(out=...) must move the version counter of the tensor it rewrote"
    assert not torch.equal(mems[1], src)
    assert same(call(700, reused=False), fresh(700)) and same(call(600, reused=True), fresh(600))
    # (ii) a write torch's counter cannot see
    try:
        m.verify_constant_memories = True
        assert same(call(500, reused=False), fresh(500))   # (the call before recorded no checksums: made again, checksums recorded)
        assert same(call(450, reused=True), fresh(450))
        v0 = mems[0]._version
        mems[0].data.copy_(mems[0] * 0.5)
        assert mems[0]._version == v0                   # ... which is the whole problem
        with pytest.raises(RuntimeError, match="rewritten between two forwards"):
            call(400)
        assert same(call(400, reused=False), fresh(400))   # after the refusal the projections are made again
        m.verify_constant_memories = False
        m.assume_constant_memories = False
        mems[0].data.copy_(mems[0] * 2.0)
        assert same(call(300, reused=False), fresh(300))
    finally:
        m.verify_constant_memories = False
        m.assume_constant_memories = True
    # (iii) same memories, another query length: 16 tokens (Be = 14: row-tile path) then 34 (tile kernels)
    x2 = to_dev(inputs.make_plain_batch(seed=79, Be=Be, L=34, S=S, pad_tail=(2, 5, 1, 0, 0))["sample"])
    assert same(call(250, reused=False), fresh(250))
    assert same(call(200, x2, reused=True), fresh(200, x2))
    assert same(call(150, reused=True), fresh(150))


def test_forward_and_attention_sampling_under_inference_mode():
    """pytorch_lightning's Trainer runs the reference's test loop under torch.inference_mode(): every conditioning tensor is an inference
    tensor, whose version counter cannot be read (RuntimeError).  Denoiser.forward must work there -- the same-memories reuse then keys on a
    device checksum instead -- and so must the loop drop-in's attention forward (last_step_attention calls the denoiser)."""
    import torch
    from convofusion_amd.sampler import sample
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    from convofusion_amd import scheduler
    L, S, Be = 16, (6, 40, 6, 8, 1), 14
    inp = inputs.make_plain_batch(seed=81, Be=Be, L=L, S=S, pad_tail=(2, 5, 1, 0, 0))
    m = hip_denoiser(1234, 1.0)
    with torch.no_grad():
        want = [m(to_dev(inp["sample"]), torch.tensor(t), [to_dev(q) for q in inp["memories"]], mem_mask_dict={k: to_dev(v) for k, v in inp["masks"].items()})
                for t in (900, 500)]
    with torch.inference_mode():
        x = to_dev(inp["sample"])
        mems = [to_dev(q) for q in inp["memories"]]
        masks = {k: to_dev(v) for k, v in inp["masks"].items()}
        assert mems[0].is_inference()
        got = [m(x, torch.tensor(t), mems, mem_mask_dict=masks) for t in (900, 500)]     # the second call reuses (checksum signature)
        assert m.last_forward_reused
        mems[1].mul_(1.5)                                                                 # no version counter to move: the checksum sees it
        moved = m(x, torch.tensor(500), mems, mem_mask_dict=masks)
        assert not m.last_forward_reused
    for g, w in zip(got, want):
        assert torch.equal(g[0], w[0]) and all(torch.equal(p, q) for p, q in zip(g[1], w[1]))
    with torch.no_grad():
        mm = [to_dev(q) for q in inp["memories"]]
        mm[1].mul_(1.5)
        want_moved = hip_denoiser(1234, 1.0)(to_dev(inp["sample"]), torch.tensor(500), mm, mem_mask_dict={k: to_dev(v) for k, v in inp["masks"].items()})
    assert torch.equal(moved[0], want_moved[0])
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    cb = inputs.make_cfg_batch(seed=3, B=2, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
    plain = sample(m, sch, [to_dev(q) for q in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}, B=2, L=L, num_inference_steps=4, seed=1,
                   return_attention=True)
    with torch.inference_mode():
        lat, att = sample(m, sch, [to_dev(q) for q in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}, B=2, L=L, num_inference_steps=4,
                          seed=1, return_attention=True)
    assert torch.equal(lat, plain[0]) and all(torch.equal(a, b) for a, b in zip(att, plain[1]))


def test_the_cross_attention_block_is_float32_exact_on_the_ill_conditioned_chunk():
    """Round 5's heavy-tailed stress case at the headline row shape (tests/golden/heavy_c2.npz, outlier factor 20): one guidance chunk (the
    listener-id chunk of utterance 5) ends 1.9e-3 from the float64 reference where float32 is 3e-4, all of it at ONE query token of layer 4's
    cross-attention.  The round-5 review asked for a precision escape -- an exact score product.  This test is the measurement that says what
    such a knob could buy: layer 4's cross-attention block of that chunk recomputed in FLOAT64 (reference formulation, cross_attention.py:578-652)
    (a) from the HIP path's OWN input to the block, (b) from the float32 oracle's input.  The HIP block must agree with (a) as well as the
    float32 oracle agrees with (b) -- a few 1e-6 of the update: the split-pair block is float32-exact even here -- while (a) and (b) differ
    by three orders of magnitude more: the block amplifies the 2e-4 difference of its INPUT (the 22-bit operands of layers 0 - 3 against
    float32's 24), which no precision inside the block can remove.  (profiles/r06_heavy_c2_exact_block.log; tools/heavy_c2_debug.py EXACT=4.)"""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.denoiser import Denoiser
    from oracle import denoiser_ref, weights
    from tests.gpu_helpers import ABL, DENOISER_KW, read_debug, to_dev
    from tests.helpers import heavy_state_dict, load_golden
    g = load_golden("heavy_c2")
    meta = [int(v) for v in g["meta"]]
    B, L, S, pad, t, seed, u = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13], meta[14]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, uncond_pad_tail=pad)
    idx = np.array([c * B + u for c in range(7)])
    mems = [inputs.add_outlier_tokens(q, seed + j)[rm][idx] for j, (q, rm) in enumerate(zip(cb["unique"], cb["row_map"]))]
    masks = {k: (v[idx] if v is not None else None) for k, v in cb["masks"].items()}
    x_np = np.concatenate([cb["init"][u:u + 1]] * 7)
    sd = weights.extend_pe(heavy_state_dict(20.0), 1536)
    taps = {}
    denoiser_ref.denoiser_forward(sd, x_np, t, mems, masks, taps=taps)
    m = Denoiser(ablation=ABL, **DENOISER_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in heavy_state_dict(20.0).items()}, strict=True)
    m = m.cuda().eval()
    m.return_attention = False
    layer, chunk = 4, 5
    # the block in float64, reference formulation (tests/xattn_ref.py), on this chunk's memories
    from tests.xattn_ref import block_unfolded
    mem_taps = {"mem." + name: taps["mem." + name][:, chunk:chunk + 1] for name in inputs.MEM_NAMES}
    chunk_masks = {k: (None if v is None else np.asarray(v)[chunk:chunk + 1]) for k, v in masks.items()}

    def cross64(x):
        return block_unfolded(sd, layer, x[None], mem_taps, chunk_masks)[0][0]

    lib = _lib.load()
    hip = {}
    m.engine("cuda", mem_len=max(S))      # (the handle exists from the first forward on; the taps are set on it before that)
    try:
        for stage, key in ((3 + 4 * layer, "in"), (4 + 4 * layer, "out")):
            _lib.check(lib.cfd_debug_stop_stage(m._handle, stage))
            with torch.no_grad():
                m(to_dev(x_np), torch.tensor(t), [to_dev(v) for v in mems], mem_mask_dict={k: to_dev(v) for k, v in masks.items()})
            hip[key] = read_debug(m, "x", (7, L, 512))[chunk].astype(np.float64)
    finally:
        _lib.check(lib.cfd_debug_stop_stage(m._handle, 0))
    ref_in = taps[f"l{layer}.after_tb1"].transpose(1, 0, 2)[chunk].astype(np.float64)
    ref_out = taps[f"l{layer}.after_cross"].transpose(1, 0, 2)[chunk].astype(np.float64)
    ex_hip, ex_ref = cross64(hip["in"]), cross64(ref_in)
    n = np.linalg.norm
    local_hip = n((hip["out"] - hip["in"]) - ex_hip) / n(ex_ref)          # what precision inside the block could remove
    local_f32 = n((ref_out - ref_in) - ex_ref) / n(ex_ref)                # float32's own error in the block
    carried = n(ex_hip - ex_ref) / n(ex_ref)                              # the input difference, amplified by the block
    print(f"layer {layer} cross-attention, chunk {chunk}: HIP block vs float64 on its own input {local_hip:.2e}, float32 oracle likewise {local_f32:.2e}, "
          f"float64 block on the two inputs {carried:.2e} (inputs differ by {n(hip['in'] - ref_in) / n(ref_in):.2e})")
    assert local_hip < 2e-5 and local_hip < 5 * local_f32 + 1e-6
    assert carried > 30 * local_hip          # the chunk's error is carried in, not made here

