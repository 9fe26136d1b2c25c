"""-m gpu: the tile kernels' self-attention with V read token-major (attn_fused.hpp).

At every L != 16 the tile-kernel forward makes q | k | v in ONE projection launch (rows of 1536 columns) and
self_attn_fused_kernel builds its V^T fragments from those token rows with transposed LDS reads: a [key][feature] image, lane group g
reading keys 4g .. 4g+3 and 16+4g .. 16+4g+3 of 16 features.  What can go wrong there is the order of the keys inside a 32-key
block, the slot swizzle of the image, and the last tile, whose padding slots hold clamped copies of token L - 1.

Every case runs Denoiser.forward on a handle created with CFD_ROWTILE=0 (small problems on the tile kernels, as
test_developer_knobs_keep_parity forces them), 7 guidance chunks of B = 2 utterances with short memories, against the numpy oracle:
the residual stream behind the out-projection of layers 0 and 1 (debug stop stages 2 and 6) and the final output, each to the
relative L2 the forward goldens are held to.  Denoiser.forward runs every layer on all 14 rows (only a sampling run shares layer 0's rows
between the guidance chunks, and a debug stop stage switches the sharing off), so these cases do NOT run layer 0 on shared rows; the kernel
sees the row count only as grid.z, and the sampling-run tests at the headline shape (tests/test_gpu_sampler.py) run layer 0 on shared rows.
"""
import numpy as np
import pytest

from oracle import denoiser_ref, inputs
from tests.helpers import rel_l2, state_dict

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-4            # tests/test_gpu_forward.py
B, S, PAD, T = 2, (6, 40, 6, 8, 1), (2, 5, 1, 0, 0), 417


def _denoiser(sd):
    """A Denoiser with weights `sd` whose library handle is created with the row-tile path off (the knob is read at cfd_create)."""
    import os
    import torch
    from convofusion_amd.denoiser import Denoiser
    from tests.gpu_helpers import ABL, DENOISER_KW
    keep = os.environ.get("CFD_ROWTILE")
    os.environ["CFD_ROWTILE"] = "0"
    try:
        m = Denoiser(ablation=ABL, **DENOISER_KW)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m = m.cuda().eval()
        m.engine(torch.device("cuda"))
    finally:
        if keep is None:
            os.environ.pop("CFD_ROWTILE", None)
        else:
            os.environ["CFD_ROWTILE"] = keep
    return m


@pytest.fixture(scope="module")
def plain():
    return _denoiser(state_dict())


def _case(L, seed):
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=PAD)
    return np.concatenate([cb["init"]] * 7), cb["memories"], cb["masks"]


def _compare(m, sd, sample, mems, masks, label):
    """[(what, rel L2 against the oracle)] for the taps behind the out-projection of layers 0 and 1 and for the output; the output itself."""
    import torch
    from convofusion_amd import _lib
    from tests.gpu_helpers import read_debug, to_dev
    taps = {}
    want, _ = denoiser_ref.denoiser_forward(sd, sample, T, mems, masks, taps=taps)
    Be, L = sample.shape[:2]
    x = to_dev(sample)
    dm = [to_dev(v) for v in mems]
    dk = {k: to_dev(v) for k, v in masks.items()}
    lib = _lib.load()
    report = []
    try:
        for layer in (0, 1):
            _lib.check(lib.cfd_debug_stop_stage(m._handle, 2 + 4 * layer))
            with torch.no_grad():
                m(x, torch.tensor(T), dm, mem_mask_dict=dk)
            got = read_debug(m, "x", (Be, L, 512))
            assert np.isfinite(got).all(), f"{label}: layer {layer} tap is not finite"
            report.append((f"l{layer}.after_self", rel_l2(got, taps[f"l{layer}.after_self"].transpose(1, 0, 2))))
    finally:
        _lib.check(lib.cfd_debug_stop_stage(m._handle, 0))
    with torch.no_grad():
        out, _ = m(x, torch.tensor(T), dm, mem_mask_dict=dk)
    out = out.cpu().numpy()
    assert np.isfinite(out).all(), f"{label}: output is not finite"
    report.append(("out", rel_l2(out, want)))
    print(label, " ".join(f"{k} {e:.2e}" for k, e in report))
    return report, taps


# 18: one partial key tile and one partial query tile.  34: the second key tile holds 2 real keys and 30 clamped ones.
# 66: three key tiles, both stages of the double buffer re-used.  130: two query workgroups, the second with a single active wave.
@pytest.mark.parametrize("L", [18, 34, 66, 130])
def test_token_major_self_attention_matches_oracle(plain, L):
    sample, mems, masks = _case(L, 500 + L)
    report, _ = _compare(plain, state_dict(), sample, mems, masks, f"L = {L}:")
    bad = [(k, e) for k, e in report if not e < FWD_TOL]
    assert not bad, bad


def _scaled_self_attention(qk, v, layers=(0, 1)):
    sd = {k: val.copy() for k, val in state_dict().items()}
    for l in layers:
        p = f"decoder.layers.{l}.self_attn.in_proj_"
        for name in ("weight", "bias"):
            a = sd[p + name]
            a[:1024] *= np.float32(qk)
            a[1024:] *= np.float32(v)
    return sd


def test_one_dominant_key_per_query_and_large_values():
    """A wrong key order inside a 32-key block must not hide under near-uniform probabilities: the q and k projections of layers 0 and 1
    are scaled until a typical query's softmax is dominated by ONE key (checked below in float64 from the oracle's own layer-0 input),
    and the value projection is scaled so that the attention output is the larger part of the residual stream behind it.  L = 66: two
    whole 32-key blocks and a partial one."""
    L = 66
    sd = _scaled_self_attention(qk=4.0, v=16.0)
    sample, mems, masks = _case(L, 777)
    m = _denoiser(sd)
    report, taps = _compare(m, sd, sample, mems, masks, "dominant key:")
    # the premise, layer 0, all 4 heads: the largest probability of a row
    x0 = taps["x0"].transpose(1, 0, 2).astype(np.float64)
    p = "decoder.layers.0."
    xc = x0 - x0.mean(-1, keepdims=True)
    h = xc / np.sqrt((xc * xc).mean(-1, keepdims=True) + 1e-5) * sd[p + "norm1.weight"] + sd[p + "norm1.bias"]
    w, b = sd[p + "self_attn.in_proj_weight"].astype(np.float64), sd[p + "self_attn.in_proj_bias"].astype(np.float64)
    q = (h @ w[:512].T + b[:512]).reshape(-1, L, 4, 128)
    k = (h @ w[512:1024].T + b[512:1024]).reshape(-1, L, 4, 128)
    sc = np.einsum("bqhd,bkhd->bhqk", q, k) / np.sqrt(128.0)
    pr = np.exp(sc - sc.max(-1, keepdims=True))
    pmax = (pr / pr.sum(-1, keepdims=True)).max(-1)
    print("largest probability per row: median", float(np.median(pmax)), "share of rows above 0.5:", float((pmax > 0.5).mean()))
    assert np.median(pmax) > 0.5
    bad = [(k_, e) for k_, e in report if not e < FWD_TOL]
    assert not bad, bad


def test_padding_slots_of_the_last_key_tile_carry_no_weight():
    """L = 34: the second key tile holds keys 32 and 33 and 30 slots beyond L, which the kernel fills with clamped copies of token 33's k
    and v rows (finite operands) and gives probability exactly 0.  With the value projection of layers 0 and 1 scaled up a hundredfold,
    any weight on those 30 copies, or a non-finite product in their slots, would move the rows away from the oracle, whose L = 34 has
    no such slots at all."""
    L = 34
    sd = _scaled_self_attention(qk=1.0, v=100.0)
    sample, mems, masks = _case(L, 888)
    m = _denoiser(sd)
    report, _ = _compare(m, sd, sample, mems, masks, "padding slots:")
    bad = [(k, e) for k, e in report if not e < FWD_TOL]
    assert not bad, bad

