"""CPU: the stage functions of tests/t5_ref.py (one launch of cfd_t5_encode each) -- their composition is ``encode`` / ``project``, they
honour ``dtype``, masks with holes agree with transformers -- and the fixture tests/golden/t5_edges.npz."""
import os

import numpy as np
import pytest
import torch

from tests import t5_ref
from tests.test_t5_host import hf_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "t5_enc.npz"))
GE = np.load(os.path.join(ROOT, "tests", "golden", "t5_edges.npz"))


def compose(sd, ids, mask, dtype=np.float64):
    """the stages chained by hand, keeping every intermediate: (per block x_in, qkv, ctx, h, f, x_out), hidden, projected"""
    n, T = ids.shape
    x = np.asarray(sd["shared.weight"], dtype)[ids]
    blocks = []
    for l in range(t5_ref.num_layers_of(sd)):
        qkv = t5_ref.stage_qkv(sd, l, x, dtype)
        ctx = t5_ref.stage_attn(sd, qkv, mask, T, dtype)
        h = t5_ref.stage_attn_out(sd, l, x, ctx, dtype)
        f = t5_ref.stage_ff_in(sd, l, h, dtype)
        out = t5_ref.stage_ff_out(sd, l, h, f, dtype)
        blocks.append((x, qkv, ctx, h, f, out))
        x = out
    return blocks, t5_ref.stage_final(sd, x, False, dtype), t5_ref.stage_final(sd, x, True, dtype)


@pytest.mark.parametrize("name", ["A", "C"])
def test_composition_of_the_stages_is_encode_and_project(name):
    """<= 1e-12 against ``encode`` / ``project`` and the taps behind every block; shapes of every stage; and the fixture of the end-to-end
    tests (transformers' float32 output) lies within its own recorded error of the composition, as it does of ``encode``."""
    nl, seed, lens, T = t5_ref.CASES[name]
    sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)
    ids, mask = t5_ref.case_inputs(name)
    n = len(lens)
    blocks, hidden, projected = compose(sd, ids, mask)
    taps = []
    want = t5_ref.encode(sd, ids, mask, taps)
    assert hidden.dtype == np.float64 and hidden.shape == want.shape == (n, T, 768)
    assert np.abs(hidden - want).max() <= 1e-12
    assert np.abs(projected - t5_ref.project(sd, want)).max() <= 1e-12
    assert len(taps) == nl and all(np.abs(t - b[5]).max() <= 1e-12 for t, b in zip(taps, blocks))
    for x, qkv, ctx, h, f, out in blocks:
        assert qkv.shape == (n, T, 2304) and ctx.shape == h.shape == out.shape == (n, T, 768) and f.shape == (n, T, 3072) and (f >= 0).all()
    stored = G[name + "_out_f32"]
    assert stored.shape == projected.shape
    assert t5_ref.rel_err(stored, projected) <= float(G[name + "_f32_ref_err_proj"]) * (1 + 1e-6)


def test_stages_take_flat_rows_and_honour_dtype():
    """[rows, width] inputs (what the GPU tests read from the device) give the [n, T, width] values; float32 stays float32 and lies where
    single precision puts it: 1e-8 .. 1e-5 from float64, not 0 (a silent upcast) and not more."""
    sd = t5_ref.make_state(1, 13, t5_ref.VOCAB)
    ids, mask = t5_ref.prefix_inputs(5, (1, 7, 4), 7)
    (blk,), hidden, projected = compose(sd, ids, mask)
    (b32,), h32, p32 = compose(sd, ids, mask, np.float32)
    for a, b in zip(blk + (hidden, projected), b32 + (h32, p32)):
        assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == b.shape
    for a, b in zip(blk[1:] + (hidden, projected), b32[1:] + (h32, p32)):
        assert 1e-8 < t5_ref.rel_err(b, a) < 1e-5
    x, qkv, ctx, h, f, out = (v.reshape(21, -1) for v in blk)
    assert np.array_equal(t5_ref.stage_qkv(sd, 0, x), qkv)
    assert np.array_equal(t5_ref.stage_attn(sd, qkv, mask, 7).reshape(21, -1), ctx)
    assert np.array_equal(t5_ref.stage_attn_out(sd, 0, x, ctx), h)
    assert np.array_equal(t5_ref.stage_ff_out(sd, 0, h, f), out)


def test_attention_stage_without_a_key_is_nan_for_that_sequence_only():
    sd = t5_ref.make_state(1, 13, t5_ref.VOCAB)
    ids, mask = t5_ref.prefix_inputs(6, (5, 1, 3), 5)
    qkv = t5_ref.stage_qkv(sd, 0, sd["shared.weight"][ids])
    want = t5_ref.stage_attn(sd, qkv, mask, 5)
    mask[1] = 0
    got = t5_ref.stage_attn(sd, qkv, mask, 5)
    assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], want[[0, 2]]) and np.isfinite(want).all()


def test_hole_masks_are_what_they_say():
    m = t5_ref.hole_masks(129)
    assert m.shape == (3, 129) and m.dtype == np.uint8
    assert not m[0, :64].any() and m[0, 64:].all()
    assert m[1, :64].all() and not m[1, 64:128].any() and m[1, 128] == 1
    assert m[2, 0::2].all() and not m[2, 1::2].any()


def test_attention_stage_with_holes_matches_transformers_in_float64():
    """the hole masks of the GPU tests (T = 129) through ``encode`` -- that is, ``stage_attn`` -- against ``T5EncoderModel(...).double()``
    under ``keep_norm_dtype``: <= 1e-10 at every position (tests/test_t5_host.py does the same for prefix masks)"""
    nl, seed, _, _ = t5_ref.EDGE_CASES["H"]
    sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)
    ids, mask = t5_ref.edge_inputs("H")
    model = t5_ref.keep_norm_dtype(hf_model(sd, nl).double())
    with torch.no_grad():
        want = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long()).last_hidden_state.numpy()
    got = t5_ref.encode(sd, ids, mask)
    assert got.shape == want.shape and np.isfinite(got).all() and np.abs(got - want).max() <= 1e-10
    # a hole is no prefix: with the prefix mask of the same length the result differs
    assert np.abs(got - t5_ref.encode(sd, ids, np.sort(mask, axis=1)[:, ::-1])).max() > 1e-3


def test_edge_fixture_matches_the_restatement():
    """the stored inputs are the ones the tests regenerate; the restatement was within 1e-10 of transformers' float64 when the fixture was
    made; the stored float32 sample lies within its recorded error of the restatement (no transformers needed)"""
    assert set(t5_ref.EDGE_CASES) == {"L12", "T256", "H"}
    for name, (nl, seed, lens, T) in t5_ref.EDGE_CASES.items():
        ids, mask = t5_ref.edge_inputs(name)
        assert ids.dtype == np.int32 and mask.dtype == np.uint8 and ids.shape == mask.shape and ids.shape[1] == T
        assert np.array_equal(ids, GE[name + "_ids"]) and np.array_equal(mask, GE[name + "_mask"])
        assert float(GE[name + "_restatement_err"]) <= 1e-10
        assert 1e-8 < float(GE[name + "_f32_ref_err_hidden"]) < 1e-5 and 1e-8 < float(GE[name + "_f32_ref_err_proj"]) < 1e-5
        sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)
        want = t5_ref.project(sd, t5_ref.encode(sd, ids, mask))
        stored = GE[name + "_out_f32"]
        sub = want[:, ::t5_ref.EDGE_STORED[name]]
        assert stored.shape == sub.shape
        err = np.abs(stored - sub).max() / np.sqrt((want * want).mean())
        assert err <= float(GE[name + "_f32_ref_err_proj"]) * (1 + 1e-6)
    assert np.array_equal(t5_ref.edge_inputs("H")[1], t5_ref.hole_masks(129))
    assert t5_ref.edge_inputs("L12")[1].sum(1).tolist() == [9, 4] and t5_ref.edge_inputs("T256")[1].sum(1).tolist() == [256, 193]
