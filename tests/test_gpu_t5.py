"""GPU tests: the T5 text encoder in one HIP call (cfd_t5_encode, convofusion_amd/text.py) against the float64 restatement tests/t5_ref.py.
No transformers import: the weights are seeded (t5_ref.make_state), the gate's base comes from tests/golden/t5_enc.npz."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import t5_ref

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "t5_enc.npz"))
WI, WO = ("encoder.block.1.layer.1.DenseReluDense.%s.weight" % m for m in ("wi", "wo"))
FACTOR = 4.0      # a different reduction order (MFMA k-blocking against torch's) over the blocks, on top of what the reference's own float32 loses


@functools.lru_cache(maxsize=None)
def state(name, boosted=0):
    nl, seed, _, _ = t5_ref.CASES[name]
    sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)
    if boosted:      # block 1's feed-forward intermediates x boosted (a power of two: the function is unchanged)
        sd[WI] = sd[WI] * np.float32(boosted)
        sd[WO] = sd[WO] / np.float32(boosted)
    return sd


@functools.lru_cache(maxsize=None)
def reference(name, boosted=0):
    """(hidden, projected) float64, computed once and shared (callers do not write to them)"""
    sd = state(name, boosted)
    ids, mask = t5_ref.case_inputs(name)
    assert np.array_equal(ids, G[name + "_ids"]) and np.array_equal(mask, G[name + "_mask"])
    hidden = t5_ref.encode(sd, ids, mask)
    return hidden, t5_ref.project(sd, hidden)


@functools.lru_cache(maxsize=None)
def encoder(name, boosted=0):
    from convofusion_amd.text import T5TextEncoder
    sd = state(name, boosted)
    enc = T5TextEncoder.from_parts(t5_ref.stub_text_model(sd), None, t5_ref.projection_module(sd))
    return enc.cuda().eval()


def run(name, boosted=0, project=True, rows=None, T=None):
    import torch
    ids, mask = t5_ref.case_inputs(name)
    if rows is not None:
        ids, mask = ids[rows, :T], mask[rows, :T]
    out = encoder(name, boosted).encode_ids(torch.from_numpy(np.ascontiguousarray(ids)), torch.from_numpy(np.ascontiguousarray(mask)), project=project)
    return out.cpu().numpy()


def t5_info():
    """cfd_debug_read "t5.info" of the tests' handle: launches of the last call, token rows, workspace bytes, launches of 128 x 128 blocks"""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.conditioning import _engine_handle
    dev = torch.device("cuda", torch.cuda.current_device())
    info = torch.zeros(4, device=dev)
    _lib.check(_lib.load().cfd_debug_read(_engine_handle(dev), b"t5.info", C.c_void_p(info.data_ptr()), 4))
    return [int(v) for v in info.tolist()]


def check(name, boosted=0):
    hidden, proj = reference(name, boosted)
    e_h = t5_ref.rel_err(run(name, boosted, project=False), hidden)
    e_p = t5_ref.rel_err(run(name, boosted, project=True), proj)
    g_h, g_p = FACTOR * float(G[name + "_f32_ref_err_hidden"]), FACTOR * float(G[name + "_f32_ref_err_proj"])
    print(f"case {name}{' x %d' % boosted if boosted else ''}: hidden {e_h:.3e} (gate {g_h:.3e}), projected {e_p:.3e} (gate {g_p:.3e})")
    assert e_h <= g_h and e_p <= g_p, (e_h, g_h, e_p, g_p)


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_parity_with_float64_at_every_position(name):
    """Last hidden state and projected output against the float64 restatement, padded positions included; max-abs over output RMS, gate
    4 x the reference's own float32 loss (fixture).  Measured on the MI355X (hidden / projected): A 2.21e-6 / 2.21e-6 (gates
    1.05e-5 / 1.00e-5), B 1.43e-6 / 1.84e-6 (6.56e-6 / 9.14e-6), C 1.76e-6 / 1.27e-6 (2.96e-6 / 3.26e-6),
    D 1.82e-6 / 2.42e-6 (8.80e-6 / 1.29e-5)."""
    check(name)
    launches, rows, _, big = t5_info()
    nl, _, lens, T = t5_ref.CASES[name]
    assert launches == 5 * nl + 1 and rows == len(lens) * T
    # D's 2080 rows are there for the 128 x 128 blocks of the q | k | v and Wi products (a 256-CU device); the small cases never take them
    assert big == (2 if name == "D" else 0), big


def test_bits_do_not_depend_on_the_block_shape():
    """Sequences of case D encoded alone (every product in 64 x 64 blocks) give the bits of their valid rows in the 2080-row batch (q | k | v
    and Wi in 128 x 128 blocks): the first (full length), a short one and the last."""
    full = run("D")
    assert t5_info()[3] == 2
    _, _, lens, _ = t5_ref.CASES["D"]
    for s in (0, int(np.argmin(lens)), len(lens) - 1):
        alone = run("D", rows=[s], T=lens[s])
        assert t5_info()[3] == 0
        assert np.array_equal(alone[0], full[s, :lens[s]]), (s, lens[s])


@pytest.mark.parametrize("boost", [512, 65536])
def test_feed_forward_intermediates_past_fp16_range(boost):
    """Case A with block 1's wi x boost and wo / boost, same gate.  x 512 is the stated case; with these seeded weights (rows of wi have
    norm 1, so intermediates are of order 1) it reaches ~2 500, so x 65 536 is run as well and there the restatement's feed-forward
    intermediates are asserted to pass fp16's 65 504.  Measured on the MI355X: both give the unboosted run's 2.21e-6 / 2.21e-6 (scaling
    by a power of two commutes with every rounding); the x 65 536 intermediates reach 3.2e5."""
    sd = state("A", boost)
    ids, mask = t5_ref.case_inputs("A")
    taps = []
    t5_ref.encode(sd, ids, mask, taps)
    # block 1's input; its feed-forward reads the stream behind its attention, of the same size: a lower bound is enough here
    peak = np.abs(t5_ref.rms(taps[0], np.float64(sd[WI.replace("DenseReluDense.wi", "layer_norm")])) @ np.float64(sd[WI]).T).max()
    print("boost", boost, "feed-forward intermediate peak ~", peak)
    assert boost < 65536 or peak > 65504.0, peak
    check("A", boosted=boost)


def test_a_sequence_has_the_same_bits_alone_and_in_the_batch():
    """Each sequence of case A encoded alone at T = its own length gives the bits of its valid rows in the batch; two calls give the
    same bits."""
    full = run("A")
    assert np.array_equal(full, run("A"))
    _, _, lens, _ = t5_ref.CASES["A"]
    for s, n in enumerate(lens):
        alone = run("A", rows=[s], T=n)
        assert alone.shape == (1, n, 512)
        assert np.array_equal(alone[0], full[s, :n]), (s, n)


class StubEncoding(SimpleNamespace):
    def word_ids(self, i):
        return self._word_ids[i]


def stub_tokenizer(texts, return_tensors="pt", padding=True):
    """words -> ids by a fixed hash into [3, vocab), <bos> 1, <eos> 2, <pad> 0; word_ids like a fast tokenizer's"""
    import torch
    assert return_tensors == "pt" and padding is True
    rows, words = [], []
    for t in texts:
        toks = t.split()
        rows.append([1 if w == "<bos>" else 2 if w == "<eos>" else 3 + sum(map(ord, w)) % (t5_ref.VOCAB - 3) for w in toks])
        words.append(list(range(len(toks))))
    T = max(map(len, rows))
    ids = torch.tensor([r + [0] * (T - len(r)) for r in rows], dtype=torch.long)
    mask = torch.tensor([[1] * len(r) + [0] * (T - len(r)) for r in rows], dtype=torch.long)
    return StubEncoding(input_ids=ids, attention_mask=mask, _word_ids=[w + [None] * (T - len(w)) for w in words])


def test_drop_in_forward_encodes_distinct_strings_only():
    import torch
    from convofusion_amd import text
    sd = state("A")
    enc = text.T5TextEncoder.from_parts(t5_ref.stub_text_model(sd), stub_tokenizer, t5_ref.projection_module(sd)).cuda().eval()
    spk, lsn, none = "so what do you think about that", "well i am not sure", "-" * 10
    # the 7-way guidance pattern of one utterance (speaker texts, then listener texts): 14 strings, 3 distinct
    texts = [spk, none, spk, none, none, none, spk] + [lsn, none, none, lsn, none, none, lsn]
    emb, mask, wmap = enc(texts, return_map=True)
    T = len(spk.split()) + 2
    assert tuple(emb.shape) == (14, T, 512) and emb.dtype == torch.float32 and emb.is_cuda
    assert tuple(mask.shape) == (14, T) and mask.dtype == torch.bool
    assert enc.last_call == {"n_texts": 14, "n_encoded": 3, "T": T, "launches": 11}
    assert t5_info()[:2] == [11, 3 * T]                    # what the library recorded: 5 launches per block + 1, on the 3 distinct strings' rows
    for i, a in enumerate(texts):
        for j, b in enumerate(texts):
            if a == b:
                assert torch.equal(emb[i], emb[j]) and torch.equal(mask[i], mask[j])
    assert mask[0].all() and mask[1].sum() == 1 and mask[7].sum() == len(lsn.split()) + 2
    assert wmap[0][:T] == ["<bos>"] + spk.split() + ["<eos>"] and wmap[1] == [none] + [""] * (T - 1)
    # against the restatement on the tokenizer's own ids
    tok = stub_tokenizer([f"<bos> {spk} <eos>", none, f"<bos> {lsn} <eos>"])
    want = t5_ref.project(sd, t5_ref.encode(sd, tok.input_ids.numpy(), tok.attention_mask.numpy()))
    got = emb[[0, 1, 7]].cpu().numpy()
    assert t5_ref.rel_err(got, want) <= FACTOR * float(G["A_f32_ref_err_proj"])
    _, _, no_map = enc(texts)
    assert no_map is None
    with pytest.raises(NotImplementedError):
        enc.train()(texts)
    # install: the mirror replaces the reference's encoder and shares its parameters
    old = SimpleNamespace(text_model=enc.text_model, tokenizer=stub_tokenizer, projection=enc.projection, training=False)
    model = SimpleNamespace(text_audio_encoder=SimpleNamespace(text_encoder=old))
    assert text.install(model) is model and model.text_audio_encoder.text_encoder is old          # default: nothing changes
    text.install(model, fused_text=True)
    new = model.text_audio_encoder.text_encoder
    assert isinstance(new, text.T5TextEncoder) and new.text_model is old.text_model and new.projection is old.projection
    assert new.projection[1].weight is old.projection[1].weight and not new.training
    assert torch.equal(new(texts)[0], emb)
    text.uninstall(model)
    assert model.text_audio_encoder.text_encoder is old


@pytest.mark.parametrize("change, code", [(dict(T=257), -2), (dict(d_ff=2048), -1), (dict(gated_act=1), -1), (dict(n_seq=0), -2)])
def test_unsupported_calls_are_refused_before_any_launch(change, code):
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.conditioning import _engine_handle
    dev = torch.device("cuda:0")
    buf = torch.zeros(1 << 16, device=dev)
    ids = torch.zeros(1024, device=dev, dtype=torch.int32)
    mask = torch.ones(1024, device=dev, dtype=torch.uint8)
    a = _lib.T5Args(wpack=buf.data_ptr(), vocab=1, d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=1, gated_act=0, eps=1e-6, n_seq=1,
                    T=4, ids=ids.data_ptr(), mask=mask.data_ptr(), rel_bias=buf.data_ptr())
    for k, v in change.items():
        setattr(a, k, v)
    h = _engine_handle(dev)
    got = _lib.load().cfd_t5_encode(h, C.byref(a), C.c_void_p(buf.data_ptr()), None)
    assert got == code, (got, _lib.load().cfd_last_error())
    info = torch.zeros(4, device=dev)
    _lib.check(_lib.load().cfd_debug_read(h, b"t5.info", C.c_void_p(info.data_ptr()), 4))
    assert info[0].item() == 0           # launches of the last call
