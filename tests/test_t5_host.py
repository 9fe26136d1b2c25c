"""CPU: the float64 restatement tests/t5_ref.py against transformers' T5EncoderModel, the fixture tests/golden/t5_enc.npz, and the host
side of convofusion_amd.text (state-dict keys, weight packing, de-duplication, relative-position table, refusals)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import t5_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "t5_enc.npz"))


def hf_model(sd, num_layers):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.T5Config(vocab_size=t5_ref.VOCAB, d_model=t5_ref.D, d_kv=t5_ref.DKV, num_heads=t5_ref.H, d_ff=t5_ref.FF,
                                num_layers=num_layers, feed_forward_proj="relu", dropout_rate=0.0)
    model = transformers.T5EncoderModel(cfg).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("projection.")}, strict=True)
    return model


@pytest.mark.parametrize("name", ["A", "C"])
def test_restatement_matches_transformers_in_float64(name):
    """<= 1e-10 at every position, padded ones included.  (``.double()`` with t5_ref.keep_norm_dtype: transformers' norm squares in
    float32 whatever the module's dtype, which alone would leave 5e-7.)"""
    nl, seed, _, _ = t5_ref.CASES[name]
    sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)
    ids, mask = t5_ref.case_inputs(name)
    model = t5_ref.keep_norm_dtype(hf_model(sd, nl).double())
    with torch.no_grad():
        want = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long()).last_hidden_state.numpy()
    got = t5_ref.encode(sd, ids, mask)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-10
    proj = t5_ref.projection_module(sd).double()
    with torch.no_grad():
        want_p = proj(torch.from_numpy(want)).numpy()
    assert np.abs(t5_ref.project(sd, got) - want_p).max() <= 1e-10


def test_bucket_table_equals_transformers():
    pytest.importorskip("transformers")
    from transformers.models.t5.modeling_t5 import T5Attention
    from convofusion_amd import text
    d = np.arange(-255, 256)
    want = T5Attention._relative_position_bucket(torch.from_numpy(d), bidirectional=True, num_buckets=32, max_distance=128).numpy()
    assert np.array_equal(t5_ref.bucket(d), want)
    assert np.array_equal(text.relative_bucket(torch.from_numpy(d)).numpy(), want)
    assert set(want.tolist()) == set(range(32)) - {16}   # every bucket a distance can have (16 would be a positive distance of 0), the >= 128 cap included


def test_bucket_table_without_transformers():
    """the restatement's and the mirror's bucket functions agree, and the known values hold: exact below 8, the cap from 128 on"""
    from convofusion_amd import text
    d = np.arange(-255, 256)
    b = t5_ref.bucket(d)
    assert np.array_equal(text.relative_bucket(torch.from_numpy(d)).numpy(), b)
    at = lambda x: int(b[x + 255])
    assert [at(x) for x in range(-7, 8)] == [7, 6, 5, 4, 3, 2, 1, 0, 17, 18, 19, 20, 21, 22, 23]
    assert at(-128) == at(-255) == 15 and at(128) == at(255) == 31 and at(8) == at(9) == 24 and at(-8) == 8
    w = torch.arange(32 * 12, dtype=torch.float32).reshape(32, 12)
    tab = text.rel_bias_table(w, 5)
    assert tuple(tab.shape) == (12, 9) and tab[3, 4].item() == w[0, 3].item() and tab[3, 5].item() == w[17, 3].item() and tab[0, 0].item() == w[4, 0].item()


def test_fixture_matches_the_restatement():
    """the stored float32 reference outputs lie within their own recorded error of the float64 restatement (no transformers needed)"""
    for name, (nl, seed, _, _) in t5_ref.CASES.items():
        sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)
        ids, mask = t5_ref.case_inputs(name)
        assert np.array_equal(ids, G[name + "_ids"]) and np.array_equal(mask, G[name + "_mask"])
        want = t5_ref.project(sd, t5_ref.encode(sd, ids, mask))
        stored = G[name + "_out_f32"]
        ss, ps = t5_ref.STORED[name]
        sub = want[::ss, ::ps]
        assert stored.shape == sub.shape
        err = np.abs(stored - sub).max() / np.sqrt((want * want).mean())
        assert err <= float(G[name + "_f32_ref_err_proj"]) * (1 + 1e-6) and float(G[name + "_restatement_err"]) <= 1e-10
        assert 1e-8 < float(G[name + "_f32_ref_err_hidden"]) < 1e-5


def test_mirror_state_dict_keys_equal_the_reference_layout():
    transformers = pytest.importorskip("transformers")
    from convofusion_amd import text
    cfg = transformers.T5Config(vocab_size=t5_ref.VOCAB, d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=2, feed_forward_proj="relu")
    model = transformers.T5EncoderModel(cfg)
    enc = text.T5TextEncoder.from_parts(model, None, torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(768, 512)))
    want = {"text_model." + k for k in model.state_dict()} | {"projection.1.weight", "projection.1.bias"}
    assert set(enc.state_dict()) == want
    assert enc.text_max_length == 200 and enc.latent_dim == 512
    import inspect
    assert str(inspect.signature(text.T5TextEncoder.__init__)) == \
        "(self, modelpath: str, finetune: bool = False, last_hidden_state: bool = False, latent_dim: list = [1, 256], **kwargs) -> None"
    # the stub the GPU tests use carries the same names
    sd = t5_ref.make_state(2, 1, t5_ref.VOCAB)
    assert set(t5_ref.stub_text_model(sd).state_dict()) == set(model.state_dict())


def test_pack_unpack_round_trip_and_invalidation():
    from convofusion_amd import text
    sd = t5_ref.make_state(2, 3, t5_ref.VOCAB)
    model = t5_ref.stub_text_model(sd)
    state = model.state_dict()
    pack = text.pack_weights(state, 2)
    assert pack.dtype == torch.float32 and pack.numel() == text.pack_floats(t5_ref.VOCAB, 2) == 64 * 768 + 2 * 7079424 + 768
    back = text.unpack_weights(pack, t5_ref.VOCAB, 2)
    assert set(back) == {k for k, _ in text.pack_layout(t5_ref.VOCAB, 2)}
    for k, v in back.items():
        assert torch.equal(v, state[k]), k
    # q | k | v lie behind one another: the [2304][768] matrix of the fused product
    off = 64 * 768 + 768
    assert torch.equal(pack[off:off + 3 * 768 * 768].view(2304, 768)[768:1536], state["encoder.block.0.layer.0.SelfAttention.k.weight"])
    with pytest.raises(ValueError):
        text.unpack_weights(pack[:-1], t5_ref.VOCAB, 2)
    bad = dict(state)
    bad["encoder.block.1.layer.1.DenseReluDense.wi.weight"] = torch.zeros(2048, 768)
    with pytest.raises(ValueError):
        text.pack_weights(bad, 2)
    # the pack is made lazily and dropped by repack(), load_state_dict and an in-place update
    enc = text.T5TextEncoder.from_parts(model, None, t5_ref.projection_module(sd))
    assert enc._pack is None
    key, first, _ = enc._packed()
    assert enc._packed()[1] is first
    enc.repack()
    assert enc._pack is None and enc._packed()[1] is not first
    enc.load_state_dict(enc.state_dict())
    assert enc._pack is None
    second = enc._packed()[1]
    with torch.no_grad():
        model.encoder.final_layer_norm.weight.mul_(2.0)
    third = enc._packed()[1]
    assert third is not second and torch.equal(third[-768:], second[-768:] * 2)


def test_install_on_a_module_tree_keeps_the_state_dict_and_uninstall_restores():
    """model, holder and the old encoder are nn.Modules, as in the reference: the kept original must not become a child of the model"""
    import pickle
    from torch import nn
    import convofusion_amd
    from convofusion_amd import text
    sd = t5_ref.make_state(1, 4, 8)

    class Old(nn.Module):
        def __init__(self):
            super().__init__()
            self.text_max_length = 200
            self.tokenizer = None
            self.text_model = t5_ref.stub_text_model(sd)
            self.projection = t5_ref.projection_module(sd)

    model = nn.Module()
    model.text_audio_encoder = nn.Module()
    model.text_audio_encoder.text_encoder = old = Old().eval()
    before = model.state_dict()
    assert any(k.startswith("text_audio_encoder.text_encoder.text_model.") for k in before)
    assert text.install(model) is model and model.text_audio_encoder.text_encoder is old
    text.install(model, fused_text=True)
    new = model.text_audio_encoder.text_encoder
    assert isinstance(new, text.T5TextEncoder) and new.text_model is old.text_model and new.projection is old.projection and not new.training
    assert list(model.state_dict()) == list(before) and [n for n, _ in model.named_children()] == ["text_audio_encoder"]
    assert vars(model)["_cfd_text_encoder"] is old
    model.load_state_dict({k: v.clone() for k, v in before.items()}, strict=True)      # a checkpoint loaded after the swap: strict, and ...
    assert new._pack is None                                                              # ... the mirror's hook saw it
    text.install(model, fused_text=True)                                                  # idempotent
    assert model.text_audio_encoder.text_encoder is new and vars(model)["_cfd_text_encoder"] is old
    assert convofusion_amd.uninstall(model) is model                                      # the package's uninstall puts the original back
    assert model.text_audio_encoder.text_encoder is old and "_cfd_text_encoder" not in vars(model)
    assert list(model.state_dict()) == list(before)
    text.install(model, fused_text=True)
    text.uninstall(model)
    assert model.text_audio_encoder.text_encoder is old
    # the mirror pickles (its load_state_dict hook is a module-level function), without its packed copy
    new._packed()
    again = pickle.loads(pickle.dumps(new))
    assert again._pack is None and set(again.state_dict()) == set(new.state_dict())


def test_relative_bias_update_drops_the_bias_tables():
    from convofusion_amd import text
    sd = t5_ref.make_state(1, 6, 8)
    model = t5_ref.stub_text_model(sd)
    enc = text.T5TextEncoder.from_parts(model, None, t5_ref.projection_module(sd))
    first = enc._rel_bias(5)
    assert enc._rel_bias(5) is first
    w = model.state_dict(keep_vars=True)[text.REL_BIAS_KEY]
    with torch.no_grad():
        w.add_(1.0)                  # in place: same storage, version bump
    second = enc._rel_bias(5)
    assert second is not first and torch.equal(second, first + 1.0)


def test_unique_index():
    from convofusion_amd import text
    uniq, index = text.unique_index(["a", "-", "a", "-", "-", "b", "a"])
    assert uniq == ["a", "-", "b"] and index == [0, 1, 0, 1, 1, 2, 0]
    assert text.unique_index([]) == ([], []) and text.unique_index(["x"]) == (["x"], [0])
    texts = ["s", "n", "s", "n", "n", "n", "s"] + ["l", "n", "n", "l", "n", "n", "l"]
    uniq, index = text.unique_index(texts)
    assert len(uniq) == 3 and [uniq[i] for i in index] == texts


def test_host_refusals():
    from types import SimpleNamespace
    from convofusion_amd import _lib, text
    cfg = t5_ref.stub_text_model(t5_ref.make_state(1, 2, 8)).config
    assert text.check_config(cfg) == (1, 1e-6)
    for change in (dict(d_ff=2048), dict(feed_forward_proj="gated-gelu"), dict(is_gated_act=True), dict(num_layers=13), dict(d_model=512),
                   dict(relative_attention_num_buckets=64)):
        with pytest.raises(ValueError):
            text.check_config(SimpleNamespace(**{**vars(cfg), **change}))
    ok = torch.zeros(2, 4, dtype=torch.long)
    text.check_ids(ok, torch.ones(2, 4), 8)
    for ids, mask in ((ok + 8, torch.ones(2, 4)), (ok - 1, torch.ones(2, 4)), (ok, torch.tensor([[1, 1, 0, 0], [0, 0, 0, 0]])),
                      (torch.zeros(1, 257, dtype=torch.long), torch.ones(1, 257)), (ok, torch.ones(2, 3)), (ok[0], torch.ones(4))):
        with pytest.raises(ValueError):
            text.check_ids(ids, mask, 8)
    sd = t5_ref.make_state(1, 2, 8)
    enc = text.T5TextEncoder.from_parts(t5_ref.stub_text_model(sd), None, t5_ref.projection_module(sd))
    with pytest.raises(NotImplementedError):          # a fresh module is in training mode: inference only
        enc.encode_ids(ok, torch.ones(2, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.eval().encode_ids(ok, torch.ones(2, 4))
    # the C ABI: the struct's layout and the declaration
    assert C.sizeof(_lib.T5Args) == 96 and _lib.T5Args.eps.offset == 36 and _lib.T5Args.ids.offset == 48 and _lib.T5Args.proj_dim.offset == 88
    header = open(os.path.join(ROOT, "include", "cfdenoise.h")).read()
    assert "cfd_t5_encode" in _lib.SYMBOLS and re.search(r"\bint cfd_t5_encode\(cfd_handle h, const cfd_t5_args\* a, float\* out, void\* stream\);", header)


def test_launcher_binds_the_text_encoder_only_on_request():
    import sys
    from convofusion_amd import run, text
    saved = {k: sys.modules.get(k) for k in (run.REF_T5_MODULE, run.REF_DENOISER_MODULE, "diffusers")}
    try:
        sys.modules.pop(run.REF_T5_MODULE, None)
        assert run.REF_T5_MODULE + ".T5TextEncoder" not in run.redirect_targets() and run.REF_T5_MODULE not in sys.modules
        assert run.REF_T5_MODULE + ".T5TextEncoder" in run.redirect_targets(fused_text=True)
        assert sys.modules[run.REF_T5_MODULE].T5TextEncoder is text.T5TextEncoder
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
