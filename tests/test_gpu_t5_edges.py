"""GPU tests: the edges of cfd_t5_encode through the public call (convofusion_amd.text) and the C ABI -- t5-base's twelve blocks, T5_MAX_T,
masks with holes, refusals, stray ids, a sequence without a key.  The float64 reference is tests/t5_ref.py; the end-to-end gates' base
comes from tests/golden/t5_edges.npz (transformers' own float32 loss on the same case, make_golden_t5_edges.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import t5_ref

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "t5_edges.npz"))
FACTOR = 4.0      # as tests/test_gpu_t5.py


def make_encoder(sd):
    from convofusion_amd.text import T5TextEncoder
    return T5TextEncoder.from_parts(t5_ref.stub_text_model(sd), None, t5_ref.projection_module(sd)).cuda().eval()


def encode(enc, ids, mask, project=True):
    import torch
    return enc.encode_ids(torch.from_numpy(np.ascontiguousarray(ids)), torch.from_numpy(np.ascontiguousarray(mask)), project=project).cpu().numpy()


def t5_info():
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.conditioning import _engine_handle
    dev = torch.device("cuda", torch.cuda.current_device())
    info = torch.zeros(4, device=dev)
    _lib.check(_lib.load().cfd_debug_read(_engine_handle(dev), b"t5.info", C.c_void_p(info.data_ptr()), 4))
    return [int(v) for v in info.tolist()]


def direct_call(enc, ids, mask, project=True):
    """cfd_t5_encode on the encoder's own packed weights and bias table, WITHOUT the host's checks of ids and mask (text.check_ids)"""
    import torch
    from convofusion_amd import _lib, text
    from convofusion_amd.conditioning import _engine_handle
    dev = enc._device()
    num_layers, eps = text.check_config(enc.text_model.config)
    _, pack, _ = enc._packed()
    n_seq, T = ids.shape
    ids_d = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
    mask_d = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(dev)
    bias = enc._rel_bias(T)
    lin = enc.projection[1]
    w, b = lin.weight.detach().float().contiguous(), lin.bias.detach().float().contiguous()
    a = _lib.T5Args(wpack=pack.data_ptr(), vocab=t5_ref.VOCAB, d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=num_layers, gated_act=0,
                    eps=eps, n_seq=n_seq, T=T, ids=ids_d.data_ptr(), mask=mask_d.data_ptr(), rel_bias=bias.data_ptr())
    if project:
        a.proj_w, a.proj_b, a.proj_dim = w.data_ptr(), b.data_ptr(), w.shape[0]
    out = torch.empty(n_seq, T, w.shape[0] if project else 768, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().cfd_t5_encode(_engine_handle(dev), C.byref(a), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["L12", "T256", "H"])
def test_end_to_end_parity_at_the_edges(name):
    """L12: twelve blocks (t5-base's depth; blocks are addressed up to T5_MAX_LAYERS), 2 sequences at T = 9, one padded, 61 launches.
    T256: T5_MAX_T, lengths 256 and 193.  H: the three masks with holes at T = 129.  Last hidden state and projected output against the
    float64 restatement at every position; gate 4 x the reference's own float32 loss on the case (fixture).

    Measured on the MI355X (hidden / projected): L12 2.64e-6 / 2.48e-6 (gates 1.19e-5 / 1.24e-5), T256 1.44e-6 / 1.78e-6
    (7.33e-6 / 9.73e-6), H 1.69e-6 / 1.72e-6 (7.10e-6 / 9.12e-6)."""
    nl, seed, _, T = t5_ref.EDGE_CASES[name]
    sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)              # (not cached: twelve blocks are 340 MB)
    ids, mask = t5_ref.edge_inputs(name)
    assert np.array_equal(ids, G[name + "_ids"]) and np.array_equal(mask, G[name + "_mask"])
    hidden = t5_ref.encode(sd, ids, mask)
    proj = t5_ref.project(sd, hidden)
    assert np.isfinite(proj).all()
    enc = make_encoder(sd)
    e_h = t5_ref.rel_err(encode(enc, ids, mask, project=False), hidden)
    e_p = t5_ref.rel_err(encode(enc, ids, mask, project=True), proj)
    assert t5_info()[:2] == [5 * nl + 1, ids.size] and (name != "L12" or t5_info()[0] == 61)
    g_h, g_p = FACTOR * float(G[name + "_f32_ref_err_hidden"]), FACTOR * float(G[name + "_f32_ref_err_proj"])
    print(f"case {name}: hidden {e_h:.3e} (gate {g_h:.3e}), projected {e_p:.3e} (gate {g_p:.3e})")
    assert e_h <= g_h and e_p <= g_p, (e_h, g_h, e_p, g_p)


@pytest.mark.parametrize("change, code", [(dict(num_layers=13), -1), (dict(num_layers=0), -1), (dict(proj_dim=96), -1), (dict(proj_b=None), -1)])
def test_more_unsupported_calls_are_refused_before_any_launch(change, code):
    """One block past T5_MAX_LAYERS, no block, a projection width that is no multiple of 64, a projection without its bias."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.conditioning import _engine_handle
    dev = torch.device("cuda:0")
    buf = torch.zeros(1 << 16, device=dev)
    ids = torch.zeros(1024, device=dev, dtype=torch.int32)
    mask = torch.ones(1024, device=dev, dtype=torch.uint8)
    a = _lib.T5Args(wpack=buf.data_ptr(), vocab=1, d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=1, gated_act=0, eps=1e-6, n_seq=1,
                    T=4, ids=ids.data_ptr(), mask=mask.data_ptr(), rel_bias=buf.data_ptr(), proj_w=buf.data_ptr(), proj_b=buf.data_ptr(), proj_dim=64)
    for k, v in change.items():
        setattr(a, k, v)
    h = _engine_handle(dev)
    got = _lib.load().cfd_t5_encode(h, C.byref(a), C.c_void_p(buf.data_ptr()), None)
    assert got == code, (got, _lib.load().cfd_last_error())
    info = torch.zeros(4, device=dev)
    _lib.check(_lib.load().cfd_debug_read(h, b"t5.info", C.c_void_p(info.data_ptr()), 4))
    assert info[0].item() == 0           # launches of the last call


def test_a_stray_id_reads_the_nearest_row_of_the_table():
    """Python refuses ids outside the vocabulary; a caller of the C ABI may pass one.  T5GemmArgs::id_max clamps it: a negative id reads
    row 0, one past the table row vocab - 1 -- in the q | k | v product's rows and in the residual of the first block alike."""
    sd = t5_ref.make_state(1, 24, t5_ref.VOCAB)
    enc = make_encoder(sd)
    ids, mask = t5_ref.prefix_inputs(3600, (6, 3), 6)
    stray, clamped = ids.copy(), ids.copy()
    stray[0, :2], clamped[0, :2] = (-5, t5_ref.VOCAB + 7), (0, t5_ref.VOCAB - 1)
    stray[1, 1], clamped[1, 1] = np.iinfo(np.int32).max, t5_ref.VOCAB - 1
    stray[1, 2], clamped[1, 2] = np.iinfo(np.int32).min, 0
    want = encode(enc, clamped, mask)
    assert np.array_equal(direct_call(enc, clamped, mask), want)
    assert np.array_equal(direct_call(enc, stray, mask), want)
    assert np.array_equal(direct_call(enc, stray, mask, project=False), encode(enc, clamped, mask, project=False))
    assert not np.array_equal(direct_call(enc, ids, mask), want)       # (the replaced ids do matter)


def test_a_sequence_without_a_key_is_nan_and_leaves_the_others_alone():
    """t5_attn_kernel: "a sequence with no key at all gives NaN rows" (0 x 1 / 0 at the end of the empty softmax; every read is in bounds).  Python refuses
    such a mask, the C ABI does not: every value of that sequence is NaN, and the other sequences have the bits they have when that
    sequence holds one token."""
    sd = t5_ref.make_state(1, 24, t5_ref.VOCAB)
    enc = make_encoder(sd)
    ids, mask = t5_ref.prefix_inputs(3601, (70, 1, 33), 70)            # (two key tiles; the middle sequence loses its only key)
    want = encode(enc, ids, mask)
    empty = mask.copy()
    empty[1] = 0
    for project in (True, False):
        got = direct_call(enc, ids, empty, project=project)
        assert np.isnan(got[1]).all()
        assert np.array_equal(got[[0, 2]], encode(enc, ids, mask, project=project)[[0, 2]]) and np.isfinite(got[[0, 2]]).all()
    assert np.isfinite(want).all()
    ref = t5_ref.stage_attn(sd, t5_ref.stage_qkv(sd, 0, sd["shared.weight"][ids]), empty, 70)
    assert np.isnan(ref[1]).all() and np.isfinite(ref[[0, 2]]).all()   # the restatement says the same
