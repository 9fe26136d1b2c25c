"""CPU tests of the VAE test infrastructure at depths other than 5: the seeded state dict at any odd num_layers, the float64 restatements
of encode (tests/vae_encode_ref.py) and of decode and its sweep (tests/vae_vjp_ref.py) against the imported reference at num_layers 1 and
9 (tests/golden/vae_depths.npz, made by tests/golden/make_golden_vae_depths.py), the packed sizes against the headers' macros, and which
(num_layers, seqs_per_group) pairs the encoder's LDS formula admits."""
import numpy as np
import pytest

from oracle import vae_ref, vae_weights
from tests import vae_encode_ref, vae_vjp_ref
from tests.helpers import load_golden
from tests.test_vae_encode_host import ABL, KW

DEPTHS = (1, 3, 5, 7, 9)


def test_state_dict_follows_the_depth_and_keeps_its_default():
    assert [k for k, _ in vae_weights.key_shapes()] == [k for k, _ in vae_weights.key_shapes(5)] and len(vae_weights.key_shapes()) == 337
    a, b = vae_weights.make_state_dict(), vae_weights.make_state_dict(num_layers=5)
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    for nl in DEPTHS:
        nb = (nl - 1) // 2
        keys = [k for k, _ in vae_weights.key_shapes(nl)]
        # per encoder layer 12 entries, per decoder layer 18, per linear block 2, per stack's norm 2; 5 tokens / PEs, 8 embedding / final
        assert len(keys) == len(set(keys)) == 13 + 2 * (12 * nl + 2 * nb + 2) + 2 * (18 * nl + 2 * nb + 2)
        for part in ("body_encoder.", "hands_decoder."):
            assert (f"{part}input_blocks.{nb - 1}.norm1.weight" in keys) == (nb > 0)
            assert f"{part}input_blocks.{nb}.norm1.weight" not in keys and f"{part}linear_blocks.{nb}.weight" not in keys
            assert f"{part}middle_block.norm1.weight" in keys
    for bad in (0, 4, -1):
        with pytest.raises(ValueError):
            vae_weights.key_shapes(bad)


@pytest.mark.parametrize("nl", DEPTHS)
def test_mirror_loads_the_state_dict_strictly(nl):
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    m = ConvoFusionVae(ablation=ABL, **dict(KW, num_layers=nl))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict(num_layers=nl).items()}, strict=True)


@pytest.mark.parametrize("nl", (1, 9))
def test_encode_restatement_matches_the_reference(nl):
    """num_layers 1: the middle block is the last layer and there is no skip tensor; 9: four skip tensors popped in reverse.  1e-5 max abs:
    the bar of tests/test_vae_encode_host.py."""
    G = load_golden("vae_depths")
    f, lens = vae_encode_ref.shape_cases()[vae_encode_ref.DEPTH_CASE]
    mu, lv, feats = vae_encode_ref.encode(vae_weights.make_state_dict(num_layers=nl), f, lens, num_layers=nl)
    assert mu.shape == G[f"enc{nl}.mu"].shape == (2, 9, 128) and mu.dtype == np.float64
    e_mu, e_lv = float(np.abs(mu - G[f"enc{nl}.mu"]).max()), float(np.abs(lv - G[f"enc{nl}.logvar"]).max())
    print(f"num_layers {nl}: float64 restatement vs the reference's encode: mu {e_mu:.2e} logvar {e_lv:.2e}")
    assert e_mu < 1e-5 and e_lv < 1e-5
    assert np.array_equal(feats[..., :3], G[f"enc{nl}.root"]) and np.array_equal(feats[..., 3:], f[..., 3:])
    assert np.abs(f[:2, :, [0, 2]]).mean() > 40 and np.abs(feats[:2, :, [0, 2]]).mean() < 5          # the root offsets are gone


@pytest.mark.parametrize("nl", (1, 9))
def test_decode_restatements_match_the_reference(nl):
    """The float64 forward and sweep of tests/vae_vjp_ref.py: the forward under 1e-5 max abs of the reference's float32 decode, the sweep
    against the reference's float64 autograd under relative L2 1e-9 -- both sides are float64 (unit round-off 1.1e-16) over at most 9
    layers of 128- to 1024-term sums, so anything above a few thousand round-offs is a different formula.  oracle/vae_ref.decode (float32
    numpy, the checker of the decode tests) under its own 1e-4."""
    G = load_golden("vae_depths")
    sd = vae_weights.make_state_dict(num_layers=nl)
    z, lens, d = vae_vjp_ref.depth_case_inputs()
    feats, d_z, taps = vae_vjp_ref.decode_vjp(sd, z, lens, d, num_layers=nl)
    e_f = float(np.abs(feats - G[f"dec{nl}.feats"]).max())
    rel, row = vae_vjp_ref.errors(d_z, G[f"dec{nl}.grad"])
    e_o = float(np.abs(vae_ref.decode(sd, z, lens, num_layers=nl) - G[f"dec{nl}.feats"]).max())
    print(f"num_layers {nl}: restated decode vs the reference {e_f:.2e}; sweep vs float64 autograd rel L2 {rel:.2e} worst row {row:.2e}; "
          f"oracle.vae_ref {e_o:.2e}")
    assert feats.shape == G[f"dec{nl}.feats"].shape == (2, 40, 189) and e_f < 1e-5 and e_o < 1e-4
    assert d_z.shape == z.shape and rel < 1e-9 and row < 1e-9
    assert not feats[1, 17:].any() and not G[f"dec{nl}.feats"][1, 17:].any()
    assert set(taps) >= {f"{k}.{s}.{l}" for k in ("g", "dz", "x") for s in range(2) for l in range(nl)}


def test_encode_restatement_in_float32():
    """dtype=torch.float32 runs everything behind the root subtraction in float32: a float32 result a float32 distance from float64."""
    import torch
    f, lens = vae_encode_ref.shape_cases()["span"]
    sd = vae_weights.make_state_dict(num_layers=3)
    mu, lv, feats = vae_encode_ref.encode(sd, f, lens, num_layers=3)
    mu32, lv32, feats32 = vae_encode_ref.encode(sd, f, lens, num_layers=3, dtype=torch.float32)
    assert (mu.dtype, mu32.dtype, lv32.dtype, feats32.dtype) == (np.float64, np.float32, np.float32, np.float32)
    assert np.array_equal(feats, feats32)
    for a, b in ((mu32, mu), (lv32, lv)):
        err = float(np.abs(a - b).max())
        assert 1e-8 < err < 1e-5, err          # float32 round-off (6e-8) through 3 layers on values of order 1: neither float64 nor broken


def test_packed_sizes_match_the_headers_at_every_depth():
    from convofusion_amd.vae import decoder_pack_floats, encoder_pack_floats
    D, FF, T = 128, 1024, 18
    # csrc/vae_enc.hpp: VE_LAYER0 = emb W + emb b + 2 tokens + 18 PE rows; VL_SIZE; VE_LIN_SIZE; the final norm
    ve_layer0 = D * D + D + 2 * D + T * D
    vl_size = 2 * D + 3 * D * D + 3 * D + D * D + D + 2 * D + FF * D + FF + D * FF + D
    ve_lin = 2 * D * D + D
    # csrc/vae_dec.hpp: DL_SIZE (every matrix twice: F and T), DLIN_SIZE, DT_SIZE; then 256 + 16 PE rows
    dl_size = (2 * D + 2 * 3 * D * D + 3 * D + 2 * D * D + D) * 2 + 2 * D + 2 * FF * D + FF + 2 * FF * D + D
    dlin, dt = 4 * D * D + D, 2 * D + 2 * D * D + D
    assert (ve_layer0, vl_size, ve_lin, dl_size, dlin, dt) == (19072, 329856, 32896, 789376, 65664, 33152)
    want = {1: (349184, 1679872), 3: (1041792, 4968704), 5: (1734400, 8257536), 7: (2427008, 11546368), 9: (3119616, 14835200)}
    for nl in DEPTHS:
        nb = (nl - 1) // 2
        ve_stack = ve_layer0 + nl * vl_size + nb * ve_lin + 2 * D
        vd_pack = 2 * (nl * dl_size + nb * dlin + dt) + (256 + 16) * D
        assert (ve_stack, vd_pack) == want[nl]
        assert encoder_pack_floats(nl) == ve_stack and decoder_pack_floats(nl) == vd_pack


def test_packs_have_those_sizes():
    """The packers themselves (they assert their own length against *_pack_floats) at the two ends of the range."""
    import torch
    from convofusion_amd.vae import ConvoFusionVae, decoder_pack_floats, encoder_pack_floats
    for nl in (1, 9):
        m = ConvoFusionVae(ablation=ABL, **dict(KW, num_layers=nl)).eval()
        assert m._encoder_pack(torch.device("cpu")).numel() == 2 * encoder_pack_floats(nl)
        assert m._decoder_pack(torch.device("cpu")).numel() == decoder_pack_floats(nl)


def test_admitted_workgroup_shapes_follow_the_lds_formula():
    from tests.test_gpu_vae_encode_shapes import PAIRS, REFUSED, admitted, lds_bytes
    assert lds_bytes(2, 2) == 77120 and lds_bytes(4, 2) == 154176            # 5 layers: what the launcher asks for at RT = 2 and 4
    assert {nl: admitted(nl) for nl in DEPTHS} == {1: (1, 2, 3), 3: (1, 2, 3), 5: (1, 2, 3), 7: (1, 2), 9: (1,)}
    assert REFUSED == [(7, 3), (9, 2), (9, 3)] and len(PAIRS) == 12
