"""GPU tests of cfd_vae_encode (csrc/vae_enc.hpp) at every depth and workgroup shape it accepts: odd num_layers 1 - 9 and 1, 2 or 3 chunk
sequences per workgroup (``seqs_per_group``; the kernel's RT = 2, 3, 4 row tiles), through the C ABI with the shape named explicitly and
through ``ConvoFusionVae.encode`` (the automatic choice).

Cases (tests/vae_encode_ref.shape_cases): one (1 sequence), span (4), mix (9, root offsets, an empty batch item), seven (7) -- partial
last groups, a group that spans two batch items, chunks with 16, 5, 1 and 0 valid frames.  Which (num_layers, seqs_per_group) pairs fit
the 160 KiB of LDS is worked out here from a restatement of ve_lds_bytes: depths 1, 3, 5 take 1 - 3, depth 7 takes 1 - 2, depth 9 takes 1.
Every admitted pair and the automatic choice run on mix; one, span and seven run at depths 1, 5 and 9.

Gate of the parity tests: max abs over mu and logvar against the float64 restatement (tests/vae_encode_ref.py), at most 4 x the float32
restatement's own max-abs distance from float64 on the same case and depth (computed here on the CPU), and under the project's 1e-4.

Measured on an MI355X, max abs over mu and logvar against float64 (as a multiple of the float32 restatement's distance); every admitted
seqs_per_group and the automatic choice gave the same bits, so there is one figure per (case, num_layers):
    num_layers      1                 3                 5                 7                 9
    mix     3.5e-06 (1.86 x)  4.2e-06 (1.59 x)  3.2e-06 (1.09 x)  4.7e-06 (1.12 x)  3.7e-06 (0.89 x)
    one     2.7e-06 (1.30 x)                    3.2e-06 (1.09 x)                    5.3e-06 (1.39 x)
    span    2.5e-06 (1.38 x)                    3.8e-06 (1.31 x)                    4.0e-06 (1.23 x)
    seven   3.0e-06 (1.22 x)                    3.5e-06 (1.02 x)                    6.1e-06 (1.67 x)
against the reference's own float32 encode of mix (tests/golden/vae_depths.npz): 3.0e-06 at num_layers 1, 5.5e-06 at 9.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import vae_weights
from tests import vae_encode_ref
from tests.helpers import load_golden
from tests.test_vae_encode_host import ABL, KW

pytestmark = pytest.mark.gpu

CFD_OK, CFD_E_ARG, CFD_E_SHAPE = 0, -1, -2
DEPTHS = (1, 3, 5, 7, 9)
FACTOR = 4.0          # the factor of tests/test_gpu_t5.py and tests/test_gpu_audio.py for a float32 kernel against a float32 restatement
CAP = 1e-4            # the project's bar on mu / logvar (tests/test_gpu_vae_encode.py)
GUARD = 4096          # floats of NaN kept on either side of each output
LDS_MAX = 160 * 1024


def lds_bytes(rt, nb):
    """ve_lds_bytes(rt, nb) restated: x and nb skip tensors of 16 rt rows x (128 + 4) floats, Q | K | V of one head at (64 + 4) floats a
    row, mean and rstd per row, 16 ints of valid-frame counts"""
    rows = 16 * rt
    return 4 * (rows * (132 * (1 + nb) + 3 * 68 + 2) + 16)


def admitted(nl):
    """the seqs_per_group values G (the launcher runs them on RT = G + 1 row tiles) whose workgroup fits LDS at num_layers ``nl``"""
    return tuple(g for g in (1, 2, 3) if lds_bytes(g + 1, (nl - 1) // 2) <= LDS_MAX)


PAIRS = [(nl, g) for nl in DEPTHS for g in admitted(nl)]
REFUSED = [(nl, g) for nl in DEPTHS for g in (1, 2, 3) if g not in admitted(nl)]
# every admitted pair and the automatic choice on mix; the other cases at depths 1, 5 and 9
RUNS = [("mix", nl, g) for nl in DEPTHS for g in admitted(nl) + (0,)]
RUNS += [(name, nl, g) for name in ("one", "span", "seven") for nl in (1, 5, 9) for g in admitted(nl) + (0,)]


@functools.lru_cache(maxsize=None)
def _sd(nl):
    return vae_weights.make_state_dict(num_layers=nl)


@functools.lru_cache(maxsize=None)
def _model(nl):
    import torch
    from convofusion_amd.vae import ConvoFusionVae
    m = ConvoFusionVae(ablation=ABL, **dict(KW, num_layers=nl))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(nl).items()}, strict=True)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _restated(name, nl):
    """(mu, logvar, feats) of the float64 restatement and the float32 restatement's max-abs distance from it, once per (case, depth)"""
    import torch
    f, lens = vae_encode_ref.shape_cases()[name]
    mu, lv, feats = vae_encode_ref.encode(_sd(nl), f, lens, num_layers=nl)
    mu32, lv32, _ = vae_encode_ref.encode(_sd(nl), f, lens, num_layers=nl, dtype=torch.float32)
    assert mu32.dtype == np.float32
    base = max(float(np.abs(mu32 - mu).max()), float(np.abs(lv32 - lv).max()))
    return mu, lv, feats, base


def c_encode(nl, f, lens, spg, check=True):
    """One cfd_vae_encode with seqs_per_group = spg on features ``f`` (numpy or a device tensor).  Both outputs are views into NaN-filled
    buffers with GUARD floats on either side.  Returns (rc, mulv [2 (mu, logvar), 2 (body, hands), n_seq, 128], feats_out, guards intact)."""
    import torch
    from convofusion_amd import _lib
    from convofusion_amd.conditioning import _engine_handle
    dev = torch.device("cuda", torch.cuda.current_device())
    x = (torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f).to(dev).contiguous()
    bs, nframes, nf = x.shape
    n_seq = bs * nframes // 16
    pack = _model(nl)._encoder_pack(dev)
    lens_d = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    mbuf = torch.full((2 * GUARD + 4 * n_seq * 128,), float("nan"), device=dev)
    fbuf = torch.full((2 * GUARD + bs * nframes * nf,), float("nan"), device=dev)
    mulv, feats = mbuf[GUARD:-GUARD].view(2, 2, n_seq, 128), fbuf[GUARD:-GUARD].view(bs, nframes, nf)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = _lib.load().cfd_vae_encode(_engine_handle(dev), ptr(pack), 128, 2, 1024, nl, 1, ptr(x), bs, nframes, x.stride(1), ptr(lens_d),
                                    ptr(mulv), ptr(feats), spg, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if check:
        _lib.check(rc)
    guards = all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all()) for b in (mbuf, fbuf))
    return rc, mulv, feats, guards


@functools.lru_cache(maxsize=None)
def _device(name, nl, spg):
    """(mulv, feats_out, guards intact) of one explicit-shape call on a case, as numpy arrays; shared by the tests that only read them"""
    f, lens = vae_encode_ref.shape_cases()[name]
    _, mulv, feats, guards = c_encode(nl, f, lens, spg)
    return mulv.cpu().numpy(), feats.cpu().numpy(), guards


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name,nl,spg", RUNS)
def test_parity_with_float64(name, nl, spg):
    """mu and logvar of every sequence against the float64 restatement; the returned features bit for bit.  Measured on the MI355X
    (the table at the head of this file): 0.89 x to 1.86 x the float32 restatement's own distance, 2.5e-06 to 6.1e-06 max abs."""
    mu, lv, want_feats, base = _restated(name, nl)
    mulv, feats, _ = _device(name, nl, spg)
    e_mu, e_lv = float(np.abs(mulv[0] - mu).max()), float(np.abs(mulv[1] - lv).max())
    err = max(e_mu, e_lv)
    print(f"{name} num_layers {nl} seqs_per_group {spg}: mu {e_mu:.3e} logvar {e_lv:.3e} max abs vs float64; float32 restatement {base:.3e} "
          f"({err / base:.2f} x)")
    assert np.isfinite(mulv).all()
    assert err <= FACTOR * base and err < CAP
    assert _same_bits(feats, want_feats)


@pytest.mark.parametrize("nl", (1, 9))
def test_restatement_at_this_depth_is_the_reference_s(nl):
    """The device against the imported reference's own float32 outputs at depths 1 and 9 (tests/golden/vae_depths.npz), under the bar of
    tests/test_gpu_vae_encode.py -- the float64 restatement the other tests use is pinned to the same file on the CPU."""
    G = load_golden("vae_depths")
    mulv, feats, _ = _device(vae_encode_ref.DEPTH_CASE, nl, 1)
    e_mu, e_lv = float(np.abs(mulv[0] - G[f"enc{nl}.mu"]).max()), float(np.abs(mulv[1] - G[f"enc{nl}.logvar"]).max())
    print(f"num_layers {nl}: HIP encode vs the reference: mu max abs {e_mu:.3e} logvar {e_lv:.3e}")
    assert e_mu < CAP and e_lv < CAP
    assert _same_bits(feats[..., :3], G[f"enc{nl}.root"])


@pytest.mark.parametrize("name,nl", [("mix", nl) for nl in DEPTHS] + [(n, nl) for n in ("one", "span", "seven") for nl in (1, 5, 9)])
def test_every_workgroup_shape_gives_the_same_bits(name, nl):
    """A row's arithmetic has the same k order (ve_mm) and key order (the attention loop) whatever RT is: mu, logvar and the returned
    features of every admitted seqs_per_group and of the automatic choice are the same bits.  Held on the MI355X for all 12 admitted
    pairs (the library is built with floating-point contraction off, so no instantiation fuses a multiply-add the others do not)."""
    want_m, want_f, _ = _device(name, nl, 1)
    for spg in admitted(nl)[1:] + (0,):
        got_m, got_f, _ = _device(name, nl, spg)
        diff = np.abs(got_m - want_m).max()
        assert _same_bits(got_m, want_m), f"seqs_per_group {spg} vs 1: mu / logvar differ by up to {diff:.3e}"
        assert _same_bits(got_f, want_f), spg


@pytest.mark.parametrize("spg", (3, 1))
def test_a_sequence_does_not_depend_on_its_neighbours(spg):
    """Each sequence of mix encoded alone (bs 1, its own 16 frames, its own valid length) gives the bits of its rows in the full call."""
    nl = 5
    f, lens = vae_encode_ref.shape_cases()["mix"]
    full_m, full_f, _ = _device("mix", nl, spg)
    n_chunks = f.shape[1] // 16
    for sq in range(f.shape[0] * n_chunks):
        b, c = divmod(sq, n_chunks)
        nv = min(max(lens[b] - 16 * c, 0), 16)
        _, m1, f1, guards = c_encode(nl, f[b:b + 1, 16 * c:16 * c + 16], [nv], spg)
        assert guards
        assert _same_bits(m1.cpu().numpy()[:, :, 0], full_m[:, :, sq]), (sq, nv)
        assert _same_bits(f1.cpu().numpy()[0], full_f[b, 16 * c:16 * c + 16]), (sq, nv)


@pytest.mark.parametrize("spg", (3, 1))
def test_masked_frames_are_not_read_as_keys(spg):
    """Frames at or beyond each length overwritten with finite values of order 1e3: mu and logvar keep their bits.  (Frame 0 of a chunk,
    which the root subtraction of the chunk's valid frames reads, is itself valid whenever the chunk has a valid frame, so it stays.)"""
    nl = 5
    f, lens = vae_encode_ref.shape_cases()["mix"]
    g = f.copy()
    rng = np.random.Generator(np.random.PCG64(31))
    changed = 0
    for b, n in enumerate(lens):
        g[b, n:] = (1e3 * rng.standard_normal(g[b, n:].shape)).astype(np.float32)
        changed += f.shape[1] - n
    assert changed == 79 and np.isfinite(g).all()
    _, mulv, feats, guards = c_encode(nl, g, lens, spg)
    want = _device("mix", nl, spg)[0]
    assert guards and _same_bits(mulv.cpu().numpy(), want)
    assert _same_bits(feats.cpu().numpy(), vae_encode_ref.root_subtract(g).numpy())     # the garbage is returned root-subtracted, as the reference would


@pytest.mark.parametrize("name,nl,spg", RUNS)
def test_only_what_belongs_to_the_call_is_written(name, nl, spg):
    """No NaN of the fill is left in mu / logvar of any sequence or in the returned features (a partial last group included), and the
    guard bands on either side of both buffers are still all NaN."""
    mulv, feats, guards = _device(name, nl, spg)
    assert not np.isnan(mulv).any() and not np.isnan(feats).any()
    assert guards


def test_refusals_come_before_any_launch():
    from convofusion_amd import _lib
    f, lens = vae_encode_ref.shape_cases()["mix"]
    asked = [(nl, g, CFD_E_SHAPE) for nl, g in REFUSED] + [(5, 4, CFD_E_ARG), (5, -1, CFD_E_ARG)]
    assert len(asked) == 5
    for nl, spg, want in asked:
        rc, mulv, feats, guards = c_encode(nl, f, lens, spg, check=False)
        msg = _lib.load().cfd_last_error().decode()
        print(f"num_layers {nl} seqs_per_group {spg}: {rc}: {msg}")
        assert rc == want, (nl, spg, rc, msg)
        assert guards and bool(mulv.isnan().all()) and bool(feats.isnan().all())


@pytest.mark.parametrize("nl", (9, 1))
def test_python_path_at_other_depths(nl):
    """``ConvoFusionVae(num_layers=nl).encode`` on mix: the gate of test_parity_with_float64 and the bits of the explicit-shape calls."""
    import torch
    f, lens = vae_encode_ref.shape_cases()["mix"]
    mu, lv, want_feats, base = _restated("mix", nl)
    latent, dist, feats = _model(nl).encode(torch.from_numpy(f).cuda(), lens)
    got_mu, got_lv = dist.mean.cpu().numpy(), (2 * dist.stddev.log()).cpu().numpy()
    err = max(float(np.abs(got_mu - mu).max()), float(np.abs(got_lv - lv).max()))
    print(f"mix num_layers {nl} through encode(): {err:.3e} max abs vs float64 ({err / base:.2f} x the float32 restatement's {base:.3e})")
    assert tuple(latent.shape) == (2, 3, 3, 128)
    assert err <= FACTOR * base and err < CAP
    want_m, want_f, _ = _device("mix", nl, 1)
    assert _same_bits(got_mu, want_m[0])                                    # mu as the kernel wrote it
    assert torch.equal(dist.stddev, torch.from_numpy(want_m[1]).cuda().exp().pow(0.5))   # std = encode's own arithmetic on that logvar
    assert _same_bits(feats.cpu().numpy(), want_f) and _same_bits(want_f, want_feats)
