"""GPU: ``cfd_denoise_guide_pose`` (``Denoiser.guide_pose``) -- one guided update by a key-pose loss in POSE space as a device call --
against the float64 restatement tests/pose_guide_ref.py, and its state on a handle it shares with ``cfd_denoise_guide`` and
``cfd_vae_decode``.

Gates.  feats, d_out, grad and x_new against float64, relative L2 and worst row (``tests/vae_vjp_ref.errors``; feats by 189-wide rows):
8 x the distance of the float32 numpy restatement of the same case from float64, the convention and margin of tests/test_gpu_vae_vjp.py --
the chain (denoiser forward, decoder forward, decoder sweep, denoiser sweep) is longer than either call's, so neither call's absolute gate
is assumed.  The loss: relative 1e-5 (``LOSS_GATE`` of tests/test_gpu_guide.py with the tenfold its issue allowed: the reduction runs over
189 x frames instead of 128 x tokens).  Everything structural -- ties, determinism, reuse, rows independent of the batch, the stale
decode ticket -- is exact.  A worst-row figure is the row's error over the RMS row norm of the whole tensor, so it never rests on a
zero row; every free token's row of the float64 gradient is checked to be non-zero on the CPU.

Measured on an MI355X (relative L2 / worst row, as multiples of the float32 numpy yardstick in brackets):
    minimum  loss 1.8e-8  feats 6.0e-7 / 6.7e-7 (1.70 x / 1.77 x)  d_out 6.9e-7 / 8.1e-7 (1.57 x / 1.56 x)  grad 7.2e-7 / 7.9e-7 (1.52 x / 1.51 x)  x_new 2.6e-8 / 2.8e-8 (1.02 x / 1.02 x)
    ragged   loss 2.7e-8  feats 8.1e-7 / 1.1e-6 (1.51 x / 1.10 x)  d_out 2.0e-6 / 5.4e-6 (0.59 x / 0.47 x)  grad 1.9e-6 / 4.4e-6 (1.48 x / 1.39 x)  x_new 2.7e-8 / 3.3e-8 (1.02 x / 1.06 x)
    product  loss 2.1e-7  feats 7.3e-6 / 1.1e-5 (0.58 x / 0.50 x)  d_out 2.1e-5 / 1.4e-4 (0.70 x / 0.73 x)  grad 2.1e-5 / 6.3e-5 (0.73 x / 0.77 x)  x_new 1.1e-7 / 3.3e-7 (0.74 x / 0.77 x)
    tied     loss 6.2e-8  feats 2.6e-6 / 5.2e-6 (0.90 x / 0.82 x)  d_out 1.1e-5 / 3.3e-5 (0.69 x / 0.67 x)  grad 1.0e-5 / 3.2e-5 (0.64 x / 0.73 x)  x_new 2.9e-8 / 4.1e-8 (0.88 x / 0.77 x)
    rows66   loss 1.4e-8  feats 9.4e-7 / 1.3e-6 (0.90 x / 0.95 x)  d_out 1.3e-6 / 2.5e-6 (1.00 x / 0.89 x)  grad 1.5e-6 / 2.7e-6 (1.00 x / 1.03 x)  x_new 2.5e-8 / 3.2e-8 (1.00 x / 1.00 x)
every call 225 launches on the row-tile engine and 23 on the decoder (173 + 23 reusing the memory side).
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import inputs, vae_weights
from tests import pose_guide_ref
from tests.helpers import state_dict
from tests.test_gpu_guide import S_PRODUCT, S_SMALL, _cfg_case, acp, same
from tests.vae_vjp_ref import errors

pytestmark = pytest.mark.gpu

GATE = 8.0            # x the float32 numpy restatement's own distance from float64
LOSS_GATE = 1e-5
NF, BODY = 189, 69
HANDS = slice(BODY, NF)
ONE_HAND = slice(BODY, BODY + 60)


@functools.lru_cache(maxsize=None)
def pose_case(name):
    """minimum: B = 1, L = 2, n = 2, 16 frames (one chunk per part).  ragged: B = 2, L = 6, n = 3 with row maps, lengths (48, 37) -- a
    ragged last frame tile -- one selected frame beyond row 1's length, hands columns only.  product: B = 1, L = 16, n = 6, 128 frames,
    frame 73, one hand's 60 columns, the default combine.  tied: three windows with ``longform.window_ties(1, 3)`` and one more entry, so
    that token 8 of window 0 has two tokens tied to it; the key frames of window 1 lie in its first half, whose tokens are tied.
    rows66: B = 33, L = 2, n = 2 -- 66 batch rows, bs = 33."""
    from convofusion_amd import longform
    from convofusion_amd.sampler import default_guidance_weights
    rng = np.random.Generator(np.random.PCG64(900 + len(name)))
    tie = None
    if name in ("minimum", "tied", "rows66"):
        B, L, n, S, t, F = dict(minimum=(1, 2, 2, S_SMALL, 5, 16), tied=(3, 16, 2, S_SMALL, 613, 128), rows66=(33, 2, 2, (3, 5, 6, 2, 1), 77, 16))[name]
        inp = inputs.make_plain_batch(seed=800 + len(name), Be=n * B, L=L, S=S, pad_tail=(2, 0, 3, 0, 0))
        uniq, umasks, maps, mems_rows, masks_rows, x = inp["memories"], inp["masks"], None, inp["memories"], inp["masks"], inp["sample"][:B]
        w = np.zeros((B, n), dtype=np.float32)
        w[:, 1] = 7.5
        if name == "tied":
            tie = longform.window_ties(1, 3, L).numpy().copy()
            tie[2, 9] = 0 * L + 8          # a second token on the source of (1, 0)
    else:
        B, L, chunks, S, t, pad, F = dict(ragged=(2, 6, (0, 1, 2), S_SMALL, 250, (2, 0, 3, 0, 0), 48),
                                          product=(1, 16, (0, 1, 2, 3, 4, 5), S_PRODUCT, 433, (5, 0, 7, 0, 0), 128))[name]
        n = len(chunks)
        uniq, umasks, maps, mems_rows, masks_rows, x = _cfg_case(750 + len(name), B, L, S, pad, chunks)
        w = np.tile(np.asarray(default_guidance_weights(7, 7.5), dtype=np.float32)[list(chunks)], (B, 1))
        if name == "ragged":
            w = np.array([[0.0, 0.4, 0.25], [0.0, 1.5, 2.0]], dtype=np.float32)
    lengths = [F] * B
    target = (rng.standard_normal((B, F, NF), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    fm = np.zeros((B, F), dtype=np.float32)
    cm = np.zeros(NF, dtype=np.float32)
    if name == "minimum":
        fm[0, 3] = fm[0, 11] = 1
        cm[:] = 1
    elif name == "ragged":
        lengths = [48, 37]
        fm[0, 5] = fm[0, 47] = fm[1, 20] = fm[1, 40] = 1          # (1, 40) lies beyond row 1's 37 frames
        cm[HANDS] = 1
    elif name == "product":
        fm[0, 73] = 1
        cm[ONE_HAND] = 1
    elif name == "tied":
        fm[0, 100] = fm[1, 10] = fm[1, 40] = fm[2, 90] = 1        # window 1: frames of its tied first half
        cm[:] = 1
    else:
        fm[:, 7] = 1
        cm[:] = 1
    a = acp(t)
    return SimpleNamespace(name=name, B=B, L=L, n=n, t=t, F=F, x=np.ascontiguousarray(x, dtype=np.float32), uniq=uniq, umasks=umasks, maps=maps,
                           mems_rows=mems_rows, masks_rows=masks_rows, w=w, lengths=lengths, target=target, fm=fm, cm=cm, tie=tie, s0=a ** 0.5,
                           s1=(1.0 - a) ** 0.5, inv_n=1.0 / (float(fm.sum()) * float(cm.sum())), step=0.5)


CASES = ("minimum", "ragged", "product", "tied", "rows66")


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64"):
    c = pose_case(name)
    return pose_guide_ref.guide_pose(state_dict(1234, 1.0), vae_weights.make_state_dict(), c.x, c.t, c.mems_rows, c.masks_rows, c.w, c.lengths,
                                     c.target, c.fm, c.cm, c.s0, c.s1, c.inv_n, c.step, tie=c.tie, dtype=np.dtype(dtype))


def vae_model():
    from tests.test_gpu_vae_vjp import _model
    return _model()


@functools.lru_cache(maxsize=None)
def dev_case(name):
    """The case's tensors on the device, made once: their addresses are part of what the library compares."""
    from tests.gpu_helpers import to_dev
    c = pose_case(name)
    return SimpleNamespace(x=to_dev(c.x), mems=[to_dev(m) for m in c.uniq], masks={k: (None if v is None else to_dev(v)) for k, v in c.umasks.items()},
                           maps=None if c.maps is None else [to_dev(r) for r in c.maps], w=to_dev(c.w), target=to_dev(c.target), fm=to_dev(c.fm),
                           cm=to_dev(c.cm), tie=None if c.tie is None else to_dev(c.tie.astype(np.int32)))


ALL = ("loss", "grad", "x_new", "d_out", "feats")


def call(m, name, t=None, reuse=0, step=None, want=ALL, rows=None, fm=None, x_new=None, x=None):
    """One ``Denoiser.guide_pose`` call of the case (``rows``: a slice of its latent rows, with their chunks' memories)."""
    import torch
    c, d = pose_case(name), dev_case(name)
    xs, w, target, fmask, mems, masks, maps, lengths = d.x if x is None else x, d.w, d.target, d.fm if fm is None else fm, d.mems, d.masks, d.maps, c.lengths
    inv_n = c.inv_n
    if rows is not None:
        sel = torch.cat([torch.arange(k * c.B + rows.start, k * c.B + rows.stop) for k in range(c.n)]).to(xs.device)
        xs, w, target, fmask = xs[rows].contiguous(), w[rows].contiguous(), target[rows].contiguous(), fmask[rows].contiguous()
        lengths = lengths[rows]
        if maps is None:
            mems = [e[sel].contiguous() for e in mems]
            masks = {k: (None if v is None else v[sel].contiguous()) for k, v in masks.items()}
        else:
            maps = [r[sel].contiguous() for r in maps]
    tt = c.t if t is None else t
    a = acp(tt)
    return m.guide_pose(xs, tt, mems, masks, w, vae_model(), target, fmask, feature_mask=d.cm, lengths=lengths, sqrt_acp=a ** 0.5,
                        sqrt_1m_acp=(1.0 - a) ** 0.5, step=c.step if step is None else step, inv_n=inv_n, tie=d.tie, row_maps=maps,
                        reuse_memory_side=reuse, want=want, x_new=x_new)


def feats_errors(got, want):
    """``errors`` for rows of 189 features."""
    got, want = np.asarray(got, np.float64).reshape(-1, NF), np.asarray(want, np.float64).reshape(-1, NF)
    err = np.linalg.norm(got - want, axis=-1)
    rms = np.sqrt(float((want * want).sum()) / want.shape[0]) + 1e-300
    return float(np.linalg.norm(err) / (np.linalg.norm(want) + 1e-300)), float(err.max() / rms)


@pytest.mark.parametrize("name", CASES)
def test_guide_pose_matches_float64(name):
    """Fails on a tree without the feature: ``Denoiser.guide_pose`` and the symbol cfd_denoise_guide_pose do not exist there."""
    import torch
    from tests.gpu_helpers import hip_denoiser, read_debug
    m = hip_denoiser(1234, 1.0)
    c = pose_case(name)
    r64, r32 = reference(name), reference(name, "float32")
    # the input constraint, on the CPU: every free token's gradient row is non-zero (a tied token's is 0 by construction)
    free = np.ones(c.B * c.L, dtype=bool) if c.tie is None else c.tie.reshape(-1) < 0
    assert np.linalg.norm(r64["grad"].reshape(-1, 128), axis=1)[free].min() > 0
    got = call(m, name)
    info, vinfo = read_debug(m, "weg.info", (5,)), read_debug(m, "vae.info", (2,))
    loss, grad, x_new, d_out, feats = (v.cpu().numpy() for v in got)
    el = abs(float(loss) - r64["loss"]) / abs(r64["loss"])
    fl = abs(r32["loss"] - r64["loss"]) / abs(r64["loss"])
    line = [f"{name}: B={c.B} L={c.L} n={c.n} F={c.F} t={c.t} launches {int(info[0])} + vae {int(vinfo[0])}; loss {float(loss):.6e} vs float64 "
            f"{el:.2e} (float32 numpy {fl:.2e})"]
    errs, yard = {}, {}
    for key, v in (("feats", feats), ("d_out", d_out), ("grad", grad), ("x_new", x_new)):
        fn = feats_errors if key == "feats" else errors
        errs[key], yard[key] = fn(v, r64[key]), fn(r32[key], r64[key])
        line.append(f"{key} rel L2 {errs[key][0]:.2e} worst row {errs[key][1]:.2e} ({errs[key][0] / yard[key][0]:.2f} x / "
                    f"{errs[key][1] / yard[key][1]:.2f} x of float32 numpy {yard[key][0]:.2e} / {yard[key][1]:.2e})")
    print("; ".join(line))
    assert int(vinfo[0]) == 23                     # the saving decode (12 launches at 5 layers) and its sweep (11)
    assert el <= LOSS_GATE
    for key in errs:
        assert errs[key][0] <= GATE * yard[key][0] and errs[key][1] <= GATE * yard[key][1], key
    for b, nfr in enumerate(c.lengths):
        assert not feats[b, nfr:].any()
    # determinism: a second call returns the same bits of all five outputs; what is not asked for changes nothing of the rest
    assert same(got, call(m, name))
    only = call(m, name, want=("x_new",))
    assert [v is None for v in only] == [True, True, False, True, True] and torch.equal(only[2], got[2])
    # x_new may alias x
    x2 = dev_case(name).x.clone()
    call(m, name, want=("x_new",), x=x2, x_new=x2)
    assert torch.equal(x2, got[2])
    # step 0 with no tie leaves x as it is, bit for bit
    if c.tie is None:
        assert torch.equal(call(m, name, step=0.0, want=("x_new",))[2], dev_case(name).x)


def test_a_row_without_a_selected_frame_does_not_move_and_a_frame_beyond_a_length_pulls_nothing():
    import torch
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    d = dev_case("ragged")
    fm = d.fm.clone()
    fm[0] = 0
    _, grad, x_new, _, _ = call(m, "ragged", fm=fm)
    assert not grad[0].any() and torch.equal(x_new[0], d.x[0]) and bool(grad[1].any())
    # row 1 keeps only its frame beyond the length: it counts target^2 towards the loss and leaves zero gradient
    fm[1] = 0
    fm[1, 40] = 1
    loss, grad, x_new, _, feats = call(m, "ragged", fm=fm)
    c = pose_case("ragged")
    want = c.inv_n * float((c.target[1, 40, HANDS].astype(np.float64) ** 2).sum())
    assert not grad.any() and torch.equal(x_new, d.x) and not feats[1, 37:].any()
    assert abs(float(loss) - want) <= 1e-6 * want


def test_tied_tokens_fold_onto_their_sources_and_follow_them():
    import torch
    from tests import guide_ref
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    c, d = pose_case("tied"), dev_case("tied")
    _, grad, x_new, _, _ = call(m, "tied")
    tie = torch.from_numpy(c.tie.reshape(-1).astype(np.int64)).to(grad.device)
    tied = tie >= 0
    flat_g, flat_x, flat_in = grad.reshape(-1, 128), x_new.reshape(-1, 128), d.x.reshape(-1, 128)
    assert int(tied.sum()) == 17 and not flat_g[tied].any()
    assert torch.equal(flat_x[tied], flat_x[tie[tied]])                      # every tied token is its source, bit for bit
    assert bool((flat_x[~tied] != flat_in[~tied]).any(dim=1).all())          # every free token moved
    assert int((tie == 8).sum()) == 2 and bool(flat_g[8].any())              # one token with two tokens tied to it
    # the gradient of a source is the folded sum of the rows the same call gives on x~ without a tie (ascending, as the kernel sums)
    xt = torch.from_numpy(guide_ref.gather_tie(c.x, c.tie)).to(grad.device)
    a = acp(c.t)
    g_tilde = m.guide_pose(xt, c.t, d.mems, d.masks, d.w, vae_model(), d.target, d.fm, feature_mask=d.cm, lengths=c.lengths, sqrt_acp=a ** 0.5,
                           sqrt_1m_acp=(1.0 - a) ** 0.5, step=c.step, inv_n=c.inv_n, want=("grad",))[1]
    assert np.array_equal(guide_ref.fold(g_tilde.cpu().numpy(), c.tie), grad.cpu().numpy())
    # gradient reaches window 1's tied first half: the sources of those tokens (window 0's second half) carry window 1's key frames
    assert bool(g_tilde.reshape(3, 16, 128)[1, :8].any(dim=1).all())


def test_rows_beyond_64_agree_with_per_utterance_calls_bit_for_bit():
    import torch
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    c = pose_case("rows66")
    assert c.n * c.B == 66
    whole = call(m, "rows66", want=("grad", "x_new", "d_out", "feats"))
    for b in (0, 1, 17, 32):
        part = call(m, "rows66", want=("grad", "x_new", "d_out", "feats"), rows=slice(b, b + 1))
        assert torch.equal(part[1][0], whole[1][b]) and torch.equal(part[2][0], whole[2][b]) and torch.equal(part[4][0], whole[4][b]), b
        assert torch.equal(part[3].reshape(c.n, c.L, 128), whole[3].reshape(c.n, c.B, c.L, 128)[:, b]), b


def test_memory_side_reuse_and_sharing_with_the_latent_guide_call():
    """reuse_memory_side = 2 at another timestep: a fresh call's bits, 52 launches fewer.  The two guide calls share one signature (the
    header says so): a cfd_denoise_guide call between two pose calls and a pose call between two cfd_denoise_guide calls leave every
    result a fresh call's bits, reused or not."""
    from convofusion_amd import _lib
    from tests.gpu_helpers import hip_denoiser, read_debug
    m = hip_denoiser(1234, 1.0)
    memory_side = (2 + 2 * int(m.num_layers)) + (6 * 5 + 2)
    launches = lambda: int(read_debug(m, "weg.info", (5,))[0])
    name = "product"
    c, d = pose_case(name), dev_case(name)
    fresh = {t: call(m, name, t=t) for t in (433, 432)}
    full = launches()
    assert same(call(m, name, t=433, reuse=2), fresh[433]) and launches() == full          # builds the tables: nothing to reuse yet
    assert same(call(m, name, t=432, reuse=2), fresh[432]) and launches() == full - memory_side == full - 52

    def latent(t, reuse):
        a = acp(t)
        tg, mk = d.x * 0.5, (d.x[:, :, 0] * 0 + 1)
        return m.guide(d.x, t, d.mems, d.masks, d.w, tg, mk, sqrt_acp=a ** 0.5, sqrt_1m_acp=(1.0 - a) ** 0.5, step=0.5, row_maps=d.maps,
                       reuse_memory_side=reuse, want=("loss", "grad", "x_new", "d_out"))
    fresh_latent = {t: latent(t, 0) for t in (433, 432)}
    # pose, latent, pose
    assert same(call(m, name, t=433, reuse=2), fresh[433])
    assert same(latent(432, 2), fresh_latent[432])
    assert same(call(m, name, t=432, reuse=2), fresh[432])
    # latent, pose, latent
    assert same(latent(433, 2), fresh_latent[433])
    assert same(call(m, name, t=433, reuse=2), fresh[433])
    assert same(latent(432, 2), fresh_latent[432])
    # a refused pose call between two reused calls costs the second nothing
    call(m, name, t=433, reuse=2)
    before = launches()
    with pytest.raises(_lib.CfdError, match="reuse_memory_side = 1 is not 0 or 2"):
        call(m, name, t=433, reuse=1)
    assert launches() == before
    assert same(call(m, name, t=432, reuse=2), fresh[432]) and launches() == full - memory_side


def test_a_decode_ticket_on_the_same_handle_goes_stale_and_the_sweep_names_this_call():
    import torch
    from convofusion_amd import _lib
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    lib, h = _lib.load(), m.engine(torch.device("cuda"))
    vae = vae_model()
    pack = vae._decoder_pack(torch.device("cuda"))
    z = torch.zeros(2, 1, 1, 128, device="cuda")
    lens = torch.tensor([16], dtype=torch.int32, device="cuda")
    args = _lib.VaeDecodeArgs(pack.data_ptr(), 128, 2, 1024, vae.num_layers, 1, 16, 1, z.data_ptr(), lens.data_ptr())
    ticket = C.c_uint64(0)
    _lib.check(lib.cfd_vae_decode(h, C.byref(args), None, C.byref(ticket), None))
    torch.cuda.synchronize()
    assert ticket.value != 0 and lib.cfd_vae_decode_ticket(h) == ticket.value
    call(m, "minimum", want=("x_new",))
    assert lib.cfd_vae_decode_ticket(h) == 0
    d_feats, d_z = torch.zeros(1, 16, NF, device="cuda"), torch.zeros_like(z)
    code = lib.cfd_vae_decode_sweep(h, ticket.value, d_feats.data_ptr(), d_z.data_ptr(), None)
    msg = lib.cfd_last_error().decode()
    assert code == -3 and "stale" in msg and "cfd_denoise_guide_pose" in msg, msg


def test_library_refuses_before_any_launch_and_names_the_limit():
    import torch
    from convofusion_amd import _lib
    from tests.gpu_helpers import hip_denoiser, read_debug
    m = hip_denoiser(1234, 1.0)
    h = m.engine(torch.device("cuda"))
    lib = _lib.load()
    vae = vae_model()
    pack = vae._decoder_pack(torch.device("cuda"))
    call(m, "minimum")
    before = read_debug(m, "weg.info", (5,)), read_debug(m, "vae.info", (2,))

    def raw(B=1, L=16, n=2, S=(3, 5, 6, 2, 1), t=5, F=128, pose_null=False, **over):
        Be = n * B if n > 0 else 1
        x = torch.zeros(B, L, 128, device="cuda")
        arr, keep = m.pack_memories([torch.zeros(Be, s, 512, device="cuda") for s in S], {})
        w = torch.zeros(B, max(n, 1), device="cuda")
        tie = torch.full((B, L), -1, dtype=torch.int32, device="cuda")
        Fa = max(F, 1)
        tg, fm, cm = torch.zeros(B, Fa, NF, device="cuda"), torch.ones(B, Fa, device="cuda"), torch.ones(NF, device="cuda")
        lens = torch.full((B,), Fa, dtype=torch.int32, device="cuda")
        a = _lib.GuideArgs()
        a.B, a.L, a.n, a.timestep, a.sqrt_acp, a.sqrt_1m_acp = B, L, n, t, 0.9, 0.4
        a.x, a.mem, a.w, a.step = x.data_ptr(), arr, w.data_ptr(), 0.1
        p = _lib.GuidePose(pack.data_ptr(), 128, 2, 1024, vae.num_layers, F, lens.data_ptr(), tg.data_ptr(), fm.data_ptr(), cm.data_ptr(), 1.0 / NF)
        outs = dict(loss=None, grad=C.c_void_p(x.data_ptr()), x_new=None, d_out=None, feats=None)
        for k, v in over.items():
            if k == "tie":
                a.tie = tie.data_ptr()
            elif k in ("args_target", "args_mask"):
                setattr(a, k[5:], x.data_ptr())
            elif k in outs:
                outs[k] = v
            elif k.startswith("pose_"):
                setattr(p, k[5:], v)
            else:
                setattr(a, k, v)
        code = lib.cfd_denoise_guide_pose(h, C.byref(a), None if pose_null else C.byref(p), outs["loss"], outs["grad"], outs["x_new"], outs["d_out"],
                                          outs["feats"], None)
        msg = lib.cfd_last_error().decode()
        assert np.array_equal(read_debug(m, "weg.info", (5,)), before[0]) and np.array_equal(read_debug(m, "vae.info", (2,)), before[1]), msg
        del keep
        return code, msg

    for kw, text in ((dict(L=34, F=256), "n_chunks <= 16 (got 17)"),
                     (dict(B=257, n=1), "Be * L = 4112 token rows exceed guide_max_rows = 4096"),
                     (dict(S=(24, 897, 24, 8, 1)), "1056 padded keys of the five memories together exceed RT_MAX_KEYS = 1024"),
                     (dict(t=1000), "timestep 1000 outside the timestep table"),
                     (dict(n=0), "n = 0 guidance chunks"),
                     (dict(L=15), "L = 15 is odd"),
                     (dict(F=129), "nframes = 129 exceeds 16 * (L / 2) = 128"),
                     (dict(L=32, F=257), "1 <= nframes <= 256 (got 257)"),
                     (dict(F=0), "1 <= nframes <= 256 (got 0)"),
                     (dict(pose_num_layers=4), "odd num_layers <= 9"),
                     (dict(pose_num_heads=4), "2 heads"),
                     (dict(pose_null=True), "pose is NULL"),
                     (dict(pose_wpack=None), "pose->wpack is NULL"),
                     (dict(pose_lengths=None), "pose->lengths is NULL"),
                     (dict(pose_target=None), "pose->target is NULL"),
                     (dict(pose_frame_mask=None), "pose->frame_mask is NULL"),
                     (dict(pose_feature_mask=None), "pose->feature_mask is NULL"),
                     (dict(pose_inv_n=0.0), "inv_n = 0 is not positive"),
                     (dict(args_target=True), "args->target is not NULL"),
                     (dict(args_mask=True), "args->mask is not NULL"),
                     (dict(tie=True), "a tie without its tie_csr"),
                     (dict(reuse_memory_side=1), "reuse_memory_side = 1 is not 0 or 2"),
                     (dict(grad=None), "none of loss, grad, x_new, d_out and feats is asked for")):
        code, msg = raw(**kw)
        assert code == -1 and text in msg, (kw, code, msg)
    # the Python wrapper refuses in the same words' limits before any device work
    x = torch.zeros(1, 16, 128, device="cuda")
    mems = [torch.zeros(2, s, 512, device="cuda") for s in (3, 5, 6, 2, 1)]
    with pytest.raises(NotImplementedError, match="nframes = 136 is not in"):
        m.guide_pose(x, 5, mems, {}, torch.zeros(1, 2, device="cuda"), vae, torch.zeros(1, 136, NF), torch.ones(1, 136), sqrt_acp=0.9,
                     sqrt_1m_acp=0.4, step=0.1)
    assert np.array_equal(read_debug(m, "weg.info", (5,)), before[0])
