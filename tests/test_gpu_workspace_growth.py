"""-m gpu: a one-call unit's result does not depend on how its workspace came to be large enough -- tests/test_gpu_workspace.py's
question, asked of the units that size, grow and carve a workspace of their own through ``carve`` / ``DBuf::grow`` (csrc/owned.hpp).

Every case runs three calls on a fresh handle: a small call on the exactly sized workspace, a larger call that must grow it, and the
small call again over the larger allocation.  The two small results are equal bit for bit, and equal to the same call on the suite's
cached handle, whose workspaces have by then grown through whatever ran before.  Growth is asserted, not assumed: by the workspace-bytes
field of "audio.info" / "t5.info" / "metrics.info", and for the units without one by the process's live device buffers
(cfd_debug_live_buffers), which the larger call must raise and the small call behind it must leave alone.

The units on the engine handle (audio, onsets, T5, motion evaluation, diversity, the fused VAE decode and its VJP) get a fresh handle in
``conditioning._engine_handle.cache`` for the case; cfd_denoise_guide, cfd_denoise_vjp_mem and cfd_weg_step a ``Denoiser`` of their own.
Shapes, weights and inputs are those of each unit's own test file, at its smallest case and the next size up.  Bits only: no tolerance."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _live_bytes():
    from convofusion_amd import _lib
    n, nbytes = C.c_longlong(-1), C.c_longlong(-1)
    _lib.check(_lib.load().cfd_debug_live_buffers(C.byref(n), C.byref(nbytes)))
    return int(nbytes.value)


@contextlib.contextmanager
def fresh_engine_handle():
    """A new engine handle in place of the cached one; the cached one comes back and the new one is released afterwards."""
    import torch
    from convofusion_amd import _lib, conditioning
    idx = torch.cuda.current_device()
    cached = conditioning._engine_handle(torch.device("cuda", idx))      # (made here when no test before this one asked for it)
    fresh = _lib.create_handle(idx)
    conditioning._engine_handle.cache[idx] = fresh
    try:
        yield fresh
    finally:
        conditioning._engine_handle.cache[idx] = cached
        torch.cuda.synchronize()
        _lib.load().cfd_destroy(fresh)


def _same(a, b):
    import torch
    assert len(a) == len(b)
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


def _small_large_small(small, large, ws_bytes):
    """The three calls on the handle in use; returns the two small results.  ``ws_bytes``: the read-out growth is asserted by."""
    import torch
    first = small()
    torch.cuda.synchronize()
    exact = ws_bytes()
    assert exact > 0
    large()
    torch.cuda.synchronize()
    grown = ws_bytes()
    assert grown > exact, (exact, grown)
    again = small()
    torch.cuda.synchronize()
    assert ws_bytes() == grown
    return first, again


def _on_a_fresh_engine_handle(small, large, ws_bytes):
    want = small()                                  # the suite's cached handle
    with fresh_engine_handle():
        first, again = _small_large_small(small, large, ws_bytes)
    assert _same(first, again), "the small call depends on the allocation it runs in"
    assert _same(first, want), "a fresh handle and the cached one disagree"


def _waves(n_wave, n_samples, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn(n_wave, n_samples, generator=g)).cuda()


# ---------------------------------------------------------------- the engine handle's units
def test_audio_encode():
    from tests.test_gpu_audio import audio_info, front_end
    fe = front_end("small")
    small_y, large_y = _waves(1, 500, 1), _waves(4, 4000, 2)

    def call(y):
        r = fe.forward(y, normalize=True)
        return r.mel, r.memory, r.activity, r.peak

    _on_a_fresh_engine_handle(lambda: call(small_y), lambda: call(large_y), lambda: audio_info()[3])


def test_audio_onsets():
    import torch
    from tests import onset_ref
    from tests.test_gpu_onsets import audio_info, detector, dev
    det = detector(small=True)
    small_y = dev(onset_ref.swell_wave()[None])                                      # 4096 samples, the shortest clip of the unit's tests
    large_y = dev(np.stack([onset_ref.swell_wave(n=8192, seed=40 + u) for u in range(4)]))

    def call(y):
        r = det.forward(y)
        torch.cuda.synchronize()
        n = int(r.n_total.item())                                                     # (entries behind the last onset are not written)
        return r.csr[0], r.csr[1][:n], r.frames_raw[:n], r.frames[:n], r.envelope, r.rms, r.n_total

    _on_a_fresh_engine_handle(lambda: call(small_y), lambda: call(large_y), lambda: audio_info()[3])


def test_t5_encode():
    import torch
    from tests import t5_ref
    from tests.test_gpu_t5 import encoder, t5_info
    enc = encoder("C")                                                                # one layer, seeded weights
    assert t5_ref.CASES["C"][0] == 1

    def inputs_of(lens, T, seed):
        r = np.random.RandomState(seed)
        ids, mask = np.zeros((len(lens), T), np.int32), np.zeros((len(lens), T), np.uint8)
        for s, n in enumerate(lens):
            ids[s, :n], mask[s, :n] = r.randint(1, t5_ref.VOCAB, n), 1
        return torch.from_numpy(ids), torch.from_numpy(mask)

    small_in, large_in = inputs_of((5,), 5, 3), inputs_of((70, 33, 1), 70, 4)        # 5 rows; 210 rows across three 64-row blocks
    _on_a_fresh_engine_handle(lambda: (enc.encode_ids(*small_in),), lambda: (enc.encode_ids(*large_in),), lambda: t5_info()[2])


def test_motion_eval_with_the_embedding():
    from convofusion_amd import metrics
    from tests.test_gpu_metrics import batch, dev, metrics_info, small_net
    net = small_net()                                                                 # feature_length 12
    pred = dev(batch(128)[0])

    def call(n):
        r = metrics.motion_eval(pred[:n].contiguous(), fgd_net=net, want={"l1div", "embedding"})
        return r["l1div"], r["embedding"]

    _on_a_fresh_engine_handle(lambda: call(1), lambda: call(3), lambda: metrics_info()[2])


def test_motion_diversity():
    import torch
    from convofusion_amd import metrics
    from tests.test_gpu_metrics import metrics_info
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(40, 333, generator=g).cuda()                                   # n = 40: 3 x 3 tiles of 16 rows; n = 2: one
    _on_a_fresh_engine_handle(lambda: (metrics.diversity(rows[:2].contiguous()),), lambda: (metrics.diversity(rows),), lambda: metrics_info()[2])


@pytest.mark.parametrize("which", ["decode_fused", "decode_vjp"])
def test_vae_decode(which):
    import torch
    from tests.test_gpu_vae_depths import _model
    m = _model(1)

    def inputs_of(bs, lens, n_chunks, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(2, bs, n_chunks, 128, generator=g).cuda(), lens, torch.randn(bs, max(lens), 189, generator=g).cuda()

    small_in, large_in = inputs_of(1, [16], 1, 6), inputs_of(2, [48, 33], 3, 7)

    def call(z, lens, d):
        if which == "decode_vjp":
            return m.decode_vjp(z, lens, d)
        with torch.no_grad():
            return (m.decode(z, lens, fused=True),)

    _on_a_fresh_engine_handle(lambda: call(*small_in), lambda: call(*large_in), _live_bytes)


# ---------------------------------------------------------------- the gradient engine's callers, on a Denoiser of their own
def _on_a_fresh_denoiser(small, large):
    """small(m), large(m): the calls on Denoiser ``m``"""
    from tests.gpu_helpers import hip_denoiser
    want = small(hip_denoiser(1234, 1.0))
    m = hip_denoiser.__wrapped__(1234, 1.0)
    first, again = _small_large_small(lambda: small(m), lambda: large(m), _live_bytes)
    assert _same(first, again), "the small call depends on the allocation it runs in"
    assert _same(first, want), "a fresh handle and the cached one disagree"


def test_denoise_guide():
    from tests.test_gpu_guide import call
    # two_tokens: B = 1, L = 2, n = 2; len18_t0: B = 2, L = 18, n = 3 with row maps
    _on_a_fresh_denoiser(lambda m: call(m, "two_tokens"), lambda m: call(m, "len18_t0"))


def test_denoise_vjp_mem():
    from oracle import inputs
    from tests.gpu_helpers import dev_inputs, to_dev
    from tests.test_gpu_mem_vjp import MEM_NAMES, cotangent, dev_case, mem_case
    t = mem_case("tiny")[1]                                                           # B = 1, L = 4, S = (3, 5, 6, 2, 1)
    x1, mems1, masks1, _ = dev_case("tiny")
    two = inputs.make_plain_batch(seed=54, Be=2, L=4, S=(3, 5, 6, 2, 1), pad_tail=(1, 0, 2, 0, 0))
    x2, (mems2, masks2) = to_dev(two["sample"]), dev_inputs(two)
    c1, c2 = to_dev(cotangent("tiny", tuple(x1.shape))), to_dev(cotangent("two", tuple(x2.shape)))

    def call(m, x, mems, masks, c):
        out, grad, d_mem = m.vjp_memories(x, t, mems, masks, c)
        return (out, grad, *[d_mem[k] for k in MEM_NAMES])

    _on_a_fresh_denoiser(lambda m: call(m, x1, mems1, masks1, c1), lambda m: call(m, x2, mems2, masks2, c2))


def test_weg_step():
    import torch
    from convofusion_amd import weg
    from tests.gpu_helpers import dev_inputs, to_dev
    from tests.test_gpu_weg_rows import _grad_case
    inp, t, _, focus = _grad_case(12)                                                 # L = 16, S = (6, 20, 12, 8, 1)
    mems, masks = dev_inputs(inp)
    x = to_dev(inp["sample"])

    def call(m, B):
        mb, kb = [v[:B].contiguous() for v in mems], {k: (v[:B].contiguous() if v is not None else None) for k, v in masks.items()}
        losses, mx, grad = weg.loss_and_grad_rows(m, x[:B].contiguous(), t, mb, kb, focus[:B])
        return torch.from_numpy(np.asarray(losses)), grad, torch.stack([v for row in mx for v in row])

    _on_a_fresh_denoiser(lambda m: call(m, 1), lambda m: call(m, 2))
