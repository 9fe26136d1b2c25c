"""CPU (-m "not gpu"): per-modality guidance weights on the host -- the accepted forms and their [N][B][8] table, the refusals, the
restated weighted combine against the reference's, the shard slicing, the launcher's CFD_RUN_MODALITY_WEIGHTS and the C prototype of
cfd_sample_begin_weighted."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import modality_ref

N, B, G_SCALE = 5, 3, 7.5


def _table(w, n=N, b=B, g=G_SCALE, chunks=7):
    from convofusion_amd.sampler import modality_weight_table
    t = modality_weight_table(w, g, n, b, chunks)
    assert t.dtype == np.float32 and t.shape == (n, b, 8)
    return t


def _want(rows):
    return modality_ref.weight_table(np.broadcast_to(np.asarray(rows, dtype=np.float64), (N, B, 6)), G_SCALE)


def test_reference_weights_are_the_default_paths_weights():
    """The dict {} / the reference's values give the factors SamplingRun writes into cfd_sample_args.guidance_weight today."""
    from convofusion_amd.sampler import REFERENCE_MODALITY_WEIGHTS, MODALITY_NAMES
    assert MODALITY_NAMES == modality_ref.NAMES
    assert tuple(REFERENCE_MODALITY_WEIGHTS[k] for k in MODALITY_NAMES) == modality_ref.REFERENCE
    want = np.zeros((N, B, 8), dtype=np.float32)
    want[:, :, 1:6] = np.float32(7.5)
    for form in ({}, dict(REFERENCE_MODALITY_WEIGHTS), [1, 1, 1, 1, 1, 0], torch.tensor([1.0, 1, 1, 1, 1, 0])):
        assert np.array_equal(_table(form), want) and not np.signbit(_table(form)).any()


@pytest.mark.parametrize("form", ["dict", "row", "row_tensor", "per_utt", "per_utt_f32", "schedule", "schedule_bcast"])
def test_every_form_broadcasts_to_the_table_bit_for_bit(form):
    rng = np.random.default_rng(3)
    sched = rng.uniform(-1.0, 3.0, size=(N, B, 6))
    sched[:, :, 3] = 0.0
    if form == "dict":
        w, rows = dict(text=2, audio=0.5, lsnid=1.25), (2.0, 0.5, 1.0, 1.0, 1.25, 0.0)
    elif form == "row":
        rows = (0.3, 0.0, 1.7, 2.0, 0.1, 0.9)
        w = np.array(rows)
    elif form == "row_tensor":
        rows = (0.3, 0.0, 1.7, 2.0, 0.1, 0.9)
        w = torch.tensor(rows, dtype=torch.float64)
    elif form == "per_utt":
        rows = sched[0]
        w = rows.tolist()
    elif form == "per_utt_f32":        # float32 weights are taken exactly (float32 -> double is exact)
        rows = sched[0].astype(np.float32).astype(np.float64)
        w = torch.from_numpy(sched[0].astype(np.float32))
    elif form == "schedule":
        rows, w = sched, torch.from_numpy(sched)
    else:
        rows, w = np.broadcast_to(sched[:, :1], (N, B, 6)), sched[:, :1]
    got = _table(w)
    want = _want(rows)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # column 0 (the unconditional chunk) and column 7 (no chunk) stay 0
    assert got[0, 0, 0] == 0.0 and np.all(got[..., 7] == 0.0)


def test_the_product_is_taken_in_double():
    w = 1 / 7 + 1e-9              # float32(7.5 * w) differs from float32(7.5) * float32(w) here
    got = _table([w, 1, 1, 1, 1, 0])[0, 0, 1]
    assert got == np.float32(7.5 * w)
    assert np.float32(np.float32(7.5) * np.float32(w)) != np.float32(7.5 * w)


@pytest.mark.parametrize("bad", [
    dict(txt=1.0), dict(text=float("nan")), dict(audio=float("inf")), dict(text="x"), [1, 1, 1, 1, 1], np.ones((B + 1, 6)),
    np.ones((N + 1, B, 6)), np.ones((N, 2, 6)), np.ones((1, N, B, 6)), np.ones((N, B, 7)), [1, 1, float("nan"), 1, 1, 0],
    torch.tensor([[1.0, 1, 1, 1, 1, float("inf")]] * B), "text=1", 3.0])
def test_refusals(bad):
    with pytest.raises(ValueError):
        _table(bad)


def test_refusals_of_the_run_shape():
    with pytest.raises(ValueError):
        _table({}, chunks=1)
    with pytest.raises(ValueError):
        _table({}, chunks=6)
    with pytest.raises(ValueError):                # guidance_scale * w beyond float32
        _table([1e38, 1, 1, 1, 1, 0], g=1e3)
    from convofusion_amd.sampler import check_modality_weights
    assert check_modality_weights(None) is None
    assert check_modality_weights(dict(all=1)) == dict(text=1.0, audio=1.0, spk=1.0, apb=1.0, lsnid=1.0, all=1.0)
    with pytest.raises(ValueError):
        check_modality_weights(np.ones((2, 3, 4, 6)))


def test_restated_combine_with_reference_weights_equals_the_oracle_bit_for_bit():
    from oracle import sampler_ref
    rng = np.random.default_rng(11)
    Bc, L = 4, 16
    noise_pred = rng.standard_normal((7 * Bc, L, 128)).astype(np.float32)
    noise_pred[3 * Bc:4 * Bc] *= np.float32(1e-3)       # (differences of mixed magnitude)
    table = modality_ref.weight_table(np.broadcast_to(np.array(modality_ref.REFERENCE), (1, Bc, 6)), 7.5)
    got = modality_ref.cfg_combine_weighted(noise_pred, table[0])
    want = sampler_ref.cfg_combine(noise_pred, 7.5)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # per-utterance factors: row b uses its own
    w = np.zeros((1, Bc, 6))
    w[0, 2] = (1, 0, 0, 0, 0, 0)
    got = modality_ref.cfg_combine_weighted(noise_pred, modality_ref.weight_table(w, 2.0)[0])
    u, t = noise_pred[:Bc], noise_pred[Bc:2 * Bc]
    assert np.array_equal(got[2], u[2] + np.float32(2.0) * (t[2] - u[2])) and np.array_equal(got[[0, 1, 3]], u[[0, 1, 3]])


def test_golden_weights_schedule():
    w = modality_ref.golden_weights(20)
    on = [i for i in range(20) if w[i, 0].any()]
    assert on == list(range(6, 14))                       # iterations [0.3 N, 0.7 N)
    assert np.all(w[:, :, 3] == 0) and np.all(np.diff(w[:, 1, 0]) > 0)


def test_shard_slicing():
    from convofusion_amd.distributed import sample_sharded, shard_modality_weights
    total = 5
    sched = np.arange(4 * total * 6, dtype=np.float64).reshape(4, total, 6)
    per = sched[0]
    assert shard_modality_weights(None, 1, 3, total) is None
    assert shard_modality_weights(dict(text=2), 1, 3, total) == dict(text=2)
    assert np.array_equal(shard_modality_weights(per[0], 1, 3, total), per[0])
    assert np.array_equal(shard_modality_weights(per, 1, 3, total), per[1:3])
    assert np.array_equal(shard_modality_weights(torch.from_numpy(sched), 2, 5, total).numpy(), sched[:, 2:5])
    assert np.array_equal(shard_modality_weights(sched[:, :1], 2, 5, total), sched[:, :1])
    with pytest.raises(ValueError):
        shard_modality_weights(per[:4], 0, 2, total)
    with pytest.raises(ValueError):
        shard_modality_weights(sched[:, :3], 0, 2, total)
    seen = {}

    def fn(enc, masks, B, first_utterance, **kw):
        seen.update(kw, B=B, first=first_utterance)
        return torch.zeros((B, 16, 128))

    enc = [torch.zeros((7 * total, 3, 512)) for _ in range(5)]
    sample_sharded(fn, enc, {}, total)
    assert seen == dict(B=total, first=0)                 # no keyword when no weights are given (unchanged call)
    sample_sharded(fn, enc, {}, total, modality_weights=per)
    assert np.array_equal(seen["modality_weights"], per)


def test_launcher_parses_the_environment_variable():
    from convofusion_amd.run import parse_modality_weights
    assert parse_modality_weights(None) is None and parse_modality_weights("") is None and parse_modality_weights("  ") is None
    assert parse_modality_weights("text=2,audio=0.5") == dict(text=2.0, audio=0.5)
    assert parse_modality_weights(" all = 1 , lsnid=0, ") == dict(all=1.0, lsnid=0.0)
    for bad in ("text", "text=x", "txt=1", "text=1,text=2", "=1", "text=nan", "audio=inf"):
        with pytest.raises(ValueError):
            parse_modality_weights(bad)


def test_install_keeps_the_weights():
    import convofusion_amd
    from types import SimpleNamespace
    from convofusion_amd.denoiser import Denoiser
    from convofusion_amd.scheduler import DDPMScheduler
    from tests.gpu_helpers import ABL, DENOISER_KW
    model = SimpleNamespace(denoiser=Denoiser(ablation=ABL, **DENOISER_KW), scheduler=DDPMScheduler())
    convofusion_amd.install(model, modality_weights=dict(text=2))
    assert model._cfd_modality_weights == dict(text=2.0, audio=1.0, spk=1.0, apb=1.0, lsnid=1.0, all=0.0)
    convofusion_amd.uninstall(model)
    assert not hasattr(model, "_cfd_modality_weights")
    with pytest.raises(ValueError):
        convofusion_amd.install(model, modality_weights=dict(speaker=1))
    convofusion_amd.install(model)
    assert model._cfd_modality_weights is None


def test_ctypes_prototype_of_the_weighted_entry_point():
    from convofusion_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert "cfd_sample_begin_weighted" in _lib.SYMBOLS
    fn = lib.cfd_sample_begin_weighted
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.POINTER(_lib.SampleArgs), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    # (a null handle is refused before anything touches a device)
    assert fn(None, None, None, 1, None, None) == -1
    assert b"null" in lib.cfd_last_error()
