"""GPU tests: motion evaluation in HIP (cfd_motion_eval, cfd_motion_diversity, convofusion_amd/metrics.py) against the float64 restatement
tests/metrics_ref.py and the reference's recorded outputs (tests/golden/metrics.npz).  Beat masks and SRGR counts must be EQUAL (the seeded
inputs carry no knife-edge decision: tests/test_oracle_metrics.py); a real-valued output may lie at most FACTOR = 4 x as far from the
float64 restatement as the float32 restatement of the same formulas does on the same input, a distance measured by the generator and
stored in the fixture.  No entry is excluded anywhere.  Measured distances are printed."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import metrics_ref as R

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics.npz"))
FACTOR = R.FACTOR
E_ARG, E_SHAPE = -1, -2
NET_SEED, PACK_SEED = 41, 43


def _handle():
    import torch
    from convofusion_amd.conditioning import _engine_handle
    return _engine_handle(torch.device("cuda", torch.cuda.current_device()))


def metrics_info():
    """cfd_debug_read "metrics.info": launches of the last call (0: refused), sequences, workspace bytes"""
    import torch
    from convofusion_amd import _lib
    info = torch.zeros(3, device="cuda")
    _lib.check(_lib.load().cfd_debug_read(_handle(), b"metrics.info", C.c_void_p(info.data_ptr()), 3))
    return [int(v) for v in info.tolist()]


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def seeds(T):
    return [int(s) for s in G[f"T{T}_seeds"]]


@functools.lru_cache(maxsize=None)
def batch(T):
    """(pred, target, semantic) float32 of the case's sequences, and their onset lists; shared, read-only"""
    ss = seeds(T)
    return (np.stack([R.motion(s, T) for s in ss]), np.stack([R.target_of(s, T) for s in ss]), np.stack([R.semantic_of(s, T) for s in ss]),
            [R.onsets_of(s, R.ONSET_COUNTS[i % len(R.ONSET_COUNTS)], T) for i, s in enumerate(ss)])


@functools.lru_cache(maxsize=None)
def processed64(T):
    return np.stack([R.process_motion(R.motion(s, T)) for s in seeds(T)])


@functools.lru_cache(maxsize=None)
def small_net():
    import torch
    from convofusion_amd.metrics import FGDNet
    net = FGDNet(128, 189, 12)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in R.make_fgd_state(12, NET_SEED).items()})
    return net.eval()


def within(name, got, want, gate):
    d = R.rel(got, want)
    print(f"  {name}: {d:.3e} (gate {gate:.3e})")
    assert d <= gate, (name, d, gate)


# ---------------------------------------------------------------- 1. stage A
@pytest.mark.parametrize("with_target", [True, False])
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("T", [128, 40])
def test_stage_a_against_float64(T, order, with_target):
    import torch
    from convofusion_amd import metrics
    pred, target, sem, onsets = batch(T)
    assert [len(o) for o in onsets][:2] == [0, 1] and (T != 128 or [len(o) for o in onsets] == [0, 1, 7, 7, 1])
    B, sigma = pred.shape[0], R.SIGMAS[order]
    r = metrics.motion_eval(dev(pred), dev(target) if with_target else None, dev(sem) if with_target else None, onsets, order=order, sigma=sigma)
    torch.cuda.synchronize()
    assert metrics_info()[:2] == [1, B]
    r = {k: v.cpu().numpy() for k, v in r.items()}
    assert ("srgr" in r) == ("srgr_count" in r) == ("jitter" in r) == with_target
    print(f"T = {T}, order {order}, target {with_target}:")
    assert np.array_equal(r["beats"], G[f"T{T}_o{order}_ref_beats"])
    ref_align = G[f"T{T}_o{order}_ref_align"]
    for i in range(B):
        x = pred[i]
        within(f"l1div[{i}]", r["l1div"][i], R.l1div_partial(x), FACTOR * float(G[f"T{T}_base_l1div"]))
        within(f"processed[{i}]", r["processed"][i], processed64(T)[i], FACTOR * float(G[f"T{T}_base_processed"]))
        if len(onsets[i]):
            want = R.align_score(G[f"T{T}_o{order}_ref_beats"][i][5], onsets[i], sigma)
            assert abs(want - ref_align[i]) < 1e-12
            within(f"align[{i}]", r["align"][i], want, FACTOR * float(G[f"T{T}_o{order}_base_align"]))
        else:
            assert r["align"][i] == 0.0 and np.isnan(ref_align[i])      # left out of the mean by the caller, and counted
        if with_target:
            total, count, _ = R.srgr_partial(x, target[i], sem[i])
            assert r["srgr_count"][i] == count == G[f"T{T}_srgr_count"][i]
            within(f"srgr[{i}]", r["srgr"][i], total, FACTOR * float(G[f"T{T}_base_srgr"]))
            within(f"jitter[{i}]", r["jitter"][i], R.jitter_sum(x, target[i]), FACTOR * float(G[f"T{T}_base_jitter"]))


def test_evaluator_aggregates_as_the_reference_does():
    """l1div over all frames, srgr over frames x 63, jitter per sequence, the alignment over the sequences that have onsets"""
    import torch
    from convofusion_amd.metrics import MotionEvaluator
    pred, target, sem, onsets = batch(128)
    ev = MotionEvaluator()
    ev.update(dev(pred), dev(target), dev(sem), onsets)
    got = ev.compute()
    torch.cuda.synchronize()
    B, T = pred.shape[:2]
    assert got["align_counted"] == 4 and got["fgd"] is None
    within("align", got["align"], np.nanmean(G["T128_o10_ref_align"]), FACTOR * float(G["T128_o10_base_align"]))
    within("l1div", got["l1div"], sum(R.l1div_partial(x) for x in pred) / (B * T), FACTOR * float(G["T128_base_l1div"]))
    within("srgr", got["srgr"], np.mean([R.srgr_partial(pred[i], target[i], sem[i])[0] for i in range(B)]) / (T * 63), FACTOR * float(G["T128_base_srgr"]))
    within("jitter", got["jitter"], np.mean([R.jitter_sum(pred[i], target[i]) for i in range(B)]) / ((T - 1) * 189), FACTOR * float(G["T128_base_jitter"]))
    within("diversity_pred", got["diversity_pred"], R.avg_distance(processed64(128).astype(np.float32)), FACTOR * float(G["div7_base"]))
    assert got["diversity_target"] > 0


# ---------------------------------------------------------------- 2. stage B
def test_embedding_width_12_every_reduction_with_an_odd_tail():
    """K = 567, 36, 96, 72 and the 708-deep fold: none a multiple of the 32-deep k tile; M = 126, 124, 61, 59 and N = 12, 24 inside one block"""
    import torch
    from convofusion_amd import metrics
    x3 = processed64(128)[:3].astype(np.float32)
    net = small_net()
    got = net(dev(x3))
    torch.cuda.synchronize()
    assert metrics_info()[:2] == [6, 3]
    want = R.embed(R.make_fgd_state(12, NET_SEED), x3)
    print("embedding, F = 12:")
    within("mu", got.cpu().numpy(), want, FACTOR * float(G["emb12_base"]))
    # the net on the processed motion inside the call is the net on the processed output
    r = metrics.motion_eval(dev(np.stack([R.motion(s) for s in seeds(128)[:3]])), fgd_net=net, want={"processed", "embedding"})
    assert torch.equal(net(r["processed"]), r["embedding"])


def test_embedding_product_width():
    import torch
    from convofusion_amd import metrics
    parts = R.make_folded_parts(300, PACK_SEED)
    assert np.array_equal(parts[4][0][::37, ::1009], G["pack300_spot"])
    flat = dev(np.concatenate([t.reshape(-1) for wb in parts for t in wb]))
    assert flat.numel() == metrics.pack_floats(300)
    x2 = processed64(128)[:2].astype(np.float32)
    net = SimpleNamespace(feature_length=300, pack=lambda d: flat)
    got = metrics.motion_eval(dev(x2), fgd_net=net, want={"embedding"}, embed_raw=True)["embedding"]
    torch.cuda.synchronize()
    assert metrics_info()[:2] == [6, 2]
    print("embedding, F = 300:")
    within("mu", got.cpu().numpy(), R.embed_folded(parts, x2), FACTOR * float(G["emb300_base"]))


def test_embedding_in_more_than_one_pass_of_128_sequences():
    """130 sequences: a pass of 128 and one of 2 through the net's workspace; every row the bits of the same motion in a batch of 5, with
    and without the processed motion going to the caller"""
    import torch
    from convofusion_amd import metrics
    five = dev(batch(128)[0])
    want = metrics.motion_eval(five, fgd_net=small_net(), want={"processed", "embedding"})
    many = five.repeat(26, 1, 1)
    for names in ({"processed", "embedding"}, {"embedding"}):
        got = metrics.motion_eval(many, fgd_net=small_net(), want=names)
        torch.cuda.synchronize()
        assert metrics_info()[:2] == [1 + 2 * 5, 130]
        for k in names:
            assert torch.equal(got[k], want[k].repeat(26, *([1] * (want[k].dim() - 1)))), k
    raw = small_net()(want["processed"].repeat(26, 1, 1))
    assert torch.equal(raw, want["embedding"].repeat(26, 1))


# ---------------------------------------------------------------- 3. bits
def test_a_sequence_has_the_same_bits_alone_in_the_batch_and_again():
    import torch
    from convofusion_amd import metrics
    pred, target, sem, onsets = batch(128)
    kw = dict(fgd_net=small_net(), order=10, sigma=0.3)
    whole = metrics.motion_eval(dev(pred), dev(target), dev(sem), onsets, **kw)
    again = metrics.motion_eval(dev(pred), dev(target), dev(sem), onsets, **kw)
    alone = metrics.motion_eval(dev(pred[2:3]), dev(target[2:3]), dev(sem[2:3]), onsets[2:3], **kw)
    torch.cuda.synchronize()
    assert set(whole) == {"l1div", "srgr", "srgr_count", "jitter", "beats", "align", "processed", "embedding"}
    for k in whole:
        assert torch.equal(whole[k], again[k]), k
        assert torch.equal(whole[k][2:3], alone[k]), k
        assert not torch.isnan(whole[k].double()).any(), k


# ---------------------------------------------------------------- 4. streaming and the Frechet distance
def test_streaming_statistics_and_fgd():
    import torch
    from convofusion_amd.metrics import MotionEvaluator
    pred = batch(128)[0]
    one, two = MotionEvaluator(small_net()), MotionEvaluator(small_net())
    one.update(dev(pred))
    two.update(dev(pred[:3]))
    two.update(dev(pred[3:]))
    a, b = one.state_dict()["pred"], two.state_dict()["pred"]
    assert a[0] == b[0] == 5
    d = float(np.abs(a - b).max() / np.abs(a).max())
    print(f"statistics, 3 + 2 against 5: {d:.3e}")
    assert d <= 1e-12
    e = R.embed(R.make_fgd_state(12, NET_SEED), processed64(128).astype(np.float32))
    within("statistics against float64", a, R.stats_of(e), 2 * FACTOR * float(G["emb12_base"]))      # (products of two embeddings)

    sets = [np.stack([R.motion(first + i) * np.float32(1.0 if first == 200 else 1.1) for i in range(48)]) for first in (200, 300)]
    ev = MotionEvaluator(small_net())
    ev.update(dev(sets[0][:32]), dev(sets[1][:32]))
    ev.update(dev(sets[0][32:]), dev(sets[1][32:]))
    got = ev.compute()["fgd"]
    torch.cuda.synchronize()
    state = R.make_fgd_state(12, NET_SEED)
    want = R.frechet(*[R.embed(state, np.stack([R.process_motion(x) for x in s]).astype(np.float32)) for s in sets])
    print("FGD of two 48-sequence sets:", got, "float64 restatement", want, "reference", float(G["fgd_ref"]))
    within("fgd", got, want, FACTOR * float(G["fgd_base"]))
    within("fgd against the reference", got, float(G["fgd_ref"]), FACTOR * float(G["fgd_base"]) + float(G["fgd_ref_dist"]))


# ---------------------------------------------------------------- 5. diversity
def test_diversity():
    import torch
    from convofusion_amd import metrics
    rows = np.stack([R.process_motion(R.motion(int(s))).astype(np.float32) for s in G["div7_seeds"]])
    got = float(metrics.diversity(dev(rows)))
    assert metrics_info()[:2] == [2, 7]
    print("diversity:")
    within("N = 7", got, R.avg_distance(rows), FACTOR * float(G["div7_base"]))
    # two motions 1e-4 of their norm apart: a float32 Gram-matrix form (|a|^2 + |b|^2 - 2 a.b) loses this distance
    near = np.stack([rows[0], (rows[0].astype(np.float64) * (1 + 1e-4)).astype(np.float32)])
    want = R.avg_distance(near)
    assert 0.5e-4 < want / np.linalg.norm(near[0].astype(np.float64)) < 2e-4
    within("N = 2, nearly equal", float(metrics.diversity(dev(near))), want, FACTOR * float(G["div2_base"]))
    # more than one block of 16 rows, a row length that is no multiple of the 64-wide k tile
    many = rows.reshape(21, -1)[:19, :8063].copy()
    base = R.rel(R.avg_distance(many, np.float32), R.avg_distance(many))
    within("N = 19, D = 8063", float(metrics.diversity(dev(many))), R.avg_distance(many), FACTOR * base)
    assert torch.equal(metrics.diversity(dev(many)), metrics.diversity(dev(many)))


# ---------------------------------------------------------------- 6. refusals
def test_refusals_come_before_any_launch():
    import torch
    from convofusion_amd import _lib, metrics
    lib, h = _lib.load(), _handle()
    x = torch.zeros(2, 130, 189, device="cuda")
    sem = torch.zeros(2, 130, device="cuda")
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    times = torch.zeros(3, dtype=torch.float64, device="cuda")
    off = torch.zeros(3, dtype=torch.int32, device="cuda")

    def call(T=128, stride=189, launches=0, **kw):
        metrics.motion_eval(x[:, :128].contiguous(), want={"l1div"})                       # a good call first: 1 launch on record
        assert metrics_info()[0] == 1
        a = _lib.MotionEvalArgs()
        a.pred, a.n_seq, a.n_frames, a.stride, a.fps, a.order, a.sigma, a.srgr_threshold = x.data_ptr(), 2, T, stride, 25.0, 10, 0.3, 0.3
        a.l1div = out.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        code = lib.cfd_motion_eval(h, C.byref(a), None)
        assert metrics_info()[0] == launches, kw
        return code
    assert call(T=23) == E_SHAPE
    assert call(T=129) == E_SHAPE
    assert call(stride=188) == E_SHAPE
    assert call(onset_t=times.data_ptr(), n_onsets=3) == E_ARG                             # onsets without offsets
    assert call(align=out.data_ptr()) == E_ARG
    assert call(target=x.data_ptr(), srgr=out.data_ptr()) == E_ARG                          # target without semantic where SRGR is asked
    assert call(semantic=sem.data_ptr(), srgr_count=out.data_ptr()) == E_ARG
    assert call(jitter=out.data_ptr()) == E_ARG
    assert call(embedding=out.data_ptr()) == E_ARG                                          # no pack
    assert call(T=64, embedding=out.data_ptr(), fgd_pack=x.data_ptr(), feature_length=12) == E_SHAPE
    assert call(order=0) == E_ARG
    assert call(launches=1, onset_off=off.data_ptr(), onset_t=times.data_ptr(), n_onsets=3, align=out.data_ptr()) == 0    # and the same call, complete
    assert lib.cfd_motion_diversity(h, C.c_void_p(x.data_ptr()), 1, 100, C.c_void_p(out.data_ptr()), None) == E_SHAPE
    assert metrics_info()[0] == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. end to end
def test_decoded_motions_go_in_without_a_host_copy():
    import torch
    from oracle import vae_weights
    from convofusion_amd.metrics import MotionEvaluator
    from convofusion_amd.vae import ConvoFusionVae
    from tests.test_oracle_vae import ABL, KW, cases
    vae = ConvoFusionVae(ablation=ABL, **KW)
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    z, lengths = cases()["ragged"]
    decoded = vae.cuda().eval().decode(torch.from_numpy(z).cuda(), lengths)
    assert decoded.shape == (3, 128, 189) and decoded.is_cuda
    results = []
    for motions in (decoded, torch.from_numpy(decoded.cpu().numpy().copy()).cuda()):
        ev = MotionEvaluator(small_net())
        ev.update(motions, onsets=[[0.5, 1.0], [], [2.0]])
        results.append((ev.compute(), ev.state_dict()["pred"]))
    (a, sa), (b, sb) = results
    assert np.array_equal(sa, sb) and np.isfinite(sa).all() and sa[0] == 3
    assert a == b and a["align_counted"] == 2 and a["diversity_pred"] > 0 and a["l1div"] > 0 and a["srgr"] is None
