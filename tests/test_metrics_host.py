"""Host side of the motion evaluation (convofusion_amd/metrics.py, cfd_motion_eval): the struct layout against the header, the CPU
refusal, the state-dict mapping, the folded affine map against the unfolded chain in float64, the result-directory reader and the
Frechet distance from saved statistics.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "cfdenoise.h")).read()


def test_struct_layout_and_entries_match_the_header():
    from convofusion_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*cfd_motion_eval_args;", hdr).group(1)
    kinds = {"int": C.c_int, "long long": C.c_longlong, "double": C.c_double}
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        ctype, names = re.match(r"\s*(?:const\s+)?([\w ]+?)\s*(\*?\s*\w+(?:\s*,\s*\*?\s*\w+)*)\s*$", decl).groups()
        for n in names.split(","):
            fields.append((n.replace("*", "").strip(), C.c_void_p if "*" in n else kinds[ctype.strip()]))
    assert fields == list(_lib.MotionEvalArgs._fields_)
    assert _lib.MotionEvalArgs.stride.offset == 32 and _lib.MotionEvalArgs.fps.offset == 40 and _lib.MotionEvalArgs.sigma.offset == 56
    assert C.sizeof(_lib.MotionEvalArgs) == 184
    assert "int cfd_motion_eval(cfd_handle h, const cfd_motion_eval_args* a, void* stream);" in hdr
    assert "int cfd_motion_diversity(cfd_handle h, const float* x, int n, long long d, double* out, void* stream);" in hdr
    assert {"cfd_motion_eval", "cfd_motion_diversity"} <= set(_lib.SYMBOLS)


def test_pack_size_matches_the_kernel_header():
    from convofusion_amd import metrics
    src = open(os.path.join(ROOT, "convofusion_amd", "csrc", "metrics_eval.hpp")).read()
    expr = re.search(r"me_pack_floats\(int F\) \{\s*const size_t f = \(size_t\)F;\s*return ([^;]+);", src).group(1)
    for F in (1, 12, 300):
        assert eval(expr.replace("ME_FEAT", "189"), {"f": F}) == metrics.pack_floats(F)
    assert metrics.pack_floats(300) * 4 < 32 << 20          # the folded net at the product width: 30 MB, not 456


def test_no_cpu_path():
    from convofusion_amd.metrics import FGDNet, MotionEvaluator, diversity
    net = FGDNet(128, 189, 12).eval()
    x = torch.zeros(2, 128, 189)
    with pytest.raises(NotImplementedError):
        net(x)
    with pytest.raises(NotImplementedError):
        MotionEvaluator().update(x)
    with pytest.raises(NotImplementedError):
        diversity(x)
    with pytest.raises(NotImplementedError):
        net.train()(x)
    with pytest.raises(ValueError):
        FGDNet(64, 189, 12)


def test_state_dict_keys_and_the_module_prefix_rule():
    from convofusion_amd.metrics import FGDNet
    state = {k: torch.from_numpy(np.asarray(v)) for k, v in R.make_fgd_state(12, 41).items()}
    net = FGDNet(128, 189, 12)
    assert set(net.state_dict().keys()) == set(state.keys())
    assert all(net.state_dict()[k].shape == state[k].shape for k in state)
    net.load_state_dict(state)
    # a checkpoint saved from DataParallel, with the decoder half in it
    wrapped = {"module." + k: v for k, v in state.items()}
    wrapped["module.decoder.pre_net.0.weight"] = torch.zeros(3, 3)
    other = FGDNet(128, 189, 12)
    other.load_state_dict(wrapped)
    assert all(torch.equal(other.state_dict()[k], state[k]) for k in state)
    with pytest.raises(RuntimeError):
        FGDNet(128, 189, 12).load_state_dict({k: v for k, v in state.items() if "fc_mu" not in k})


def _unfolded(net, x):
    """The module's own layers in float64, nothing folded: poses [B, 128, 189] -> mu"""
    enc = net.pose_encoder.double()
    with torch.no_grad():
        h = enc.net(torch.from_numpy(x).double().transpose(1, 2)).flatten(1)
        return enc.fc_mu(enc.out_net(h)).numpy()


@pytest.mark.parametrize("F", [12, 300])
def test_folded_map_equals_the_unfolded_chain(F):
    """Measured (float64, relative to the largest entry): 1.0e-15 at F = 12, 1.0e-15 at F = 300 -- rounding only."""
    from convofusion_amd.metrics import FGDNet
    torch.manual_seed(5)
    net = FGDNet(128, 189, F)
    if F == 12:
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in R.make_fgd_state(12, 41).items()})
    else:                                       # default initialisation; BatchNorm statistics away from (0, 1)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.normal_(0, 0.1)
    net.eval()
    parts = [(w.numpy(), b.numpy()) for w, b in net.folded()]
    assert [p[0].shape for p in parts] == [(F, 567), (2 * F, 3 * F), (2 * F, 8 * F), (F, 6 * F), (F, 59 * F)]
    x = np.stack([R.process_motion(R.motion(s)) for s in (0, 1)]).astype(np.float32)
    got, want = R.embed_folded(parts, x), _unfolded(net, x)
    d = R.rel(got, want)
    print(f"folded against unfolded, F = {F}: {d:.2e}")
    assert d < 1e-13
    assert net.pack("cpu").numel() == sum(w.size + b.size for w, b in parts) and net.pack("cpu").dtype == torch.float32
    if F == 12:                                 # and the restatement's layer-by-layer net says the same
        assert R.rel(R.embed(R.make_fgd_state(12, 41), x), want) < 1e-13


def test_fold_refuses_another_slope():
    from convofusion_amd.metrics import FGDNet
    net = FGDNet(128, 189, 4).eval()
    net.pose_encoder.out_net[2] = torch.nn.LeakyReLU(0.2)
    with pytest.raises(ValueError, match="negative_slope"):
        net.folded()


def test_result_directory_reader(tmp_path):
    from convofusion_amd.metrics import read_result_dir
    rng = np.random.default_rng(0)
    want = {}
    for i, name in enumerate(("b/x", "a/y", "a/x")):
        d = tmp_path / name
        d.mkdir(parents=True)
        want[name] = (rng.standard_normal((128, 189)).astype(np.float32), rng.standard_normal((128, 63, 3)).astype(np.float32),
                      rng.uniform(size=(128, 1)).astype(np.float32))
        np.save(d / "gt.npy", want[name][0])
        np.save(d / "pred.npy", want[name][1])
        np.save(d / "sem_lsn.npy", want[name][2])
        if i == 1:
            np.save(d / "onsets.npy", np.array([0.5, 1.25]))
    (tmp_path / "stray.npy").write_bytes(b"")
    gt, pred, sem, ons = read_result_dir(str(tmp_path))
    assert gt.shape == pred.shape == (3, 128, 189) and sem.shape == (3, 128)
    for row, name in enumerate(("a/x", "a/y", "b/x")):                  # sorted, as the reference's glob + sort
        assert np.array_equal(gt[row], want[name][0]) and np.array_equal(pred[row], want[name][1].reshape(128, 189))
        assert np.array_equal(sem[row], want[name][2].reshape(-1))
    assert [len(o) for o in ons] == [0, 2, 0]
    with pytest.raises(FileNotFoundError):
        read_result_dir(str(tmp_path / "a" / "x"))


def test_compute_from_saved_and_reloaded_statistics(tmp_path):
    from convofusion_amd.metrics import FGDNet, MotionEvaluator, frechet_distance_from_stats
    rng = np.random.default_rng(3)
    ea, eb = rng.standard_normal((40, 6)), rng.standard_normal((50, 6)) * 1.3 + 0.2
    want = R.frechet(ea, eb)
    assert abs(frechet_distance_from_stats(R.stats_of(ea), R.stats_of(eb)) - want) < 1e-9 * want
    # streaming: the state of two batches is the sum of their states
    assert np.allclose(R.stats_of(ea[:25]) + R.stats_of(ea[25:]), R.stats_of(ea), rtol=1e-13)
    ev = MotionEvaluator(FGDNet(128, 189, 6).eval())
    ev.load_state_dict({"pred": R.stats_of(ea), "target": R.stats_of(eb)})
    assert abs(ev.compute()["fgd"] - want) < 1e-9 * want
    np.savez(tmp_path / "state.npz", **{k: v for k, v in ev.state_dict().items() if v is not None})
    again = MotionEvaluator(FGDNet(128, 189, 6).eval(), order=12, sigma=1.25)
    again.load_state_dict(dict(np.load(tmp_path / "state.npz")))
    r = again.compute()
    assert abs(r["fgd"] - want) < 1e-9 * want
    assert r["align"] is None and r["l1div"] is None and r["diversity_pred"] is None
    with pytest.raises(ValueError):
        MotionEvaluator(FGDNet(128, 189, 5).eval()).load_state_dict({"target": R.stats_of(eb)})
    with pytest.raises(ValueError):
        frechet_distance_from_stats(R.stats_of(ea[:1]), R.stats_of(eb))
