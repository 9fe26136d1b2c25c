"""The attention-concentration census of a sampling run (cfd_sample_args.census_tau, cfd_sample_census, ``SamplingRun.census``) and the
opt-in ``operands="auto"`` built on it: the census is invisible in the latents, it reports the oracle's peak
probabilities, it separates the seeded goldens from the heavy-tailed stress case, and "auto" is bit for bit one of the two policies."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from oracle import denoiser_ref, inputs, philox_ref
from tests.helpers import heavy_state_dict, load_golden, rel_l2, state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sched(kind="ddpm"):
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    return scheduler.DDIMScheduler(**SCHED_KW) if kind == "ddim" else scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)


def _model(sd):
    import torch
    from convofusion_amd.denoiser import Denoiser
    from tests.gpu_helpers import ABL, DENOISER_KW
    m = Denoiser(ablation=ABL, **DENOISER_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    m.return_attention = False
    return m


def _seeded_c2():
    """traj_c2_ddpm5's inputs: the seeded headline batch (B = 32, L = 196, 1500 audio keys)."""
    from tests.gpu_helpers import hip_denoiser, to_dev
    g = load_golden("traj_c2_ddpm5")
    meta = [int(v) for v in g["meta"]]
    B, L, S, pad, seed = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[13]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, uncond_pad_tail=pad)
    return hip_denoiser(1234, 1.0), [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}, B, L, seed


def _heavy_c2():
    """heavy_c2's inputs (outlier-token memories) with the outlier factor 8 weights: the headline shape where attention concentrates."""
    from tests.gpu_helpers import to_dev
    g = load_golden("heavy_c2_ddpm50")
    meta = [int(v) for v in g["meta"]]
    B, L, S, pad, n, seed, u = meta[0], meta[1], tuple(meta[2:7]), tuple(meta[7:12]), meta[12], meta[13], meta[14]
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad, uncond_pad_tail=pad)
    mems = [to_dev(inputs.add_outlier_tokens(uq, seed + j)[rm]) for j, (uq, rm) in enumerate(zip(cb["unique"], cb["row_map"]))]
    return _model(heavy_state_dict(8.0)), mems, {k: to_dev(v) for k, v in cb["masks"].items()}, B, L, seed, n, u, g


def _run(m, mems, masks, B, L, n, seed, steps=None, **kw):
    from convofusion_amd.sampler import SamplingRun
    with SamplingRun(m, _sched(), mems, masks, B, L, n, guidance_scale=7.5, seed=seed, **kw) as r:
        r.steps(n if steps is None else steps)
        lat = r.read()
        cen = r.census()
    return lat, cen


def test_census_off_is_invisible_and_on_changes_nothing():
    """Headline shape, 5 DDPM steps, policies 0 and 15: census_tau = 0 (the field's zero default) and a census at CENSUS_TAU give the same
    latents bit for bit as a run that never set the field."""
    import torch
    from convofusion_amd.sampler import CENSUS_TAU
    m, mems, masks, B, L, seed = _seeded_c2()
    for pol in (0, 15):
        base, c0 = _run(m, mems, masks, B, L, 5, seed, operands=pol)
        zero, cz = _run(m, mems, masks, B, L, 5, seed, operands=pol, census_tau=0.0)
        on, con = _run(m, mems, masks, B, L, 5, seed, operands=pol, census_tau=CENSUS_TAU)
        print(f"policy {pol}: census {json.dumps({k: v for k, v in con.items() if not k.startswith('layer')})}")
        assert torch.isfinite(base).all() and torch.equal(zero, base) and torch.equal(on, base), pol
        assert not c0["measured"] and not cz["measured"] and c0["rows_seen"] == 0 and c0["worst_layer"] == -1
        assert con["measured"] and con["iterations"] == 5 and con["rows_seen"] > 0 and con["tau"] == pytest.approx(CENSUS_TAU)


def test_census_matches_the_oracle_peak_probabilities():
    """One DDPM iteration with fixed initial latents on the fused kernel (B = 2, L = 64: the tile kernels; tests/conftest.py lifts the fused
    kernel's workgroup threshold), a 300-key audio memory (long, and long enough for layer 0's de-duplicated launch): peak_max and every
    layer_peak against the maximum over the 7 guidance rows of the numpy oracle's audio attention, and rows_seen against the rows the kernel
    evaluates -- 14 x 64 per layer, and in layer 0 one row per distinct (utterance, audio instance) pair and query."""
    import torch
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L, S, n = 2, 64, (8, 300, 12, 8, 1), 5
    cb = inputs.make_cfg_batch(seed=11, B=B, L=L, S=S, pad_tail=(2, 0, 3, 0, 0))
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    init = philox_ref.normal_tensor(5, 0, list(range(B)), 1, L)
    sched = _sched()
    t0 = int(sched.timestep_table(n)[1][0])
    m = hip_denoiser(1234, 1.0)
    with SamplingRun(m, sched, mems, masks, B, L, n, guidance_scale=7.5, seed=5, init_latents=torch.from_numpy(init).cuda(),
                     census_tau=0.005) as r:
        r.steps(1)
        c = r.census()
    _, att = denoiser_ref.denoiser_forward(state_dict(1234, 1.0), np.concatenate([init] * 7), t0, cb["memories"], cb["masks"])
    want = att[1].max(axis=(0, 2, 3))                                  # [layers]
    over = (att[1].max(axis=3) > 0.005).sum(axis=(0, 2))               # rows above tau, per layer
    rm = cb["row_map"][1]
    distinct = len({(b, int(rm[g * B + b])) for b in range(B) for g in range(7)})
    print("census", c["layer_peak"], "oracle", want.tolist(), "over", c["layer_over"], over.tolist(), "rows", c["rows_seen"])
    assert c["measured"] and c["iterations"] == 1
    np.testing.assert_allclose(c["layer_peak"], want, rtol=1e-3)
    assert c["peak_max"] == pytest.approx(float(want.max()), rel=1e-3) and c["worst_layer"] == int(np.argmax(want))
    assert c["rows_seen"] == 8 * 7 * B * L + distinct * L
    # (rows within the tolerance of tau may fall on either side; none is, for these inputs, for the layers >= 1 compared here)
    assert c["layer_over"][1:] == over[1:].tolist()


def test_census_separates_seeded_from_heavy_tailed_attention():
    """At CENSUS_TAU: the seeded headline golden's inputs (traj_c2_ddpm5) never trip the census, the heavy-tailed stress inputs do."""
    from convofusion_amd.sampler import CENSUS_TAU
    m, mems, masks, B, L, seed = _seeded_c2()
    _, cs = _run(m, mems, masks, B, L, 5, seed, census_tau=CENSUS_TAU)
    mh, memsh, masksh, Bh, Lh, seedh, n, u, g = _heavy_c2()
    _, ch = _run(mh, memsh, masksh, Bh, Lh, n, seedh, steps=5, census_tau=CENSUS_TAU)
    for name, c in (("seeded traj_c2_ddpm5", cs), ("heavy_c2 factor 8", ch)):
        print(f"{name}: peak_max {c['peak_max']:.4f} (layer {c['worst_layer']}), rows_over {c['rows_over']} of {c['rows_seen']}, "
              f"layer peaks {[round(v, 4) for v in c['layer_peak']]}")
    assert cs["measured"] and cs["rows_over"] == 0 and cs["peak_max"] < CENSUS_TAU
    assert ch["measured"] and ch["rows_over"] > 0 and ch["peak_max"] > CENSUS_TAU


def test_auto_is_one_of_the_two_policies_bit_for_bit():
    """operands="auto": on the seeded inputs the policy-15 run (no warning), on the heavy-tailed inputs -- after a warning -- the policy-0 run."""
    import torch
    from convofusion_amd.sampler import sample
    m, mems, masks, B, L, seed = _seeded_c2()
    kw = dict(B=B, L=L, num_inference_steps=5, seed=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        auto = sample(m, _sched(), mems, masks, operands="auto", **kw)
    assert torch.equal(auto, sample(m, _sched(), mems, masks, operands=15, **kw))
    mh, memsh, masksh, Bh, Lh, seedh, n, u, g = _heavy_c2()
    kw = dict(B=Bh, L=Lh, num_inference_steps=5, seed=seedh)
    with pytest.warns(UserWarning, match="operands=0"):
        auto = sample(mh, _sched(), memsh, masksh, operands="auto", **kw)
    assert torch.equal(auto, sample(mh, _sched(), memsh, masksh, operands=0, **kw))


def test_auto_keeps_the_budget_on_heavy_tailed_ddpm50():
    """heavy_c2 with 50 guided DDPM steps at B = 32 (tests/golden/heavy_c2_ddpm50.npz: the restated loop driving the reference denoiser for
    utterance 5): "auto" falls back to pairs and row 5 ends within 1e-3 of the reference; policy 15's distance is printed for the record."""
    from convofusion_amd.sampler import sample
    mh, mems, masks, B, L, seed, n, u, g = _heavy_c2()
    kw = dict(B=B, L=L, num_inference_steps=n, seed=seed)
    with pytest.warns(UserWarning, match="operands=0"):
        auto = sample(mh, _sched(), mems, masks, operands="auto", **kw).cpu().numpy()
    e_auto = rel_l2(auto[u], g["latents"][:, 0])
    e15 = rel_l2(sample(mh, _sched(), mems, masks, operands=15, **kw).cpu().numpy()[u], g["latents"][:, 0])
    print(f"heavy_c2 DDPM-50 row {u} vs the reference: auto {e_auto:.2e}, policy 15 {e15:.2e}; golden peaks per layer at iterations "
          f"0 / 25 / 49: {[np.round(g[k], 3).tolist() for k in ('peak_it0', 'peak_it25', 'peak_it49')]}")
    assert np.isfinite(auto).all() and e_auto < 1e-3


_NOT_MEASURED = r"""
import json, sys, warnings
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from oracle import inputs
from convofusion_amd.sampler import SamplingRun, sample, CENSUS_TAU
from tests.test_gpu_operand_census import _sched
from tests.gpu_helpers import hip_denoiser, to_dev
B, L, S = 2, 16, (6, 200, 6, 8, 1)
cb = inputs.make_cfg_batch(seed=3, B=B, L=L, S=S, pad_tail=(2, 0, 1, 0, 0))
mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
m = hip_denoiser(1234, 1.0)
out = {}
with SamplingRun(m, _sched(), mems, masks, B, L, 4, seed=3, census_tau=CENSUS_TAU) as r:
    r.steps(4); out["rowtile"] = r.census()
kw = dict(B=B, L=L, num_inference_steps=4, seed=3)
with warnings.catch_warnings():
    warnings.simplefilter("error")
    out["auto_equal"] = bool(torch.equal(sample(m, _sched(), mems, masks, operands="auto", **kw), sample(m, _sched(), mems, masks, **kw)))
print("RESULT " + json.dumps(out))
"""


def test_paths_without_the_fused_kernel_report_not_measured():
    """A small run on the library's default path (the row-tile kernels: a fresh process without tests/conftest.py's threshold) and a run
    on the tile kernels that keeps the attention maps (att_ring: the fused kernel's ATT instance) report measured = False, and "auto" on the
    row-tile path is the default run bit for bit."""
    from convofusion_amd.sampler import CENSUS_TAU, SamplingRun
    from tests.gpu_helpers import hip_denoiser, to_dev
    B, L = 2, 64
    cb = inputs.make_cfg_batch(seed=11, B=B, L=L, S=(8, 300, 12, 8, 1), pad_tail=(2, 0, 3, 0, 0))
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}
    with SamplingRun(hip_denoiser(1234, 1.0), _sched(), mems, masks, B, L, 4, seed=3, census_tau=CENSUS_TAU, attention_ring=True) as r:
        r.steps(4)
        ring = r.census()
    assert not ring["measured"] and ring["rows_seen"] == 0 and ring["iterations"] == 4, ring
    env = {k: v for k, v in os.environ.items() if k != "CFD_FUSED_XATTN_MIN_WGS"}
    p = subprocess.run([sys.executable, "-c", _NOT_MEASURED, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(out)
    assert not out["rowtile"]["measured"] and out["rowtile"]["rows_seen"] == 0 and out["rowtile"]["iterations"] == 4
    assert out["auto_equal"]
