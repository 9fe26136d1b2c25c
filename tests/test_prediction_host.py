"""CPU: ``prediction_type="sample"`` (an x0-predicting denoiser, the reference's TRAIN.ABLATION.PREDICT_EPSILON: False) without a
device -- the constructor surface of the scheduler mirrors, every refusal between kinds (``resolve_run_kind`` on CPU tensors, and the
entry points that refuse before they touch a device), the place of cfd_sample_args.prediction_type in the struct, the scheduler part
of cfd_sample_args, the closed forms of the restated steps (tests/prediction_ref.py) and the null-handle refusal of the two ``_pred``
entry points.

The three closed-form tests (test_ddpm_last_step*, test_ddim_step_moves*, test_dpmpp_first_order*) check the restatement itself, not the
library: they run only tests/prediction_ref.py and so pass with or without the feature; every other test here needs it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from convofusion_amd import _lib, scheduler
from convofusion_amd.sampler import fill_scheduler_args, resolve_run_kind
from tests.prediction_ref import DDIMSampleRef, DDPMSampleRef, DPMSolverSampleRef

YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
B, L, N = 2, 16, 10
U24 = 2.0 ** -24      # float32 unit round-off

RING = torch.zeros((N + 1, B, L, 128))
NOISE = torch.ones((N, B, L, 128))
SOURCE = torch.zeros((B, L, 128))
KEEP = torch.zeros((B, L), dtype=torch.bool)
KEEP[0, :4] = True
TIE = torch.full((B, L), -1, dtype=torch.int64)
TIE[1, :8] = torch.arange(8, 16)


def _sample_sched(kind, **kw):
    cls = dict(ddpm=scheduler.DDPMScheduler, ddim=scheduler.DDIMScheduler, dpmpp=scheduler.DPMSolverMultistepScheduler)[kind]
    return cls(**YAML, prediction_type="sample", **kw)


def test_constructor_surface():
    for kind in ("ddpm", "ddim", "dpmpp"):
        s = _sample_sched(kind)
        assert s.config.prediction_type == "sample" and s.config["prediction_type"] == "sample"
        cls = type(s)
        assert cls(**YAML).config.prediction_type == "epsilon"            # the default stays
        for bad in ("v_prediction", "junk", "", None, 1):
            with pytest.raises(NotImplementedError, match="prediction_type"):
                cls(**YAML, prediction_type=bad)
    with pytest.raises(NotImplementedError, match="DDIMInverseScheduler: only prediction_type='epsilon'"):
        scheduler.DDIMInverseScheduler(**YAML, prediction_type="sample")
    assert scheduler.DDIMInverseScheduler(**YAML).config.prediction_type == "epsilon"
    assert _lib.PREDICTION_TYPES == {"epsilon": 0, "sample": 1}


def _resolve(sch, eta=0.0, **kw):
    return resolve_run_kind(sch, sch.timestep_table(N)[1], eta, B=B, L=L, **kw)


def _forged_inverse():
    """A kind-3 scheduler whose config was edited after construction (the constructor itself refuses the type)."""
    s = scheduler.DDIMInverseScheduler(**YAML)
    s.config["prediction_type"] = "sample"
    return s


REFUSALS = {
    "inversion": (_forged_inverse, {}, "a DDIM inversion run (DDIMInverseScheduler) runs"),
    "anchored": (lambda: _sample_sched("ddim", clip_sample=False), dict(anchor_trajectory=RING), "an anchored run (anchor_trajectory) runs"),
    "replay": (lambda: _sample_sched("ddpm"), dict(noise_space=(RING, NOISE)), "the replay of a noise space (noise_space) runs"),
    "dyadic ddpm": (lambda: _sample_sched("ddpm"), dict(dynamic_memories=(0,)), "a run with dynamic memories (a dyadic run) runs"),
    "dyadic ddim": (lambda: _sample_sched("ddim"), dict(dynamic_memories=(0,)), "a run with dynamic memories (a dyadic run) runs"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_between_kinds(case):
    make, kw, what = REFUSALS[case]
    with pytest.raises(NotImplementedError) as e:
        _resolve(make(), **kw)
    assert str(e.value) == (f"{what} with prediction_type='epsilon' only: with prediction_type='sample' it has no reference trajectory to "
                            "be checked against")


def test_refusals_of_the_entry_points():
    """invert_ddpm, sample_parallel, sample_with_weg, DyadicRun and reperform_motion refuse the type by name, before any device work."""
    from types import SimpleNamespace
    from convofusion_amd import edit
    from convofusion_amd.denoiser import Denoiser
    from convofusion_amd.dyadic import DyadicRun
    from convofusion_amd.sampler import invert_ddpm, sample_parallel, sample_with_weg
    abl = SimpleNamespace(SKIP_CONNECT=True, VAE_TYPE="convofusion", DIFF_PE_TYPE="convofusion", CAUSAL_ATTN=False)
    den = Denoiser(ablation=abl, nfeats=189, condition="text+audio", latent_dim=[1, 128], ff_size=1024, num_layers=1, num_heads=4,
                   dropout=0.1, normalize_before=True, activation="gelu", flip_sin_to_cos=True, position_embedding="sine", arch="trans_dec",
                   freq_shift=0, text_encoded_dim=512, audio_encoded_dim=512)
    sch = _sample_sched("ddpm")
    with pytest.raises(NotImplementedError, match="invert_ddpm .* prediction_type='epsilon' only"):
        invert_ddpm(den, sch, [], None, source_latents=SOURCE, num_inference_steps=N)
    with pytest.raises(NotImplementedError, match="sample_parallel .* prediction_type='epsilon' only"):
        sample_parallel(den, sch, [], None, B=B, L=L, num_inference_steps=N)
    with pytest.raises(NotImplementedError, match="focus_indices.* prediction_type='epsilon' only"):
        sample_with_weg(den, sch, [], None, [[1]], {}, B=B, L=L, num_inference_steps=N)
    with pytest.raises(NotImplementedError, match="DyadicRun .* prediction_type='epsilon' only"):
        DyadicRun(den, None, sch, None, None, None, None, B, L, N, shared_weights=True)
    model = SimpleNamespace(scheduler=sch)
    enc = [torch.zeros((7 * B, 1, 512))]
    with pytest.raises(NotImplementedError, match="reperform_motion .* prediction_type='epsilon' only"):
        edit.reperform_motion(model, torch.zeros((B, 8, 189)), [8] * B, enc, enc)


def test_what_composes_and_the_operand_policy():
    """Edits, ties and preseq resolve as for an epsilon run; operands None / "auto" become 0 (pairs), an explicit policy stays; an
    epsilon run's operands are untouched."""
    from convofusion_amd.run_kind import _AUTO_RUN
    for kind in ("ddpm", "ddim", "dpmpp"):
        sch = _sample_sched(kind)
        assert _resolve(sch).operands == 0 and _resolve(sch, operands="auto").operands == 0 and _resolve(sch, operands=_AUTO_RUN).operands == 0
        assert _resolve(sch, operands=15).operands == 15
        k = _resolve(sch, source_latents=SOURCE, keep_mask=KEEP, strength=0.5)
        assert k.edit is not None and k.first_iteration == 5 and k.operands == 0
        assert _resolve(sch, tie=TIE).tie is not None
        assert _resolve(sch, preseq=torch.zeros((B, 4, 128))).edit is None
    eps = scheduler.DDPMScheduler(**YAML)
    assert _resolve(eps).operands is None and _resolve(eps, operands="auto").operands == "auto"


def test_sample_args_field_sits_in_a_padding_hole():
    """cfd_sample_args.prediction_type: the 4 bytes between num_timesteps and att_ring that were padding; sizeof and the neighbours'
    offsets as tests/test_cabi_and_host.py pins them."""
    S = _lib.SampleArgs
    assert S.prediction_type.offset == S.num_timesteps.offset + 4 and S.prediction_type.size == 4
    assert S.num_timesteps.offset == S.timesteps.offset + 8
    assert S.att_ring.offset == S.timesteps.offset + 16 == S.prediction_type.offset + 4
    assert S.timesteps.offset == S.mem.offset + 5 * 32 + 8
    assert S.operand_policy.offset == S.att_ring.offset + 5 * 8 and S.census_tau.offset == S.operand_policy.offset + 4
    assert C.sizeof(S) == S.mem.offset + 5 * 32 + 8 + 16 + 5 * 8 + 8
    assert S().prediction_type == 0                                       # ctypes' zero-initialised default: epsilon
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfdenoise.h")).read()
    assert header.index("int num_timesteps;") < header.index("int prediction_type;") < header.index("float* att_ring[CFD_NUM_MEM];")


def test_fill_scheduler_args_reads_the_config():
    for kind, want in (("ddpm", 1), ("ddim", 1), ("dpmpp", 1)):
        sch = _sample_sched(kind)
        a = _lib.SampleArgs()
        keep = fill_scheduler_args(a, sch, N, sch.timestep_table(N)[1])
        assert a.prediction_type == want and a.scheduler == sch.KIND and keep
    for cls in (scheduler.DDPMScheduler, scheduler.DDIMScheduler, scheduler.DPMSolverMultistepScheduler, scheduler.DDIMInverseScheduler):
        sch = cls(**YAML)
        a = _lib.SampleArgs()
        a.prediction_type = 7
        keep = fill_scheduler_args(a, sch, N, sch.timestep_table(N)[1])
        assert a.prediction_type == 0 and keep


def _draws(seed, shape=(2, 16, 128)):
    r = np.random.default_rng(seed)
    return r.uniform(-2.0, 2.0, shape).astype(np.float32), r.standard_normal(shape).astype(np.float32)


def test_ddpm_last_step_returns_the_clipped_output_exactly():
    """At t = 0 the posterior mean's coefficients are c0 = 1 and cx = 0 exactly (abar_prev = 1) and no noise is added: prev = clip(out)."""
    out, x = _draws(1)
    for clip in (True, False):
        s = DDPMSampleRef(clip_sample=clip)
        s.set_timesteps(20)
        assert int(s.timesteps[-1]) == 0
        prev = s.step(out, 0, x)
        want = np.clip(out, -1, 1) if clip else out
        assert np.array_equal(prev, want) and np.array_equal(s.pred_original_sample, want)
    assert (np.abs(out) > 1).any()


def test_ddim_step_moves_a_noised_x0_to_the_next_level():
    """eta 0, x = sa x0 + sb e, out = x0 (|x0| < 1: the clip does not act): prev = sa' x0 + sb' e.  Float32 bound, per element: the
    cancellation x - sa x0 carries (|x| + |sa x0|) u relative to sb, scaled by the direction coefficient; the products and the sum a few u
    of their magnitudes (u = 2^-24); 4 u of the sum of those magnitudes covers the roundings of x itself as well."""
    x0 = (0.5 * _draws(2)[0]).astype(np.float32)
    e = _draws(3)[1]
    s = DDIMSampleRef(clip_sample=True)
    s.set_timesteps(N)
    ac = s.alphas_cumprod.astype(np.float64)
    for i, t in enumerate(s.timesteps):
        t, tp = int(t), int(t) - 1000 // N
        a, ap = ac[t], (ac[tp] if tp >= 0 else 1.0)
        sa, sb = np.float32(np.sqrt(s.alphas_cumprod[t])), np.float32(np.sqrt(np.float32(1) - s.alphas_cumprod[t]))
        x = (sa * x0 + sb * e).astype(np.float32)
        prev = s.step(x0, t, x, eta=0.0)
        want = np.sqrt(ap) * x0.astype(np.float64) + np.sqrt(1 - ap) * e.astype(np.float64)
        bound = 4 * U24 * (np.sqrt(ap) * np.abs(x0) + np.sqrt(1 - ap) * (np.abs(x) + np.sqrt(a) * np.abs(x0)) / np.sqrt(1 - a) + np.abs(want) + 1e-30)
        err = np.abs(prev.astype(np.float64) - want)
        assert (err <= bound).all(), (t, float((err / bound).max()))
        assert np.array_equal(s.pred_original_sample, x0)


def test_dpmpp_first_order_step_moves_a_noised_x0_to_the_next_level():
    """Order 1 (the first step after set_timesteps), x = alpha x0 + sigma e, out = x0: x' = alpha' x0 + sigma' e, because
    alpha' exp(-h) = alpha sigma' / sigma.  Float32 bound: h = lambda' - lambda is a difference of two float32 logs, so exp(-h) carries
    (|lambda'| + |lambda| + 1) u relative; that error enters through the two terms (sigma'/sigma) x and alpha' (exp(-h) + 1) x0.
    8 u (|lambda'| + |lambda| + 1) of the sum of those magnitudes."""
    x0 = _draws(4)[0]
    e = _draws(5)[1]
    for n in (10, 50):
        s = DPMSolverSampleRef(**YAML)
        s.set_timesteps(n)
        for i in (0, n // 2, n - 1):
            s.model_outputs, s.lower_order_nums = [None, None], 0
            t = int(s.timesteps[i])
            tp = 0 if i == n - 1 else int(s.timesteps[i + 1])
            al, si, alp, sip = (float(v) for v in (s.alpha_t[t], s.sigma_t[t], s.alpha_t[tp], s.sigma_t[tp]))
            x = (s.alpha_t[t] * x0 + s.sigma_t[t] * e).astype(np.float32)
            prev = s.step(x0, t, x)
            want = alp * x0.astype(np.float64) + sip * e.astype(np.float64)
            lam = abs(float(s.lambda_t[t])) + abs(float(s.lambda_t[tp])) + 1.0
            eh = (al * sip) / (si * alp)
            bound = 8 * U24 * lam * (sip / si * np.abs(x) + alp * (eh + 1.0) * np.abs(x0) + 1e-30)
            err = np.abs(prev.astype(np.float64) - want)
            assert (err <= bound).all(), (n, t, float((err / bound).max()))
            assert np.array_equal(s.pred_original_sample, x0) and s.lower_order_nums == 1


def test_pred_entry_points_refuse_a_null_handle():
    """Both calls are exported, and refuse a null handle (CFD_E_ARG) before anything else; the refusal of a bad prediction_type needs a
    handle: tests/test_gpu_prediction.py."""
    lib = _lib.load()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.cfd_scheduler_step_pred(None, 0, p, 8, 8, 1, 0, 0.0, 1, 1, p, None, p, 8, None, None) == -1
    assert lib.cfd_dpmsolver_step_pred(None, p, 8, 2, 1, -1, 1, p, None, p, p, 8, None) == -1
    assert {"cfd_scheduler_step_pred", "cfd_dpmsolver_step_pred"} <= set(_lib.SYMBOLS)
