"""numpy float32 restatement of the scheduler steps for ``prediction_type="sample"`` (the denoiser predicts the clean latent x0, the
reference's TRAIN.ABLATION.PREDICT_EPSILON: False, convofusion/models/modeltype/convofusion.py:101-103) -- TEST INFRASTRUCTURE, the
checker of convofusion_amd.scheduler's mirrors and of the fused loop's cfd_sample_args.prediction_type = 1.

Subclasses of oracle.scheduler_ref.DDPMSchedulerRef / DDIMSchedulerRef and tests.dpmsolver_ref.DPMSolverMultistepRef: tables, timestep
tables and coefficients are theirs, ``step`` keeps their call shape (oracle.sampler_ref.diffusion_reverse drives them unchanged) and
reads ``model_output`` as x0.  Each operation is rounded to float32 on its own.

  DDPM   x0 = out, clipped to [-1, 1] with clip_sample; prev = c0 x0 + cx x (+ sigma z for t > 0).  diffusers 0.14.0's DDPMScheduler.step
         for "sample", unambiguous.
  DPM++  x0 = out (0.14.0's convert_model_output for "sample" under dpmsolver++); the multistep update and its history as for epsilon.
  DDIM   x0 = out; eps_hat = (x - sqrt(abar_t) out) / sqrt(1 - abar_t) from the UNCLIPPED output; x0 clipped with clip_sample;
         prev = sqrt(abar_prev) x0 + sqrt(1 - abar_prev - std^2) eps_hat (+ std z).  The form of later diffusers releases; 0.14.0's
         published source is believed to put the model output itself into the direction term, which is no DDIM step for an x0-predicting
         model.  diffusers is not installed here: neither form is pinned against the package.
"""
import numpy as np

from oracle.scheduler_ref import DDIMSchedulerRef, DDPMSchedulerRef
from tests.dpmsolver_ref import DPMSolverMultistepRef

F32 = np.float32


def _clip(x0, clip):
    return np.clip(x0, F32(-1.0), F32(1.0)) if clip else x0


class DDPMSampleRef(DDPMSchedulerRef):
    def step(self, model_output, t, sample, noise=None):
        sb, sa, c0, cx, sigma = self.coefficients(t)
        x0 = _clip(np.asarray(model_output, dtype=F32), self.clip_sample)
        prev = ((c0 * x0).astype(F32) + (cx * sample).astype(F32)).astype(F32)
        if int(t) > 0:
            prev = (prev + (sigma * noise).astype(F32)).astype(F32)
        self.pred_original_sample = x0
        return prev


class DDIMSampleRef(DDIMSchedulerRef):
    def step(self, model_output, t, sample, eta=0.0, noise=None):
        sb, sa, sp, dirc, std = self.coefficients(t, eta)
        out = np.asarray(model_output, dtype=F32)
        eps_hat = ((sample - (sa * out).astype(F32)).astype(F32) / sb).astype(F32)
        x0 = _clip(out, self.clip_sample)
        prev = ((sp * x0).astype(F32) + (dirc * eps_hat).astype(F32)).astype(F32)
        if eta > 0:
            prev = (prev + (std * noise).astype(F32)).astype(F32)
        self.pred_original_sample = x0
        return prev


class DPMSolverSampleRef(DPMSolverMultistepRef):
    def step(self, model_output, t, sample, noise=None):
        """The parent's ``step`` with x0 = model_output (``noise``: accepted for oracle.sampler_ref and ignored)."""
        i = self._index(t)
        n = len(self.timesteps)
        t = int(t)
        prev_t = 0 if i == n - 1 else int(self.timesteps[i + 1])
        lower_order_final = i == n - 1 and n < 15
        x0 = np.asarray(model_output, dtype=F32)
        self.model_outputs = [self.model_outputs[1], x0]
        lam_t, lam_s0 = self.lambda_t[prev_t], self.lambda_t[t]
        h = F32(lam_t - lam_s0)
        ratio = F32(self.sigma_t[prev_t] / self.sigma_t[t])
        ca = F32(self.alpha_t[prev_t] * F32(np.exp(-h) - F32(1.0)))
        if self.lower_order_nums < 1 or lower_order_final:
            prev = ((ratio * sample).astype(F32) - (ca * x0).astype(F32)).astype(F32)
        else:
            m0, m1 = self.model_outputs[1], self.model_outputs[0]
            h0 = F32(lam_s0 - self.lambda_t[int(self.timesteps[i - 1])])
            r0 = F32(h0 / h)
            d1 = (F32(F32(1.0) / r0) * (m0 - m1).astype(F32)).astype(F32)
            prev = (((ratio * sample).astype(F32) - (ca * m0).astype(F32)).astype(F32) - (F32(F32(0.5) * ca) * d1).astype(F32)).astype(F32)
        self.lower_order_nums = min(self.lower_order_nums + 1, 2)
        self.pred_original_sample = x0
        return prev
