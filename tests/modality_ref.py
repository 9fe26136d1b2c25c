"""Restated modality-guidance combine with per-modality weights -- TEST INFRASTRUCTURE (numpy, float32 like the reference).

The reference combine (convofusion/models/modeltype/convofusion.py:527-541; restated in oracle.sampler_ref.cfg_combine) hard-codes
w_c = 1 for the five single-modality chunks and w_c = 0 for the full-conditioning chunk.  With w_c edited it computes, per chunk,
``self.guidance_scale * w_c * (e_c - e_0)``: the factor ``guidance_scale * w_c`` is a Python (double) product, applied to the float32
difference as one float32 factor, and the six terms are summed left to right before e_0 is added.  ``cfg_combine_weighted`` restates
that with one factor per utterance; ``weight_table`` builds the factors; ``golden_weights`` is the schedule of the
traj_modality_*.npz goldens (tests/golden/make_golden_modality.py).
"""
import numpy as np

F32 = np.float32
CFG_CHUNKS = 7
NAMES = ("text", "audio", "spk", "apb", "lsnid", "all")     # guidance chunks 1 - 6, the reference's variable names
REFERENCE = (1.0, 1.0, 1.0, 1.0, 1.0, 0.0)


def weight_table(w, guidance_scale):
    """w: [N, B, 6] weights w_c -> float32 [N, B, 8] factors float32(guidance_scale * w_c) (product in double), column 0 = 0."""
    w = np.asarray(w, dtype=np.float64)
    out = np.zeros(w.shape[:2] + (8,), dtype=F32)
    out[:, :, 1:7] = (float(guidance_scale) * w).astype(F32)
    return out


def cfg_combine_weighted(noise_pred, factors):
    """noise_pred [7B, ...] chunk-major (all_drop, text_only, audio_only, spk_only, apb_only, lsnid_only, full); factors [B, 8] float32 of
    this iteration (column k = chunk k's factor).  e_0 + (((((n_1 + n_2) + n_3) + n_4) + n_5) + n_6), n_k = factor_k * (e_k - e_0)."""
    u, t, a, s, p, i, f = np.split(noise_pred, CFG_CHUNKS, axis=0)
    B = u.shape[0]
    w = np.asarray(factors, dtype=F32).reshape((B, 8) + (1,) * (u.ndim - 1))
    n_text = w[:, 1] * (t - u)
    n_audio = w[:, 2] * (a - u)
    n_spk = w[:, 3] * (s - u)
    n_apb = w[:, 4] * (p - u)
    n_lsn = w[:, 5] * (i - u)
    n_all = w[:, 6] * (f - u)
    return (u + (n_text + n_audio + n_spk + n_apb + n_lsn + n_all)).astype(F32)


def golden_weights(N):
    """[N, 2, 6] weights of the goldens: utterance 0 guided only inside iterations [0.3 N, 0.7 N) (an interval schedule), utterance 1 on a
    linear ramp (i + 1) / N; apb is 0 for both (a chunk a pruned run drops), the full-conditioning chunk is guided for utterance 1."""
    w = np.zeros((N, 2, 6), dtype=np.float64)
    for i in range(N):
        if 0.3 * N <= i < 0.7 * N:
            w[i, 0] = (2.0, 0.5, 1.0, 0.0, 1.5, 0.0)
        w[i, 1] = np.array((1.0, 1.5, 0.5, 0.0, 0.0, 0.25)) * ((i + 1) / N)
    return w
