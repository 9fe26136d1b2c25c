"""ctypes binding of libcfdenoise.so (the C ABI in include/cfdenoise.h).

There is no CPU fallback: importing this module without the built library, or creating a handle
without an MI355X, raises.
"""
import ctypes as C
import os

import torch  # noqa: F401  -- must be imported BEFORE the library: torch bundles its own libamdhip64 and the two
#                               HIP runtimes must not both be loaded (loading ours first breaks device discovery)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CFD_LIB", os.path.join(HERE, "libcfdenoise.so"))  # CFD_LIB: developer override

NUM_MEM = 5
MEM_NAMES = ("spkemb", "alsn", "tlsn", "apb", "lsnemb")
PROF_CLASSES = ("gemm_token", "gemm_mem", "gemm_attn", "rows", "other", "xattn")

SYMBOLS = [
    "cfd_create", "cfd_destroy", "cfd_last_error", "cfd_source_hash", "cfd_load_tensor", "cfd_finalize_weights",
    "cfd_set_timestep_table", "cfd_forward", "cfd_forward_same_memories", "cfd_sample_begin", "cfd_sample_steps", "cfd_sample_position",
    "cfd_sample_read", "cfd_scheduler_step", "cfd_add_noise", "cfd_philox_normal", "cfd_profile_forward",
    "cfd_test_gemm", "cfd_debug_stop_stage", "cfd_debug_read", "cfd_bench_gemm", "cfd_linear_act",
    "cfd_layer_norm", "cfd_mha", "cfd_add", "cfd_zero_rows", "cfd_gemm_f32", "cfd_softmax", "cfd_softmax_bwd",
    "cfd_layer_norm_bwd", "cfd_ew", "cfd_weg_focus", "cfd_sample_write", "cfd_sample_inpaint", "cfd_weg_eval", "cfd_dyadic_steps",
    "cfd_sample_census", "cfd_dpmsolver_step", "cfd_test_step_coefficients", "cfd_test_gemm_epi",
    "cfd_vae_encode", "cfd_sample_begin_weighted", "cfd_sample_begin_edit", "cfd_sample_begin_invert", "cfd_sample_begin_anchored",
    "cfd_sample_begin_tied", "cfd_ddpm_invert", "cfd_sample_begin_replay", "cfd_sample_parallel", "cfd_test_picard_stride",
    "cfd_test_picard_sweep", "cfd_debug_weg_stop", "cfd_debug_weg_fill", "cfd_scheduler_step_pred", "cfd_dpmsolver_step_pred",
    "cfd_debug_forward_operands", "cfd_denoise_vjp", "cfd_debug_live_buffers", "cfd_vae_decode_vjp", "cfd_denoise_vjp_mem",
    "cfd_vae_decode", "cfd_vae_decode_sweep", "cfd_vae_decode_ticket", "cfd_debug_vae_workspace", "cfd_denoise_guide", "cfd_guide_tie_csr",
    "cfd_denoise_guide_pose", "cfd_weg_step", "cfd_test_weg_focus_rows", "cfd_t5_encode", "cfd_audio_encode",
    "cfd_audio_power", "cfd_motion_eval", "cfd_motion_diversity", "cfd_audio_onsets", "cfd_audio_encoder_vjp",
]

# cfd_sample_args.prediction_type / the _pred entry points, by the schedulers' config string
PREDICTION_TYPES = {"epsilon": 0, "sample": 1}


class CfdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libcfdenoise error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("latent_dim", C.c_int), ("text_encoded_dim", C.c_int), ("ff_size", C.c_int),
                ("num_layers", C.c_int), ("num_heads", C.c_int), ("device", C.c_int)]


class Memory(C.Structure):
    _fields_ = [("data", C.c_void_p), ("row_map", C.c_void_p), ("key_padding_mask", C.c_void_p),
                ("U", C.c_int), ("S", C.c_int)]


class Mat(C.Structure):
    """cfd_mat: element (z1, z2, r, c) = p[z1*b1 + z2*b2 + r*rs + c*cs]."""
    _fields_ = [("p", C.c_void_p), ("rs", C.c_longlong), ("cs", C.c_longlong), ("b1", C.c_longlong), ("b2", C.c_longlong)]


class DyadicProj(C.Structure):
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("hidden", C.c_int), ("out_dim", C.c_int),
                ("spk_a", C.c_void_p), ("spk_b", C.c_void_p), ("tmp", C.c_void_p)]


class SampleArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("L", C.c_int), ("G", C.c_int), ("guidance_weight", C.c_float * 8),
                ("scheduler", C.c_int), ("num_train_timesteps", C.c_int), ("num_inference_steps", C.c_int),
                ("clip_sample", C.c_int), ("eta", C.c_float), ("set_alpha_to_one", C.c_int),
                ("steps_offset", C.c_int), ("alphas_cumprod", C.c_void_p), ("init_latents", C.c_void_p),
                ("step_noise", C.c_void_p), ("seed", C.c_uint64), ("first_utterance", C.c_uint32),
                ("preseq", C.c_void_p), ("preseq_len", C.c_int), ("mem", Memory * NUM_MEM),
                ("skip_zero_weight_chunks", C.c_int), ("dynamic_memory_mask", C.c_int),
                ("timesteps", C.c_void_p), ("num_timesteps", C.c_int), ("prediction_type", C.c_int),   # (in the padding in front of att_ring)
                ("att_ring", C.c_void_p * NUM_MEM),
                ("operand_policy", C.c_int), ("census_tau", C.c_float)]


CENSUS_MAX_LAYERS = 16


class EditArgs(C.Structure):
    """cfd_edit_args: the source latents (dev [B][L][128]), the keep mask (dev uint8 [B][L] or NULL) and the first iteration k0."""
    _fields_ = [("source", C.c_void_p), ("keep", C.c_void_p), ("first_iteration", C.c_int)]


class TieArgs(C.Structure):
    """cfd_tie_args: the tie table (dev int32 [B][L]: -1 or the flat index b' * L + l' of the token's source in the same run)."""
    _fields_ = [("tie", C.c_void_p)]


class AnchorArgs(C.Structure):
    """cfd_anchor_args: an inversion trajectory (dev [steps + 1][B][L][128]), its steps / B / L, and the keep mask (dev uint8 [B][L] or NULL)."""
    _fields_ = [("trajectory", C.c_void_p), ("steps", C.c_int), ("B", C.c_int), ("L", C.c_int), ("keep", C.c_void_p)]


class DdpmInvertArgs(C.Structure):
    """cfd_ddpm_invert_args: source (dev [B][L][128]), HOST weight table [N][B][8] or NULL with prune, level noise (dev [N][B][L][128] or
    NULL: Philox stream 2), the outputs trajectory (dev [N + 1][B][L][128]) and noise (dev [N][B][L][128]), levels per batch (0: from the
    workspace budget in bytes, 0: 4 GiB)."""
    _fields_ = [("source", C.c_void_p), ("weights", C.c_void_p), ("prune", C.c_int), ("level_noise", C.c_void_p), ("trajectory", C.c_void_p),
                ("noise", C.c_void_p), ("levels_per_batch", C.c_int), ("workspace_bytes", C.c_size_t)]


class ParallelArgs(C.Structure):
    """cfd_parallel_args: HOST weight table [N][B][8] or NULL with prune, the tolerance, levels per batch (0: from the workspace budget in
    bytes, 0: 4 GiB), max_sweeps (0: N), the outputs latents (dev [B][L][128]) and trajectory (dev [N + 1][B][L][128] or NULL)."""
    _fields_ = [("weights", C.c_void_p), ("prune", C.c_int), ("tolerance", C.c_float), ("levels_per_batch", C.c_int),
                ("workspace_bytes", C.c_size_t), ("max_sweeps", C.c_int), ("latents", C.c_void_p), ("trajectory", C.c_void_p)]


class ParallelStats(C.Structure):
    """cfd_parallel_stats: J, G_eval and the sweeps of a cfd_sample_parallel call; strides: HOST int32 [strides_capacity] or NULL."""
    _fields_ = [("levels_per_batch", C.c_int), ("chunks_evaluated", C.c_int), ("sweeps", C.c_int), ("strides", C.c_void_p),
                ("strides_capacity", C.c_int)]


class ReplayArgs(C.Structure):
    """cfd_replay_args: a recorded noise space (trajectory dev [steps + 1][B][L][128], noise dev [steps][B][L][128]), its steps / B / L, the
    keep mask (dev uint8 [B][L] or NULL) and the first iteration k0."""
    _fields_ = [("trajectory", C.c_void_p), ("noise", C.c_void_p), ("steps", C.c_int), ("B", C.c_int), ("L", C.c_int), ("keep", C.c_void_p),
                ("first_iteration", C.c_int)]


class Census(C.Structure):
    """cfd_census: the attention-concentration census of a sampling run (cfd_sample_census)."""
    _fields_ = [("tau", C.c_float), ("measured", C.c_int), ("iterations", C.c_int), ("worst_layer", C.c_int), ("peak_max", C.c_float),
                ("rows_over", C.c_uint32), ("rows_seen", C.c_uint32), ("layer_peak", C.c_float * CENSUS_MAX_LAYERS),
                ("layer_over", C.c_uint32 * CENSUS_MAX_LAYERS)]


class WegArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("L", C.c_int), ("timestep", C.c_int), ("latents", C.c_void_p), ("mem", Memory * NUM_MEM),
                ("tok_off", C.c_void_p), ("tok_idx", C.c_void_p), ("last", C.c_int), ("kernel3", C.c_float * 3), ("reuse_memory_side", C.c_int)]


class WegRowsArgs(C.Structure):
    """cfd_weg_rows_args: one word-excitation-guidance evaluation and gated update of B rows that are each their own utterance
    (cfd_weg_step)."""
    _fields_ = [("B", C.c_int), ("L", C.c_int), ("timestep", C.c_int), ("latents", C.c_void_p), ("mem", Memory * NUM_MEM),
                ("tok_off", C.c_void_p), ("tok_idx", C.c_void_p), ("last_rows", C.c_void_p), ("kernel3", C.c_float * 3),
                ("row_step", C.c_void_p), ("tie", C.c_void_p), ("tie_csr", C.c_void_p), ("reuse_memory_side", C.c_int)]


class VjpArgs(C.Structure):
    """cfd_vjp_args: one denoiser forward whose vector-Jacobian product with respect to the sample is wanted (cfd_denoise_vjp)."""
    _fields_ = [("Be", C.c_int), ("L", C.c_int), ("timestep", C.c_int), ("sample", C.c_void_p), ("mem", Memory * NUM_MEM)]


class GuideArgs(C.Structure):
    """cfd_guide_args: one key-pose guided update of B latent rows under n evaluated guidance chunks (cfd_denoise_guide)."""
    _fields_ = [("B", C.c_int), ("L", C.c_int), ("n", C.c_int), ("timestep", C.c_int), ("sqrt_acp", C.c_float), ("sqrt_1m_acp", C.c_float),
                ("x", C.c_void_p), ("mem", Memory * NUM_MEM), ("w", C.c_void_p), ("target", C.c_void_p), ("mask", C.c_void_p),
                ("inv_n", C.c_float), ("step", C.c_float), ("tie", C.c_void_p), ("tie_csr", C.c_void_p), ("reuse_memory_side", C.c_int)]


class GuidePose(C.Structure):
    """cfd_guide_pose: the pose-space loss of one guided update (cfd_denoise_guide_pose)."""
    _fields_ = [("wpack", C.c_void_p), ("d_model", C.c_int), ("num_heads", C.c_int), ("ff_size", C.c_int), ("num_layers", C.c_int),
                ("nframes", C.c_int), ("lengths", C.c_void_p), ("target", C.c_void_p), ("frame_mask", C.c_void_p), ("feature_mask", C.c_void_p),
                ("inv_n", C.c_float)]


class VaeDecodeVjpArgs(C.Structure):
    """cfd_vae_decode_vjp_args: one ConvoFusionVae.decode whose vector-Jacobian product with respect to z is wanted (cfd_vae_decode_vjp)."""
    _fields_ = [("wpack", C.c_void_p), ("d_model", C.c_int), ("num_heads", C.c_int), ("ff_size", C.c_int), ("num_layers", C.c_int),
                ("bs", C.c_int), ("nframes", C.c_int), ("n_chunks", C.c_int), ("z", C.c_void_p), ("lengths", C.c_void_p),
                ("d_feats", C.c_void_p)]


class VaeDecodeArgs(C.Structure):
    """cfd_vae_decode_args: one ConvoFusionVae.decode on the fused forward (cfd_vae_decode); cfd_vae_decode_vjp_args without the cotangent."""
    _fields_ = VaeDecodeVjpArgs._fields_[:-1]


class T5Args(C.Structure):
    """cfd_t5_args: one T5 text-encoder call (cfd_t5_encode)."""
    _fields_ = [("wpack", C.c_void_p), ("vocab", C.c_int), ("d_model", C.c_int), ("d_kv", C.c_int), ("num_heads", C.c_int), ("d_ff", C.c_int),
                ("num_layers", C.c_int), ("gated_act", C.c_int), ("eps", C.c_float), ("n_seq", C.c_int), ("T", C.c_int), ("ids", C.c_void_p),
                ("mask", C.c_void_p), ("rel_bias", C.c_void_p), ("proj_w", C.c_void_p), ("proj_b", C.c_void_p), ("proj_dim", C.c_int)]


class AudioArgs(C.Structure):
    """cfd_audio_args: one log-Mel front-end call (cfd_audio_encode)."""
    _fields_ = [("wave", C.c_void_p), ("n_wave", C.c_int), ("n_samples", C.c_longlong), ("normalize", C.c_int), ("n_fft", C.c_int), ("hop", C.c_int),
                ("n_mels", C.c_int), ("twiddle", C.c_void_p), ("window", C.c_void_p), ("melfb", C.c_void_p), ("mel_range", C.c_void_p),
                ("amin", C.c_float), ("top_db", C.c_float), ("n_win", C.c_int), ("win_start", C.c_void_p), ("win_frames", C.c_int),
                ("w0", C.c_void_p), ("b0", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("hidden", C.c_int), ("latent", C.c_int), ("act_chunk", C.c_int), ("act_amin_power", C.c_float), ("act_thresh_power", C.c_float)]


class AudioEncArgs(C.Structure):
    """cfd_audio_enc_args: AudioConvEncoder's input rows, widths and parameters (cfd_audio_encoder_vjp)."""
    _fields_ = [("x", C.c_void_p), ("n_rows", C.c_longlong), ("in_dim", C.c_int), ("hidden", C.c_int), ("latent", C.c_int),
                ("w0", C.c_void_p), ("b0", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p)]


class OnsetArgs(C.Structure):
    """cfd_onset_args: one onset-detection call (cfd_audio_onsets)."""
    _fields_ = [("wave", C.c_void_p), ("n_wave", C.c_int), ("n_samples", C.c_longlong), ("normalize", C.c_int), ("n_fft", C.c_int), ("hop", C.c_int),
                ("n_mels", C.c_int), ("twiddle", C.c_void_p), ("window", C.c_void_p), ("melfb", C.c_void_p), ("mel_range", C.c_void_p),
                ("amin", C.c_float), ("top_db", C.c_float), ("lag", C.c_int), ("pad_frames", C.c_int), ("pre_max", C.c_int), ("post_max", C.c_int),
                ("pre_avg", C.c_int), ("post_avg", C.c_int), ("wait", C.c_int), ("delta", C.c_float), ("time_hop", C.c_int), ("time_sr", C.c_double),
                ("capacity", C.c_int), ("envelope", C.c_void_p), ("rms", C.c_void_p), ("frames_raw", C.c_void_p), ("frames", C.c_void_p)]


class MotionEvalArgs(C.Structure):
    """cfd_motion_eval_args: one motion-evaluation call (cfd_motion_eval)."""
    _fields_ = [("pred", C.c_void_p), ("target", C.c_void_p), ("semantic", C.c_void_p), ("n_seq", C.c_int), ("n_frames", C.c_int),
                ("stride", C.c_longlong), ("fps", C.c_double), ("order", C.c_int), ("sigma", C.c_double), ("srgr_threshold", C.c_double),
                ("onset_off", C.c_void_p), ("onset_t", C.c_void_p), ("n_onsets", C.c_int), ("fgd_pack", C.c_void_p), ("feature_length", C.c_int), ("embed_raw", C.c_int),
                ("l1div", C.c_void_p), ("srgr", C.c_void_p), ("srgr_count", C.c_void_p), ("jitter", C.c_void_p), ("beats", C.c_void_p),
                ("align", C.c_void_p), ("processed", C.c_void_p), ("embedding", C.c_void_p), ("stats", C.c_void_p)]


# cfd_test_epi_args.kind (include/cfdenoise_dev.h)
EPI_F32, EPI_SPLIT, EPI_RESID, EPI_RESID_STAT, EPI_QKVT, EPI_LN_F32, EPI_LN_SPLIT, EPI_LN_QKVT = range(8)


class TestEpiArgs(C.Structure):
    """cfd_test_epi_args: one launch of the split-pair GEMM with one of the product's epilogues (cfd_test_gemm_epi)."""
    _fields_ = [("kind", C.c_int), ("I", C.c_int), ("J", C.c_int), ("K", C.c_int), ("tile_cfg", C.c_int), ("gelu", C.c_int),
                ("perm32", C.c_int), ("natural", C.c_int), ("X", C.c_void_p), ("Y", C.c_void_p), ("y_sp", C.c_void_p),
                ("bias", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("ln_stat", C.c_void_p), ("ln_eps", C.c_float),
                ("x", C.c_void_p), ("out", C.c_void_p), ("out2", C.c_void_p), ("stat", C.c_void_p), ("tile_cfg_used", C.c_int)]


# cfd_test_picard_args.stages (include/cfdenoise_dev.h)
PICARD_FILL, PICARD_LOAD, PICARD_STEP, PICARD_SCAN = 1, 2, 4, 8


class TestPicardArgs(C.Structure):
    """cfd_test_picard_args: the kernels of a cfd_sample_parallel sweep around the forward, on the caller's predictions
    (cfd_test_picard_sweep)."""
    _fields_ = [("stages", C.c_int), ("B", C.c_int), ("L", C.c_int), ("G", C.c_int), ("N", C.c_int), ("slots", C.c_int), ("base", C.c_int),
                ("off", C.c_int), ("J", C.c_int), ("ring", C.c_void_p), ("fill_src", C.c_int), ("fill_lo", C.c_int), ("fill_hi", C.c_int),
                ("sample_sp", C.c_void_p), ("eps", C.c_void_p), ("coef", C.c_void_p), ("Gc", C.c_int), ("pos", C.c_int * 8),
                ("w", C.c_float * 8), ("clip", C.c_int), ("wtab", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64),
                ("first_utterance", C.c_uint32), ("s", C.c_void_p), ("err", C.c_void_p)]


_lib = None


def _built_hash():
    """The source hash embedded in the built library file ("missing" if there is none)."""
    try:
        with open(LIB_PATH, "rb") as f:
            blob = f.read()
    except OSError:
        return "missing"
    k = blob.find(b"cfd-src-hash:")
    return blob[k + 13:k + 29].decode(errors="replace") if k >= 0 else "missing"


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m convofusion_amd.build` "
            "(hipcc --offload-arch=gfx950).  convofusion_amd has no CPU fallback.")
    if "CFD_LIB" not in os.environ:      # (a developer override is taken as it is)
        from . import build
        want = build.source_hash()
        if _built_hash() != want:
            # built from other sources (an update changed csrc/ or include/cfdenoise.h): a stale library would mis-read
            # struct arguments instead of failing.  hipcc needs no GPU, so rebuild before the file is mapped; without hipcc refuse.
            # One process rebuilds (file lock: the ranks of a multi-GPU launch all get here at once); build.build() writes to a
            # temporary name and renames it into place, and the hash is read again before the file is mapped.
            import fcntl
            try:
                lock = open(LIB_PATH + ".lock", "w")
            except OSError as e:    # read-only install: the package directory cannot hold the lock (nor a rebuilt library)
                raise ImportError(f"{LIB_PATH} was built from other sources (hash {_built_hash()}, sources {want}) and the package "
                                  f"directory is not writable ({e}); run `python -m convofusion_amd.build` where it is") from e
            with lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    have = _built_hash()
                    if have != want:
                        try:
                            build.build(force=True)
                        except Exception as e:
                            raise ImportError(f"{LIB_PATH} was built from other sources (hash {have}, sources {want}) and could not be "
                                              f"rebuilt ({e}); run `python -m convofusion_amd.build`") from e
                        if _built_hash() != want:
                            raise ImportError(f"{LIB_PATH}: rebuilt library still carries hash {_built_hash()}, sources are {want}")
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
    lib = C.CDLL(LIB_PATH)
    lib.cfd_last_error.restype = C.c_char_p
    lib.cfd_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    lib.cfd_destroy.argtypes = [C.c_void_p]
    lib.cfd_destroy.restype = None
    lib.cfd_load_tensor.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.cfd_finalize_weights.argtypes = [C.c_void_p]
    lib.cfd_set_timestep_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.cfd_forward_same_memories.argtypes = [C.c_void_p]
    lib.cfd_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                C.POINTER(Memory), C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]
    lib.cfd_sample_begin.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.c_void_p]
    lib.cfd_sample_begin_weighted.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    lib.cfd_sample_begin_edit.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.POINTER(EditArgs), C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                          C.c_void_p]
    lib.cfd_sample_begin_tied.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.POINTER(EditArgs), C.POINTER(TieArgs), C.c_void_p, C.c_int,
                                          C.POINTER(C.c_int), C.c_void_p]
    lib.cfd_sample_begin_invert.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    lib.cfd_sample_begin_anchored.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.POINTER(AnchorArgs), C.c_void_p, C.c_int,
                                              C.POINTER(C.c_int), C.c_void_p]
    lib.cfd_ddpm_invert.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.POINTER(DdpmInvertArgs), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.c_void_p]
    lib.cfd_sample_parallel.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.POINTER(ParallelArgs), C.POINTER(ParallelStats), C.c_void_p]
    lib.cfd_sample_begin_replay.argtypes = [C.c_void_p, C.POINTER(SampleArgs), C.POINTER(ReplayArgs), C.c_void_p, C.c_int,
                                            C.POINTER(C.c_int), C.c_void_p]
    lib.cfd_sample_steps.argtypes = [C.c_void_p, C.c_int]
    lib.cfd_sample_position.argtypes = [C.c_void_p]
    lib.cfd_sample_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.cfd_sample_census.argtypes = [C.c_void_p, C.POINTER(Census)]
    lib.cfd_scheduler_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.cfd_dpmsolver_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]
    lib.cfd_scheduler_step_pred.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.cfd_dpmsolver_step_pred.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.cfd_test_step_coefficients.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int,
                                               C.POINTER(C.c_float)]
    lib.cfd_test_picard_stride.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int]
    lib.cfd_test_picard_sweep.argtypes = [C.c_void_p, C.POINTER(TestPicardArgs), C.c_void_p]
    lib.cfd_add_noise.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]
    lib.cfd_philox_normal.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_void_p]
    lib.cfd_profile_forward.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.cfd_test_gemm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_void_p]
    lib.cfd_test_gemm_epi.argtypes = [C.c_void_p, C.POINTER(TestEpiArgs), C.c_void_p]
    lib.cfd_bench_gemm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    lib.cfd_linear_act.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p]
    lib.cfd_layer_norm.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    lib.cfd_mha.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                            C.c_void_p, C.c_void_p]
    lib.cfd_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.cfd_zero_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
    lib.cfd_vae_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                   C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.cfd_gemm_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Mat), C.POINTER(Mat), C.POINTER(Mat),
                                 C.c_void_p, C.c_float, C.c_int, C.c_void_p]
    lib.cfd_softmax.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.cfd_softmax_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
    lib.cfd_layer_norm_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float,
                                       C.c_int, C.c_void_p]
    lib.cfd_ew.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_longlong,
                           C.c_longlong, C.c_float, C.c_void_p]
    lib.cfd_weg_focus.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_sample_write.argtypes = [C.c_void_p, C.c_void_p]
    lib.cfd_sample_inpaint.argtypes = [C.c_void_p]
    lib.cfd_weg_eval.argtypes = [C.c_void_p, C.POINTER(WegArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
    lib.cfd_weg_step.argtypes = [C.c_void_p, C.POINTER(WegRowsArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_test_weg_focus_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_denoise_vjp.argtypes = [C.c_void_p, C.POINTER(VjpArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_denoise_vjp_mem.argtypes = [C.c_void_p, C.POINTER(VjpArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]
    lib.cfd_denoise_guide.argtypes = [C.c_void_p, C.POINTER(GuideArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_guide_tie_csr.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
    lib.cfd_denoise_guide_pose.argtypes = [C.c_void_p, C.POINTER(GuideArgs), C.POINTER(GuidePose), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
    lib.cfd_vae_decode_vjp.argtypes = [C.c_void_p, C.POINTER(VaeDecodeVjpArgs), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_vae_decode.argtypes = [C.c_void_p, C.POINTER(VaeDecodeArgs), C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    lib.cfd_vae_decode_sweep.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_vae_decode_ticket.argtypes = [C.c_void_p]
    lib.cfd_vae_decode_ticket.restype = C.c_uint64
    lib.cfd_t5_encode.argtypes = [C.c_void_p, C.POINTER(T5Args), C.c_void_p, C.c_void_p]
    lib.cfd_audio_encode.argtypes = [C.c_void_p, C.POINTER(AudioArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_audio_onsets.argtypes = [C.c_void_p, C.POINTER(OnsetArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_audio_encoder_vjp.argtypes = [C.c_void_p, C.POINTER(AudioEncArgs), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
    lib.cfd_motion_eval.argtypes = [C.c_void_p, C.POINTER(MotionEvalArgs), C.c_void_p]
    lib.cfd_motion_diversity.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.cfd_audio_power.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cfd_debug_vae_workspace.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    lib.cfd_dyadic_steps.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DyadicProj), C.c_int]
    lib.cfd_debug_stop_stage.argtypes = [C.c_void_p, C.c_int]
    lib.cfd_debug_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    lib.cfd_debug_weg_stop.argtypes = [C.c_void_p, C.c_int]
    lib.cfd_debug_forward_operands.argtypes = [C.c_void_p, C.c_int]
    lib.cfd_debug_weg_fill.argtypes = [C.c_void_p, C.c_float]
    lib.cfd_debug_live_buffers.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    for name in SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("cfd_last_error", "cfd_destroy", "cfd_source_hash", "cfd_vae_decode_ticket"):
            fn.restype = C.c_int
    _lib = lib
    return lib


def wrote(*tensors):
    """Tell torch that the library wrote these caller-owned tensors through their raw pointers: bumps their version counters
    (``torch.autograd.graph.increment_version``), which is what ``Denoiser.forward`` keys its reuse of the memories' projections on --
    a ctypes write is otherwise invisible to it (the same-memories staleness hole of round 5)."""
    live = [t for t in tensors if t is not None]
    if live:
        torch.autograd.graph.increment_version(live)


def check(code):
    if code != 0:
        raise CfdError(code, load().cfd_last_error().decode())
    return code


def create_handle(device_index=0, num_layers=9, latent_dim=128, d_model=512, ff_size=1024, num_heads=4):
    lib = load()
    cfg = Config(latent_dim, d_model, ff_size, num_layers, num_heads, device_index)
    h = C.c_void_p()
    check(lib.cfd_create(C.byref(cfg), C.byref(h)))
    return h
