"""Motion evaluation on the HIP path: Frechet gesture distance (FGD), beat alignment, diversity, L1 diversity, SRGR and jitter of decoded
motions [B, T, 189] in one library call per batch (cfd_motion_eval, csrc/metrics_eval.hpp) plus one for the diversity
(cfd_motion_diversity).

The reference scores its results on the host with quant_eval/ (metric_eval.py, dyadic_eval.py, jitter_metric.py, motion_autoencoder.py):
one motion at a time through a 114 M-parameter auto-encoder and a Python double loop over all pairs.  ``MotionEvaluator.update`` takes the
tensor ``ConvoFusionVae.decode`` returns, without a host copy.  The audio onsets of the beat alignment are detected on the device too when
the waveforms are given (``audio=``: ``audio.OnsetDetector``, what the reference's ``Alignment.load_audio`` gets from librosa; librosa is
not a dependency and agreement with it is not verified).  What stays with the caller: resampling, decoding audio files other than plain
16-bit PCM, and the FGD net's checkpoint.

``FGDNet`` mirrors ``HalfEmbeddingNet``'s pose encoder and its state-dict keys.  ``nn.LeakyReLU(True)`` in its ``out_net``
(motion_autoencoder.py:52,55,58) sets negative_slope = True = 1.0: the identity.  So ``out_net`` followed by ``fc_mu`` is one affine map
59 F -> F, folded here in float64: 17 700 x 300 numbers at the product width instead of 113 M.  The eval-mode BatchNorms are folded too.
Not built: the commented-out ``smoothing()``, the decoder half of the auto-encoder, training.  Inference only, CUDA
tensors only, no CPU fallback.
"""
import ctypes as C
import glob
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib

FEAT, JOINTS = 189, 63
T_MIN, T_MAX, EMB_FRAMES = 24, 128, 128
TRACK_JOINTS = (5, 6, 7, 9, 10, 11)          # the beat tracks of cfd_motion_eval, in this order; the alignment uses the last (right wrist)
DIV_MAX_N = 8192


def pack_floats(F):
    """Floats of the folded pack (me_pack_floats of csrc/metrics_eval.hpp)."""
    F = int(F)
    return F * 3 * FEAT + F + 2 * F * 3 * F + 2 * F + 2 * F * 8 * F + 2 * F + F * 6 * F + F + F * 59 * F + F


def _conv_norm_act(cin, cout, down):
    return nn.Sequential(nn.Conv1d(cin, cout, 4 if down else 3, 2 if down else 1), nn.BatchNorm1d(cout), nn.LeakyReLU(0.2, True))


class _PoseEncoder(nn.Module):
    """The parameter layout of the reference's PoseEncoderConv (motion_autoencoder.py:39-63) for 128 frames."""

    def __init__(self, dim, F):
        super().__init__()
        self.net = nn.Sequential(_conv_norm_act(dim, F, False), _conv_norm_act(F, 2 * F, False), _conv_norm_act(2 * F, 2 * F, True),
                                 nn.Conv1d(2 * F, F, 3))
        # (the activations carry no parameters; the slope of 1.0 is what nn.LeakyReLU(True) means)
        self.out_net = nn.Sequential(nn.Linear(59 * F, 20 * F), nn.BatchNorm1d(20 * F), nn.LeakyReLU(1.0),
                                     nn.Linear(20 * F, 4 * F), nn.BatchNorm1d(4 * F), nn.LeakyReLU(1.0),
                                     nn.Linear(4 * F, 2 * F), nn.BatchNorm1d(2 * F), nn.LeakyReLU(1.0),
                                     nn.Linear(2 * F, F))
        self.fc_mu = nn.Linear(F, F)
        self.fc_logvar = nn.Linear(F, F)


def _bn_affine(bn):
    """Eval-mode BatchNorm as y = s x + o, float64."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return s, bn.bias.detach().double() - bn.running_mean.detach().double() * s


class FGDNet(nn.Module):
    """``HalfEmbeddingNet(pose_length, pose_dim, feature_length)``'s embedding on the device.  Same constructor, same state-dict keys
    under ``pose_encoder.``; ``decoder.*`` entries of a checkpoint are ignored; keys may carry the ``module.`` prefix that
    ``load_fidnet_checkpoints`` (metric_eval.py:359-373) strips.  ``forward(poses [B, 128, 189])`` returns mu [B, feature_length]."""

    def __init__(self, pose_length=128, pose_dim=189, feature_length=300):
        super().__init__()
        if int(pose_length) != EMB_FRAMES or int(pose_dim) != FEAT:
            raise ValueError(f"FGDNet: the HIP path is built for pose_length {EMB_FRAMES} and pose_dim {FEAT} (got {pose_length}, {pose_dim})")
        if not 1 <= int(feature_length) <= 1024:
            raise ValueError(f"FGDNet: 1 <= feature_length <= 1024 (got {feature_length})")
        self.feature_length = int(feature_length)
        self.pose_encoder = _PoseEncoder(FEAT, self.feature_length)
        self._packs = {}

    @staticmethod
    def map_state_dict(state):
        """The reference's prefix rule, then without the decoder: if the FIRST key contains "module", the first 7 characters of every
        key up to the first one without it are cut (and the rest dropped, as the reference's loop breaks there)."""
        keys = list(state.keys())
        if keys and "module" in keys[0]:
            out = {}
            for k in keys:
                if "module" not in k:
                    break
                out[k[7:]] = state[k]
            state = out
        return {k: v for k, v in state.items() if not k.startswith("decoder.")}

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        self._packs = {}
        return super().load_state_dict(self.map_state_dict(state_dict), strict=strict, **kwargs)

    def folded(self):
        """The folded pack's parts in float64: [(W [N, k C_in], b [N]) x 4 convolutions, (W [F, 59 F] frame-major, b [F])]."""
        if self.training:
            raise NotImplementedError("the HIP FGDNet is inference-only (call .eval())")
        enc, F = self.pose_encoder, self.feature_length
        parts = []
        for i in range(4):
            conv = enc.net[i][0] if i < 3 else enc.net[3]
            w, b = conv.weight.detach().double(), conv.bias.detach().double()
            if i < 3:
                s, o = _bn_affine(enc.net[i][1])
                w, b = w * s[:, None, None], b * s + o
            parts.append((w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous(), b))          # [N][kk][c]
        # out_net and fc_mu, composed from the output side so every product has F rows
        for m in enc.out_net:
            if isinstance(m, nn.LeakyReLU) and float(m.negative_slope) != 1.0:
                raise ValueError("FGDNet: out_net's activations must have negative_slope 1.0 (the reference's nn.LeakyReLU(True))")
        Wm, bm = enc.fc_mu.weight.detach().double(), enc.fc_mu.bias.detach().double()
        for idx in (9, 7, 6, 4, 3, 1, 0):
            m = enc.out_net[idx]
            if isinstance(m, nn.Linear):
                bm = bm + Wm @ m.bias.detach().double()
                Wm = Wm @ m.weight.detach().double()
            else:
                s, o = _bn_affine(m)
                bm = bm + Wm @ o
                Wm = Wm * s[None, :]
        # flatten(1) of [B, F, 59] is channel-major (c * 59 + t); the device's rows are frame-major (t * F + c)
        Wm = Wm.reshape(F, F, 59).permute(0, 2, 1).reshape(F, 59 * F).contiguous()
        parts.append((Wm, bm))
        return parts

    def pack(self, device):
        """The folded pack on ``device``, float32 [pack_floats(F)], built once per device."""
        device = torch.device(device)
        p = self._packs.get(device)
        if p is None:
            flat = torch.cat([t.reshape(-1) for wb in self.folded() for t in wb]).to(torch.float32)
            assert flat.numel() == pack_floats(self.feature_length)
            p = flat.to(device)
            self._packs[device] = p
        return p

    def forward(self, poses):
        if self.training:
            raise NotImplementedError("the HIP FGDNet is inference-only (call .eval())")
        if poses.device.type != "cuda":
            raise NotImplementedError("FGDNet runs on an MI355X only (tensors must be on 'cuda'); no CPU fallback")
        return motion_eval(poses, fgd_net=self, want=("embedding",), embed_raw=True)["embedding"]


def _dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_default_detector = None


def detect_onsets(audio, n_seq, dev, onset_detector=None):
    """The CSR pair (offsets int32 [n_seq + 1], times float64 [capacity]) of the waveforms ``audio`` [n_seq, n_samples], float32 on ``dev``;
    everything is checked before device work."""
    global _default_detector
    if not isinstance(audio, torch.Tensor) or audio.dim() != 2 or not audio.is_floating_point() or int(audio.shape[0]) != n_seq:
        raise ValueError(f"motion_eval: audio must be a float tensor [{n_seq}, n_samples], one waveform per sequence")
    if audio.device != dev:
        raise ValueError("motion_eval: audio must be on pred's device")
    if onset_detector is None:
        if _default_detector is None:
            from .audio import OnsetDetector
            _default_detector = OnsetDetector()
        onset_detector = _default_detector
    return onset_detector.forward(audio).csr


def motion_eval(pred, target=None, semantic=None, onsets=None, *, fgd_net=None, stats=None, fps=25, order=10, sigma=0.3, srgr_threshold=0.3,
                want=None, embed_raw=False, audio=None, onset_detector=None):
    """One cfd_motion_eval call.  pred / target [B, T, >=189] float32 on the device (the last axis may be a wider view: its stride is
    passed on), semantic [B, T]; onsets: a list of B sequences of onset times in seconds (an empty one: no onsets), or a pair
    (offsets int32 [B + 1], times float64 [n]) already on the device.  audio: instead of onsets, the B waveforms [B, n_samples] float32
    on the device; their onsets are detected there by ``onset_detector`` (None: ``audio.OnsetDetector()``, the reference's settings) and
    go to the alignment on the same stream without visiting the host.  ``embed_raw``: the net embeds pred as it is (``FGDNet.forward``), not
    the processed motion (what the reference's scripts feed it).  Returns a dict of device tensors; ``want`` limits it."""
    if audio is not None and onsets is not None:
        raise ValueError("motion_eval: give onsets or audio, not both")
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3 or pred.dtype != torch.float32:
        raise ValueError("motion_eval: pred must be a float32 tensor [B, T, 189]")
    if pred.device.type != "cuda":
        raise NotImplementedError("convofusion_amd.metrics runs on an MI355X only (tensors must be on 'cuda'); no CPU fallback")
    dev = pred.device
    B, T, W = (int(v) for v in pred.shape)
    if W < FEAT:
        raise ValueError(f"motion_eval: a frame is {FEAT} floats (got {W})")
    if audio is not None:
        onsets = detect_onsets(audio, B, dev, onset_detector)

    def rows(x, name):
        if x.shape != pred.shape or x.dtype != torch.float32 or x.device != dev:
            raise ValueError(f"motion_eval: {name} must match pred's shape, dtype and device")
        if x.stride(2) != 1 or x.stride(0) != T * x.stride(1):
            x = x.contiguous()
        return x
    pred = rows(pred, "pred")
    if target is not None:
        target = rows(target, "target")
        if target.stride(1) != pred.stride(1):
            pred, target = pred[..., :FEAT].contiguous(), target[..., :FEAT].contiguous()
    if semantic is not None:
        semantic = semantic.to(device=dev, dtype=torch.float32).reshape(B, T).contiguous()
    a = _lib.MotionEvalArgs()
    a.pred, a.target, a.semantic = pred.data_ptr(), _dptr(target), _dptr(semantic)
    a.n_seq, a.n_frames, a.stride = B, T, pred.stride(1)
    a.fps, a.order, a.sigma, a.srgr_threshold = float(fps), int(order), float(sigma), float(srgr_threshold)
    keep = []
    if onsets is not None:
        if isinstance(onsets, tuple) and len(onsets) == 2 and isinstance(onsets[0], torch.Tensor):
            off, times = onsets
            if off.dtype != torch.int32 or off.numel() != B + 1 or times.dtype != torch.float64 or off.device != dev or times.device != dev:
                raise ValueError("motion_eval: onsets as tensors are (int32 [B + 1], float64 [n]) on pred's device")
        else:
            if len(onsets) != B:
                raise ValueError(f"motion_eval: {B} sequences but {len(onsets)} onset lists")
            lists = [np.asarray(o, dtype=np.float64).reshape(-1) for o in onsets]
            off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(o) for o in lists])]).astype(np.int32)).to(dev)
            times = torch.from_numpy(np.concatenate(lists + [np.zeros(1)])).to(dev)[:-1] if lists else torch.zeros(0, dtype=torch.float64, device=dev)
        keep += [off, times]
        a.onset_off, a.onset_t, a.n_onsets = off.data_ptr(), times.data_ptr() if times.numel() else None, int(times.numel())
    out = {}

    def give(name, shape, dtype, ok=True):
        if ok and (want is None or name in want):
            out[name] = torch.empty(shape, device=dev, dtype=dtype)
            setattr(a, name, out[name].data_ptr())
    give("l1div", (B,), torch.float64)
    give("srgr", (B,), torch.float64, target is not None and semantic is not None)
    give("srgr_count", (B,), torch.int32, target is not None and semantic is not None)
    give("jitter", (B,), torch.float64, target is not None)
    give("beats", (B, len(TRACK_JOINTS), T - 1), torch.uint8)
    give("align", (B,), torch.float64, onsets is not None)
    give("processed", (B, T, FEAT), torch.float32)
    if fgd_net is not None and T == EMB_FRAMES:
        pk = fgd_net.pack(dev)
        keep.append(pk)
        a.fgd_pack, a.feature_length, a.embed_raw = pk.data_ptr(), fgd_net.feature_length, int(bool(embed_raw))
        if embed_raw and pred.stride(1) != FEAT:
            pred = pred[..., :FEAT].contiguous()
            a.pred, a.stride = pred.data_ptr(), FEAT
        give("embedding", (B, fgd_net.feature_length), torch.float32)
        if stats is not None:
            F = fgd_net.feature_length
            if stats.dtype != torch.float64 or stats.numel() != 1 + F + F * F or stats.device != dev or not stats.is_contiguous():
                raise ValueError("motion_eval: stats must be a contiguous float64 tensor [1 + F + F * F] on pred's device")
            a.stats = stats.data_ptr()
    elif fgd_net is not None and want is not None and "embedding" in want:
        raise ValueError(f"motion_eval: the embedding net takes {EMB_FRAMES} frames (got {T})")
    from .conditioning import _engine_handle
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().cfd_motion_eval(_engine_handle(dev), C.byref(a), C.c_void_p(stream)))
    return out


def diversity(x):
    """The mean pairwise Euclidean distance of the rows of x [N, ...] (float32, on the device) as a float64 device scalar."""
    if x.device.type != "cuda":
        raise NotImplementedError("convofusion_amd.metrics runs on an MI355X only (tensors must be on 'cuda'); no CPU fallback")
    n = int(x.shape[0])
    x = x.reshape(n, -1).to(torch.float32).contiguous()
    out = torch.empty(1, device=x.device, dtype=torch.float64)
    from .conditioning import _engine_handle
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.load().cfd_motion_diversity(_engine_handle(x.device), C.c_void_p(x.data_ptr()), n, int(x.shape[1]), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(stream)))
    return out[0]


def frechet_distance_from_stats(stats_a, stats_b, eps=1e-6):
    """The reference's FIDCalculator (metric_eval.py:21-90) from two states [n | sum e | sum e e^T] in float64: mean, np.cov's ddof = 1
    covariance, scipy.linalg.sqrtm of the product, the eps fallback when that is not finite, the imaginary-part rule (1e10, as
    ``frechet_distance`` returns, when the diagonal's imaginary part exceeds 1e-3)."""
    try:
        from scipy import linalg
    except ImportError as e:
        raise RuntimeError("convofusion_amd.metrics: the Frechet distance needs scipy (scipy.linalg.sqrtm); install scipy -- the formula is "
                           "not replaced by another one") from e

    def moments(s):
        s = np.asarray(s, dtype=np.float64).reshape(-1)
        F = int(round((-1 + np.sqrt(1 + 4 * (s.size - 1))) / 2))
        if 1 + F + F * F != s.size:
            raise ValueError("frechet_distance_from_stats: a state is [1 + F + F * F] float64")
        n = s[0]
        if n < 2:
            raise ValueError(f"frechet_distance_from_stats: a covariance needs at least 2 embeddings (got {int(n)})")
        mu = s[1:1 + F] / n
        return mu, (s[1 + F:].reshape(F, F) - n * np.outer(mu, mu)) / (n - 1)
    mu1, s1 = moments(stats_a)
    mu2, s2 = moments(stats_b)
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(s1.shape[0]) * eps
        covmean = linalg.sqrtm((s1 + offset).dot(s2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            return 1e10
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


class MotionEvaluator:
    """Accumulates the reference's metrics over batches of decoded motions.  Defaults: metric_eval.py:451-452 (the dyadic script's are
    order 12, sigma 1.25).  ``fgd_net``: an ``FGDNet`` (eval mode) or None (no FGD)."""

    def __init__(self, fgd_net=None, fps=25, order=10, sigma=0.3, srgr_threshold=0.3):
        self.fgd_net, self.fps, self.order, self.sigma, self.srgr_threshold = fgd_net, fps, int(order), float(sigma), float(srgr_threshold)
        self.reset()

    def reset(self):
        self._stats = {"pred": None, "target": None}
        self._proc = {"pred": [], "target": []}
        self._sums = []           # per update: (l1div, srgr, jitter, align, counted) as device scalars or None
        self._frames = self._frames_srgr = self._seqs_jitter = 0
        self._loaded = {"pred": None, "target": None}     # statistics from load_state_dict (numpy), until an update continues them

    def _state(self, which, dev):
        if self.fgd_net is None:
            return None
        if self._stats[which] is None:
            F = self.fgd_net.feature_length
            if self._loaded[which] is not None:             # saved statistics are continued, not replaced
                self._stats[which] = torch.from_numpy(self._loaded[which].copy()).to(dev)
            else:
                self._stats[which] = torch.zeros(1 + F + F * F, dtype=torch.float64, device=dev)
        return self._stats[which]

    def _host_stats(self, which):
        s = self._stats[which]
        return s.cpu().numpy() if s is not None else self._loaded[which]

    def update(self, pred, target=None, semantic=None, onsets=None, audio=None, onset_detector=None):
        """pred [B, T, 189] float32 on the device, straight from ``vae.decode``; target likewise; semantic [B, T]; onsets: B lists of onset
        times in seconds, or audio: the B waveforms [B, n_samples] on the device, whose onsets are detected there (``onset_detector``:
        None for the reference's settings).  Nothing is copied to the host; with audio the sequences without an onset are counted on the
        device from the offsets, and ``compute()`` reads the count."""
        if audio is not None and onsets is not None:
            raise ValueError("MotionEvaluator.update: give onsets or audio, not both")
        if pred.device.type != "cuda":
            raise NotImplementedError("convofusion_amd.metrics runs on an MI355X only (tensors must be on 'cuda'); no CPU fallback")
        B, T = int(pred.shape[0]), int(pred.shape[1])
        embed = self.fgd_net is not None and T == EMB_FRAMES
        kw = dict(fps=self.fps, order=self.order, sigma=self.sigma, srgr_threshold=self.srgr_threshold)
        want = {"l1div", "srgr", "jitter", "align", "processed"}
        from_audio = audio is not None
        if from_audio:
            onsets = detect_onsets(audio, B, pred.device, onset_detector)
        r = motion_eval(pred, target, semantic, onsets, fgd_net=self.fgd_net if embed else None,
                        stats=self._state("pred", pred.device) if embed else None, want=want, **kw)
        self._proc["pred"].append(r["processed"])
        counted = None
        if "align" in r and from_audio:
            has = onsets[0][1:] > onsets[0][:-1]
            counted = has.sum()                     # (a device scalar: compute() reads it)
            align = (r["align"] * has).sum()
        elif "align" in r:
            off = np.concatenate([[0], np.cumsum([len(o) for o in onsets])]) if not isinstance(onsets, tuple) else onsets[0].cpu().numpy()
            has = torch.from_numpy(np.diff(off) > 0).to(pred.device)
            counted = int((np.diff(off) > 0).sum())
            align = (r["align"] * has).sum()
        self._sums.append((r["l1div"].sum(), r["srgr"].sum() if "srgr" in r else None, (r["jitter"] / ((T - 1) * FEAT)).sum() if "jitter" in r else None,
                           align if counted is not None else None, counted))
        self._frames += B * T
        if "srgr" in r:
            self._frames_srgr += B * T
        if "jitter" in r:
            self._seqs_jitter += B
        if target is not None:
            t = motion_eval(target, fgd_net=self.fgd_net if embed else None, stats=self._state("target", pred.device) if embed else None,
                            want={"processed"}, **kw)
            self._proc["target"].append(t["processed"])

    def _diversity(self, which):
        if not self._proc[which]:
            return None
        shapes = {tuple(p.shape[1:]) for p in self._proc[which]}
        n = sum(int(p.shape[0]) for p in self._proc[which])
        if len(shapes) != 1 or n < 2:
            return None
        return float(diversity(torch.cat(self._proc[which])))

    def compute(self):
        """A dict: fgd, align, align_counted, diversity_pred, diversity_target, l1div, srgr, jitter (None where the inputs for it were not given)."""
        def total(i):
            vals = [s[i] for s in self._sums if s[i] is not None]
            return float(torch.stack(vals).sum()) if vals else None
        out = dict.fromkeys(("fgd", "align", "align_counted", "diversity_pred", "diversity_target", "l1div", "srgr", "jitter"))
        sp, st = self._host_stats("pred"), self._host_stats("target")
        if sp is not None and st is not None:
            out["fgd"] = frechet_distance_from_stats(sp, st)
        counted = sum(int(s[4]) for s in self._sums if s[4] is not None)
        if any(s[4] is not None for s in self._sums):
            out["align_counted"] = counted
            out["align"] = total(3) / counted if counted else None
        out["diversity_pred"], out["diversity_target"] = self._diversity("pred"), self._diversity("target")
        if self._frames:
            out["l1div"] = total(0) / self._frames
        if self._frames_srgr:
            out["srgr"] = total(1) / (self._frames_srgr * JOINTS)
        if self._seqs_jitter:
            out["jitter"] = total(2) / self._seqs_jitter
        return out

    def state_dict(self):
        """The Frechet statistics (numpy float64, or None): ``pred`` and ``target``.  A ground-truth set's ``target`` state can be saved
        once and given to another evaluator with ``load_state_dict``."""
        def host(which):
            s = self._host_stats(which)
            return None if s is None else np.array(s)
        return {"pred": host("pred"), "target": host("target"),
                "fps": self.fps, "order": self.order, "sigma": self.sigma, "srgr_threshold": self.srgr_threshold}

    def load_state_dict(self, state):
        """Reuse saved statistics: ``compute()`` takes them as they are, and a later ``update`` adds to them."""
        for which in ("pred", "target"):
            t = state.get(which)
            if t is not None:
                t = np.asarray(t, dtype=np.float64).reshape(-1).copy()
                if self.fgd_net is not None and t.size != 1 + self.fgd_net.feature_length * (1 + self.fgd_net.feature_length):
                    raise ValueError("MotionEvaluator.load_state_dict: the statistics were made by a net of another feature_length")
            self._loaded[which] = t
            self._stats[which] = None


def read_result_dir(path):
    """The reference's result layout (metric_eval.py:455-476): every ``*/*/gt.npy`` under ``path``, sorted, with ``pred.npy`` and
    ``sem_lsn.npy`` beside it and optionally ``onsets.npy`` (onset times in seconds; the reference detects them from ``lsn_audio.wav``
    with librosa).  Returns (gt [N, T, 189], pred, sem [N, T], onsets: a list of N arrays, or None if no directory has the file)."""
    files = sorted(glob.glob(os.path.join(path, "*", "*", "gt.npy")))
    if not files:
        raise FileNotFoundError(f"no */*/gt.npy under {path}")
    gt, pred, sem, ons, any_onsets = [], [], [], [], False
    for f in files:
        d = os.path.dirname(f)
        gt.append(np.load(f).reshape(-1, FEAT).astype(np.float32))
        pred.append(np.load(os.path.join(d, "pred.npy")).reshape(-1, FEAT).astype(np.float32))
        sem.append(np.load(os.path.join(d, "sem_lsn.npy")).reshape(-1).astype(np.float32))
        o = os.path.join(d, "onsets.npy")
        any_onsets |= os.path.exists(o)
        ons.append(np.load(o).reshape(-1).astype(np.float64) if os.path.exists(o) else np.zeros(0))
    T = gt[0].shape[0]
    if any(g.shape[0] != T or p.shape[0] != T or s.shape[0] != T for g, p, s in zip(gt, pred, sem)):
        raise ValueError("read_result_dir: every gt / pred / sem_lsn must have the same number of frames")
    return np.stack(gt), np.stack(pred), np.stack(sem), ons if any_onsets else None


WAV_RATE = 16000


def read_wav_pcm16(path, rate=WAV_RATE):
    """A 16-bit PCM mono wav file at ``rate`` as float32 in [-1, 1) (samples / 32768), read with the standard library.  Anything else
    raises: resampling and other encodings stay with the caller."""
    import wave
    try:
        with wave.open(path, "rb") as w:
            ch, width, sr, n, comp = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes(), w.getcomptype()
            raw = w.readframes(n)
    except (wave.Error, EOFError) as e:
        raise ValueError(f"{path}: not a plain PCM wav file ({e}); resampling and other encodings stay with the caller") from e
    if ch != 1 or width != 2 or sr != int(rate) or comp != "NONE":
        raise ValueError(f"{path}: {ch} channel(s), {8 * width}-bit, {sr} Hz, compression {comp}: only 16-bit PCM mono at {int(rate)} Hz is read "
                         "here; resampling and other encodings stay with the caller")
    return np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768.0)


def read_result_audio(path):
    """``lsn_audio.wav`` beside every ``*/*/gt.npy`` under ``path`` (the order of ``read_result_dir``) as float32 [N, n_samples]; the clips
    must be equally long."""
    files = sorted(glob.glob(os.path.join(path, "*", "*", "gt.npy")))
    if not files:
        raise FileNotFoundError(f"no */*/gt.npy under {path}")
    waves = [read_wav_pcm16(os.path.join(os.path.dirname(f), "lsn_audio.wav")) for f in files]
    if any(len(w) != len(waves[0]) for w in waves) or len(waves[0]) < 1:
        raise ValueError("read_result_audio: every lsn_audio.wav must have the same, non-zero number of samples (equal-length clips only)")
    return np.stack(waves)


def evaluate_result_dir(path, fgd_net=None, batch=64, device="cuda", detect_onsets=False, onset_detector=None, **kwargs):
    """Score a directory of the reference's results; ``kwargs`` go to ``MotionEvaluator``.  Returns ``compute()``'s dict.
    detect_onsets: the onsets of the alignment come from ``lsn_audio.wav`` beside each ``gt.npy`` (16-bit PCM mono at 16 kHz), detected
    on the device by ``onset_detector`` (None: the reference's settings); ``onsets.npy`` files are then not used."""
    gt, pred, sem, ons = read_result_dir(path)
    audio = read_result_audio(path) if detect_onsets else None
    ev = MotionEvaluator(fgd_net, **kwargs)
    for s in range(0, gt.shape[0], int(batch)):
        e = min(s + int(batch), gt.shape[0])
        if audio is not None:
            ev.update(torch.from_numpy(pred[s:e]).to(device), torch.from_numpy(gt[s:e]).to(device), torch.from_numpy(sem[s:e]).to(device),
                      audio=torch.from_numpy(audio[s:e]).to(device), onset_detector=onset_detector)
            continue
        ev.update(torch.from_numpy(pred[s:e]).to(device), torch.from_numpy(gt[s:e]).to(device), torch.from_numpy(sem[s:e]).to(device),
                  ons[s:e] if ons is not None else None)
    return ev.compute()
