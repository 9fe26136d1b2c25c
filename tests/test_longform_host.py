"""Host side of long-form synthesis (no GPU): the tie table of half-overlapping windows, the stitched token sequence, the split into runs,
the refusals of ``check_tie`` and of ``sample_sharded``, the restated tied loop against the restated edit loop, the frame stitching against
the reference's expression, and the ctypes mirror of cfd_tie_args / cfd_sample_begin_tied against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import edit_ref, longform_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_ties_layout():
    from convofusion_amd.longform import window_ties
    U, W, L = 2, 3, 16
    tie = window_ties(U, W, L)
    assert tie.dtype == torch.int32 and tuple(tie.shape) == (U * W, L)
    for u in range(U):
        for w in range(W):
            for l in range(L):
                want = (u * W + w - 1) * L + l + L // 2 if (w > 0 and l < L // 2) else -1
                assert int(tie[u * W + w, l]) == want, (u, w, l)
    assert (window_ties(4, 1) == -1).all() and tuple(window_ties(4, 1).shape) == (4, 16)
    t8 = window_ties(1, 2, L=8)
    assert t8[1].tolist() == [4, 5, 6, 7, -1, -1, -1, -1] and (t8[0] == -1).all()
    longform_ref.check_ties(tie.numpy(), np.zeros((U * W, L), bool))        # the table keeps its own contract
    for bad in (dict(n_utterances=0, n_windows=2), dict(n_utterances=1, n_windows=0), dict(n_utterances=1, n_windows=2, L=15)):
        with pytest.raises(ValueError):
            window_ties(**bad)


def test_stitched_sequence_indexing():
    from convofusion_amd.longform import stitch_tokens
    U, W, L = 2, 4, 16
    win = torch.arange(U * W * L, dtype=torch.float32).reshape(U, W, L, 1).expand(U, W, L, 128).contiguous()
    seq = stitch_tokens(win)
    assert tuple(seq.shape) == (U, (W + 1) * L // 2, 128)
    for u in range(U):
        for t in range(seq.shape[1]):
            w, l = (0, t) if t < L else (1 + (t - L) // (L // 2), L // 2 + (t - L) % (L // 2))
            assert float(seq[u, t, 0]) == float(win[u, w, l, 0]), (u, t)
    assert torch.equal(stitch_tokens(win[:, :1]), win[:, 0])


def test_window_groups_split_by_max_rows():
    from convofusion_amd.longform import group_ties, window_groups, window_ties
    assert window_groups(2, 3) == [(0, 6)] and window_groups(2, 3, 6) == [(0, 6)] and window_groups(2, 3, 100) == [(0, 6)]
    assert window_groups(3, 3, 7) == [(0, 6), (6, 9)]                 # whole utterances while they fit
    assert window_groups(2, 3, 3) == [(0, 3), (3, 6)]
    assert window_groups(1, 4, 2) == [(0, 2), (2, 4)]
    assert window_groups(2, 5, 2) == [(0, 2), (2, 4), (4, 5), (5, 7), (7, 9), (9, 10)]      # never across two utterances
    assert window_groups(1, 3, 1) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError):
        window_groups(1, 3, 0)
    for U, W, m in ((2, 3, None), (3, 3, 7), (2, 5, 2), (1, 4, 1)):
        full = window_ties(U, W)
        seen = []
        for a, b in window_groups(U, W, m):
            tie, carried = group_ties(a, b, W)
            seen += list(range(a, b))
            inside = full[a:b].long() >= a * 16
            assert torch.equal(tie.long(), torch.where(inside, full[a:b].long() - a * 16, torch.full_like(full[a:b].long(), -1)))
            assert torch.equal(carried, (full[a:b] >= 0) & ~inside)   # a tie that leaves the run becomes a kept token
            if m is not None:
                assert b - a <= m
        assert seen == list(range(U * W))


def _tie(B=2, L=16, **entries):
    t = torch.full((B, L), -1, dtype=torch.int32)
    for k, v in entries.items():
        b, l = (int(x) for x in k[1:].split("_"))
        t[b, l] = v
    return t


def test_check_tie_accepts_and_refuses():
    from convofusion_amd.sampler import check_tie
    B, L = 2, 16
    assert check_tie(None, None, B, L) is None
    good = _tie(t1_0=8, t1_1=9)
    out = check_tie(good, None, B, L)
    assert out.dtype == torch.int32 and torch.equal(out, good) and out.is_contiguous()
    assert torch.equal(check_tie(good.long(), torch.zeros(B, L, dtype=torch.bool), B, L), good)
    keep = torch.zeros(B, L, dtype=torch.bool)
    keep[0, 0] = True
    assert check_tie(good, keep, B, L) is not None                    # a kept token that is neither a source nor tied
    cases = {
        "out of range (high)": (_tie(t1_0=B * L), None, r"tie\[1\]\[0\]"),
        "out of range (low)": (_tie(t0_3=-2), None, r"tie\[0\]\[3\]"),
        "self-tie": (_tie(t1_2=L + 2), None, r"tie\[1\]\[2\].*itself"),
        "chain": (_tie(t1_0=8, t0_8=3), None, r"itself tied"),
        "source kept": (good, torch.arange(B * L).reshape(B, L) == 8, r"tie\[1\]\[0\].*keep"),
        "kept and tied": (good, torch.arange(B * L).reshape(B, L) == L, r"\(1, 0\).*both"),
        "wrong shape": (torch.full((B, L + 1), -1, dtype=torch.int32), None, r"\[B, L\]"),
        "float dtype": (torch.full((B, L), -1.0), None, "integer"),
        "bool dtype": (torch.zeros((B, L), dtype=torch.bool), None, "integer"),
        "not a tensor": ([[-1] * L] * B, None, "integer"),
    }
    for what, (tie, km, msg) in cases.items():
        with pytest.raises(ValueError, match=msg):
            check_tie(tie, km, B, L)
    for what, kw in {"preseq": dict(preseq=torch.zeros(B, 4, 128)), "strength": dict(strength=0.5), "inversion": dict(scheduler_kind=3),
                     "anchor": dict(anchored=True), "dyadic": dict(dynamic_memories=(0,))}.items():
        with pytest.raises(ValueError, match="tie"):
            check_tie(good, None, B, L, **kw)
    for kind in (0, 1, 2):
        assert check_tie(good, None, B, L, scheduler_kind=kind) is not None


def test_sample_sharded_keeps_ties_inside_a_slice():
    """One process is rank 0 of 1 (the whole batch): the table passes through; shard_tie renumbers a slice and refuses a tie that leaves it."""
    from convofusion_amd.distributed import sample_sharded, shard_tie
    from convofusion_amd.longform import window_ties
    total, L = 6, 16
    tie = window_ties(2, 3)
    seen = {}

    def fn(enc, masks, B, first_utterance, **kw):
        seen.update(kw, B=B)
        return torch.zeros(B, L, 128)

    enc = [torch.zeros(7 * total, 3, 512)] * 5
    sample_sharded(fn, enc, {}, total, tie=tie)
    assert torch.equal(seen["tie"], tie) and seen["B"] == total
    assert torch.equal(shard_tie(tie, 3, 6, total), window_ties(1, 3))            # utterance 1 on its own rank: renumbered
    with pytest.raises(ValueError, match="crosses"):
        shard_tie(tie, 1, 3, total)                                                 # window 1 without its window 0
    with pytest.raises(ValueError, match="crosses"):
        shard_tie(tie, 2, 4, total)                                                 # window 2 of utterance 0 without its window 1
    assert torch.equal(shard_tie(tie, 0, 2, total), tie[:2])                        # (a source may stay without its tied token)
    with pytest.raises(ValueError):
        sample_sharded(fn, enc, {}, total, tie=tie[:4])


@pytest.mark.parametrize("kind", ["ddpm", "dpmpp"])
def test_restated_tied_loop_without_ties_is_the_restated_edit_loop(kind):
    """longform_ref.tied_reverse with a table of -1 equals edit_ref.edit_reverse (k0 = 0) bit for bit, with and without kept tokens, and a
    real table changes exactly the rows that are tied: the yardstick is sound."""
    from oracle import philox_ref, scheduler_ref
    from tests.dpmsolver_ref import DPMSolverMultistepRef
    from tests.test_edit_host import _fake_denoiser
    from convofusion_amd.longform import window_ties
    B, L, n, seed = 4, 16, 10, 9
    mk = (lambda: DPMSolverMultistepRef(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")) \
        if kind == "dpmpp" else scheduler_ref.DDPMSchedulerRef
    init = philox_ref.normal_tensor(seed, 0, range(B), 1, L)
    noise = lambda i, t: philox_ref.normal_tensor(seed, i, range(B), 0, L)   # noqa: E731
    src = (0.8 * philox_ref.normal_tensor(seed, 0, range(B), 2, L)).astype(np.float32)
    fn = _fake_denoiser(seed)
    none = np.full((B, L), -1)
    for keep in (np.zeros((B, L), bool), np.arange(B * L).reshape(B, L) % 5 == 0):
        want, wsnaps = edit_ref.edit_reverse(fn, mk(), None, None, init, noise, src, keep, 0, num_inference_steps=n, keep_steps=(1, 4))
        got, gsnaps = longform_ref.tied_reverse(fn, mk(), None, None, init, noise, none, source=src, keep=keep, num_inference_steps=n,
                                                keep_steps=(1, 4))
        assert np.array_equal(got, want) and all(np.array_equal(gsnaps[k], wsnaps[k]) for k in (1, 4))
    tie = window_ties(2, 2, L).numpy()
    tied, snaps = longform_ref.tied_reverse(fn, mk(), None, None, init, noise, tie, num_inference_steps=n, keep_steps=(3,))
    plain, _ = longform_ref.tied_reverse(fn, mk(), None, None, init, noise, none, num_inference_steps=n)
    for b in (1, 3):
        assert np.array_equal(tied[b, :L // 2], tied[b - 1, L // 2:])             # the final copy
        assert not np.array_equal(tied[b], plain[b]) and np.array_equal(tied[b - 1], plain[b - 1])   # only the tied rows move
        if kind == "ddpm":     # a snapshot is the latents as stepped (each token with its own step noise), not yet copied
            assert not np.array_equal(snaps[3][b, :L // 2], snaps[3][b - 1, L // 2:])


def test_stitch_frames_is_the_references_expression():
    """unbounded_synthesis.py:460-468 window by window: the root's x / z moved onto the previous window's frame 64, y left alone; each
    later window contributes its second half."""
    from convofusion_amd.longform import stitch_frames
    g = torch.Generator().manual_seed(5)
    U, W, F, nf = 2, 3, 128, 189
    feats = torch.randn((U, W, F, nf), generator=g)
    out = stitch_frames(feats)
    assert tuple(out.shape) == (U, (W + 1) * F // 2, nf)
    prev, want = None, []
    for w in range(W):
        feats_rst = feats[:, w].clone()
        if prev is not None:
            feats_rst[:, :, :3] = feats_rst[:, :, :3] - feats_rst[:, :1, :3] * torch.tensor([1, 0, 1])
            feats_rst[:, :, :3] = feats_rst[:, :, :3] + (prev[:, :1, :3] * torch.tensor([1, 0, 1]))
        want.append(feats_rst if w == 0 else feats_rst[:, F // 2:])
        prev = feats_rst[:, F // 2:, :]
    assert torch.equal(out, torch.cat(want, dim=1))
    assert torch.equal(out[:, :F], feats[:, 0]) and torch.equal(out[:, F:, 3:], feats[:, 1:, F // 2:, 3:].reshape(U, -1, nf - 3))


def test_ctypes_mirror_and_header_agree():
    from convofusion_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cfdenoise.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} cfd_tie_args;", hdr).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [f for f, _ in _lib.TieArgs._fields_] == ["tie"]
    assert "const int32_t* tie" in " ".join(body.split())
    assert (_lib.TieArgs.tie.offset, C.sizeof(_lib.TieArgs)) == (0, 8)
    decl = " ".join(re.search(r"int cfd_sample_begin_tied\(([^)]*)\);", hdr).group(1).split())
    assert decl == ("cfd_handle h, const cfd_sample_args* args, const cfd_edit_args* edit, const cfd_tie_args* tie, const float* weights, "
                    "int prune, int* chunks_evaluated, void* stream")
    assert "cfd_sample_begin_tied" in _lib.SYMBOLS
    build.build()
    lib = _lib.load()
    fn = lib.cfd_sample_begin_tied
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.POINTER(_lib.SampleArgs), C.POINTER(_lib.EditArgs), C.POINTER(_lib.TieArgs), C.c_void_p, C.c_int,
                           C.POINTER(C.c_int), C.c_void_p]
    assert fn(None, None, None, None, None, 1, None, None) == -1      # (refused before anything touches a device)
    assert b"null" in lib.cfd_last_error()
