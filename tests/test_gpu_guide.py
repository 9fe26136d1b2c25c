"""GPU: ``cfd_denoise_guide`` (``Denoiser.guide``) -- one key-pose guided update as a device call -- against the float64 restatement
tests/guide_ref.py, and its state on a handle it shares with ``cfd_weg_eval`` and ``cfd_denoise_vjp``.

Gates.  d_out, grad and x_new against float64: ``F64_GRAD_GATE`` of tests/test_gpu_weg.py (relative L2 5.44e-5, worst row 3.46e-4) --
the new gradient is a fixed linear combination of that sweep's outputs.  The loss: relative 1e-6, the WEG golden's loss gate (ten times
that was allowed for the extra float32 reduction and not needed).  Everything structural -- ties, determinism, reuse, rows independent of the batch -- is exact.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import inputs
from tests import guide_ref
from tests.helpers import state_dict
from tests.test_gpu_weg import F64_GRAD_GATE
from tests.weg_bwd_ref import tap_errors

pytestmark = pytest.mark.gpu

LOSS_GATE = 1e-6          # the WEG golden's loss gate: the extra float32 reduction did not need the tenfold the issue allowed (measured: at most 3.4e-7)
S_SMALL = (6, 20, 12, 8, 1)
S_PRODUCT = (24, 161, 24, 8, 1)


def acp(t):
    """alphas_cumprod[t] of the scaled-linear schedule of tests/gpu_helpers.SCHED_KW, in float64."""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return float(np.cumprod(1.0 - betas)[t])


def _cfg_case(seed, B, L, S, pad_tail, chunks):
    """The chunks ``chunks`` of a 7-chunk guidance batch over B + 1 distinct memories: (unique memories, their masks, the row maps of
    the evaluated rows, the memories and masks expanded per row)."""
    cb = inputs.make_cfg_batch(seed=seed, B=B, L=L, S=S, pad_tail=pad_tail)
    rows = np.concatenate([np.arange(c * B, (c + 1) * B) for c in chunks])
    maps = [np.ascontiguousarray(cb["row_map"][j][rows]) for j in range(5)]
    umasks = {}
    for j, k in enumerate(inputs.MEM_NAMES):
        mk = cb["masks"][k]
        umasks[k] = None if mk is None else np.stack([mk[list(cb["row_map"][j]).index(u)] for u in range(B + 1)])
    return (cb["unique"], umasks, maps, [cb["memories"][j][rows] for j in range(5)],
            {k: (None if v is None else v[rows]) for k, v in cb["masks"].items()}, cb["init"])


@functools.lru_cache(maxsize=None)
def guide_case(name):
    """two_tokens: B = 1, L = 2, n = 2 (the seed's and the update's tails).  len18_t0: B = 2, L = 18, n = 3 with row maps over B + 1
    memories at timestep 0 (a partial second tile; 1 - sum w on chunk 0).  product: B = 1, L = 16, n = 6 at the product's memory
    lengths with the default combine.  holes: B = 3, n = 2, masks with holes on all five memories, a key-pose mask that keeps ONE token
    of one row, w different per row.  windows / shared: B = 3 as three windows of one utterance with ``longform.window_ties(1, 3)`` /
    a hand-made table in which two tokens share one source.  rows768: B = 8, L = 16, n = 6 -- 768 token rows, 48 tiles, beyond the
    differentiable forward's 700.  rows66: B = 33, L = 2, n = 2 -- more batch rows than travel in the kernel arguments (64)."""
    from convofusion_amd import longform
    from convofusion_amd.sampler import default_guidance_weights
    rng = np.random.Generator(np.random.PCG64(500 + len(name)))
    tie = None
    if name in ("two_tokens", "holes", "windows", "shared", "rows66"):
        B, L, n, S, t = dict(two_tokens=(1, 2, 2, S_SMALL, 5), holes=(3, 16, 2, (24, 161, 24, 8, 2), 321), windows=(3, 16, 2, S_SMALL, 613),
                             shared=(3, 16, 2, S_SMALL, 250), rows66=(33, 2, 2, (3, 5, 6, 2, 1), 77))[name]
        inp = inputs.make_plain_batch(seed=600 + len(name), Be=n * B, L=L, S=S, pad_tail=(2, 0, 3, 0, 0) if name != "holes" else (0,) * 5)
        if name == "holes":
            for j, k in enumerate(inputs.MEM_NAMES):
                mk = rng.random((n * B, S[j])) < 0.3
                mk[0, 0] = True
                mk[:, -1] = False
                mk[1] = False
                inp["masks"][k] = mk
        uniq, umasks, maps, mems_rows, masks_rows, x = inp["memories"], inp["masks"], None, inp["memories"], inp["masks"], inp["sample"][:B]
        w = np.zeros((B, n), dtype=np.float32)
        w[:, 1] = 7.5 if name != "holes" else np.array([7.5, 1.0, 3.25], dtype=np.float32)
        if name == "windows":
            tie = longform.window_ties(1, 3, L).numpy()
        if name == "shared":
            tie = np.full((B, L), -1, dtype=np.int32)
            tie[1, 0] = tie[2, 5] = 0 * L + 9          # two tokens on one source
            tie[2, 0] = 1 * L + 3
    else:
        B, L, chunks, S, t, pad = dict(len18_t0=(2, 18, (0, 1, 2), S_SMALL, 0, (2, 0, 3, 0, 0)),
                                       product=(1, 16, (0, 1, 2, 3, 4, 5), S_PRODUCT, 433, (5, 0, 7, 0, 0)),
                                       rows768=(8, 16, (0, 1, 2, 3, 4, 5), S_SMALL, 500, (2, 0, 3, 0, 0)))[name]
        n = len(chunks)
        uniq, umasks, maps, mems_rows, masks_rows, x = _cfg_case(700 + len(name), B, L, S, pad, chunks)
        w = np.tile(np.asarray(default_guidance_weights(7, 7.5), dtype=np.float32)[list(chunks)], (B, 1))
        if name == "len18_t0":
            w = np.array([[0.0, 0.4, 0.25], [0.0, 1.5, 2.0]], dtype=np.float32)
    target = (rng.standard_normal((B, L, 128), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    mask = np.zeros((B, L), dtype=np.float32)
    if name == "holes":
        mask[1, 7] = 1
    elif name in ("windows", "shared"):
        mask[0, 9] = mask[1, 2] = mask[2, 5] = mask[2, 12] = 1      # on a source, on tied tokens, on a free token
    else:
        mask[:, 1::3] = 1
    a = acp(t)
    return SimpleNamespace(name=name, B=B, L=L, n=n, t=t, x=np.ascontiguousarray(x, dtype=np.float32), uniq=uniq, umasks=umasks, maps=maps,
                           mems_rows=mems_rows, masks_rows=masks_rows, w=w, target=target, mask=mask, tie=tie, s0=a ** 0.5,
                           s1=(1.0 - a) ** 0.5, inv_n=1.0 / (float(mask.sum()) * 128), step=0.5)


CASES = ("two_tokens", "len18_t0", "product", "holes", "windows", "shared", "rows768", "rows66")


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64"):
    c = guide_case(name)
    return guide_ref.guide(state_dict(1234, 1.0), c.x, c.t, c.mems_rows, c.masks_rows, c.w, c.target, c.mask, c.s0, c.s1, c.inv_n, c.step,
                           tie=c.tie, dtype=np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def dev_case(name):
    """The case's tensors on the device, made once: their addresses are part of what the library compares."""
    from tests.gpu_helpers import to_dev
    c = guide_case(name)
    return SimpleNamespace(x=to_dev(c.x), mems=[to_dev(m) for m in c.uniq], masks={k: (None if v is None else to_dev(v)) for k, v in c.umasks.items()},
                           maps=None if c.maps is None else [to_dev(r) for r in c.maps], w=to_dev(c.w), target=to_dev(c.target),
                           mask=to_dev(c.mask), tie=None if c.tie is None else to_dev(c.tie.astype(np.int32)))


ALL = ("loss", "grad", "x_new", "d_out")


def call(m, name, t=None, reuse=0, step=None, want=ALL, rows=None):
    """One ``Denoiser.guide`` call of the case (``rows``: a slice of its latent rows, with their chunks' memories)."""
    import torch
    c, d = guide_case(name), dev_case(name)
    x, w, target, mask, mems, masks, maps = d.x, d.w, d.target, d.mask, d.mems, d.masks, d.maps
    inv_n = c.inv_n
    if rows is not None:
        sel = torch.cat([torch.arange(k * c.B + rows.start, k * c.B + rows.stop) for k in range(c.n)]).to(x.device)
        x, w, target, mask = x[rows].contiguous(), w[rows].contiguous(), target[rows].contiguous(), mask[rows].contiguous()
        if maps is None:
            mems = [e[sel].contiguous() for e in mems]
            masks = {k: (None if v is None else v[sel].contiguous()) for k, v in masks.items()}
        else:
            maps = [r[sel].contiguous() for r in maps]
    tt = c.t if t is None else t
    a = acp(tt)
    return m.guide(x, tt, mems, masks, w, target, mask, sqrt_acp=a ** 0.5, sqrt_1m_acp=(1.0 - a) ** 0.5, step=c.step if step is None else step,
                   inv_n=inv_n, tie=d.tie, row_maps=maps, reuse_memory_side=reuse, want=want)


def same(a, b):
    import torch
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("name", CASES)
def test_guide_matches_float64(name):
    """Fails on a tree without the feature: ``Denoiser.guide`` and the symbol cfd_denoise_guide do not exist there."""
    import torch
    from tests.gpu_helpers import hip_denoiser, read_debug
    m = hip_denoiser(1234, 1.0)
    c = guide_case(name)
    r64, r32 = reference(name), reference(name, "float32")
    got = call(m, name)
    info = read_debug(m, "weg.info", (5,))
    loss, grad, x_new, d_out = (v.cpu().numpy() for v in got)
    rows = lambda v: np.asarray(v).reshape(-1, 128)
    el = abs(float(loss) - r64["loss"]) / abs(r64["loss"])
    fl = abs(r32["loss"] - r64["loss"]) / abs(r64["loss"])
    line = [f"{name}: B={c.B} L={c.L} n={c.n} t={c.t} launches {int(info[0])}; loss {float(loss):.6e} vs float64 {el:.2e} (float32 numpy {fl:.2e})"]
    errs = {}
    for key, v in (("d_out", d_out), ("grad", grad), ("x_new", x_new)):
        errs[key] = tap_errors(rows(v), rows(r64[key]))
        f = tap_errors(rows(r32[key]), rows(r64[key]))
        line.append(f"{key} rel L2 {errs[key][0]:.2e} worst row {errs[key][1]:.2e} (float32 numpy {f[0]:.2e} / {f[1]:.2e})")
    print("; ".join(line))
    assert el <= LOSS_GATE
    for key in ("d_out", "grad", "x_new"):
        assert errs[key][0] <= F64_GRAD_GATE[0] and errs[key][1] <= F64_GRAD_GATE[1], key
    # determinism: a second call returns the same bits of all four outputs; what is not asked for changes nothing of the rest
    assert same(got, call(m, name))
    only = call(m, name, want=("x_new",))
    assert only[0] is None and only[1] is None and only[3] is None and torch.equal(only[2], got[2])
    # x_new may alias x
    d = dev_case(name)
    x2 = d.x.clone()
    a = acp(c.t)
    m.guide(x2, c.t, d.mems, d.masks, d.w, d.target, d.mask, sqrt_acp=a ** 0.5, sqrt_1m_acp=(1.0 - a) ** 0.5, step=c.step, inv_n=c.inv_n,
            tie=d.tie, row_maps=d.maps, want=("x_new",), x_new=x2)
    assert torch.equal(x2, got[2])
    # step 0 with no tie leaves x as it is, bit for bit
    if c.tie is None:
        assert torch.equal(call(m, name, step=0.0, want=("x_new",))[2], d.x)


@pytest.mark.parametrize("name", ("windows", "shared"))
def test_tied_tokens_fold_onto_their_sources_and_follow_them(name):
    import torch
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    c, d = guide_case(name), dev_case(name)
    _, grad, x_new, _ = call(m, name)
    tie = torch.from_numpy(c.tie.reshape(-1).astype(np.int64)).to(grad.device)
    tied = tie >= 0
    flat_g, flat_x, flat_in = grad.reshape(-1, 128), x_new.reshape(-1, 128), d.x.reshape(-1, 128)
    assert int(tied.sum()) > 0 and not flat_g[tied].any()
    assert torch.equal(flat_x[tied], flat_x[tie[tied]])                      # every tied token is its source, bit for bit
    assert bool((flat_x[~tied] != flat_in[~tied]).any(dim=1).all())          # every free token moved
    # the gradient of a source is the folded sum: the same call without a tie on x~ gives the rows g~, and the fold of those is exact
    # up to the float32 sum's order, which the restatement fixes as the kernel does (ascending)
    xt = torch.from_numpy(guide_ref.gather_tie(c.x, c.tie)).to(grad.device)
    a = acp(c.t)
    g_tilde = m.guide(xt, c.t, d.mems, d.masks, d.w, d.target, d.mask, sqrt_acp=a ** 0.5, sqrt_1m_acp=(1.0 - a) ** 0.5, step=c.step,
                      inv_n=c.inv_n, want=("grad",))[1]
    assert np.array_equal(guide_ref.fold(g_tilde.cpu().numpy(), c.tie), grad.cpu().numpy())
    if name == "shared":
        src = 9
        assert int((tie == src).sum()) == 2 and bool(flat_g[src].any())


def test_rows_beyond_700_agree_with_per_utterance_calls_bit_for_bit():
    """768 token rows in one call against eight calls of 96 rows on the same inputs: rows are independent, and no reduction of the
    forward, the sweep or the new kernels depends on the tile count, so the gradient rows agree bit for bit (the loss is a sum over the
    whole batch and is compared in test_guide_matches_float64)."""
    import torch
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    c = guide_case("rows768")
    assert c.n * c.B * c.L == 768
    whole = call(m, "rows768", want=("grad", "x_new", "d_out"))
    for b in range(c.B):
        part = call(m, "rows768", want=("grad", "x_new", "d_out"), rows=slice(b, b + 1))
        assert torch.equal(part[1][0], whole[1][b]) and torch.equal(part[2][0], whole[2][b]), b
        assert torch.equal(part[3].reshape(c.n, c.L, 128), whole[3].reshape(c.n, c.B, c.L, 128)[:, b]), b


def test_memory_side_reuse_returns_a_fresh_call_s_bits_and_skips_its_launches():
    import torch
    from convofusion_amd import weg
    from tests.gpu_helpers import hip_denoiser, read_debug
    from tests.test_gpu_weg import state_walk_inputs
    m = hip_denoiser(1234, 1.0)
    nl = int(m.num_layers)
    memory_side = (2 + 2 * nl) + (6 * 5 + 2)
    launches = lambda: int(read_debug(m, "weg.info", (5,))[0])
    name = "product"
    fresh = {t: call(m, name, t=t) for t in (433, 432)}
    full = launches()
    first = call(m, name, t=433, reuse=2)                 # builds the tables over every timestep: nothing to reuse yet
    assert launches() == full and same(first, fresh[433])
    second = call(m, name, t=432, reuse=2)                # another timestep, the memory side of the call before
    assert launches() == full - memory_side and same(second, fresh[432])
    # a cfd_denoise_vjp and a cfd_weg_eval in between each make the next guide call run its memory side again, in both orders
    c, d = guide_case(name), dev_case(name)
    xin = d.x.repeat(c.n, 1, 1)
    inp, wm, wk, eot = state_walk_inputs()["L16"]
    from tests.gpu_helpers import to_dev
    lat, eot = to_dev(inp["sample"]), to_dev(eot)

    def vjp():
        return m.vjp(xin, 433, d.mems, d.masks, torch.ones_like(xin), row_maps=d.maps)[1]

    def weg_eval(mode):
        r = weg.loss_and_grad(m, lat, 500, wm, wk, [[2, 5]], True, eot, same_conditioning=mode)
        return float(r[0]), r[3].clone()

    g_vjp, g_weg = vjp(), weg_eval(False)
    for between in (vjp, lambda: weg_eval("memories")):
        assert same(call(m, name, t=433, reuse=2), fresh[433])
        call(m, name, t=432, reuse=2)
        assert launches() == full - memory_side
        between()
        assert same(call(m, name, t=432, reuse=2), fresh[432])
        assert launches() == full
    # ... and neither of them reuses what a guide call left: their results keep their bits around guide calls
    call(m, name, t=433, reuse=2)
    assert torch.equal(vjp(), g_vjp)
    weg_eval("memories")
    call(m, name, t=432, reuse=2)
    again = weg_eval("memories")
    assert again[0] == g_weg[0] and torch.equal(again[1], g_weg[1])
    assert same(call(m, name, t=432, reuse=0), fresh[432])


def test_a_refused_call_leaves_the_previous_call_s_memory_side_to_reuse():
    from convofusion_amd import _lib
    from tests.gpu_helpers import hip_denoiser, read_debug
    m = hip_denoiser(1234, 1.0)
    memory_side = (2 + 2 * int(m.num_layers)) + (6 * 5 + 2)
    launches = lambda: int(read_debug(m, "weg.info", (5,))[0])
    name = "product"
    fresh = call(m, name, t=432)
    full = launches()
    call(m, name, t=433, reuse=2)                        # a fresh call: it builds the tables over every timestep and runs everything
    assert launches() == full
    with pytest.raises(_lib.CfdError, match="reuse_memory_side = 1 is not 0 or 2"):
        call(m, name, t=433, reuse=1)                     # refused before the call begins: what the call before left stands
    assert launches() == full
    after = call(m, name, t=432, reuse=2)                 # another timestep, the memory side of the call before the refused one
    assert launches() == full - memory_side and same(after, fresh)


def test_library_refuses_before_any_launch_and_names_the_limit():
    import torch
    from convofusion_amd import _lib
    from tests.gpu_helpers import hip_denoiser, read_debug
    m = hip_denoiser(1234, 1.0)
    h = m.engine(torch.device("cuda"))
    lib = _lib.load()
    call(m, "two_tokens")
    before = read_debug(m, "weg.info", (5,))

    def raw(B=1, L=16, n=2, S=(3, 5, 6, 2, 1), t=5, **over):
        Be = n * B if n > 0 else 1
        x = torch.zeros(B, L, 128, device="cuda")
        arr, keep = m.pack_memories([torch.zeros(Be, s, 512, device="cuda") for s in S], {})
        w, mask = torch.zeros(B, max(n, 1), device="cuda"), torch.ones(B, L, device="cuda")
        tie = torch.full((B, L), -1, dtype=torch.int32, device="cuda")
        a = _lib.GuideArgs()
        a.B, a.L, a.n, a.timestep, a.sqrt_acp, a.sqrt_1m_acp = B, L, n, t, 0.9, 0.4
        a.x, a.mem, a.w, a.target, a.mask, a.inv_n, a.step = x.data_ptr(), arr, w.data_ptr(), x.data_ptr(), mask.data_ptr(), 1.0 / 128, 0.1
        outs = dict(loss=None, grad=C.c_void_p(x.data_ptr()), x_new=None, d_out=None)
        for k, v in over.items():
            if k == "tie":
                a.tie = tie.data_ptr()
            elif k in outs:
                outs[k] = v
            else:
                setattr(a, k, v)
        code = lib.cfd_denoise_guide(h, C.byref(a), outs["loss"], outs["grad"], outs["x_new"], outs["d_out"], None)
        msg = lib.cfd_last_error().decode()
        assert np.array_equal(read_debug(m, "weg.info", (5,)), before), msg
        del keep
        return code, msg

    for kw, text in ((dict(L=34), "L = 34 exceeds RT_MAX_L = 32"),
                     (dict(B=257, n=1), "Be * L = 4112 token rows exceed guide_max_rows = 4096"),
                     (dict(S=(24, 897, 24, 8, 1)), "1056 padded keys of the five memories together exceed RT_MAX_KEYS = 1024"),
                     (dict(t=1000), "timestep 1000 outside the timestep table"),
                     (dict(n=0), "n = 0 guidance chunks"),
                     (dict(target=None), "target is NULL"),
                     (dict(mask=None), "mask is NULL"),
                     (dict(inv_n=0.0), "inv_n = 0 is not positive"),
                     (dict(tie=True), "a tie without its tie_csr"),
                     (dict(reuse_memory_side=1), "reuse_memory_side = 1 is not 0 or 2"),
                     (dict(grad=None), "none of loss, grad, x_new and d_out is asked for")):
        code, msg = raw(**kw)
        assert code == -1 and text in msg, (kw, code, msg)
    assert raw(L=15)[0] == -2          # odd length: CFD_E_SHAPE like every entry point
    # at the limit the call runs: 4096 token rows
    x = torch.zeros(256, 16, 128, device="cuda")
    out = m.guide(x, 5, [torch.zeros(256, s, 512, device="cuda") for s in (3, 5, 6, 2, 1)], {}, torch.zeros(256, 1, device="cuda"),
                  torch.ones_like(x), torch.ones(256, 16, device="cuda"), sqrt_acp=0.9, sqrt_1m_acp=0.4, step=0.1, want=("loss", "grad"))
    assert bool(torch.isfinite(out[0])) and bool(torch.isfinite(out[1]).all())
    # the host-side inverse table refuses what check_tie refuses
    for bad, text in (([5, -1, -1], "is not -1 or a token"), ([0, -1, -1], "ties the token to itself"), ([1, 2, -1], "itself tied")):
        t = np.asarray(bad, dtype=np.int32)
        csr = np.zeros(2 * t.size + 1, dtype=np.int32)
        assert lib.cfd_guide_tie_csr(t.ctypes.data, t.size, csr.ctypes.data) == -1 and text in lib.cfd_last_error().decode()
