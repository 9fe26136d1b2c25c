"""GPU: ``cfd_denoise_vjp`` (the vector-Jacobian product of one denoiser forward with respect to its sample, on the row-tile kernels),
autograd through ``Denoiser.forward`` on top of it, its state on a handle it shares with ``cfd_weg_eval`` and an open sampling run,
and ``sampler.sample_with_loss_guidance``.

Gates.  Against the float64 restatement tests/vjp_ref.py: the project's float64 gradient gates, ``F64_GRAD_GATE`` of
tests/test_gpu_weg.py (relative L2 over the gradient 5.44e-5, worst token row 3.46e-4) -- the sweep runs the same kernels behind the
same split-pair forward.  Against the reference's own autograd (tests/golden/vjp.npz): rel L2 < 1e-3.  Everything structural is exact.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import inputs
from tests import vjp_ref
from tests.helpers import load_golden, rel_l2, state_dict
from tests.test_gpu_weg import F64_GRAD_GATE, _shape_case
from tests.test_oracle_weg import CASES as WEG_CASES, weg_case
from tests.weg_bwd_ref import tap_errors

pytestmark = pytest.mark.gpu

S_PRODUCT = (24, 161, 24, 8, 1)


@functools.lru_cache(maxsize=None)
def vjp_case(name):
    """(inputs with per-row memories, timestep, distinct memories or None, row maps or None, masks of the distinct memories or None).
    len2: two tokens per row; len18_t0: a partial second token tile per row, timestep 0; len32: the limit; big_keys: 672 padded keys
    (rt_xbwd_dy_kernel<RT_MAX_KEYS>); holes: B = 3, masks with holes on all five memories; row_maps: the product shape -- B = 1, the
    7-chunk guidance batch over B + 1 distinct memories."""
    if name in ("len2", "big_keys", "holes"):
        inp, t, _ = _shape_case(name)
        return inp, t, None, None, None
    if name == "len18_t0":
        return inputs.make_plain_batch(seed=41, Be=2, L=18, S=(6, 20, 12, 8, 1), pad_tail=(2, 0, 3, 0, 0)), 0, None, None, None
    if name == "len32":
        return inputs.make_plain_batch(seed=42, Be=1, L=32, S=(6, 20, 40, 8, 1), pad_tail=(2, 3, 0, 0, 0)), 700, None, None, None
    assert name == "row_maps"
    cb = inputs.make_cfg_batch(seed=43, B=1, L=16, S=S_PRODUCT, pad_tail=(5, 0, 7, 0, 0))
    sample = np.random.Generator(np.random.PCG64(44)).standard_normal((7, 16, 128), dtype=np.float32)
    umasks = {}
    for j, k in enumerate(inputs.MEM_NAMES):      # masks of the distinct memories: row u's mask is that of a batch row that maps to u
        mk = cb["masks"][k]
        umasks[k] = None if mk is None else np.stack([mk[list(cb["row_map"][j]).index(u)] for u in range(2)])
    return dict(sample=sample, memories=cb["memories"], masks=cb["masks"]), 433, cb["unique"], cb["row_map"], umasks


VJP_CASES = ("len2", "len18_t0", "len32", "big_keys", "holes", "row_maps")


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64"):
    inp, t = vjp_case(name)[:2]
    c = vjp_ref.cotangent(9000 + len(name), inp["sample"].shape)
    return (c,) + vjp_ref.out_and_vjp(state_dict(1234, 1.0), inp["sample"], t, inp["memories"], inp["masks"], c, dtype=np.dtype(dtype))


def dev_case(name):
    """(sample, memories, masks, row maps or None) of a case on the device, as the library takes them."""
    from tests.gpu_helpers import to_dev
    inp, t, uniq, maps, umasks = vjp_case(name)
    mems = [to_dev(m) for m in (uniq if uniq is not None else inp["memories"])]
    masks = {k: to_dev(v) for k, v in (umasks if uniq is not None else inp["masks"]).items()}
    return to_dev(inp["sample"]), mems, masks, (None if maps is None else [to_dev(r) for r in maps])


def forward_c(m, x, t, mems, masks, row_maps=None):
    """cfd_forward on the same inputs (``Denoiser.forward`` takes no row maps)."""
    import torch
    from convofusion_amd import _lib
    h = m.engine(x.device, mem_len=max(int(e.shape[1]) for e in mems))
    arr, keep = m.pack_memories(mems, masks, row_maps)
    out = torch.empty_like(x)
    ts = (C.c_int32 * 1)(int(t))
    _lib.check(_lib.load().cfd_forward(h, C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], ts, 1, arr, C.c_void_p(out.data_ptr()), None,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    del keep
    return out


@pytest.mark.parametrize("name", VJP_CASES)
def test_vjp_matches_float64_and_is_exact_where_it_must_be(name):
    import torch
    from tests.gpu_helpers import hip_denoiser, read_debug, to_dev
    m = hip_denoiser(1234, 1.0)
    t = vjp_case(name)[1]
    x, mems, masks, maps = dev_case(name)
    Be, L, _ = x.shape
    c, o64, g64, e64 = reference(name)
    _, o32, g32, e32 = reference(name, "float32")
    out, grad = m.vjp(x, t, mems, masks, to_dev(c), row_maps=maps)
    info = read_debug(m, "weg.info", (5,))
    g_emb = read_debug(m, "weg.g", (Be * L, 512))
    e, er = tap_errors(grad.cpu().numpy().reshape(Be * L, -1), g64.reshape(Be * L, -1))
    ee, eer = tap_errors(g_emb, e64)
    f, fr = tap_errors(g32.reshape(Be * L, -1), g64.reshape(Be * L, -1))
    fe, fer = tap_errors(e32, e64)
    print(f"{name}: Be={Be} L={L} t={t} launches {int(info[0])} Sp_tot {int(info[1])} rt_xbwd_dy_kernel<{int(info[2])}>; "
          f"grad vs float64 rel L2 {e:.2e} worst row {er:.2e} (float32 numpy {f:.2e} / {fr:.2e}); at the embedding's output {ee:.2e} / {eer:.2e} "
          f"(float32 numpy {fe:.2e} / {fer:.2e}); out vs float64 {rel_l2(out.cpu().numpy(), o64):.2e}")
    assert int(info[2]) == (1024 if name == "big_keys" else 512)
    assert int(info[1]) == sum((int(s.shape[1]) + 31) // 32 * 32 for s in mems)
    assert e <= F64_GRAD_GATE[0] and er <= F64_GRAD_GATE[1]
    assert rel_l2(out.cpu().numpy(), o64) < 1e-3
    # the forward of this call is cfd_forward's, bit for bit; two identical calls are bit-identical; out may be left out
    assert torch.equal(out, forward_c(m, x, t, mems, masks, maps))
    out2, grad2 = m.vjp(x, t, mems, masks, to_dev(c), row_maps=maps)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    none, grad3 = m.vjp(x, t, mems, masks, to_dev(c), row_maps=maps, want_out=False)
    assert none is None and torch.equal(grad, grad3)
    # rows are independent: a cotangent in one batch row only leaves every other row's gradient exactly 0
    if Be > 1:
        c1 = np.zeros_like(c)
        c1[1] = c[1]
        g1 = m.vjp(x, t, mems, masks, to_dev(c1), row_maps=maps)[1]
        assert float(g1[1].abs().max()) > 0 and not g1[0].any() and not g1[2:].any()
        assert torch.equal(g1[1], grad[1])


@pytest.mark.parametrize("name", vjp_ref.GOLDEN_CASES)
def test_vjp_matches_reference_autograd(name):
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    g = load_golden("vjp")
    _, inp, t, _, _, _ = weg_case(name)
    m = hip_denoiser(WEG_CASES[name][0], WEG_CASES[name][1])
    mems, masks = dev_inputs(inp)
    c = vjp_ref.golden_cotangent(name, inp["sample"].shape)
    out, grad = m.vjp(to_dev(inp["sample"]), t, mems, masks, to_dev(c))
    eo, eg = rel_l2(out.cpu().numpy(), g[name + ".out"]), rel_l2(grad.cpu().numpy(), g[name + ".grad"])
    print(f"{name}: vs reference autograd out {eo:.2e} grad {eg:.2e}")
    assert eo < 1e-3 and eg < 1e-3


def test_forward_under_grad_is_the_inference_forward_with_a_grad_fn():
    """Fails on a tree without the feature: there ``forward`` raises NotImplementedError for a sample that requires grad."""
    import torch
    from tests.gpu_helpers import hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    t = vjp_case("holes")[1]
    x, mems, masks, _ = dev_case("holes")
    c = to_dev(reference("holes")[0])
    with torch.no_grad():
        out0, att0 = m(x, t, mems, mem_mask_dict=masks)
    xg = x.clone().requires_grad_(True)
    out, att = m(xg, t, mems, mem_mask_dict=masks)
    assert out.grad_fn is not None and torch.equal(out, out0)
    assert len(att) == 5 and all(not a.requires_grad and torch.equal(a, b) for a, b in zip(att, att0))
    (g,) = torch.autograd.grad((out * c).sum(), xg)
    assert torch.equal(g, m.vjp(x, t, mems, masks, c)[1])
    # a forward, a WEG evaluation and another differentiable forward between forward and backward do not reach the gradient
    out, _ = m(xg, t, mems, mem_mask_dict=masks)
    with torch.no_grad():
        m(x + 1.0, 7, mems, mem_mask_dict=masks)
    x2 = (x * 0.5).requires_grad_(True)
    m(x2, 900, mems, mem_mask_dict=masks)[0].sum().backward()
    (g2,) = torch.autograd.grad((out * c).sum(), xg)
    assert torch.equal(g, g2)
    # through a function of the output, on the second engine, and without the maps
    keep, m.return_attention = m.return_attention, False
    try:
        out, att = m(xg, t, mems, mem_mask_dict=masks, side_engine=True)
        assert att == []
        (g3,) = torch.autograd.grad(((out - 1.0) ** 2).sum(), xg)
        assert torch.equal(g3, m.vjp(x, t, mems, masks, 2.0 * (out0 - 1.0))[1])
    finally:
        m.return_attention = keep
    # refusals (before any device work: tests/test_vjp_host.py raises them on a module that has no device)
    with pytest.raises(NotImplementedError, match="no gradient with respect to its memories"):
        m(xg, t, [e.clone().requires_grad_(True) for e in mems], mem_mask_dict=masks)
    with pytest.raises(NotImplementedError, match="one timestep for all rows"):
        m(xg, torch.tensor([1, 2, 3]), mems, mem_mask_dict=masks)
    with pytest.raises(NotImplementedError, match="exceed the row-tile path's 32"):
        m(torch.zeros(1, 34, 128, device="cuda", requires_grad=True), t, [e[:1] for e in mems])


def test_library_names_the_limit_it_refuses():
    import torch
    from convofusion_amd import _lib
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    h = m.engine(torch.device("cuda"))
    lib = _lib.load()

    def call(Be, L, S, t=5):
        x = torch.zeros(Be, L, 128, device="cuda")
        arr, keep = m.pack_memories([torch.zeros(Be, s, 512, device="cuda") for s in S], {})
        a = _lib.VjpArgs()
        a.Be, a.L, a.timestep, a.sample, a.mem = Be, L, t, x.data_ptr(), arr
        g = torch.empty_like(x)
        return lib.cfd_denoise_vjp(h, C.byref(a), C.c_void_p(x.data_ptr()), None, C.c_void_p(g.data_ptr()), None), lib.cfd_last_error().decode()

    for args, text in (((1, 34, (3, 5, 6, 2, 1)), "L = 34 exceeds RT_MAX_L = 32"),
                       ((44, 16, (3, 5, 6, 2, 1)), "Be * L = 704 token rows exceed rt_max_rows = 700"),
                       ((1, 16, (24, 897, 24, 8, 1)), "1056 padded keys of the five memories together exceed RT_MAX_KEYS = 1024"),
                       ((1, 16, (3, 5, 6, 2, 1), 1000), "timestep 1000 outside the timestep table")):
        code, msg = call(*args)
        assert code == -1 and text in msg, (code, msg)
    assert call(1, 15, (3, 5, 6, 2, 1))[0] == -2          # odd length: CFD_E_SHAPE like every entry point


def test_three_entry_points_refuse_a_latent_call_alike_and_before_any_launch():
    """Be = 1, L = 4, S = (3, 5, 6, 2, 1): an odd L (3), timestep = the table's rows, and a memory one token past the memory PE's rows
    come back from cfd_weg_eval, cfd_denoise_vjp and cfd_denoise_vjp_mem with the same code and the same cfd_last_error text (one
    check_latent_call behind all three), each before any launch: "weg.info" still reports the launches of the call before, a
    vjp_memories whose count (the sweep plus the memory gradient's launches) neither of the other two entry points has."""
    import torch
    from convofusion_amd import _lib
    from tests.gpu_helpers import hip_denoiser, read_debug
    m = hip_denoiser(1234, 1.0)
    h = m.engine(torch.device("cuda"))
    lib = _lib.load()
    S, T = (3, 5, 6, 2, 1), 1000
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok_mems = [torch.zeros(1, s, 512, device="cuda") for s in S]
    x4 = torch.zeros(1, 4, 128, device="cuda")
    m.vjp_memories(x4, 5, ok_mems, {}, torch.ones_like(x4))
    before = read_debug(m, "weg.info", (5,))
    assert int(before[0]) > 0
    tok_off, tok_idx = np.array([0, 1], dtype=np.int32), np.array([2], dtype=np.int32)

    def calls(L, t, S):
        x = torch.zeros(1, L, 128, device="cuda")
        arr, keep = m.pack_memories([torch.zeros(1, s, 512, device="cuda") for s in S], {})
        g, small = torch.empty_like(x), torch.empty(4, device="cuda")
        px, pg = C.c_void_p(x.data_ptr()), C.c_void_p(g.data_ptr())
        w = _lib.WegArgs()
        w.B, w.L, w.timestep, w.latents, w.mem = 1, L, t, x.data_ptr(), arr
        w.tok_off, w.tok_idx, w.last = tok_off.ctypes.data, tok_idx.ctypes.data, 5
        w.kernel3 = (C.c_float * 3)(0.25, 0.5, 0.25)
        a = _lib.VjpArgs()
        a.Be, a.L, a.timestep, a.sample, a.mem = 1, L, t, x.data_ptr(), arr
        d_mem = (C.c_void_p * _lib.NUM_MEM)()
        d0 = torch.empty(1, S[0], 512, device="cuda")
        d_mem[0] = d0.data_ptr()
        got = []
        for entry in (lambda: lib.cfd_weg_eval(h, C.byref(w), C.c_void_p(small.data_ptr()), C.c_void_p(small.data_ptr()), pg, None, stream),
                      lambda: lib.cfd_denoise_vjp(h, C.byref(a), px, None, pg, stream),
                      lambda: lib.cfd_denoise_vjp_mem(h, C.byref(a), px, None, pg, d_mem, stream)):
            got.append((entry(), lib.cfd_last_error().decode()))
            assert np.array_equal(read_debug(m, "weg.info", (5,)), before), got[-1]
        del keep
        return got

    rows = m._main["mem_len"]                       # the memory PE's rows on this handle (1024, or what an earlier call extended it to)
    for what, args, code, text in (("odd L", (3, 5, S), -2, "latent length 3 is odd"),
                                   ("timestep", (4, T, S), -1, f"timestep {T} outside the timestep table ({T} rows)"),
                                   ("memory PE", (4, 5, (3, rows + 1, 6, 2, 1)), -2, f"memory alsn has {rows + 1} tokens, memory PE buffer has {rows} rows")):
        got = calls(*args)
        print(what, "->", got)
        assert got[0] == got[1] == got[2], (what, got)
        assert got[0][0] == code and text in got[0][1], (what, got)
    # the handle is as it was: the call before, again, to the bit
    g0 = m.vjp_memories(x4, 5, ok_mems, {}, torch.ones_like(x4))
    assert np.array_equal(read_debug(m, "weg.info", (5,)), before)
    assert torch.equal(g0[1], m.vjp(x4, 5, ok_mems, {}, torch.ones_like(x4))[1])


def test_weg_evaluations_around_a_vjp_reuse_nothing_it_overwrote():
    """cfd_weg_eval and cfd_denoise_vjp share the row-tile arena, the workspace and the per-timestep tables: a WEG evaluation that
    states "same conditioning" behind a VJP call -- on the SAME memories, and on others of another shape -- equals a fresh one."""
    import torch
    from convofusion_amd import weg
    from tests.gpu_helpers import hip_denoiser, to_dev
    from tests.test_gpu_weg import state_walk_inputs
    m = hip_denoiser(1234, 1.0)
    inp, mems, masks, eot = state_walk_inputs()["L16"]
    eot = to_dev(eot)
    lat, lat2 = to_dev(inp["sample"]), to_dev(inp["sample"] + np.float32(0.01))
    focus = [[2, 5]]
    xo, mo, ko, _ = dev_case("len18_t0")
    c = torch.ones_like(lat)

    def ev(latents, t, same):
        r = weg.loss_and_grad(m, latents, t, mems, masks, focus, True, eot, same_conditioning=same)
        return float(r[0]), r[1].clone(), r[3].clone()

    def same(a, b):
        return a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])

    fresh = {t: ev(lat2, t, False) for t in (500, 499)}
    for vjp_args in ((lat, 321, mems, masks, c), (xo, 0, mo, ko, torch.ones_like(xo))):
        for mode in (True, "memories"):
            for _ in range(3):                       # eager, captured, replayed: a VJP behind each
                ev(lat, 500, mode)
                g1 = m.vjp(*vjp_args)[1]
                assert same(ev(lat2, 500, mode), fresh[500]), (mode, "t 500")
                assert torch.equal(g1, m.vjp(*vjp_args)[1])
            if mode == "memories":
                m.vjp(*vjp_args)
                assert same(ev(lat2, 499, mode), fresh[499]), (mode, "t 499")
    assert same(ev(lat2, 500, False), fresh[500])


def test_vjp_between_two_steps_leaves_an_open_run_s_bits():
    import torch
    from convofusion_amd import scheduler
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    B, L, S = 1, 16, (6, 20, 12, 8, 1)
    cb = inputs.make_cfg_batch(seed=23, B=B, L=L, S=S, pad_tail=(2, 0, 3, 0, 0))
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    sch = scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)
    x, vm, vk, maps = dev_case("row_maps")
    c = torch.ones_like(x)

    def go(interleave):
        with SamplingRun(m, sch, mems, masks, B, L, 20, guidance_scale=7.5, seed=3) as run:
            grads = []
            for _ in range(4):
                run.steps(1)
                if interleave:     # on the run's own handle: the evaluation has a workspace of its own
                    grads.append(m.vjp(x, 433, vm, vk, c, row_maps=maps)[1])
                    grads.append(m.vjp(run.read(), 433, [e[:1] for e in mems], {k: (v[:1] if v is not None else None) for k, v in masks.items()},
                                       torch.ones(B, L, 128, device="cuda"))[1])
            return run.read(), grads

    plain, _ = go(False)
    mixed, grads = go(True)
    assert torch.equal(plain, mixed)
    assert all(torch.equal(g, grads[0]) for g in grads[0::2]) and float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], m.vjp(x, 433, vm, vk, c, row_maps=maps)[1])


def test_loss_guided_loop_matches_the_reference_loop_driven_by_torch_autograd():
    """3 DDIM iterations (eta 0), B = 1, L = 4, tiny memories, ``edit.keyframe_loss``: the final latents against the same loop on the
    CPU -- torch autograd through oracle.denoiser_torch for the gradient, oracle.sampler_ref's combine and oracle.scheduler_ref's step
    for the iteration -- at the trajectory gate of the short goldens (1e-3 relative); step_size 0 is ``sample`` bit for bit."""
    import torch
    from convofusion_amd import edit, sampler, scheduler
    from oracle import denoiser_torch, sampler_ref, scheduler_ref
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    B, L, N, scale, step = 1, 4, 3, 7.5, 0.5
    cb = inputs.make_cfg_batch(seed=71, B=B, L=L, S=(3, 5, 6, 2, 1), pad_tail=(1, 0, 2, 0, 0))
    target = np.random.Generator(np.random.PCG64(72)).standard_normal((B, L, 128), dtype=np.float32) * np.float32(0.5)
    keep = np.zeros((B, L), dtype=bool)
    keep[0, 1] = keep[0, 2] = True
    # ---- the reference loop on the CPU
    sd = denoiser_torch.to_torch(state_dict(1234, 1.0))
    tm = [torch.from_numpy(v) for v in cb["memories"]]
    tk = {k: (torch.from_numpy(v) if v is not None else None) for k, v in cb["masks"].items()}
    fwd = denoiser_torch.denoiser_forward.__wrapped__
    loss_cpu = edit.keyframe_loss(torch.from_numpy(target), torch.from_numpy(keep))

    def reference_loop(step_size):
        ref = scheduler_ref.DDIMSchedulerRef(**SCHED_KW)
        ref.set_timesteps(N)
        lat = cb["init"].copy()
        for t in ref.timesteps:
            x = torch.from_numpy(lat).clone().requires_grad_(True)
            with torch.enable_grad():
                e = fwd(sd, x.repeat(7, 1, 1), int(t), tm, tk)[0].view(7, B, L, 128)
                eps = e[0]
                for k in range(1, 6):
                    eps = eps + scale * (e[k] - e[0])
                a = float(ref.alphas_cumprod[int(t)])
                (g,) = torch.autograd.grad(loss_cpu((x - (1.0 - a) ** 0.5 * eps) / a ** 0.5), x)
            lat = (lat - np.float32(step_size) * g.numpy()).astype(np.float32)
            with torch.no_grad():
                pred = fwd(sd, torch.from_numpy(np.concatenate([lat] * 7)), int(t), tm, tk)[0].numpy()
            lat = ref.step(sampler_ref.cfg_combine(pred, scale), t, lat, eta=0.0)
        return lat

    want, unguided = reference_loop(step), reference_loop(0.0)
    assert rel_l2(want, unguided) > 1e-2          # (of the reference: the guidance moves the result far beyond the gate below)
    # ---- the product
    m = hip_denoiser(1234, 1.0)
    mems = [to_dev(v) for v in cb["memories"]]
    masks = {k: to_dev(v) for k, v in cb["masks"].items()}
    sch = scheduler.DDIMScheduler(**SCHED_KW)
    kw = dict(B=B, L=L, num_inference_steps=N, guidance_scale=scale, eta=0.0, init_latents=to_dev(cb["init"]))
    loss_dev = edit.keyframe_loss(to_dev(target), to_dev(keep))
    got = sampler.sample_with_loss_guidance(m, sch, mems, masks, loss_dev, step, **kw)
    e = rel_l2(got.cpu().numpy(), want)
    print(f"loss-guided DDIM-3: vs the reference loop {e:.2e}; guided vs unguided (reference) {rel_l2(want, unguided):.2e}")
    assert e < 1e-3
    plain = sampler.sample(m, sch, mems, masks, **kw)
    assert torch.equal(sampler.sample_with_loss_guidance(m, sch, mems, masks, loss_dev, 0.0, **kw), plain)
    assert torch.equal(sampler.sample_with_loss_guidance(m, sch, mems, masks, loss_dev, step, guided_iterations=(), **kw), plain)
    # a range of iterations, a per-iteration step size, distinct memories with row maps: the same loop
    uniq = [to_dev(v) for v in cb["unique"]]
    umask = {}
    for j, k in enumerate(inputs.MEM_NAMES):
        mk = cb["masks"][k]
        umask[k] = None if mk is None else to_dev(np.stack([mk[list(cb["row_map"][j]).index(u)] for u in range(B + 1)]))
    again = sampler.sample_with_loss_guidance(m, sch, uniq, umask, loss_dev, [step] * N, guided_iterations=range(N), dedup=False,
                                              row_maps=[to_dev(r) for r in cb["row_map"]], **kw)
    assert rel_l2(again.cpu().numpy(), want) < 1e-3
