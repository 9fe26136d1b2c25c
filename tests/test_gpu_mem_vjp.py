"""GPU: ``cfd_denoise_vjp_mem`` -- the vector-Jacobian product of one denoiser forward with respect to its five memories, on the row-tile
kernels (rt_xbwd_dy_kernel<.., EMIT>, rt_bwd_gemm_kernel's T and G products, rt_xbwd_dn_kernel, rt_mem_ln_bwd_kernel) --
``Denoiser.vjp_memories`` and autograd through ``Denoiser.forward(..., memory_grad=True)`` on top of it.

Gates.  Against the float64 restatement tests/mem_vjp_ref.py, over the unmasked key rows of each memory (``weg_bwd_ref.tap_errors``:
relative L2 and worst key row): ``MEM_GRAD_GATE``, by the project's rule for ``F64_GRAD_GATE`` (tests/test_gpu_weg.py) -- 4 x the largest
value measured on the MI355X over these cases, and within the caps of the tap tests (2e-4 / 2e-3).  Against the reference's own autograd
(tests/golden/mem_vjp.npz, mem_vjp_heavy.npz): rel L2 < 1e-3.  Everything structural is exact: masked keys, orphan instances, rows without cotangent,
subsets, repeated calls, the sample's gradient and the output next to ``Denoiser.vjp``.
"""
import functools

import numpy as np
import pytest

from oracle import inputs
from tests import mem_vjp_ref, vjp_ref
from tests.helpers import load_golden, rel_l2, state_dict
from tests.test_gpu_denoise_vjp import S_PRODUCT, VJP_CASES, vjp_case
from tests.test_oracle_weg import CASES as WEG_CASES, weg_case
from tests.weg_bwd_ref import tap_errors

pytestmark = pytest.mark.gpu

MEM_NAMES = inputs.MEM_NAMES
# measured on the MI355X over MEM_CASES, the largest over the five memories of a case (profiles/r29_mem_vjp_accuracy.txt): relative L2
# 1.84e-6 (len32), worst key row 2.62e-6 (row_maps)
MEM_GRAD_GATE = (4 * 1.84e-6, 4 * 2.62e-6)
assert MEM_GRAD_GATE[0] <= 2e-4 and MEM_GRAD_GATE[1] <= 2e-3

MEM_CASES = VJP_CASES + ("tiny", "shared", "orphan")


@functools.lru_cache(maxsize=None)
def mem_case(name):
    """``vjp_case`` (inputs with per-row memories, timestep, distinct memories or None, row maps or None, masks of the distinct
    memories or None) plus: tiny -- B = 1, L = 4, every memory inside one partial key block; shared -- Be = 5, every memory ONE
    instance that all rows map to; orphan -- as shared with U = 2 and no row mapping to instance 1."""
    if name in VJP_CASES:
        return vjp_case(name)
    if name == "tiny":
        return inputs.make_plain_batch(seed=51, Be=1, L=4, S=(3, 5, 6, 2, 1), pad_tail=(1, 0, 2, 0, 0)), 37, None, None, None
    assert name in ("shared", "orphan")
    Be, L, S, U = 5, 16, (6, 20, 12, 8, 1), (1 if name == "shared" else 2)
    src = inputs.make_plain_batch(seed=52, Be=U, L=L, S=S, pad_tail=(2, 0, 3, 0, 0))
    sample = np.random.Generator(np.random.PCG64(53)).standard_normal((Be, L, 128), dtype=np.float32)
    maps = [np.zeros(Be, dtype=np.int32) for _ in MEM_NAMES]
    rows = dict(sample=sample, memories=[np.ascontiguousarray(m[r]) for m, r in zip(src["memories"], maps)],
                masks={k: (None if v is None else np.ascontiguousarray(v[maps[j]])) for j, (k, v) in enumerate(src["masks"].items())})
    assert list(src["masks"]) == list(MEM_NAMES)
    return rows, 433, src["memories"], maps, src["masks"]


def cotangent(name, shape):
    return vjp_ref.cotangent(9500 + len(name), shape)


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64"):
    """(cotangent, out, grad, per-INSTANCE memory gradients) of a case at ``dtype``, computed once."""
    inp, t, uniq, maps, _ = mem_case(name)
    c = cotangent(name, inp["sample"].shape)
    out, grad, d_rows = mem_vjp_ref.out_and_vjp_mem(state_dict(1234, 1.0), inp["sample"], t, inp["memories"], inp["masks"], c, dtype=np.dtype(dtype))
    if uniq is not None:
        d_rows = [mem_vjp_ref.sum_instances(d, maps[j], uniq[j].shape[0]) for j, d in enumerate(d_rows)]
    return c, out, grad, d_rows


def dev_case(name):
    from tests.gpu_helpers import to_dev
    inp, t, uniq, maps, umasks = mem_case(name)
    mems = [to_dev(m) for m in (uniq if uniq is not None else inp["memories"])]
    masks = {k: to_dev(v) for k, v in (umasks if uniq is not None else inp["masks"]).items()}
    return to_dev(inp["sample"]), mems, masks, (None if maps is None else [to_dev(r) for r in maps])


def host_masks(name):
    """Per memory the key-padding mask of its INSTANCES as bool [U, S] (all False where there is none)."""
    inp, _, uniq, _, umasks = mem_case(name)
    mems = uniq if uniq is not None else inp["memories"]
    mk = umasks if uniq is not None else inp["masks"]
    return [np.zeros(m.shape[:2], dtype=bool) if mk[k] is None else np.asarray(mk[k]).astype(bool) for k, m in zip(MEM_NAMES, mems)]


@pytest.mark.parametrize("name", MEM_CASES)
def test_memory_gradients_match_float64_and_are_exact_where_they_must_be(name):
    import torch
    from tests.gpu_helpers import hip_denoiser, read_debug, to_dev
    m = hip_denoiser(1234, 1.0)
    t, maps_h = mem_case(name)[1], mem_case(name)[3]
    x, mems, masks, maps = dev_case(name)
    Be = x.shape[0]
    c, _, _, d64 = reference(name)
    d32 = reference(name, "float32")[3]
    cd = to_dev(c)
    out, grad, d_mem = m.vjp_memories(x, t, mems, masks, cd, row_maps=maps)
    launches = int(read_debug(m, "weg.info", (5,))[0])
    hm = host_masks(name)
    worst = [0.0, 0.0]
    for j, k in enumerate(MEM_NAMES):
        got = d_mem[k].cpu().numpy()
        assert got.shape == d64[j].shape
        live = ~hm[j]
        if maps_h is not None:        # an instance no row maps to has no gradient to compare: exact zeros, below
            used = np.isin(np.arange(got.shape[0]), np.asarray(maps_h[j]))
            live = live & used[:, None]
            for u in np.nonzero(~used)[0]:
                assert not got[u].any(), (k, "orphan instance", int(u))
        # 1. against float64 over the unmasked key rows, next to numpy float32 of the same restatement
        e, er = tap_errors(got[live], d64[j][live])
        f, fr = tap_errors(d32[j][live], d64[j][live])
        print(f"{name}.{k}: U={got.shape[0]} S={got.shape[1]} launches {launches}: vs float64 rel L2 {e:.2e} worst key row {er:.2e} "
              f"(float32 numpy {f:.2e} / {fr:.2e}); |d_mem| {np.abs(d64[j]).max():.2e}")
        worst = [max(worst[0], e), max(worst[1], er)]
        # 2. masked keys are exactly 0
        assert not got[hm[j]].any() and not d64[j][hm[j]].any(), (k, "masked keys")
    print(f"{name}: worst over the memories {worst[0]:.2e} / {worst[1]:.2e}")
    assert worst[0] <= MEM_GRAD_GATE[0] and worst[1] <= MEM_GRAD_GATE[1]
    # 4. grad and out are Denoiser.vjp's, bit for bit
    out_v, grad_v = m.vjp(x, t, mems, masks, cd, row_maps=maps)
    assert torch.equal(out, out_v) and torch.equal(grad, grad_v)
    # 5. two calls return the same bits
    _, grad2, d_mem2 = m.vjp_memories(x, t, mems, masks, cd, row_maps=maps, want_out=False)
    assert torch.equal(grad, grad2) and all(torch.equal(d_mem[k], d_mem2[k]) for k in MEM_NAMES)
    # 6. a subset returns the same bits as those memories of the all-five call (and the sample's gradient may be left out)
    for wrt in (("lsnemb",), ("alsn", "tlsn")):
        _, g_s, d_s = m.vjp_memories(x, t, mems, masks, cd, wrt=wrt, row_maps=maps, want_out=False, want_grad=(wrt == ("lsnemb",)))
        assert sorted(d_s) == sorted(wrt) and all(torch.equal(d_s[k], d_mem[k]) for k in wrt)
        assert (g_s is None) if wrt != ("lsnemb",) else torch.equal(g_s, grad)
    # 7. a cotangent confined to batch row 1 leaves every instance that only other rows map to exactly 0
    if Be > 1:
        c1 = np.zeros_like(c)
        c1[1] = c[1]
        _, _, d1 = m.vjp_memories(x, t, mems, masks, to_dev(c1), row_maps=maps, want_out=False)
        for j, k in enumerate(MEM_NAMES):
            u1 = 1 if maps_h is None else int(maps_h[j][1])
            others = [u for u in range(d1[k].shape[0]) if u != u1]
            assert float(d1[k][u1].abs().max()) > 0 and not d1[k][others].any(), k


@pytest.mark.parametrize("name", vjp_ref.GOLDEN_CASES)
def test_memory_gradients_match_reference_autograd(name):
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    g = load_golden("mem_vjp_heavy" if name == "b1_heavy" else "mem_vjp")
    _, inp, t, _, _, _ = weg_case(name)
    m = hip_denoiser(WEG_CASES[name][0], WEG_CASES[name][1])
    mems, masks = dev_inputs(inp)
    c = vjp_ref.golden_cotangent(name, inp["sample"].shape)
    _, _, d_mem = m.vjp_memories(to_dev(inp["sample"]), t, mems, masks, to_dev(c), want_out=False, want_grad=False)
    for k in MEM_NAMES:
        e = rel_l2(d_mem[k].cpu().numpy(), g[f"{name}.{k}"])
        print(f"{name}.{k}: vs reference autograd {e:.2e}")
        assert e < 1e-3, k


def test_forward_with_memory_grad_is_the_inference_forward_and_autograd_reaches_the_memories():
    import torch
    from tests.gpu_helpers import hip_denoiser, to_dev
    m = hip_denoiser(1234, 1.0)
    t = mem_case("holes")[1]
    x, mems, masks, _ = dev_case("holes")
    c = to_dev(cotangent("holes", tuple(x.shape)))
    with torch.no_grad():
        out0, att0 = m(x, t, mems, mem_mask_dict=masks)
    xg = x.clone().requires_grad_(True)
    leaf = [e.clone().requires_grad_(True) for e in mems]
    out, att = m(xg, t, leaf, mem_mask_dict=masks, memory_grad=True)
    assert out.grad_fn is not None and torch.equal(out, out0)
    assert len(att) == 5 and all(not a.requires_grad and torch.equal(a, b) for a, b in zip(att, att0))
    got = torch.autograd.grad(out, [xg] + leaf, c)
    _, grad, d_mem = m.vjp_memories(x, t, mems, masks, c)
    assert torch.equal(got[0], grad) and all(torch.equal(g, d_mem[k]) for g, k in zip(got[1:], MEM_NAMES))
    # a memory that does not require grad gets None; a sample that does not require grad is no obstacle
    some = [e.clone().requires_grad_(j in (1, 4)) for j, e in enumerate(mems)]
    out, _ = m(x, t, some, mem_mask_dict=masks, memory_grad=True)
    assert out.grad_fn is not None and torch.equal(out, out0)
    (out * c).sum().backward()
    assert [e.grad is None for e in some] == [True, False, True, True, False]
    assert torch.equal(some[1].grad, d_mem["alsn"]) and torch.equal(some[4].grad, d_mem["lsnemb"])
    # nothing requires grad, or grad is off: the inference path
    assert m(x, t, mems, mem_mask_dict=masks, memory_grad=True)[0].grad_fn is None
    with torch.no_grad():
        assert m(xg, t, leaf, mem_mask_dict=masks, memory_grad=True)[0].grad_fn is None
    # without the keyword a memory that requires grad is refused as before
    with pytest.raises(NotImplementedError, match="no gradient with respect to its memories"):
        m(xg, t, leaf, mem_mask_dict=masks)


def test_plain_vjp_launches_what_it_launched_and_the_memory_gradient_adds_its_own():
    """The product shape (Be = 7 rows of L = 16 over two distinct memories): cfd_denoise_vjp 219 launches; all five
    memories + 3 per layer + 1, whatever the subset."""
    import torch
    from tests.gpu_helpers import hip_denoiser, read_debug
    m = hip_denoiser(1234, 1.0)
    t = mem_case("row_maps")[1]
    x, mems, masks, maps = dev_case("row_maps")
    assert tuple(int(e.shape[1]) for e in mems) == S_PRODUCT
    c = torch.ones_like(x)
    m.vjp(x, t, mems, masks, c, row_maps=maps)
    assert int(read_debug(m, "weg.info", (5,))[0]) == 219
    m.vjp_memories(x, t, mems, masks, c, row_maps=maps)
    assert int(read_debug(m, "weg.info", (5,))[0]) == 219 + 3 * 9 + 1
    m.vjp_memories(x, t, mems, masks, c, wrt=("lsnemb",), row_maps=maps, want_grad=False)
    assert int(read_debug(m, "weg.info", (5,))[0]) == 219 + 3 * 9 + 1 - 1
    m.vjp_memories(x, t, mems, masks, c, wrt=(), row_maps=maps)
    assert int(read_debug(m, "weg.info", (5,))[0]) == 219


def test_library_refuses_a_call_that_wants_nothing_and_names_the_limit_it_refuses():
    import ctypes as C
    import torch
    from convofusion_amd import _lib
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    h = m.engine(torch.device("cuda"))
    lib = _lib.load()

    def call(Be, L, S, want_grad, want_mem):
        x = torch.zeros(Be, L, 128, device="cuda")
        mems = [torch.zeros(Be, s, 512, device="cuda") for s in S]
        arr, keep = m.pack_memories(mems, {})
        a = _lib.VjpArgs()
        a.Be, a.L, a.timestep, a.sample, a.mem = Be, L, 5, x.data_ptr(), arr
        g = torch.empty_like(x)
        d = [torch.empty_like(e) for e in mems]
        ptrs = (C.c_void_p * _lib.NUM_MEM)()
        for j in want_mem:
            ptrs[j] = d[j].data_ptr()
        return lib.cfd_denoise_vjp_mem(h, C.byref(a), C.c_void_p(x.data_ptr()), None, C.c_void_p(g.data_ptr()) if want_grad else None, ptrs,
                                       None), lib.cfd_last_error().decode()

    code, msg = call(1, 16, (3, 5, 6, 2, 1), False, ())
    assert code == -1 and "null argument" in msg, (code, msg)
    for args, text in (((1, 34, (3, 5, 6, 2, 1)), "L = 34 exceeds RT_MAX_L = 32"),
                       ((44, 16, (3, 5, 6, 2, 1)), "Be * L = 704 token rows exceed rt_max_rows = 700"),
                       ((1, 16, (24, 897, 24, 8, 1)), "1056 padded keys of the five memories together exceed RT_MAX_KEYS = 1024")):
        code, msg = call(*args, False, (4,))
        assert code == -1 and text in msg, (code, msg)
    assert call(1, 16, (3, 5, 6, 2, 1), False, (4,))[0] == 0 and call(1, 16, (3, 5, 6, 2, 1), True, ())[0] == 0
