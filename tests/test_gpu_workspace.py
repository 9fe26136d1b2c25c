"""-m gpu: the workspace holds what the problem's forward path addresses (setup_problem's sizing block, the table on struct Work), and no
path depends on a buffer another path happened to size.  Every case runs on a ``Denoiser`` of its own -- a fresh workspace -- and must
give, bit for bit, what the same call gives on the suite's cached ``hip_denoiser``, whose workspace has by then grown through whatever ran
before.  The calls are the ones tests/test_gpu_forward_path.py pins to each path, at the smallest shapes that take it (memories
S = (6, 20, 6, 8, 1): 160 padded keys; the seeded test weights):

  fused         8 rows of L = 48 (six workgroups of four query tiles), one timestep, no attention outputs: the pair instance.  The
                three-launch path's score buffer "sc" is not allocated: cfd_debug_read refuses it, "holds 0 bytes".
  three-launch  the same rows with per-row timesteps and attention outputs: "sc" [M][Sp_tot] is there afterwards.
  row-tile      14 rows of L = 16 (224 tokens, 14 token tiles: two 16-feature blocks per workgroup), and 3 rows of L = 18, whose second
                token tile is partial -- the smallest shape at which the cell statistics, now [M][Sp_tot / 32] float4, could be
                indexed past their end; with attention outputs.
  in both orders, on one handle each: the reverse order runs the L = 18 problem on exactly-sized buffers first.
  LayerNorm fold  three iterations of a DDPM run (a four-step schedule: the count must divide 1000) at L = 16, B = 11 (77 rows, 1 232
                tokens): ln_stat and rt_cur come from set-up, so the process's live device buffers do not change between the open
                run and its last step.
  WEG           loss_and_grad at a row-tile shape, with one-row tables and with the per-timestep tables kept on the handle: Work::now_*
                through the reverse sweep, rt_cur in the evaluation's own workspace."""
import ctypes as C

import pytest
import torch

from oracle import inputs

pytestmark = pytest.mark.gpu

S, PAD, SP_TOT = (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), 160
E_ARG = -1   # CFD_E_ARG
PAIR, NONE = 0, -1
# name -> (rows, L, per-row timesteps, attention outputs, "xa.info" instance, xattn launches of one forward)
CALLS = {
    "fused": (8, 48, False, False, PAIR, 9),
    "three-launch": (8, 48, True, True, NONE, 0),
    "row-tile L=16": (14, 16, False, True, NONE, 18),
    "row-tile L=18": (3, 18, False, True, NONE, 18),
}


def _fresh():
    from tests.gpu_helpers import hip_denoiser
    return hip_denoiser.__wrapped__(1234, 1.0)


def _live():
    from convofusion_amd import _lib
    n, nbytes = C.c_longlong(-1), C.c_longlong(-1)
    _lib.check(_lib.load().cfd_debug_live_buffers(C.byref(n), C.byref(nbytes)))
    return int(n.value), int(nbytes.value)


def _forward(m, name, data):
    Be, L, per_row, att, _, _ = CALLS[name]
    x, mems, masks = data[name]
    t = torch.arange(Be) * 37 + 100 if per_row else torch.tensor(500)
    keep = m.return_attention
    m.return_attention = att
    try:
        with torch.no_grad():
            out, maps = m(x, t, mems, mem_mask_dict=masks)
    finally:
        m.return_attention = keep
    torch.cuda.synchronize()
    return out, maps


@pytest.fixture(scope="module")
def data():
    from tests.gpu_helpers import dev_inputs, to_dev
    made = {}
    for k, (name, (Be, L, *_)) in enumerate(CALLS.items()):
        inp = inputs.make_plain_batch(seed=31 + k, Be=Be, L=L, S=S, pad_tail=PAD)
        made[name] = (to_dev(inp["sample"]), *dev_inputs(inp))
    return made


@pytest.fixture(scope="module")
def reference(data):
    """Each call once on the cached handle, whatever its workspace has grown to."""
    from tests.gpu_helpers import hip_denoiser
    m = hip_denoiser(1234, 1.0)
    return {name: _forward(m, name, data) for name in CALLS}


def _run_and_compare(m, name, data, reference, sc_absent):
    from convofusion_amd import _lib
    from tests.gpu_helpers import read_debug
    from tests.test_gpu_forward_path import _profile_handle
    Be, L, _, att, inst, n_xattn = CALLS[name]
    out, maps = _forward(m, name, data)
    info = read_debug(m, "xa.info", (7,))
    assert int(info[0]) == inst and (inst != PAIR or int(info[1]) >= 6), (name, info)
    if sc_absent:   # nothing on this handle has taken a path that owns the score buffer
        with pytest.raises(_lib.CfdError) as ei:
            read_debug(m, "sc", (1,))
        assert ei.value.code == E_ARG and "holds 0 bytes" in str(ei.value), str(ei.value)
    elif name != "fused":
        read_debug(m, "sc", (Be * L, SP_TOT))
    ref_out, ref_maps = reference[name]
    assert torch.equal(out, ref_out), name
    assert len(maps) == (5 if att else 0) == len(ref_maps)
    for j, (a, b) in enumerate(zip(maps, ref_maps)):
        assert torch.equal(a, b), (name, j)
    assert _profile_handle(m)["xattn"][1] == n_xattn, name   # the path taken: the launches of this problem's forward once more


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_each_path_sizes_its_own_buffers(data, reference, order):
    m = _fresh()
    names = list(CALLS) if order == "forward" else list(CALLS)[::-1]
    for k, name in enumerate(names):
        _run_and_compare(m, name, data, reference, sc_absent=(name == "fused" and k == 0))


def test_ln_fold_run_allocates_in_setup_only():
    from convofusion_amd import scheduler
    from convofusion_amd.sampler import SamplingRun
    from tests.gpu_helpers import SCHED_KW, hip_denoiser, to_dev
    B, L, N, N_RUN = 11, 16, 4, 3
    cb = inputs.make_cfg_batch(seed=1, B=B, L=L, S=S, pad_tail=PAD)
    mems, masks = [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}

    def latents(m, watch):
        with SamplingRun(m, scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW), mems, masks, B, L, N, seed=7) as run:
            opened = _live()
            run.steps(N_RUN)
            out = run.read()
            if watch:
                assert _live() == opened, "a launch sequence of the open run allocated"
            return out

    got = latents(_fresh(), True)
    assert torch.isfinite(got).all()
    assert torch.equal(got, latents(hip_denoiser(1234, 1.0), False))


def test_weg_evaluation_on_a_fresh_handle():
    from convofusion_amd import weg
    from tests.gpu_helpers import dev_inputs, hip_denoiser, to_dev
    inp = inputs.make_plain_batch(seed=23, Be=2, L=16, S=S, pad_tail=PAD)
    mems, masks = dev_inputs(inp)
    x = to_dev(inp["sample"])

    def evaluations(m):
        """One evaluation with one-row tables, then one with the per-timestep tables kept on the handle (this step's rows: rt_cur)."""
        res = []
        for t, same in ((500, False), (300, "memories")):
            loss, losses, mx, grad = weg.loss_and_grad(m, x, t, mems, masks, [[1, 2], [2]], False, same_conditioning=same)
            res += [loss, losses, grad, torch.stack([v for row in mx for v in row])]
        return res

    got, ref = evaluations(_fresh()), evaluations(hip_denoiser(1234, 1.0))
    assert all(torch.isfinite(v).all() for v in got)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), k
