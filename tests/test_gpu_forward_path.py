"""Which forward a problem gets (csrc/forward_path.hpp: the row-tile or the tile kernels; the row-tile, the fused or the three-launch
cross-attention; the fused kernel's instance; layer 0's lists), seen from outside: the launches per class of ONE forward
(cfd_profile_forward) and, where a cfd_forward was the last call on the handle, "xa.info"'s instance and workgroup count.  Everything goes
through the public API and the two read-outs, at B = 2, L = 16, memories S = (6, 20, 6, 8, 1) with the seeded test weights.  The expected
figures are literals: what the library printed for each set-up before the path decision moved into one function -- a change of the host
code that decides the path must leave every one of them as it is.  (tests/host/forward_path_test.cpp checks the decision's arms on the
CPU; this file checks that the launches follow it.)"""
import ctypes as C

import pytest
import torch

from oracle import inputs

pytestmark = pytest.mark.gpu

B, L, S, PAD, SEED = 2, 16, (6, 20, 6, 8, 1), (2, 0, 1, 0, 0), 7
CLASSES = ("gemm_token", "gemm_attn", "xattn", "rows")
PAIR, ATT, F16, NONE = 0, 1, 2, -1
ROWTILE0 = {"CFD_ROWTILE": "0"}                                  # (tests/conftest.py lifts the work list's length gate: the fused kernel)
THREE_LAUNCH = {"CFD_ROWTILE": "0", "CFD_FUSED_XATTN": "0"}

# set-up -> (gemm_token, gemm_attn, xattn, rows) of one forward [, ("xa.info" instance, workgroups)]
EXPECT = {
    "run":                        ((56, 9, 18, 0),),
    "run rowtile=0":              ((56, 9, 9, 39),),
    "run three-launch":           ((56, 27, 0, 61),),
    "run att_ring":               ((56, 9, 18, 0),),
    "run att_ring rowtile=0":     ((56, 9, 9, 40),),
    "run dynamic (4,)":           ((56, 9, 9, 40),),
    "run f16 rowtile=0":          ((56, 9, 9, 39), (F16, 80)),
    "forward att":                ((56, 9, 18, 0), (NONE, 16)),
    "forward att rowtile=0":      ((56, 9, 9, 39), (ATT, 16)),
    "forward att three-launch":   ((56, 27, 0, 60), (NONE, 0)),
    "forward no att rowtile=0":   ((56, 9, 9, 38), (PAIR, 16)),
    "forward f16 rowtile=0":      ((56, 9, 9, 38), (F16, 16)),
    "level batch":                ((56, 9, 9, 42),),
}


@pytest.fixture(scope="module")
def data():
    from tests.gpu_helpers import to_dev
    cb = inputs.make_cfg_batch(seed=1, B=B, L=L, S=S, pad_tail=PAD)
    return [to_dev(x) for x in cb["memories"]], {k: to_dev(v) for k, v in cb["masks"].items()}


@pytest.fixture(scope="module")
def handles():
    """One Denoiser per set of developer knobs (read once at cfd_create), made on first use."""
    from tests.gpu_helpers import hip_denoiser
    from tests.test_gpu_sampler import _handle_with_env
    made = {}

    def get(env=None):
        key = tuple(sorted((env or {}).items()))
        if key not in made:
            made[key] = _handle_with_env(env) if env else hip_denoiser(1234, 1.0)
        return made[key]
    return get


def _ddpm():
    from convofusion_amd import scheduler
    from tests.gpu_helpers import SCHED_KW
    return scheduler.DDPMScheduler(variance_type="fixed_small", **SCHED_KW)


def _counts(prof):
    return tuple(prof[k][1] for k in CLASSES)


def _profile_handle(m):
    """cfd_profile_forward on a handle with no run open: the launches of the last problem's forward once more."""
    from convofusion_amd import _lib
    ms = (C.c_float * len(_lib.PROF_CLASSES))()
    n = (C.c_int * len(_lib.PROF_CLASSES))()
    _lib.check(_lib.load().cfd_profile_forward(m._handle, ms, n))
    return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_lib.PROF_CLASSES)}


def _xa_info(m):
    from tests.gpu_helpers import read_debug
    info = read_debug(m, "xa.info", (7,))
    return int(info[0]), int(info[1])


def _check(name, *got):
    print(f"{name}: {got}")
    assert got == EXPECT[name], (name, got, EXPECT[name])


def _run_counts(m, mems, masks, **kw):
    from convofusion_amd.sampler import SamplingRun
    with SamplingRun(m, _ddpm(), mems, masks, B, L, 4, seed=SEED, **kw) as run:
        run.steps(1)
        return _counts(run.profile())


@pytest.mark.parametrize("name,env,kw", [
    ("run", None, {}),
    ("run rowtile=0", ROWTILE0, {}),                       # fused kernel, one launch per layer (no memory of 256 keys: layer 0 gets no lists of its own)
    ("run three-launch", THREE_LAUNCH, {}),
    ("run att_ring", None, dict(attention_ring=True)),
    ("run att_ring rowtile=0", ROWTILE0, dict(attention_ring=True)),   # the ATT instance + att_fixup_kernel
    ("run dynamic (4,)", None, dict(dedup=False, dynamic_memories=(4,))),   # leaves the row-tile path: the fused kernel, memory 4 projected per step
])
def test_sampling_run_paths(data, handles, name, env, kw):
    mems, masks = data
    if "dynamic_memories" in kw:
        mems = [x.clone() for x in mems]
    _check(name, _run_counts(handles(env), mems, masks, **kw))


def _padded_audio(data):
    """The memories with the audio memory padded to 100 keys (128 padded: XA_F16_MIN_KEYS), the tail masked."""
    mems, masks = list(data[0]), dict(data[1])
    n = mems[1].shape[0]
    mems[1] = torch.cat([mems[1], torch.zeros((n, 100 - S[1], 512), device="cuda")], dim=1).contiguous()
    tail = torch.zeros((n, 100), dtype=torch.bool, device="cuda")
    tail[:, S[1]:] = True
    masks["alsn"] = tail
    return mems, masks


def test_operand_policy_takes_the_f16_instance(data, handles):
    """A long enough memory: an operand-policy-15 run on the tile kernels packs its single-fp16 tiles and launches the F16 instance --
    the launch counts of the pair instance's run; the instance shows in "xa.info" -- and so does a cfd_forward under
    cfd_debug_forward_operands(15)."""
    from convofusion_amd import _lib
    mems, masks = _padded_audio(data)
    m = handles(ROWTILE0)
    counts = _run_counts(m, mems, masks, operands=15)
    _check("run f16 rowtile=0", counts, _xa_info(m))
    _lib.check(_lib.load().cfd_debug_forward_operands(m._handle, 15))
    try:
        _forward_and_check("forward f16 rowtile=0", m, mems, masks, False)
    finally:
        _lib.check(_lib.load().cfd_debug_forward_operands(m._handle, 0))


@pytest.mark.parametrize("name,env,att", [
    ("forward att", None, True),
    ("forward att rowtile=0", ROWTILE0, True),
    ("forward att three-launch", THREE_LAUNCH, True),
    ("forward no att rowtile=0", ROWTILE0, False),
])
def test_cfd_forward_paths(data, handles, name, env, att):
    _forward_and_check(name, handles(env), data[0], data[1], att)


def _forward_and_check(name, m, mems, masks, att):
    x = torch.randn((7 * B, L, 128), generator=torch.Generator().manual_seed(12)).cuda()
    keep = m.return_attention
    m.return_attention = att
    try:
        with torch.no_grad():
            m(x, torch.tensor(500), mems, mem_mask_dict=masks)
    finally:
        m.return_attention = keep
    torch.cuda.synchronize()
    info = _xa_info(m)
    _check(name, _counts(_profile_handle(m)), info)


def test_level_batch_path(data, handles):
    """A level batch (invert_ddpm over two levels): the fused kernel on memory projections made per level inside the forward."""
    from convofusion_amd import sampler
    mems, masks = data
    m = handles(None)
    src = torch.randn((B, L, 128), generator=torch.Generator().manual_seed(11)).cuda()
    sampler.invert_ddpm(m, _ddpm(), mems, masks, source_latents=src, num_inference_steps=2, seed=SEED, levels_per_batch=2)
    _check("level batch", _counts(_profile_handle(m)))
