"""Host side of the attention-concentration census (cfd_sample_census, cfd_sample_args.census_tau) and of ``operands="auto"``: struct
layouts against the header and the validation of the operand argument.  No GPU needed."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_struct(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cfdenoise.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r";", hdr).group(1)
    return [re.match(r"\s*(?:const\s+)?([\w\s\*]+?)\s*\**\s*(\w+)(\[\w+\])?\s*$", d).groups() for d in body.split(";") if d.strip()]


def test_census_struct_matches_header():
    from convofusion_amd import _lib
    fields = _header_struct("cfd_census")
    assert [f[1] for f in fields] == [f[0] for f in _lib.Census._fields_]
    kinds = {"float": C.c_float, "int": C.c_int, "uint32_t": C.c_uint32}
    for (ctype, name, arr), (pname, ptype) in zip(fields, _lib.Census._fields_):
        want = kinds[ctype.strip()]
        if arr:
            assert arr == "[CFD_CENSUS_MAX_LAYERS]" and ptype._type_ is want and ptype._length_ == _lib.CENSUS_MAX_LAYERS, name
        else:
            assert ptype is want, name
    assert re.search(r"#define CFD_CENSUS_MAX_LAYERS %d\b" % _lib.CENSUS_MAX_LAYERS, open(os.path.join(ROOT, "include", "cfdenoise.h")).read())
    assert C.sizeof(_lib.Census) == 7 * 4 + 2 * _lib.CENSUS_MAX_LAYERS * 4
    assert _lib.Census.layer_peak.offset == 28 and _lib.Census.layer_over.offset == 28 + 4 * _lib.CENSUS_MAX_LAYERS


def test_census_tau_sits_in_the_former_tail_padding():
    from convofusion_amd import _lib
    assert [f[1] for f in _header_struct("cfd_sample_args")][-2:] == ["operand_policy", "census_tau"]
    assert _lib.SampleArgs._fields_[-1] == ("census_tau", C.c_float)
    assert _lib.SampleArgs.census_tau.offset == _lib.SampleArgs.operand_policy.offset + 4
    # the struct's size is what it was with operand_policy as its last field: int + 4 bytes of padding to the 8-byte alignment
    assert C.sizeof(_lib.SampleArgs) == _lib.SampleArgs.operand_policy.offset + 8
    assert _lib.SampleArgs().census_tau == 0.0        # ctypes zero-initialises it: the census is off for every existing caller
    assert "cfd_sample_census" in _lib.SYMBOLS


def test_operands_values():
    from convofusion_amd.sampler import check_operands
    assert check_operands(None) is None and check_operands("auto") == "auto"
    assert check_operands(0) == 0 and check_operands(15) == 15
    for bad in ("fast", "AUTO", "15", "", b"auto", True, [15], 1j):
        with pytest.raises(ValueError):
            check_operands(bad)


class _NotADenoiser:
    num_layers = 9


def _loop_model(operands):
    sched = SimpleNamespace(KIND=0, init_noise_sigma=1.0, set_timesteps=lambda n: None, step=lambda model_output, timestep, sample: None)
    return SimpleNamespace(do_classifier_free_guidance=True, clf_guidance_drops=6, latent_dim=[1, 128], scheduler=sched,
                           cfg=SimpleNamespace(model=SimpleNamespace(scheduler=SimpleNamespace(num_inference_timesteps=4))),
                           guidance_scale=7.5, denoiser=_NotADenoiser(), _cfd_operands=operands)


def test_auto_is_accepted_and_bad_values_are_refused_by_the_entry_points():
    """"auto" passes the validation of sample / _loop_from_model / install (and the call then fails where it needs the GPU / a real denoiser:
    TypeError); a bad value is refused first (ValueError)."""
    import torch
    from convofusion_amd import installer, sampler
    mems = [torch.zeros(7, 4, 512) for _ in range(5)]
    for ops, exc in (("auto", TypeError), (15, TypeError), (None, TypeError), ("fast", ValueError), (2.5j, ValueError)):
        with pytest.raises(exc):
            sampler.sample(_NotADenoiser(), SimpleNamespace(KIND=0), mems, None, B=1, L=16, num_inference_steps=4, operands=ops)
        with pytest.raises(exc):
            sampler._loop_from_model(_loop_model(None), mems, None, None, [], torch.zeros(1, 16, 128), 3, operands=ops)
        with pytest.raises(exc):
            installer.install(SimpleNamespace(denoiser=None), operands=ops)
    with pytest.raises(ValueError):    # install(model, operands="auto") stored on the model, then a bad value there is refused too
        sampler._loop_from_model(_loop_model("fast"), mems, None, None, [], torch.zeros(1, 16, 128), 3)
