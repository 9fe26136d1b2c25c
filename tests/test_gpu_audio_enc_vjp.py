"""-m gpu: ``cfd_audio_encoder_vjp`` -- AudioConvEncoder's backward pass in HIP -- against the float64 numpy restatement
(tests/audio_enc_vjp_ref.py, itself held to torch autograd by tests/test_audio_enc_vjp_host.py) and a golden of the reference class.

The gate, per output tensor: relative L2 against float64 at most ``GATE`` = 4 times what the float32 run of the same restatement loses on
the same inputs, computed here (the project's rule for its float32 units).  Seeded weights (nn.Linear's default init) and Mel-dB-like rows.

Cases (widths 80 / 256 / 512 unless stated): 1, 3, 33 (one past a 32-row chunk), 322 (two product-length clips) and 545 rows (two row
segments, the second one chunk and one row long: the closing pass); widths 5 / 7 / 9 at 4 rows (tile edges in every dimension); one
all-zero row with all-zero biases (every pre-activation exactly 0: slope 0.1).

Measured on MI355X, HIP vs float64 | float32 restatement vs float64 (worst tensor of the case): profiles/audio_enc_vjp_gate.txt.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import audio_enc_vjp_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("out", "d_x") + R.KEYS
#        rows, (in, hidden, latent), zero
CASES = {"r1": (1, (80, 256, 512), False), "r3": (3, (80, 256, 512), False), "r33": (33, (80, 256, 512), False),
         "r322": (322, (80, 256, 512), False), "r545": (545, (80, 256, 512), False), "odd": (4, (5, 7, 9), False),
         "zero": (1, (80, 256, 512), True)}
LAUNCHES_ALL = {"r33": 7, "r545": 8}        # include/cfdenoise.h: 3 forward + dz2 + dz1 + d_x + 1 for the parameters (+ 1 closing pass beyond 512 rows)


@functools.lru_cache(maxsize=None)
def case(name):
    """(params, x, d_out) of a case on the host: float32, computed once and shared (callers do not write)"""
    rows, widths, zero = CASES[name]
    params = R.seeded_params(*widths, seed=21, zero_bias=zero)
    x, d = R.seeded_inputs(rows, widths[0], widths[2], seed=22 + rows)
    if zero:
        x[:] = 0.0
    return params, x, d


def encoder_of(params):
    import torch
    from convofusion_amd.conditioning import AudioConvEncoder
    hidden, in_dim = params[R.KEYS[0]].shape
    enc = AudioConvEncoder(in_dim, hidden, params[R.KEYS[4]].shape[0])
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return enc.cuda().eval()


@functools.lru_cache(maxsize=None)
def encoder(name):
    return encoder_of(case(name)[0])


def info():
    from convofusion_amd.conditioning import audio_enc_vjp_info
    return audio_enc_vjp_info("cuda")


def call(name, want=R.KEYS, want_dx=True, want_out=True):
    """{name: tensor} of one call on the case"""
    import torch
    from convofusion_amd.conditioning import audio_encoder_vjp
    from tests.gpu_helpers import to_dev
    _, x, d = case(name)
    out = torch.empty(d.shape, dtype=torch.float32, device="cuda") if want_out else None
    grads, d_x = audio_encoder_vjp(encoder(name), to_dev(x), to_dev(d), want=want, want_dx=want_dx, out=out)
    r = dict(grads)
    if want_dx:
        r["d_x"] = d_x
    if want_out:
        r["out"] = out
    torch.cuda.synchronize()
    return r


@functools.lru_cache(maxsize=None)
def full(name):
    """The all-outputs call of a case, run once and shared"""
    return call(name)


def assert_inside_the_gate(got, params, x, d, names, what):
    bad = []
    for n, e, e32 in R.gate_report({k: v.cpu().numpy() for k, v in got.items()}, x, params, d, names):
        print(f"{what}: {n:15s} HIP vs float64 {e:.2e} | float32 restatement {e32:.2e} | ratio {e / e32 if e32 else 0.0:.2f}")
        if not e <= R.GATE * e32:
            bad.append((n, e, e32))
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_is_inside_the_float32_gate(name):
    params, x, d = case(name)
    got = full(name)
    assert sorted(got) == sorted(NAMES)
    assert_inside_the_gate(got, params, x, d, NAMES, name)
    if name == "zero":
        # dz = 0.1 (d W) at both activations: the input's gradient is 0.01 d_out W2 W1 W0 and all three weight gradients vanish.  1e-5 of
        # the vector's norm: three float32 chains of at most 512 terms lose about 3 sqrt(512) 6e-8 = 4e-6; a slope of 1 would miss by 10 or 100
        w0, w1, w2 = (params[k].astype(np.float64) for k in R.KEYS[0::2])
        assert R.rel_l2(got["d_x"].cpu().numpy()[0], 0.01 * (d[0].astype(np.float64) @ w2 @ w1 @ w0)) < 1e-5
        assert not got["main.0.weight"].any() and not got["main.3.weight"].any() and not got["out_net.weight"].any()


@pytest.mark.parametrize("name", ["r33", "r545"])
def test_a_subset_call_and_a_second_call_give_the_full_calls_bits(name):
    import torch
    want = full(name)
    again = call(name)
    for k in NAMES:
        assert torch.equal(again[k], want[k]), k
    only_w2 = call(name, want=("out_net.weight",), want_dx=False, want_out=False)
    assert list(only_w2) == ["out_net.weight"] and torch.equal(only_w2["out_net.weight"], want["out_net.weight"])
    assert info()[0] == 3 + (name == "r545")                  # h1, h2, the parameter launch (+ the closing pass)
    only_dx = call(name, want=(), want_dx=True, want_out=False)
    assert list(only_dx) == ["d_x"] and torch.equal(only_dx["d_x"], want["d_x"])
    assert info()[0] == 5                                     # h1, h2, dz2, dz1, d_x
    only_b0 = call(name, want=("main.0.bias",), want_dx=False, want_out=False)      # a bias without its weight: the k-tile 0 workgroups alone
    assert torch.equal(only_b0["main.0.bias"], want["main.0.bias"])


@pytest.mark.parametrize("name", ["r33", "r322", "odd"])
def test_out_is_the_three_launch_forward(name):
    import torch
    from tests.gpu_helpers import to_dev
    with torch.no_grad():
        plain = encoder(name)(to_dev(case(name)[1]))
    assert torch.equal(full(name)["out"], plain)


@pytest.mark.parametrize("name", list(LAUNCHES_ALL))
def test_the_launch_count_is_the_documented_one(name):
    call(name)
    launches, rows, segments, ws = info()
    assert launches == LAUNCHES_ALL[name] <= 9
    assert rows == CASES[name][0] and segments == (2 if name == "r545" else 1) and ws > 0


def test_bits_do_not_depend_on_the_workspace():
    from tests.test_gpu_workspace_growth import _on_a_fresh_engine_handle
    _on_a_fresh_engine_handle(lambda: [call("r3")[k] for k in NAMES], lambda: call("r545"), lambda: info()[3])


def _raw(enc_args=None, d_out=True, out=True, d_param=True, d_x=True):
    """One raw call with valid pointers for r3's shapes except where overridden; returns the CfdError"""
    import torch
    from convofusion_amd import _lib, conditioning
    rows, (i, h, l) = 3, CASES["r3"][1]
    bufs = {n: torch.zeros(s, device="cuda") for n, s in dict(x=rows * i, w0=h * i, b0=h, w1=l * h, b1=l, w2=l * l, b2=l, d=rows * l, out=rows * l,
                                                              dx=rows * i).items()}
    a = dict(x=bufs["x"].data_ptr(), n_rows=rows, in_dim=i, hidden=h, latent=l, **{k: bufs[k].data_ptr() for k in ("w0", "b0", "w1", "b1", "w2", "b2")})
    a.update(enc_args or {})
    args = _lib.AudioEncArgs(**a)
    grads = [torch.zeros(n, device="cuda") for n in (h * i, h, l * h, l, l * l, l)]
    dp = (C.c_void_p * 6)(*[g.data_ptr() if d_param else None for g in grads])
    with pytest.raises(_lib.CfdError) as e:
        _lib.check(_lib.load().cfd_audio_encoder_vjp(conditioning._engine_handle(torch.device("cuda")), C.byref(args),
                                                     C.c_void_p(bufs["d"].data_ptr()) if d_out else None, C.c_void_p(bufs["out"].data_ptr()) if out else None,
                                                     dp, C.c_void_p(bufs["dx"].data_ptr()) if d_x else None, None))
    assert info()[0] == 0                      # refused before any launch
    return e.value


def test_every_refusal_by_code_and_message():
    ARG, SHAPE = -1, -2
    e = _raw(out=False, d_param=False, d_x=False)
    assert e.code == ARG and "nothing is wanted" in str(e)
    e = _raw({"n_rows": 0})
    assert e.code == SHAPE and "1 <= n_rows <= 2097120 (got 0)" in str(e)
    e = _raw({"n_rows": 65535 * 32 + 1})
    assert e.code == SHAPE and "1 <= n_rows <= 2097120" in str(e)
    for field, v in (("in_dim", 0), ("hidden", 1025), ("latent", 1025), ("latent", 0)):
        e = _raw({field: v})
        assert e.code == SHAPE and "1 <= in_dim, hidden, latent <= 1024" in str(e) and str(v) in str(e), field
    for field in ("x", "w0", "b0", "w1", "b1", "w2", "b2"):
        e = _raw({field: None})
        assert e.code == ARG and "NULL pointer" in str(e), field
    e = _raw(d_out=False)
    assert e.code == ARG and "d_out" in str(e)


def test_golden_of_the_reference_class():
    """tests/golden/audio_enc_vjp.npz (make_golden_audio_enc_vjp.py): float64 autograd through the reference's AudioConvEncoder in eval
    mode at 2 x 5 rows, widths 80 / 48 / 40.  The HIP result sits inside the same gate, with the golden as the float64 side."""
    import os
    import torch
    from convofusion_amd.conditioning import audio_encoder_vjp
    from tests.gpu_helpers import to_dev
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "audio_enc_vjp.npz"))
    params = {k: g["param." + k] for k in R.KEYS}
    enc = encoder_of(params)
    mel, d = g["mel"], g["d_out"]
    out = torch.empty(d.shape, dtype=torch.float32, device="cuda")
    grads, d_x = audio_encoder_vjp(enc, to_dev(mel), to_dev(d), want_dx=True, out=out)
    got = {**{k: v.cpu().numpy() for k, v in grads.items()}, "d_x": d_x.cpu().numpy(), "out": out.cpu().numpy()}
    want = {**{k: g["grad." + k] for k in R.KEYS}, "d_x": g["grad.d_x"], "out": g["out"]}
    f32 = R.encoder_vjp(mel.reshape(10, -1), params, d.reshape(10, -1), np.float32)
    bad = []
    for n in NAMES:
        e, e32 = R.rel_l2(got[n].reshape(want[n].shape), want[n]), R.rel_l2(f32[n].reshape(want[n].shape), want[n])
        print(f"golden: {n:15s} HIP vs the reference's float64 {e:.2e} | float32 restatement {e32:.2e}")
        if not e <= R.GATE * e32:
            bad.append((n, e, e32))
    assert not bad, bad


def test_autograd_leg():
    """``enc(mel, weight_grad=True)``: the plain forward's bits; ``.backward(d)`` fills ``.grad`` with the direct call's bits (and the
    input's, where it requires grad); without the keyword the output does not require grad."""
    import torch
    from tests.gpu_helpers import to_dev
    params, x, d = case("r33")
    enc = encoder_of(params)
    mel = to_dev(x).reshape(1, 33, -1)
    plain = enc(mel)
    assert not plain.requires_grad and plain.grad_fn is None
    y = enc(mel, weight_grad=True)
    assert y.requires_grad and torch.equal(y.detach(), plain)
    y.backward(to_dev(d).reshape(1, 33, -1))
    want = full("r33")
    for k, p in zip(R.KEYS, (enc.main[0].weight, enc.main[0].bias, enc.main[3].weight, enc.main[3].bias, enc.out_net.weight, enc.out_net.bias)):
        assert torch.equal(p.grad, want[k]), k
    assert info()[0] == 5                                       # h1, h2, dz2, dz1, the parameter launch: no out, no d_x
    for p in enc.parameters():
        p.grad = None
    enc.main[0].weight.requires_grad_(False)
    mel_g = mel.clone().requires_grad_(True)
    enc(mel_g, weight_grad=True).backward(to_dev(d).reshape(1, 33, -1))
    assert enc.main[0].weight.grad is None and torch.equal(mel_g.grad.reshape(33, -1), want["d_x"])
    assert torch.equal(enc.out_net.bias.grad, want["out_net.bias"])
    with torch.no_grad():
        assert not enc(mel, weight_grad=True).requires_grad
