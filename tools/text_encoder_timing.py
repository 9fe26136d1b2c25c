"""Developer tool (GPU box): the T5 text encoder -- cfd_t5_encode (csrc/t5_enc.hpp) against a float32 torch-eager statement of the same
operations on the same device, in one session: transformers' ``T5EncoderModel`` + the reference's projection where transformers imports,
otherwise an ``F.linear`` / ``softmax`` sequence of our own.

12 seeded blocks (tests/t5_ref.make_state), sequences padded to 32 tokens (every position a token: the arithmetic does not depend on the
mask).  Shapes: 3, 31 and 65 distinct sequences -- one utterance, 15 long-form windows, 32 utterances after de-duplication -- and the
14 B replicated batches the reference encodes for B = 1 and B = 32 (14 and 448 sequences), to show what de-duplication alone is worth.

Per shape and path: WINDOWS timed windows of INNER back-to-back calls between two device events behind WARM untimed calls; reported are
the median, minimum and maximum of the windows' per-call times.  From shapes: the FLOPs of the call (products, attention, projection) and
the bytes of weights it streams; achieved TFLOP/s is FLOPs over the median against the 157.3 TFLOP/s peak of v_mfma_f32_32x32x2_f32.  The
HIP output is compared with the eager one at every timed shape (max-abs over RMS).  The HIP time is the library call's alone (packed
weights, bias table and argument struct made beforehand); the eager time includes transformers' Python path.  The mirror's own host work
per call (the pack key over the parameters, the id checks, the id / mask copies) is in neither: not measured.

Usage:  python tools/text_encoder_timing.py [OUT.json]      (default profiles/text_encoder_timing.json)
"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from convofusion_amd import _lib, text  # noqa: E402
from convofusion_amd.conditioning import _engine_handle  # noqa: E402
from tests import t5_ref  # noqa: E402

LAYERS, T, VOCAB = 12, 32, 64
SHAPES = [("1 utterance, distinct", 3), ("15 windows, distinct", 31), ("32 utterances, distinct", 65), ("1 utterance, 14 B replicated", 14),
          ("32 utterances, 14 B replicated", 448)]
WARM, WINDOWS = 3, 7
PEAK_TFLOPS = 157.3


def flops(n_seq):
    rows = n_seq * T
    per_block = 2 * rows * (768 * 2304 + 768 * 768 + 2 * 768 * 3072) + 2 * 2 * n_seq * 12 * T * T * 64
    return LAYERS * per_block + 2 * rows * 768 * 512


def eager_forward(sd_dev, ids):
    """our own float32 eager statement (used when transformers does not import): the operations of tests/t5_ref.py in torch"""
    n, t = ids.shape
    x = sd_dev["shared.weight"][ids]
    pos = torch.arange(t)
    bias = sd_dev["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][text.relative_bucket(pos[None, :] - pos[:, None]).to(x.device)]
    bias = bias.permute(2, 0, 1)[None]
    rms = lambda y, g: y * torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + 1e-6) * g
    for l in range(LAYERS):
        p = f"encoder.block.{l}.layer."
        nx = rms(x, sd_dev[p + "0.layer_norm.weight"])
        q, k, v = (F.linear(nx, sd_dev[p + f"0.SelfAttention.{m}.weight"]).view(n, t, 12, 64).transpose(1, 2) for m in "qkv")
        pr = torch.softmax(q @ k.transpose(-1, -2) + bias, -1)
        x = x + F.linear((pr @ v).transpose(1, 2).reshape(n, t, 768), sd_dev[p + "0.SelfAttention.o.weight"])
        x = x + F.linear(F.relu(F.linear(rms(x, sd_dev[p + "1.layer_norm.weight"]), sd_dev[p + "1.DenseReluDense.wi.weight"])),
                         sd_dev[p + "1.DenseReluDense.wo.weight"])
    out = rms(x, sd_dev["encoder.final_layer_norm.weight"])
    return F.linear(F.relu(out), sd_dev["projection.1.weight"], sd_dev["projection.1.bias"])


def timed(fn, inner):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) / inner)
    return {"median_ms": statistics.median(per_call), "min_ms": min(per_call), "max_ms": max(per_call), "calls_per_window": inner, "windows": WINDOWS}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "text_encoder_timing.json")
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    sd = t5_ref.make_state(LAYERS, 21, VOCAB)
    enc = text.T5TextEncoder.from_parts(t5_ref.stub_text_model(sd), None, t5_ref.projection_module(sd)).to(dev).eval()
    baseline = "transformers T5EncoderModel + projection, float32 eager"
    try:
        from transformers import T5Config, T5EncoderModel
        hf = T5EncoderModel(T5Config(vocab_size=VOCAB, d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=LAYERS, feed_forward_proj="relu",
                                     dropout_rate=0.0))
        hf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("projection.")}, strict=True)
        hf = hf.to(dev).eval()
        proj = t5_ref.projection_module(sd).to(dev).eval()
        eager = lambda ids, mask: proj(hf(input_ids=ids, attention_mask=mask).last_hidden_state)
    except ImportError:
        baseline = "F.linear / softmax sequence of tools/text_encoder_timing.py, float32 eager"
        sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}
        eager = lambda ids, mask: eager_forward(sd_dev, ids)

    lib, handle = _lib.load(), _engine_handle(dev)
    _, pack, _ = enc._packed()
    bias = enc._rel_bias(T)
    pw, pb = enc.projection[1].weight.detach().contiguous(), enc.projection[1].bias.detach().contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    results = {"device": torch.cuda.get_device_name(0), "layers": LAYERS, "T": T, "baseline": baseline, "peak_tflops_f32_mfma": PEAK_TFLOPS,
               "weight_bytes_streamed": LAYERS * text.block_floats() * 4, "shapes": []}
    for label, n_seq in SHAPES:
        rng = np.random.RandomState(n_seq)
        ids = torch.from_numpy(rng.randint(1, VOCAB, size=(n_seq, T))).to(dev)
        mask = torch.ones(n_seq, T, dtype=torch.long, device=dev)
        ids32, mask8 = ids.to(torch.int32).contiguous(), mask.to(torch.uint8).contiguous()
        out = torch.empty(n_seq, T, 512, device=dev)
        a = _lib.T5Args(wpack=pack.data_ptr(), vocab=VOCAB, d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=LAYERS, gated_act=0, eps=1e-6,
                        n_seq=n_seq, T=T, ids=ids32.data_ptr(), mask=mask8.data_ptr(), rel_bias=bias.data_ptr(), proj_w=pw.data_ptr(),
                        proj_b=pb.data_ptr(), proj_dim=512)

        def hip_call():
            _lib.check(lib.cfd_t5_encode(handle, C.byref(a), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        inner = 10 if n_seq <= 65 else 3
        hip = timed(hip_call, inner)
        info = torch.zeros(4, device=dev)
        _lib.check(lib.cfd_debug_read(handle, b"t5.info", C.c_void_p(info.data_ptr()), 4))
        ref = timed(lambda: eager(ids, mask), inner)
        want = eager(ids, mask).double()
        diff = float((out.double() - want).abs().max() / want.pow(2).mean().sqrt())
        fl = flops(n_seq)
        row = {"shape": label, "n_seq": n_seq, "token_rows": n_seq * T, "gflop": fl / 1e9, "hip": hip, "eager": ref, "launches": int(info[0].item()), "launches_128x128": int(info[3].item()),
               "workspace_bytes": int(info[2].item()), "hip_tflops": fl / hip["median_ms"] / 1e9, "hip_share_of_peak": fl / hip["median_ms"] / 1e9 / PEAK_TFLOPS,
               "eager_tflops": fl / ref["median_ms"] / 1e9, "weight_stream_GBps_hip": results["weight_bytes_streamed"] / hip["median_ms"] / 1e6,
               "eager_over_hip": ref["median_ms"] / hip["median_ms"], "hip_vs_eager_max_abs_over_rms": diff}
        results["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
