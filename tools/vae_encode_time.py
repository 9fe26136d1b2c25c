"""Developer tool (GPU box): ConvoFusionVae.encode -- the fused one-launch kernel (cfd_vae_encode) against a float32 torch-eager
restatement on the GPU (standing in for the reference module) and the same encode composed from the decode's building blocks
(cfd_linear_act / cfd_layer_norm / cfd_mha / cfd_add), at (B, frames) = (32, 128), (8, 128), (1, 128), seeded weights and features,
ragged lengths.  Plus the sequences-per-workgroup sweep of the fused kernel (seqs_per_group 1 - 3, and 0 = the automatic choice).

Times are device times per encode from CUDA events around REPS back-to-back calls after WARM warm-up calls (median of 5 such
batches).  The fused "encode" time includes torch's std / rsample; "kernel" is the raw cfd_vae_encode call.

Usage:  python tools/vae_encode_time.py [OUT.json]      (default profiles/r07_vae_encode_time.json)
        python tools/vae_encode_time.py --one            (10 fused encodes at (32, 128): the subject of a kernel-trace run)
"""
import ctypes as C
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from convofusion_amd import _lib  # noqa: E402
from convofusion_amd.conditioning import ACT_GELU, _engine_handle, linear_act  # noqa: E402
from convofusion_amd.vae import ConvoFusionVae, add_, layer_norm, mha  # noqa: E402
from oracle import vae_weights  # noqa: E402

SHAPES = [(32, 128), (8, 128), (1, 128)]
REPS, WARM = 20, 3
KW = dict(nfeats=189, latent_dim=[1, 128], ff_size=1024, num_layers=5, num_heads=2, dropout=0.1, arch="encoder_decoder",
          normalize_before=True, activation="gelu", position_embedding="sine")


def model(dev):
    m = ConvoFusionVae(ablation=SimpleNamespace(MLP_DIST=False, PE_TYPE="convofusion"), **KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    return m.to(dev).eval()


def inputs(bs, nframes, dev):
    rng = np.random.Generator(np.random.PCG64(bs))
    f = torch.from_numpy(rng.standard_normal((bs, nframes, 189), dtype=np.float32)).to(dev)
    lens = [nframes] + [int(v) for v in rng.integers(16, nframes + 1, bs - 1)]
    return f, lens


def _prep(m, f, lens):
    """chunking, root subtraction, tokens, PE and key-padding mask (vae.py:162-233) in torch: [18, n, 128] per stack + mask"""
    bs, nframes, nf = f.shape
    n = bs * (nframes // 16)
    x = f.clone().reshape(n, 16, nf)
    x[:, :, :3] = x[:, :, :3] - x[:, :1, :3] * torch.tensor([1, 0, 1], device=f.device)
    valid = (torch.arange(nframes, device=f.device)[None] < torch.tensor(lens, device=f.device)[:, None]).reshape(n, 16)
    kpm = ~torch.cat([torch.ones(n, 2, dtype=torch.bool, device=f.device), valid], 1)
    return x, kpm, n


def eager_encode(m, f, lens):
    """float32 torch eager (nn modules' own forward): the reference module's arithmetic on the GPU."""
    x, kpm, n = _prep(m, f, lens)
    pe = m.query_pos_encoder.pe[:18]
    outs = []
    for enc, emb, tok, cols in ((m.body_encoder, m.body_skel_embedding, m.body_global_motion_token, slice(0, 69)),
                                (m.hands_encoder, m.hands_skel_embedding, m.hands_global_motion_token, slice(69, 189))):
        s = torch.cat([tok[:, None].expand(2, n, 128), emb(x[:, :, cols]).permute(1, 0, 2)], 0) + pe

        def layer(blk, s):
            t = blk.norm1(s)
            s = s + blk.self_attn(t, t, t, key_padding_mask=kpm, need_weights=False)[0]
            return s + blk.linear2(F.gelu(blk.linear1(blk.norm2(s))))
        xs = []
        for blk in enc.input_blocks:
            s = layer(blk, s)
            xs.append(s)
        s = layer(enc.middle_block, s)
        for blk, lin in zip(enc.output_blocks, enc.linear_blocks):
            s = layer(blk, lin(torch.cat([s, xs.pop()], -1)))
        outs.append(enc.norm(s)[:2])
    return outs


def blocks_encode(m, f, lens):
    """the same encode composed from the decode's HIP building blocks (one launch per linear / norm / attention / residual)."""
    x, kpm, n = _prep(m, f, lens)
    pe = m.query_pos_encoder.pe[:18].expand(18, n, 128).contiguous()
    outs = []
    for enc, emb, tok, cols in ((m.body_encoder, m.body_skel_embedding, m.body_global_motion_token, slice(0, 69)),
                                (m.hands_encoder, m.hands_skel_embedding, m.hands_global_motion_token, slice(69, 189))):
        e = linear_act(x[:, :, cols].contiguous(), emb.weight, emb.bias).permute(1, 0, 2)
        s = torch.cat([tok.detach()[:, None].expand(2, n, 128), e], 0).contiguous()
        add_(s, pe)

        def layer(blk, s):
            t = layer_norm(s, blk.norm1)
            add_(s, mha(blk.self_attn, t, t, t, kpm))
            h = linear_act(layer_norm(s, blk.norm2), blk.linear1.weight, blk.linear1.bias, ACT_GELU)
            add_(s, linear_act(h, blk.linear2.weight, blk.linear2.bias))
            return s
        xs = []
        for blk in enc.input_blocks:
            s = layer(blk, s)
            xs.append(s.clone())
        s = layer(enc.middle_block, s)
        for blk, lin in zip(enc.output_blocks, enc.linear_blocks):
            s = layer(blk, linear_act(torch.cat([s, xs.pop()], -1), lin.weight, lin.bias))
        outs.append(layer_norm(s, enc.norm)[:2])
    return outs


def kernel_call(m, f, lens, spg):
    """the raw cfd_vae_encode launch with seqs_per_group = spg (0 = automatic)"""
    dev = f.device
    bs, nframes, _ = f.shape
    pack = m._encoder_pack(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    mulv = torch.empty(2, 2, bs * nframes // 16, 128, device=dev)
    feats = torch.empty_like(f)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def go():
        _lib.check(_lib.load().cfd_vae_encode(_engine_handle(dev), C.c_void_p(pack.data_ptr()), 128, 2, 1024, 5, 1,
                                              C.c_void_p(f.data_ptr()), bs, nframes, 189, C.c_void_p(lens_d.data_ptr()),
                                              C.c_void_p(mulv.data_ptr()), C.c_void_p(feats.data_ptr()), spg, st))
    return go, mulv


def time_ms(fn):
    with torch.no_grad():
        for _ in range(WARM):
            fn()
        meds = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                fn()
            b.record()
            b.synchronize()
            meds.append(a.elapsed_time(b) / REPS)
    return statistics.median(meds)


def main():
    dev = torch.device("cuda", 0)
    m = model(dev)
    if "--one" in sys.argv:
        f, lens = inputs(32, 128, dev)
        for _ in range(10):
            m.encode(f, lens)
        torch.cuda.synchronize()
        print("10 encodes at (32, 128) done")
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_vae_encode_time.json")
    res = {"device": torch.cuda.get_device_name(dev), "reps": REPS, "warmup": WARM, "unit": "ms per encode (device time, CUDA events)",
           "shapes": {}}
    for bs, nframes in SHAPES:
        f, lens = inputs(bs, nframes, dev)
        with torch.no_grad():
            ref = eager_encode(m, f, lens)
            _, dist, _ = m.encode(f, lens)
            blk = blocks_encode(m, f, lens)
        got = [torch.stack([dist.mean[i], (2 * dist.stddev[i].log())]) for i in range(2)]   # per stack [mu, logvar]
        err_fused = max(float((g - r).abs().max()) for g, r in zip(got, ref))
        err_blocks = max(float((g - r).abs().max()) for g, r in zip(blk, ref))
        row = {"lengths": lens, "sequences_per_stack": bs * nframes // 16,
               "fused_encode_ms": time_ms(lambda: m.encode(f, lens)),
               "torch_eager_f32_ms": time_ms(lambda: eager_encode(m, f, lens)),
               "hip_blocks_ms": time_ms(lambda: blocks_encode(m, f, lens)),
               "max_abs_vs_eager": {"fused": err_fused, "blocks": err_blocks}, "kernel_ms_by_seqs_per_group": {}}
        for spg in (0, 1, 2, 3):
            go, _ = kernel_call(m, f, lens, spg)
            row["kernel_ms_by_seqs_per_group"][str(spg) if spg else "auto"] = time_ms(go)
        res["shapes"][f"{bs}x{nframes}"] = row
        print(f"({bs}, {nframes}):", json.dumps(row))
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
