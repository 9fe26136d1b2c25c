#!/usr/bin/env python
"""Generate tests/golden/t5_enc.npz from transformers' ``T5EncoderModel`` (5.15, CPU; ``T5Config`` builds offline) and the reference's
projection ``Sequential(ReLU, Linear)`` (t5.py:48-49).

Per case of tests/t5_ref.py (A: 2 blocks, lengths 1, 2, 17, 33, 40 padded to 40; B: 1 block, one sequence of 200; C: 1 block, one token;
D: 1 block, 65 sequences padded to 32 = 2080 token rows; vocabulary 64) the module is loaded STRICTLY with ``t5_ref.make_state``'s seeded weights and run in float32 and in ``.double()`` (with
``t5_ref.keep_norm_dtype``: transformers' norm squares in float32 whatever the module's dtype).  Stored:

    <case>_ids, <case>_mask            the inputs (tests regenerate them from the seed and compare)
    <case>_out_f32                     the float32 forward's projected output [n, T, 512] (B: every 8th position, D: every 8th sequence and 4th
                                       position -- t5_ref.STORED --, to keep the file small)
    <case>_f32_ref_err_hidden / _proj  the float32 forward's max-abs distance from the float64 forward over the float64 output's RMS, every
                                       position counted, for the last hidden state and for the projected output: what the reference's own
                                       arithmetic loses, the base of the GPU tests' gate
    <case>_restatement_err             max-abs distance of tests/t5_ref.py's float64 restatement from ``.double()`` (hidden state)

Weights are not stored (a block is 7 M floats).  Usage:  python tests/golden/make_golden_t5.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import t5_ref  # noqa: E402

torch.set_grad_enabled(False)


def reference_modules(sd, num_layers):
    from transformers import T5Config, T5EncoderModel
    cfg = T5Config(vocab_size=t5_ref.VOCAB, d_model=t5_ref.D, d_kv=t5_ref.DKV, num_heads=t5_ref.H, d_ff=t5_ref.FF, num_layers=num_layers,
                   feed_forward_proj="relu", dropout_rate=0.0)
    model = T5EncoderModel(cfg).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("projection.")}, strict=True)
    return model, t5_ref.projection_module(sd)


def main():
    out = {}
    for name, (nl, seed, _, _) in t5_ref.CASES.items():
        sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)
        ids, mask = t5_ref.case_inputs(name)
        model, proj = reference_modules(sd, nl)
        kw = dict(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long())
        h32 = model(**kw).last_hidden_state
        p32 = proj(h32)
        model, proj = t5_ref.keep_norm_dtype(model.double()), proj.double()
        h64 = model(**kw).last_hidden_state
        p64 = proj(h64)
        mine = t5_ref.encode(sd, ids, mask)
        out[name + "_ids"], out[name + "_mask"] = ids, mask
        ss, ps = t5_ref.STORED[name]
        out[name + "_out_f32"] = p32.numpy()[::ss, ::ps]
        out[name + "_f32_ref_err_hidden"] = np.float64(t5_ref.rel_err(h32.numpy(), h64.numpy()))
        out[name + "_f32_ref_err_proj"] = np.float64(t5_ref.rel_err(p32.numpy(), p64.numpy()))
        out[name + "_restatement_err"] = np.float64(np.abs(mine - h64.numpy()).max())
        print(name, "f32_ref_err hidden %.3e proj %.3e, restatement %.2e" % (out[name + "_f32_ref_err_hidden"], out[name + "_f32_ref_err_proj"],
                                                                            out[name + "_restatement_err"]))
    path = os.path.join(HERE, "t5_enc.npz")
    np.savez_compressed(path, **out)
    print("wrote t5_enc.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
