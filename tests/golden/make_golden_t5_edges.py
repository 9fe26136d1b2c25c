#!/usr/bin/env python
"""Generate tests/golden/t5_edges.npz from transformers' ``T5EncoderModel`` (5.15, CPU; ``T5Config`` builds offline) and the reference's
projection, with the conventions of make_golden_t5.py: the module is loaded STRICTLY with ``t5_ref.make_state``'s seeded weights and run in
float32 and in ``.double()`` with ``t5_ref.keep_norm_dtype``.

The cases are t5_ref.EDGE_CASES (vocabulary 64): L12 -- 12 blocks, lengths 9 and 4 at T = 9; T256 -- 1 block, lengths 256 and 193 at
T = 256; H -- 1 block, the three masks with holes of t5_ref.hole_masks at T = 129 (``attention_mask`` takes any pattern).  Stored per case:

    <case>_ids, <case>_mask            the inputs (tests regenerate them from the seed and compare)
    <case>_out_f32                     the float32 forward's projected output, every t5_ref.EDGE_STORED[case]-th position
    <case>_f32_ref_err_hidden / _proj  the float32 forward's max-abs distance from the float64 forward over the float64 output's RMS, every
                                       position counted: the base of the end-to-end gates of tests/test_gpu_t5_edges.py
    <case>_restatement_err             max-abs distance of tests/t5_ref.py's float64 restatement from ``.double()`` (hidden state)

No weights.  Usage:  python tests/golden/make_golden_t5_edges.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import t5_ref  # noqa: E402
from tests.golden.make_golden_t5 import reference_modules  # noqa: E402

torch.set_grad_enabled(False)


def main():
    out = {}
    for name, (nl, seed, _, _) in t5_ref.EDGE_CASES.items():
        sd = t5_ref.make_state(nl, seed, t5_ref.VOCAB)
        ids, mask = t5_ref.edge_inputs(name)
        model, proj = reference_modules(sd, nl)
        kw = dict(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long())
        h32 = model(**kw).last_hidden_state
        p32 = proj(h32)
        model, proj = t5_ref.keep_norm_dtype(model.double()), proj.double()
        h64 = model(**kw).last_hidden_state
        p64 = proj(h64)
        mine = t5_ref.encode(sd, ids, mask)
        out[name + "_ids"], out[name + "_mask"] = ids, mask
        out[name + "_out_f32"] = p32.numpy()[:, ::t5_ref.EDGE_STORED[name]]
        out[name + "_f32_ref_err_hidden"] = np.float64(t5_ref.rel_err(h32.numpy(), h64.numpy()))
        out[name + "_f32_ref_err_proj"] = np.float64(t5_ref.rel_err(p32.numpy(), p64.numpy()))
        out[name + "_restatement_err"] = np.float64(np.abs(mine - h64.numpy()).max())
        print(name, "f32_ref_err hidden %.3e proj %.3e, restatement %.2e" % (out[name + "_f32_ref_err_hidden"], out[name + "_f32_ref_err_proj"],
                                                                            out[name + "_restatement_err"]))
        del model, proj, sd
    path = os.path.join(HERE, "t5_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote t5_edges.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
