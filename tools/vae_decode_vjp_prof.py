"""Developer tool (GPU box): 20 ``ConvoFusionVae.decode_vjp`` calls at 128 frames / 8 chunks for rocprofv3's kernel statistics -- where the
time of a call goes, kernel by kernel (csrc/vae_dec.hpp).  A run of its own, with nothing else traced:

    rocprofv3 --kernel-trace --stats -d OUT -o vjp_bs1 --output-format csv -- python tools/vae_decode_vjp_prof.py [BS]      (default 1)

profiles/vae_decode_vjp_kernels.csv holds the vd_* rows of OUT/vjp_bs1_kernel_stats.csv.  Seeded weights and inputs.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from convofusion_amd.vae import ConvoFusionVae  # noqa: E402
from oracle import vae_weights  # noqa: E402
from tests.test_oracle_vae import ABL, KW  # noqa: E402


def main():
    bs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    vae = ConvoFusionVae(ablation=ABL, **KW)
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in vae_weights.make_state_dict().items()}, strict=True)
    vae = vae.cuda().eval()
    g = torch.Generator().manual_seed(11)
    z = torch.randn((2, bs, 8, 128), generator=g).cuda()
    d = torch.randn((bs, 128, 189), generator=g).cuda()
    for _ in range(20):
        vae.decode_vjp(z, [128] * bs, d)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
