"""Reference fixtures of the mini backbone at 384 and 480 px (tests/test_backbone_hires_gpu.py).

    python tools/gen_hires_golden.py            # writes tests/golden/backbone_mini_{384,480}.npz

Runs on the machine that holds the reference, through the committed generator (oracle.gen_golden.run_backbone_case):
577 image tokens at 384 px (593 in the fused layers), 901 at 480 px (941 with 40 text tokens).  Compact records
(about 0.3 MB each): outputs as every 17th token row, full gradients of the parameters of <= 4 096 elements (biases,
norms, q / v bias), norm + probe of the larger ones."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden  # noqa: E402

COMPACT = dict(full_out=False, full_grad_max=4096)
CASES = {
    'backbone_mini_384': dict(preset='mini', B=2, img_size=384),
    'backbone_mini_480': dict(preset='mini', B=1, img_size=480, max_text_len=40),
}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, gen_golden.REF)
    gen_golden._install_timm_standin()
    for name, kw in CASES.items():
        kw = dict(kw)
        gen_golden.run_backbone_case(name, kw.pop('preset'), kw.pop('B'), **COMPACT, **kw)


if __name__ == '__main__':
    main()
