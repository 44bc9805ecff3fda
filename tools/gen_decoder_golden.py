"""Fixtures of the dVAE decoder tests, made from the reference implementation on the CPU.

    python tools/gen_decoder_golden.py --reference <checkout of the reference project>

Runs on the development machine only: the reference's ``dall_e`` package is imported from the given checkout at run
time and nothing of it is copied.  For each case the reference ``Decoder`` is built, loaded with
``synth_dvae_decoder_state_dict(0, ...)`` under ``strict=True`` (which proves key and shape parity of the mirror's
recipe), and run in fp32 on the one-hot map of seeded random ids.  Written under tests/golden/:

    dvae_dec_small.npz     n_hid=256, vocab_size=1024, ids [2, 4, 4]     -> ids, y [2, 6, 32, 32], sim_err
    dvae_dec_full_b2.npz   default model (vocab 8192), ids [2, 14, 14]   -> ids, y [2, 6, 112, 112], sim_err
    dvae_dec_keys.json     names and shapes of the reference decoder's state dict (both models)

``sim_err`` (a scalar) is max |y - y16| where y16 is a second CPU pass of the same reference module with every
convolution's weights (all but ``input``, which the reference keeps in fp32) and every convolution's input rounded to
fp16: the operand precision the reference itself runs at on a GPU (dall_e/utils.py:37-41).  The GPU tests bound the
engine's error by a multiple of it.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from exploremultimodal_amd import synth  # noqa: E402

CASES = {
    'dvae_dec_small': dict(hw=4, kw=dict(n_hid=256, vocab_size=1024)),
    'dvae_dec_full_b2': dict(hw=14, kw=dict()),
}
KEY_SETS = {'default': dict(), 'n_hid=256,vocab_size=1024': dict(n_hid=256, vocab_size=1024)}


def seeded_ids(vocab_size, hw, seed=99):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, vocab_size, (2, hw, hw), generator=g)


def fp16_operand_pass(dec, z):
    """The reference module with fp16-rounded convolution weights (not ``input``) and fp16-rounded convolution inputs,
    accumulated in fp32 on the CPU."""
    from dall_e.utils import Conv2d
    dec = copy.deepcopy(dec)
    hooks = []
    for name, m in dec.named_modules():
        if isinstance(m, Conv2d):
            if name != 'blocks.input':
                m.w.data = m.w.data.half().float()
            hooks.append(m.register_forward_pre_hook(lambda mod, args: (args[0].half().float(),)))
    y = dec(z)
    for h in hooks:
        h.remove()
    return y


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', default=os.environ.get('VLMO_REFERENCE'), required='VLMO_REFERENCE' not in os.environ,
                    help='checkout of the reference project (the directory that holds dall_e/)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    ap.add_argument('cases', nargs='*', default=list(CASES) + ['keys'])
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from dall_e.decoder import Decoder
    torch.manual_seed(0)
    for name in args.cases:
        if name == 'keys':
            keys = {k: {n: list(t.shape) for n, t in Decoder(**kw).state_dict().items()} for k, kw in KEY_SETS.items()}
            with open(os.path.join(args.out, 'dvae_dec_keys.json'), 'w') as f:
                json.dump(keys, f, indent=0, sort_keys=True)
            print('dvae_dec_keys.json', {k: len(v) for k, v in keys.items()})
            continue
        case = CASES[name]
        dec = Decoder(**case['kw'])
        dec.load_state_dict(synth.synth_dvae_decoder_state_dict(0, **case['kw']), strict=True)
        dec.eval()
        ids = seeded_ids(dec.vocab_size, case['hw'])
        z = F.one_hot(ids, num_classes=dec.vocab_size).permute(0, 3, 1, 2).float()
        with torch.no_grad():
            y = dec(z).float()
            y16 = fp16_operand_pass(dec, z).float()
        sim_err = (y - y16).abs().max().item()
        np.savez(os.path.join(args.out, name + '.npz'), ids=ids.numpy(), y=y.numpy(),
                 sim_err=np.float32(sim_err))
        print(name, 'y', tuple(y.shape), 'max|y|', y.abs().max().item(), 'mean|y|', y.abs().mean().item(),
              'sim_err', sim_err)


if __name__ == '__main__':
    main()
