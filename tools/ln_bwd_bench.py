"""LayerNorm backward fused with the residual-branch backward (vlmo_ln_resid_bwd, ln_bwd_kernel<.., false, true>) at
the training step's shape: time (kernel + fold launch), HBM rate, and a digest of what the kernel writes (dx, dz, its
column partials; the fold's atomics are not bit-stable) for comparing two builds bit for bit.
usage: python tools/ln_bwd_bench.py [M [d]]      (default 16704 768: B = 64 fused rows of VLMo-Base)
Bytes per launch: reads dy 2 + x 4 + dres 4 + zd 2, writes dx 4 + dz 2 = 18 bytes per element."""
import hashlib
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from exploremultimodal_amd import hip
dev = 'cuda'
M = int(sys.argv[1]) if len(sys.argv) > 1 else 16704
d = int(sys.argv[2]) if len(sys.argv) > 2 else 768


def timeit(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


g = torch.Generator().manual_seed(7)
r = lambda *s: torch.randn(*s, generator=g).to(dev)
x = r(M, d) * 2 + 0.5
w, gamma = r(d) * 0.1 + 1, r(d)
dy, dres, zd = r(M, d).bfloat16(), r(M, d), r(M, d).bfloat16()
mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-12).rsqrt()
scale = torch.tensor([0.0, 1 / 0.9, 1 / 0.9, 1 / 0.9], device=dev)
ridx = (torch.arange(M, device=dev) // 261 % 4).int()
dx = torch.empty(M, d, device=dev)
dz = torch.empty(M, d, device=dev, dtype=torch.bfloat16)
dw, db, dg, dbias = (torch.zeros(d, device=dev) for _ in range(4))
dp = hip.drop_params(0.1, True)


def run():
    hip.ln_resid_bwd(dy, x, w, mean, rstd, dres, dx, dw, db, zd, gamma, scale, ridx, dz, dg, dbias, M, d, drop=dp, seed=11)


run()
torch.cuda.synchronize()
h = hashlib.sha256()
rpb = max(8, (((M + 511) // 512 + 3) // 4) * 4)
partials = hip.workspace(x.device, 4 * d)[:(M + rpb - 1) // rpb * 4 * d]      # the kernel's own column partials
for t in (dx, dz.view(torch.int16), partials):
    h.update(t.cpu().numpy().tobytes())
for rnd in range(3):
    t = timeit(run)
    print(f'ln_resid_bwd M={M} d={d} round {rnd}: {t*1e6:7.1f} us  {18.0*M*d/t/1e12:5.2f} TB/s', flush=True)
print('dx, dz, column partials sha256', h.hexdigest())
