"""Images/s of RandAugment on one GPU: 64 sources of 640 x 480 (W x H), one plan sampled with n = 2, m = 7 and the
pretraining operations from a fixed seed.

  hip        augment.RandAugment.apply on the uploaded pack: the kernels, the table upload, the output allocation.
  hip+crop   the same followed by augment.TwoViewCrop.apply with three views (224 px bicubic, 112 px Lanczos, image_aug).
  cpu        the torch restatement of the same plan (RandAugment.apply on the host buffer) on this machine's cores; the
             thread count torch uses is printed with it.  It is a correctness restatement, not a tuned host pipeline.
The device lines are timed with device events around whole batches, after a warm-up, several rounds; the JSON line holds
the median round and the spread.  The upload of the packed bytes is in no figure (DataLoaderX overlaps it).  The tool
sets no threshold; the number to hold the device lines against is the engine's 4 500 pairs/s per GPU.

    python tools/randaug_bench.py [--batch 64] [--rounds 7] [--reps 50] [--cpu-reps 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exploremultimodal_amd import augment as A

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--cpu-reps', type=int, default=1)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('randaug_bench needs a GPU: the device lines are what it is for')
    dev = 'cuda'
    g = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (args.height, args.width, 3), generator=g, dtype=torch.uint8) for _ in range(args.batch)]
    packed = A.pack_images(images)
    on_dev = {'pixels': packed['pixels'].to(dev), 'table': packed['table']}
    ra = A.RandAugment(n=2, m=7, augs=A.PRETRAIN_AUGS)
    plan = ra.sample(args.batch, g)
    tv = A.TwoViewCrop(224, 112, MEAN, STD, aug_view=True)
    sizes = [(args.height, args.width)] * args.batch
    boxes, aug_boxes = A.sample_crop_params(sizes, generator=g), A.sample_crop_params(sizes, generator=g)
    flips, aug_flips = torch.rand(args.batch, generator=g) < 0.5, torch.rand(args.batch, generator=g) < 0.5

    def run_ra():
        return ra.apply(on_dev, plan)

    def run_both():
        return tv.apply(ra.apply(on_dev, plan), boxes, flips, aug_boxes, aug_flips)

    out = run_ra()
    run_both()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.cpu_reps):
        want = ra.apply(packed, plan)
    t_cpu = (time.perf_counter() - t0) / args.cpu_reps
    differing = int((out['pixels'].cpu() != want['pixels']).sum())
    for _ in range(2):
        timed(run_ra, 3), timed(run_both, 3)
    t_ra, t_both = [], []
    for _ in range(args.rounds):
        t_ra.append(timed(run_ra, args.reps))
        t_both.append(timed(run_both, args.reps))
    names = {v: k for k, v in A.AUG_CODES.items()}
    counts = {names.get(c, 'skipped'): int((plan['ops'] == c).sum()) for c in plan['ops'].unique().tolist()}

    def ms(ts):
        return [round(1e3 * min(ts), 4), round(1e3 * statistics.median(ts), 4), round(1e3 * max(ts), 4)]

    res = {'batch': args.batch, 'source': [args.height, args.width], 'n': 2, 'm': 7, 'slots': counts,
           'hip_images_per_s': args.batch / statistics.median(t_ra), 'hip_batch_ms': ms(t_ra),
           'hip_with_crop_images_per_s': args.batch / statistics.median(t_both), 'hip_with_crop_batch_ms': ms(t_both),
           'cpu_images_per_s': args.batch / t_cpu, 'cpu_batch_ms': round(1e3 * t_cpu, 1),
           'cpu_threads': torch.get_num_threads(), 'cpu_cores_usable': len(os.sched_getaffinity(0)),
           'values_differing_from_cpu': differing, 'values': int(args.batch * args.height * args.width * 3)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
