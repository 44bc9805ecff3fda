"""Images/s of the two-view crop on one GPU: 64 sources of 640 x 480 (W x H) -> image 224 px (bicubic) + image4dalle
112 px (Lanczos) + image_aug 224 px (bicubic), random boxes and flips from a fixed seed.

  hip     augment.TwoViewCrop.apply on the uploaded pack: both kernels, the table upload, the output allocation.
  torch   the same three views per image with F.interpolate(..., mode='bicubic', antialias=True) on the same card.  torch has
          no Lanczos: its second view is bicubic too, so it does slightly less arithmetic than the hip line.
Both are timed with device events around whole batches, after a warm-up, alternating, several rounds; the JSON line holds
the median round of each and the spread.  The upload of the packed bytes is not in either figure (DataLoaderX overlaps it).

    python tools/augment_bench.py [--batch 64] [--rounds 7] [--reps 200]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from exploremultimodal_amd import augment as A

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def torch_views(images, boxes, flips, aug_boxes, aug_flips, size, second, mean, std):
    out = {'image': [], 'image4dalle': [], 'image_aug': []}
    for im, box, flip, abox, aflip in zip(images, boxes, flips, aug_boxes, aug_flips):
        chw = im.permute(2, 0, 1)[None]
        for key, (top, left, h, w), fl, S in (('image', box, flip, size), ('image4dalle', box, flip, second),
                                              ('image_aug', abox, aflip, size)):
            v = F.interpolate(chw[:, :, top:top + h, left:left + w].float(), size=(S, S), mode='bicubic', antialias=True,
                              align_corners=False)[0]
            if fl:
                v = v.flip(2)
            out[key].append(0.8 / 255 * v + 0.1 if key == 'image4dalle' else (v / 255 - mean) / std)
    return {k: torch.stack(v) for k, v in out.items()}


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
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench needs a GPU: a CPU timing says nothing about this path')
    dev = 'cuda'
    g = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (args.height, args.width, 3), generator=g, dtype=torch.uint8) for _ in range(args.batch)]
    packed = A.pack_images(images)
    on_dev = {'pixels': packed['pixels'].to(dev), 'table': packed['table']}
    dev_images = [A.unpack_image(on_dev, i) for i in range(args.batch)]
    tv = A.TwoViewCrop(224, 112, MEAN, STD, aug_view=True)
    sizes = [(args.height, args.width)] * args.batch
    boxes, aug_boxes = A.sample_crop_params(sizes, generator=g), A.sample_crop_params(sizes, generator=g)
    flips, aug_flips = torch.rand(args.batch, generator=g) < 0.5, torch.rand(args.batch, generator=g) < 0.5
    bl, fl, abl, afl = boxes.tolist(), flips.tolist(), aug_boxes.tolist(), aug_flips.tolist()
    mean, std = torch.tensor(MEAN, device=dev)[:, None, None], torch.tensor(STD, device=dev)[:, None, None]

    def run_hip():
        return tv.apply(on_dev, boxes, flips, aug_boxes, aug_flips)

    def run_torch():
        return torch_views(dev_images, bl, fl, abl, afl, 224, 112, mean, std)

    a, b = run_hip(), run_torch()       # warm-up, and the two paths agree where they compute the same thing
    diff = {k: (a[k] - b[k]).abs().max().item() for k in ('image', 'image_aug')}
    for _ in range(2):
        timed(run_hip, 3), timed(run_torch, 1)
    t_hip, t_torch = [], []
    for _ in range(args.rounds):
        t_hip.append(timed(run_hip, args.reps))
        t_torch.append(timed(run_torch, max(1, args.reps // 10)))
    crop_px = sum(h * w for _, _, h, w in bl) / args.batch
    res = {'batch': args.batch, 'source': [args.height, args.width], 'views': [224, 112, 224], 'mean_crop_pixels': crop_px,
           'hip_images_per_s': args.batch / statistics.median(t_hip),
           'hip_batch_ms': [round(1e3 * min(t_hip), 4), round(1e3 * statistics.median(t_hip), 4), round(1e3 * max(t_hip), 4)],
           'torch_images_per_s': args.batch / statistics.median(t_torch),
           'torch_batch_ms': [round(1e3 * min(t_torch), 3), round(1e3 * statistics.median(t_torch), 3),
                              round(1e3 * max(t_torch), 3)],
           'max_abs_diff_bicubic_views': diff, 'torch_second_view': 'bicubic (torch has no Lanczos)'}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
