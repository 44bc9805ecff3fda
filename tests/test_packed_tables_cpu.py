"""The host tables of a packed batch (hip.image_records, hip.crop_job_records, hip.aug_slot_records) byte for byte against
the struct layouts of include/vlmo_hip.h, written out here by hand.  No pinned memory and no library call: runs on a CPU."""
import ctypes
import struct

import numpy as np
import torch

from exploremultimodal_amd import hip

IMAGES = [(0, 1, 1), (3, 7, 5), (108, 64, 48)]
# (image, top, left, h, w, flip, S, filter, finish): h * S * 3 = 144, 2352, 1536, 48
JOBS = [(2, 3, 4, 6, 7, False, 8, hip.FILTER_BICUBIC, hip.FINISH_NORMALIZE),
        (2, 0, 0, 7, 5, True, 112, hip.FILTER_LANCZOS, hip.FINISH_MAP_PIXELS),
        (1, 0, 0, 32, 48, False, 16, hip.FILTER_BICUBIC, hip.FINISH_MAP_PIXELS),
        (0, 0, 0, 1, 1, True, 16, hip.FILTER_LANCZOS, hip.FINISH_NORMALIZE)]
OPS = [[hip.AUG_SKIP, hip.AUG_ROTATE], [hip.AUG_EQUALIZE, hip.AUG_POSTERIZE], [hip.AUG_SHEAR_X, hip.AUG_CONTRAST]]
ARG_A = [[0.0, 0.9335804264972017], [0.0, 2.0], [-0.21, 1.36]]
ARG_B = [[0.0, -0.35836794954530027], [0.0, 0.0], [0.0, 0.0]]


def test_image_records():
    rec = hip.image_records(IMAGES)
    assert rec.shape == (3,) and rec.itemsize == ctypes.sizeof(hip.Image) == 16
    assert rec.tobytes() == b''.join(struct.pack('<qii', o, H, W) for o, H, W in IMAGES)
    # the table staged behind the images starts at their byte count: 8-byte aligned for its int64 and double fields
    assert rec.nbytes % 8 == 0 and hip.image_records(IMAGES[:1]).nbytes % 8 == 0
    assert hip.image_records([]).shape == (0,)


def test_crop_job_records():
    outs = [torch.empty(3, job[6], job[6]) for job in JOBS]
    rec, total = hip.crop_job_records([job + (out,) for job, out in zip(JOBS, outs)])
    assert rec.shape == (4,) and rec.itemsize == ctypes.sizeof(hip.CropJob) == 56
    tmp_off = [0, 144, 144 + 2352, 144 + 2352 + 1536]
    assert total == tmp_off[-1] + 48
    want = b''.join(struct.pack('<10iqQ', im, top, left, h, w, int(flip), S, filt, fin, 0, off, out.data_ptr())
                    for (im, top, left, h, w, flip, S, filt, fin), off, out in zip(JOBS, tmp_off, outs))
    assert rec.tobytes() == want
    empty, none = hip.crop_job_records([])
    assert empty.shape == (0,) and none == 0


def test_aug_slot_records():
    rec = hip.aug_slot_records(np.array(OPS), np.array(ARG_A), np.array(ARG_B))
    assert rec.shape == (6,) and rec.itemsize == ctypes.sizeof(hip.AugSlot) == 24
    want = b''.join(struct.pack('<iidd', op, 0, a, b)
                    for orow, arow, brow in zip(OPS, ARG_A, ARG_B) for op, a, b in zip(orow, arow, brow))
    assert rec.tobytes() == want
