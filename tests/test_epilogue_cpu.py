"""hip._epilogue fills the Epilogue struct of gemm_nt, gemm_nt_grouped and conv2d_nhwc (field by field, on CPU tensors:
data_ptr() and stride() need no GPU, and the library is replaced by a recorder)."""
import ctypes

import torch

from exploremultimodal_amd import hip

OUT, OUT2, AUX = torch.zeros(8, 96), torch.zeros(8, 128, dtype=torch.bfloat16), torch.zeros(8, 160)
BIAS, VEC = torch.zeros(96), torch.zeros(8)
A, B = torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(96, 64, dtype=torch.bfloat16)
DEFAULTS = dict(out=OUT.data_ptr(), out2=None, bias=None, gamma=None, resid=None, row_scale=None, row_index=None,
                aux=None, ldo=96, ld2=0, relu=0, drop_thresh=0, inv_keep=1.0, beta=0.0, seed=0, colpart=None)


def _fields(e):
    return {name: getattr(e, name) for name, _ in hip.Epilogue._fields_}


def _expect(**changed):
    want = dict(DEFAULTS, **{k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in changed.items()})
    return _fields(hip.Epilogue(*[want[name] for name, _ in hip.Epilogue._fields_]))


class _Recorder:
    """stands for the C library: every entry point returns 0 and keeps the Epilogue structs it was given."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        def call(*args):
            for a in args:
                if isinstance(getattr(a, '_obj', None), hip.Epilogue):
                    self.seen.append(_fields(a._obj))
                elif isinstance(a, ctypes.Array) and a._type_ is hip.Epilogue:
                    self.seen.extend(_fields(e) for e in a)
            return 0
        return call


def _record(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(hip, '_lib', rec)
    monkeypatch.setattr(hip, '_stream', lambda: 0)
    monkeypatch.setattr(hip, 'zero_page', lambda device: VEC)
    return rec


def test_gemm_nt_epilogue_fields(monkeypatch):
    rec = _record(monkeypatch)
    cases = [
        ({}, {}),
        (dict(out2=OUT2, bias=BIAS), dict(out2=OUT2, bias=BIAS, ld2=128)),
        (dict(aux=AUX), dict(aux=AUX, ld2=160)),
        (dict(aux=AUX, out2=OUT2), dict(aux=AUX, out2=OUT2, ld2=128)),
        (dict(out2=OUT2, ldo=7, ld2=11), dict(out2=OUT2, ldo=7, ld2=11)),
        (dict(drop=(6554, 1.125), seed=(1 << 63) + 12345), dict(drop_thresh=6554, inv_keep=1.125, seed=(1 << 63) + 12345)),
        (dict(seed=-3), dict(seed=(1 << 64) - 3)),
        (dict(aux=AUX, colpart=VEC, relu=4, beta=0.5, gamma=VEC, resid=VEC, row_scale=VEC, row_index=VEC),
         dict(aux=AUX, ld2=160, colpart=VEC, relu=4, beta=0.5, gamma=VEC, resid=VEC, row_scale=VEC, row_index=VEC)),
        (dict(relu=True), dict(relu=1)),
    ]
    for kw, want in cases:
        rec.seen.clear()
        hip.gemm_nt(hip.EPI_BIAS, A, B, 8, 96, 64, OUT, tile=3, **kw)
        hip.gemm_nt(hip.EPI_BIAS, A, B, 8, 96, 64, OUT, A2=A, k1=32, **kw)
        assert rec.seen == [_expect(**want)] * 2, kw


def test_gemm_nt_grouped_epilogue_fields(monkeypatch):
    rec = _record(monkeypatch)
    o2 = torch.zeros(8, 96)
    hip.gemm_nt_grouped(hip.EPI_BIAS, [A, A], [B, B], [8, 8], 96, 64, [OUT, o2], drop=(100, 1.5), gamma=VEC,
                        per_group=[dict(bias=BIAS, seed=3), dict(out2=OUT2, seed=(1 << 63) + 1)])
    common = dict(drop_thresh=100, inv_keep=1.5, gamma=VEC)
    assert rec.seen == [_expect(bias=BIAS, seed=3, **common), _expect(out=o2, out2=OUT2, ld2=128, seed=(1 << 63) + 1, **common)]
    rec.seen.clear()
    hip.gemm_nt_grouped(hip.EPI_BIAS, [A], [B], [8], 96, 64, [OUT], aux=AUX)
    assert rec.seen == [_expect(aux=AUX, ld2=160)]


def test_conv2d_epilogue_fields(monkeypatch):
    rec = _record(monkeypatch)
    x, w = torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16), torch.zeros(96, 72, dtype=torch.bfloat16)
    cases = [({}, {}), (dict(relu_in=True), dict(relu=2)), (dict(relu=True, relu_in=True, bias=BIAS, resid=VEC, beta=0.5),
                                                           dict(relu=3, bias=BIAS, resid=VEC, beta=0.5)),
             (dict(out2=OUT2, ldo=13, relu=True), dict(out2=OUT2, ldo=13, ld2=128, relu=1))]
    for kw, want in cases:
        rec.seen.clear()
        hip.conv2d_nhwc(hip.EPI_BIAS, x, 2, 4, 4, 8, 3, w, 96, OUT, **kw)
        assert rec.seen == [_expect(**want)], kw
