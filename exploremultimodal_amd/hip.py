"""ctypes binding of libvlmo_hip.so (include/vlmo_hip.h).

PyTorch is used only for device memory and streams: every wrapper takes torch
tensors, passes raw device pointers + the caller's CURRENT stream to the C-ABI
and returns immediately (the library only enqueues work).  There is no CPU or
eager-PyTorch fallback: if the library is missing, importing this module works
but the first call raises.
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# VLMO_HIP_LIB: load another build of the same ABI (A/B timing of kernel variants in one GPU session)
LIB_PATH = os.environ.get('VLMO_HIP_LIB') or os.path.join(_HERE, 'lib', 'libvlmo_hip.so')

BF16, F16, F32 = 0, 1, 2
EPI_BIAS, EPI_BIAS_GELU, EPI_RESID, EPI_DGELU, EPI_F32, EPI_DUAL, EPI_ARGMAX, EPI_CE, EPI_CE_BWD = 0, 1, 2, 3, 4, 5, 6, 7, 8

_vp, _i32, _u32, _u64, _f32, _i64 = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32,
                                     ctypes.c_uint64, ctypes.c_float, ctypes.c_int64)


class Epilogue(ctypes.Structure):
    _fields_ = [('out', _vp), ('out2', _vp), ('bias', _vp), ('gamma', _vp),
                ('resid', _vp), ('row_scale', _vp), ('row_index', _vp), ('aux', _vp),
                ('ldo', _i32), ('ld2', _i32), ('relu', _i32),
                ('drop_thresh', _u32), ('inv_keep', _f32), ('beta', _f32),
                ('seed', _u64), ('colpart', _vp)]


_fp = _vp      # device pointers are passed as integers (tensor.data_ptr())


class BlockDesc(ctypes.Structure):
    """Mirror of VlmoBlockDesc (include/vlmo_hip.h); field order and types must match."""
    _fields_ = (
        [('M', _i32), ('d', _i32), ('hidden', _i32), ('heads', _i32),
         ('n_experts', _i32), ('exp_row0', _i32 * 2), ('exp_rows', _i32 * 2),
         ('n_attn', _i32), ('nseq', _i32 * 2), ('maxlen', _i32 * 2), ('lse_stride', _i32 * 2),
         ('attn_seed_idx', _i32 * 2), ('attn_seq0', _i32 * 2),
         ('seg', _fp * 2), ('keymask', _fp), ('eps', _f32),
         ('drop_thresh', _u32), ('attn_drop_thresh', _u32), ('inv_keep', _f32), ('attn_inv_keep', _f32),
         ('seed', _u64), ('rs1', _fp), ('rs2', _fp), ('row_index', _fp), ('tile', _i32), ('need_bwd', _i32)]
        + [(n, _fp) for n in ('g1', 'g2', 'n1w', 'n1b', 'n2w', 'n2b', 'qkv_bias', 'proj_b',
                              'qkv_w', 'qkv_wT', 'proj_w', 'proj_wT')]
        + [(n, _fp * 2) for n in ('b1', 'b2', 'w1', 'w1T', 'w2', 'w2T')]
        + [(n, _fp) for n in ('x', 'x1', 'x2', 'y1', 'qkv', 'ctx', 'zd1', 'y2', 'u', 'h', 'zd2',
                              'mean1', 'rstd1', 'mean2', 'rstd2')]
        + [('lse', _fp * 2)]
        + [(n, _fp) for n in ('dx2', 'dx1', 'dx0', 'dz2', 'du', 'dy2', 'dz1', 'dctx', 'dqkv', 'dy1',
                              'dg1', 'dg2', 'dn1w', 'dn1b', 'dn2w', 'dn2b', 'dqkv_w', 'dqkv_b',
                              'dproj_w', 'dproj_b')]
        + [(n, _fp * 2) for n in ('dw1', 'db1', 'dw2', 'db2')]
        + [('ws_main', _fp), ('ws_bytes', _i64)])


class StackDesc(ctypes.Structure):
    """Mirror of VlmoStackDesc (include/vlmo_hip.h)."""
    _fields_ = [('n_blocks', _i32), ('wgrad_batch', _i32), ('n_tmp_sets', _i32), ('wgrad_store', _i32),
                ('blocks', ctypes.POINTER(BlockDesc)), ('side_stream', _vp), ('grad_ready', ctypes.POINTER(_vp))]


class TnProblem(ctypes.Structure):
    """Mirror of VlmoTnProblem."""
    _fields_ = [('A', _vp), ('B', _vp), ('C', _vp), ('lda', _i32), ('ldb', _i32), ('ldc', _i32),
                ('M', _i32), ('N1', _i32), ('N2', _i32), ('alpha', _f32), ('accumulate', _i32)]


class TnProblemPlan(ctypes.Structure):
    """Mirror of VlmoTnProblemPlan."""
    _fields_ = [('tiles', _i32), ('splits', _i32), ('kt_per_split', _i32), ('mode', _i32), ('zero_first', _i32)]


class ColJob(ctypes.Structure):
    """Mirror of VlmoColJob."""
    _fields_ = [('kind', _i32), ('ld', _i32), ('src', _vp), ('rows', _i32), ('ncols', _i32),
                ('out', _vp * 4), ('n0', _i32), ('pad_', _i32)]


class Image(ctypes.Structure):
    """Mirror of VlmoImage."""
    _fields_ = [('offset', _i64), ('H', _i32), ('W', _i32)]


class AugSlot(ctypes.Structure):
    """Mirror of VlmoAugSlot."""
    _fields_ = [('op', _i32), ('pad_', _i32), ('a', ctypes.c_double), ('b', ctypes.c_double)]


class CropJob(ctypes.Structure):
    """Mirror of VlmoCropJob."""
    _fields_ = [('image', _i32), ('top', _i32), ('left', _i32), ('h', _i32), ('w', _i32), ('flip', _i32), ('S', _i32),
                ('filter', _i32), ('finish', _i32), ('pad_', _i32), ('tmp_off', _i64), ('out', _vp)]


_SIGS = {
    'vlmo_gemm_nt': [_i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32,
                     ctypes.POINTER(Epilogue), _vp],
    'vlmo_gemm_tn': [_i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _i64, _vp],
    'vlmo_ln_fwd': [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _f32, _vp],
    'vlmo_ln_bwd': [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp],
    'vlmo_ln_resid_bwd': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _f32, _u64,
                          _i32, _i32, _vp, _i64, _vp],
    'vlmo_attn_fwd': [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _u32, _f32,
                      _u64, _i32, _vp],
    'vlmo_attn_bwd': [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _f32,
                      _u32, _f32, _u64, _i32, _vp],
    'vlmo_attn_probs': [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    'vlmo_attn_gradcam': [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    'vlmo_resid_bwd': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _u32, _f32, _u64, _vp, _i64, _vp],
    'vlmo_colsum': [_i32, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _vp],
    'vlmo_cast_weight': [_i32, _vp, _i32, _i32, _vp, _vp, _vp],
    'vlmo_cast_weight_multi': [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    'vlmo_patchify': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    'vlmo_embed_img_finish': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _u32, _f32,
                              _u64, _vp],
    'vlmo_embed_img_bwd': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _u32, _f32,
                           _u64, _vp],
    'vlmo_embed_txt_fwd': [_vp] * 10 + [_i32, _i32, _i32, _f32, _u32, _f32, _u64, _vp],
    'vlmo_embed_txt_bwd': [_vp] * 11 + [_i32, _i32, _i32, _u32, _f32, _u64, _vp],
    'vlmo_embed_txt_rows_fwd': [_vp] * 11 + [_i32, _i32, _i32, _f32, _u32, _f32, _u64, _vp],
    'vlmo_embed_txt_rows_bwd': [_vp] * 13 + [_i64, _i32, _i32, _i32, _i32, _u32, _f32, _u64, _vp],
    'vlmo_conv2d_nhwc': [_i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp,
                         ctypes.POINTER(Epilogue), _vp],
    'vlmo_dvae_im2col': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    'vlmo_maxpool2_nhwc': [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    'vlmo_argmax_reduce': [_vp, _i32, _vp, _i32, _vp],
    'vlmo_dvae_embed': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    'vlmo_upsample2_nhwc': [_vp, _vp, _i32, _i32, _i32, _i32, _vp],
    'vlmo_dvae_out_head': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    'vlmo_conv4s2_nhwc': [_i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, ctypes.POINTER(Epilogue), _vp],
    'vlmo_convt4s2_nhwc': [_i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, ctypes.POINTER(Epilogue), _vp],
    'vlmo_dvae_patch4s2': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    'vlmo_dvae_out_head_linear': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    'vlmo_ce_reduce': [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp],
    'vlmo_stack_fwd': [ctypes.POINTER(StackDesc), _vp],
    'vlmo_stack_bwd': [ctypes.POINTER(StackDesc), _vp],
    'vlmo_gemm_tn_multi': [_i32, ctypes.POINTER(TnProblem), _i32, _vp],
    'vlmo_gemm_tn_multi_plan': [ctypes.POINTER(TnProblem), _i32, ctypes.POINTER(_i32), ctypes.POINTER(_i32),
                                ctypes.POINTER(TnProblemPlan), ctypes.POINTER(_i32), ctypes.POINTER(ctypes.c_uint16)],
    'vlmo_colwork_multi': [_i32, ctypes.POINTER(ColJob), _i32, _vp],
    'vlmo_event_create': [ctypes.POINTER(ctypes.c_void_p)],
    'vlmo_event_destroy': [_vp],
    'vlmo_stream_wait_event': [_vp, _vp],
    'vlmo_profile_start': [_i32],
    'vlmo_gemm_nt_grouped': [_i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp],
    'vlmo_mt_grad_norm': [ctypes.c_void_p, _f32, _f32, _vp, _vp, _vp],
    'vlmo_mt_adam': [ctypes.c_void_p, ctypes.c_void_p, _vp, _vp],
    'vlmo_mt_ema': [ctypes.c_void_p, _f32, _vp],
    'vlmo_mt_adam_ema': [ctypes.c_void_p, ctypes.c_void_p, _vp, _vp, _f32, _vp],
    'vlmo_side_stream_create': [_i32, ctypes.POINTER(ctypes.c_uint32), _i32, ctypes.POINTER(ctypes.c_void_p)],
    'vlmo_profile_stop': [_i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                          ctypes.POINTER(ctypes.c_int64)],
    'vlmo_gemm_nt_2src': [_i32, _i32, _i32, _vp, _i32, _i32, _f32, _vp, _i32, _vp, _i32, _i32, _i32, _i32,
                          ctypes.POINTER(Epilogue), _vp],
    'vlmo_comm_available': [],
    'vlmo_comm_unique_id': [_vp],
    'vlmo_comm_init': [ctypes.POINTER(ctypes.c_void_p), _vp, _i32, _i32],
    'vlmo_comm_destroy': [_vp],
    'vlmo_comm_count': [_vp, _vp, _vp],
    'vlmo_comm_all_reduce': [_vp, _vp, _vp, _i64, _i32, _vp],
    'vlmo_comm_reduce_scatter': [_vp, _vp, _vp, _i64, _i32, _vp],
    'vlmo_comm_all_gather': [_vp, _vp, _vp, _i64, _i32, _vp],
    'vlmo_grad_pack': [_vp, _vp, _i64, _f32, _vp],
    'vlmo_grad_unpack': [_vp, _vp, _i64, _vp],
    'vlmo_ln_gelu_fwd': [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _f32, _vp],
    'vlmo_ln_gelu_bwd': [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp,
                         _i64, _vp],
    'vlmo_vqa_bce': [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _vp, _i32, _vp],
    'vlmo_isda_update': [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    'vlmo_isda_aug_fwd': [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _i32, _vp, _i64, _vp],
    'vlmo_isda_aug_bwd': [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _i32, _vp, _i64, _vp],
    'vlmo_sim_topk': [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp, ctypes.c_size_t, _vp, _vp, _vp],
    'vlmo_crop_resample': [_vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32, ctypes.POINTER(_f32), ctypes.POINTER(_f32), _f32, _vp,
                           _i64, _vp],
    'vlmo_randaug': [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _i64, _vp],
    'vlmo_relevance_step': [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp],
}

_lib = None
ABI_VERSION = 17    # vlmo_abi_version(): struct layouts of include/vlmo_hip.h mirrored above

def lib():
    """Load (once) and return the C-ABI library; raise loudly if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: build the HIP extension first '
                '(python -c "import __graft_entry__ as g; g.build()" or '
                'make -C exploremultimodal_amd/csrc). There is no CPU fallback.')
        L = ctypes.CDLL(LIB_PATH)
        L.vlmo_last_error.restype = ctypes.c_char_p
        L.vlmo_abi_version.restype = ctypes.c_int
        if L.vlmo_abi_version() != ABI_VERSION:
            raise RuntimeError(f'{LIB_PATH} has ABI version {L.vlmo_abi_version()}, this package needs {ABI_VERSION}: '
                               'rebuild it (make -C exploremultimodal_amd/csrc)')
        L.vlmo_reduce_ws_bytes.restype = ctypes.c_int64
        L.vlmo_reduce_ws_bytes.argtypes = [_i32]
        L.vlmo_stack_bwd_ws_bytes.restype = ctypes.c_int64
        L.vlmo_stack_bwd_ws_bytes.argtypes = [_i32, _i32, _i32, _i32]
        L.vlmo_gemm_tn_ws_bytes.restype = ctypes.c_int64
        L.vlmo_isda_ws_bytes.restype = ctypes.c_int64
        L.vlmo_isda_ws_bytes.argtypes = [_i32, _i32, _i32]
        L.vlmo_gemm_tn_ws_bytes.argtypes = [_i32, _i32, _i32]
        L.vlmo_sim_topk_ws_bytes.restype = ctypes.c_int64
        L.vlmo_sim_topk_ws_bytes.argtypes = [_i32, _i32, _i32, _i32]
        L.vlmo_randaug_ws_bytes.restype = ctypes.c_int64
        L.vlmo_randaug_ws_bytes.argtypes = [_i32]
        L.vlmo_embed_txt_rows_ws_bytes.restype = ctypes.c_int64
        L.vlmo_embed_txt_rows_ws_bytes.argtypes = [_i32, _i32, _i32]
        for name, sig in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = sig
            fn.restype = ctypes.c_int
        _lib = L
    return _lib


def exported_symbols():
    return ['vlmo_last_error', 'vlmo_abi_version', 'vlmo_reduce_ws_bytes', 'vlmo_stack_bwd_ws_bytes',
            'vlmo_gemm_tn_ws_bytes', 'vlmo_isda_ws_bytes', 'vlmo_sim_topk_ws_bytes', 'vlmo_randaug_ws_bytes',
            'vlmo_embed_txt_rows_ws_bytes'] + list(_SIGS)


def _check(rc, name):
    if rc != 0:
        raise RuntimeError(f'{name} failed (rc={rc}): {lib().vlmo_last_error().decode()}')


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(t):
    return {torch.bfloat16: BF16, torch.float16: F16, torch.float32: F32}[t.dtype]


_SCRATCH = {}


def _scratch(kind, device, nbytes, floor):
    """Persistent fp32 scratch of at least ``nbytes`` (allocated no smaller than ``floor``), one per (kind, device,
    stream): reuse is ordered by the stream, and kernels on different streams never share a buffer."""
    key = (kind, device, torch.cuda.current_stream(device).cuda_stream)
    ws = _SCRATCH.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(max(nbytes, floor) // 4, dtype=torch.float32, device=device)
        _SCRATCH[key] = ws
    return ws


def workspace(device, ncols):
    """Scratch of the column-reducing kernels."""
    return _scratch('reduce', device, lib().vlmo_reduce_ws_bytes(ncols), 1 << 23)


def tn_workspace(device, nbytes):
    """Slab scratch of the weight-gradient GEMM."""
    return _scratch('tn', device, nbytes, 1 << 24)


def drop_params(p, training):
    """(thresh, inv_keep) of the counter-based dropout; thresh 0 disables it."""
    if not training or p <= 0.0:
        return 0, 1.0
    thresh = int(round(p * 65536))
    return thresh, 65536.0 / (65536 - thresh)


def _seed64(seed):
    return seed & 0xFFFFFFFFFFFFFFFF


def _epilogue(out, *, out2=None, bias=None, gamma=None, resid=None, row_scale=None, row_index=None, aux=None, ldo=None,
              ld2=None, relu=False, drop=(0, 1.0), seed=0, beta=0.0, colpart=None):
    """The Epilogue of one GEMM / convolution; ldo defaults to out's row stride, ld2 to out2's, else aux's, else 0."""
    if ld2 is None:
        ld2 = out2.stride(0) if out2 is not None else (aux.stride(0) if aux is not None else 0)
    return Epilogue(_p(out), _p(out2), _p(bias), _p(gamma), _p(resid), _p(row_scale), _p(row_index), _p(aux),
                    ldo if ldo is not None else out.stride(0), ld2, int(relu), drop[0], drop[1], beta, _seed64(seed),
                    _p(colpart))


# ------------------------------------------------------------------ wrappers

def gemm_nt(epi, A, B, M, N, K, out, *, tile=-1, lda=None, ldb=None, A2=None, k1=0, seg_scale=1.0, **epilogue):
    """``epilogue``: the keywords of ``_epilogue``.  A2 / k1 / seg_scale: two-segment reduction (vlmo_gemm_nt_2src):
    columns [0, k1) of B meet A, [k1, K) meet A2, the first segment's partial sum is multiplied by seg_scale."""
    e = _epilogue(out, **epilogue)
    if A2 is not None:
        rc = lib().vlmo_gemm_nt_2src(epi, _dt(A), tile, _p(A), lda if lda is not None else A.stride(0), k1,
                                     float(seg_scale), _p(A2), A2.stride(0), _p(B),
                                     ldb if ldb is not None else B.stride(0), M, N, K, ctypes.byref(e), _stream())
        _check(rc, 'vlmo_gemm_nt_2src')
        return
    rc = lib().vlmo_gemm_nt(epi, _dt(A), tile, _p(A), lda if lda is not None else A.stride(0),
                            _p(B), ldb if ldb is not None else B.stride(0), M, N, K,
                            ctypes.byref(e), _stream())
    _check(rc, 'vlmo_gemm_nt')


def gemm_nt_grouped(epi, As, Bs, Ms, N, K, outs, *, per_group=None, tile=-1, **common):
    """vlmo_gemm_nt_grouped: problems g = (As[g] [Ms[g], K], Bs[g] [N, K]) -> outs[g]; ``per_group[g]`` holds the
    epilogue keywords of gemm_nt that differ per group (bias, out2, seed, ...), ``common`` the shared ones."""
    n = len(As)
    es = (Epilogue * n)()
    for g in range(n):
        es[g] = _epilogue(outs[g], **{**common, **(per_group[g] if per_group else {})})
    pa = (ctypes.c_void_p * n)(*[_p(a) for a in As])
    pb = (ctypes.c_void_p * n)(*[_p(b) for b in Bs])
    ms = (ctypes.c_int32 * n)(*Ms)
    rc = lib().vlmo_gemm_nt_grouped(epi, _dt(As[0]), tile, n, pa, As[0].stride(0), pb, Bs[0].stride(0), ms, N, K, es, _stream())
    _check(rc, 'vlmo_gemm_nt_grouped')


def gemm_tn(A, B, C, M, N1, N2, alpha=1.0, splits=0, slab=True):
    ws = tn_workspace(A.device, max(splits % 1000, 16) * N1 * N2 * 4 if splits > 0 else
                      lib().vlmo_gemm_tn_ws_bytes(M, N1, N2)) if slab else None
    rc = lib().vlmo_gemm_tn(_dt(A), _p(A), A.stride(0), _p(B), B.stride(0), _p(C), C.stride(0),
                            M, N1, N2, alpha, splits, _p(ws), ws.numel() * 4 if ws is not None else 0, _stream())
    _check(rc, 'vlmo_gemm_tn')


def ln_fwd(x, w, b, y, mean, rstd, rowmap, M, d, eps):
    rc = lib().vlmo_ln_fwd(_p(x), _p(w), _p(b), _p(y), int(y.dtype == torch.float32), _p(mean),
                           _p(rstd), _p(rowmap), M, d, eps, _stream())
    _check(rc, 'vlmo_ln_fwd')


def ln_bwd(dy, rowmap, x, w, mean, rstd, dres, dx, dw, db, M, d):
    rc = lib().vlmo_ln_bwd(_p(dy), int(dy.dtype == torch.float32), _p(rowmap), _p(x), _p(w),
                           _p(mean), _p(rstd), _p(dres), _p(dx), _p(dw), _p(db), M, d, _p(ws := workspace(x.device, 2 * d)),
                           ws.numel() * 4, _stream())
    _check(rc, 'vlmo_ln_bwd')


def ln_resid_bwd(dy, x, w, mean, rstd, dres, dx, dw, db, zd, gamma, row_scale, row_index, dz, dgamma, dbias, M, d,
                 drop=(0, 1.0), seed=0):
    ws = workspace(x.device, 4 * d)
    rc = lib().vlmo_ln_resid_bwd(_p(dy), _p(x), _p(w), _p(mean), _p(rstd), _p(dres), _p(dx), _p(dw), _p(db), _p(zd),
                                 _p(gamma), _p(row_scale), _p(row_index), _p(dz), _p(dgamma), _p(dbias), drop[0], drop[1],
                                 _seed64(seed), M, d, _p(ws), ws.numel() * 4, _stream())
    _check(rc, 'vlmo_ln_resid_bwd')


def attn_fwd(qkv, seg, nseq, keymask, ctx, lse, heads, d, max_len, scale, drop=(0, 1.0), seed=0, mask_seq0=0):
    rc = lib().vlmo_attn_fwd(_p(qkv), _p(seg), nseq, _p(keymask), _p(ctx), _p(lse),
                             lse.stride(0) if lse is not None else 0, heads, d, max_len, scale,
                             drop[0], drop[1], _seed64(seed), mask_seq0, _stream())
    _check(rc, 'vlmo_attn_fwd')


def attn_bwd(qkv, ctx, dctx, lse, seg, nseq, keymask, dqkv, heads, d, max_len, scale,
             drop=(0, 1.0), seed=0, qv_colsum=None, mask_seq0=0):
    rc = lib().vlmo_attn_bwd(_p(qkv), _p(ctx), _p(dctx), _p(lse), lse.stride(0), _p(seg), nseq,
                             _p(keymask), _p(dqkv), _p(qv_colsum), heads, d, max_len, scale, drop[0], drop[1],
                             _seed64(seed), mask_seq0, _stream())
    _check(rc, 'vlmo_attn_bwd')


def attn_probs(qkv, seg, nseq, keymask, probs, heads, d, seq_len, q0, nq, head_mean, scale):
    """probs fp32 [nseq, 1 if head_mean else heads, nq, seq_len] = softmax(q k^T * scale + keymask), rows [q0, q0 + nq)."""
    rc = lib().vlmo_attn_probs(_p(qkv), _p(seg), nseq, _p(keymask), _p(probs), heads, d, seq_len, q0, nq,
                               int(bool(head_mean)), scale, _stream())
    _check(rc, 'vlmo_attn_probs')


GRADCAM_KINDS = {'cam': 0, 'attn_grad': 1, 'grad': 2}      # VLMO_GRADCAM_* of the header


def attn_gradcam(qkv, dctx, seg, nseq, keymask, out, heads, d, seq_len, q0, nq, kind, head_mean, scale):
    """out fp32 [nseq, 1 if head_mean else heads, nq, seq_len]: P * max(G, 0) ('cam'), P * G ('attn_grad') or G ('grad')
    with P of attn_probs and G = dctx v^T per head; kind is a key of GRADCAM_KINDS or its number."""
    rc = lib().vlmo_attn_gradcam(_p(qkv), _p(dctx), _p(seg), nseq, _p(keymask), _p(out), heads, d, seq_len, q0, nq,
                                 GRADCAM_KINDS.get(kind, kind), int(bool(head_mean)), scale, _stream())
    _check(rc, 'vlmo_attn_gradcam')


def resid_bwd(dx, zd, gamma, row_scale, dz, dgamma, dbias, M, d, drop=(0, 1.0), seed=0, row_index=None):
    ws = workspace(dx.device, 2 * d)
    rc = lib().vlmo_resid_bwd(_p(dx), _p(zd), _p(gamma), _p(row_scale), _p(row_index), _p(dz), _p(dgamma),
                              _p(dbias), M, d, drop[0], drop[1], _seed64(seed),
                              _p(ws), ws.numel() * 4, _stream())
    _check(rc, 'vlmo_resid_bwd')


def colsum(x, out, M, N):
    ws = workspace(x.device, N)
    rc = lib().vlmo_colsum(_dt(x), _p(x), x.stride(0), _p(out), M, N, _p(ws), ws.numel() * 4, _stream())
    _check(rc, 'vlmo_colsum')


def cast_weight(src, dst, dstT):
    rows, cols = src.shape
    ref = dst if dst is not None else dstT
    rc = lib().vlmo_cast_weight(_dt(ref), _p(src), rows, cols, _p(dst), _p(dstT), _stream())
    _check(rc, 'vlmo_cast_weight')


def cast_weight_multi(jobs):
    """jobs: [(src fp32 [rows, cols], dst or None, dstT or None)] -> one launch (per 72 jobs)."""
    n = len(jobs)
    if n == 0:
        return
    ref = jobs[0][1] if jobs[0][1] is not None else jobs[0][2]
    src = (ctypes.c_void_p * n)(*[_p(a) for a, _, _ in jobs])
    dst = (ctypes.c_void_p * n)(*[_p(b) for _, b, _ in jobs])
    dstT = (ctypes.c_void_p * n)(*[_p(c) for _, _, c in jobs])
    rows = (ctypes.c_int32 * n)(*[a.shape[0] for a, _, _ in jobs])
    cols = (ctypes.c_int32 * n)(*[a.shape[1] for a, _, _ in jobs])
    _check(lib().vlmo_cast_weight_multi(_dt(ref), n, src, rows, cols, dst, dstT, _stream()), 'vlmo_cast_weight_multi')


def patchify(img, out, patch):
    B, C, H, W = img.shape
    rc = lib().vlmo_patchify(_p(img), _p(out), B, C, H, W, patch, _stream())
    _check(rc, 'vlmo_patchify')


def embed_img_finish(proj, cls_tok, mask_tok, pos, type_row, masked, x, B, npatch, d,
                     drop=(0, 1.0), seed=0):
    rc = lib().vlmo_embed_img_finish(_p(proj), _p(cls_tok), _p(mask_tok), _p(pos), _p(type_row),
                                     _p(masked), _p(x), B, npatch, d, drop[0], drop[1],
                                     _seed64(seed), _stream())
    _check(rc, 'vlmo_embed_img_finish')


def embed_img_bwd(dx, masked, dproj, dcls, dmask, dpos, dtype_row, B, npatch, d, drop=(0, 1.0),
                  seed=0):
    rc = lib().vlmo_embed_img_bwd(_p(dx), _p(masked), _p(dproj), _p(dcls), _p(dmask), _p(dpos),
                                  _p(dtype_row), B, npatch, d, drop[0], drop[1],
                                  _seed64(seed), _stream())
    _check(rc, 'vlmo_embed_img_bwd')


def embed_txt_fwd(ids, word, pos, btype0, ln_w, ln_b, type0, x, xhat, rstd, B, T, d, eps,
                  drop=(0, 1.0), seed=0):
    rc = lib().vlmo_embed_txt_fwd(_p(ids), _p(word), _p(pos), _p(btype0), _p(ln_w), _p(ln_b),
                                  _p(type0), _p(x), _p(xhat), _p(rstd), B, T, d, eps, drop[0],
                                  drop[1], _seed64(seed), _stream())
    _check(rc, 'vlmo_embed_txt_fwd')


def embed_txt_bwd(dx, ids, xhat, rstd, ln_w, dword, dpos, dbtype0, dln_w, dln_b, dtype0, B, T, d,
                  drop=(0, 1.0), seed=0):
    rc = lib().vlmo_embed_txt_bwd(_p(dx), _p(ids), _p(xhat), _p(rstd), _p(ln_w), _p(dword),
                                  _p(dpos), _p(dbtype0), _p(dln_w), _p(dln_b), _p(dtype0), B, T, d,
                                  drop[0], drop[1], _seed64(seed), _stream())
    _check(rc, 'vlmo_embed_txt_bwd')


def embed_txt_rows_fwd(ids, src, word, pos, btype0, ln_w, ln_b, type0, x, xhat, rstd, nrows, T, d, eps,
                       drop=(0, 1.0), seed=0):
    """Row-table form of embed_txt_fwd: packed row m embeds ids.view(-1)[src[m]] at position src[m] % T."""
    rc = lib().vlmo_embed_txt_rows_fwd(_p(ids), _p(src), _p(word), _p(pos), _p(btype0), _p(ln_w), _p(ln_b),
                                       _p(type0), _p(x), _p(xhat), _p(rstd), nrows, T, d, eps, drop[0],
                                       drop[1], _seed64(seed), _stream())
    _check(rc, 'vlmo_embed_txt_rows_fwd')


def embed_txt_rows_bwd(dx, ids, off, xhat, rstd, ln_w, dword, dpos, dbtype0, dln_w, dln_b, dtype0, B, T, maxlen, d,
                       drop=(0, 1.0), seed=0):
    """Row-table form of embed_txt_bwd: off int32 [B + 1] (device) = prefix sums of the row counts, maxlen their
    maximum (a host int).  The vector gradients are summed in a fixed order through a scratch of partial rows."""
    nbytes = lib().vlmo_embed_txt_rows_ws_bytes(B, maxlen, d)
    ws = _scratch('embed_txt_rows', dx.device, nbytes, 1 << 20)
    rc = lib().vlmo_embed_txt_rows_bwd(_p(dx), _p(ids), _p(off), _p(xhat), _p(rstd), _p(ln_w), _p(dword),
                                       _p(dpos), _p(dbtype0), _p(dln_w), _p(dln_b), _p(dtype0), _p(ws),
                                       ws.numel() * 4, B, T, maxlen, d, drop[0], drop[1], _seed64(seed), _stream())
    _check(rc, 'vlmo_embed_txt_rows_bwd')


# ------------------------------------------------------------------ dVAE encoder / decoder
_ZERO = {}


def zero_page(device):
    z = _ZERO.get(device)
    if z is None:
        z = torch.zeros(256, dtype=torch.float32, device=device)
        _ZERO[device] = z
    return z


def conv2d_nhwc(epi, x, B, H, W, Cin, kw, w, Cout, out, *, out2=None, bias=None, resid=None, relu=False,
                relu_in=False, beta=0.0, ldo=None):
    """relu: ReLU on the output; relu_in: the convolution reads relu(x) (applied to the fragments, x stays as it is)."""
    e = _epilogue(out, out2=out2, bias=bias, resid=resid, relu=int(relu) | (2 if relu_in else 0), beta=beta, ldo=ldo)
    rc = lib().vlmo_conv2d_nhwc(epi, _dt(x), _p(x), B, H, W, Cin, kw, _p(w), Cout, _p(zero_page(x.device)),
                                ctypes.byref(e), _stream())
    _check(rc, 'vlmo_conv2d_nhwc')


def dvae_im2col(x, out, kw, Kpad):
    B, C, H, W = x.shape
    _check(lib().vlmo_dvae_im2col(_p(x), _p(out), B, C, H, W, kw, Kpad, _stream()), 'vlmo_dvae_im2col')


def maxpool2_nhwc(x, raw, relu, B, H, W, C):
    _check(lib().vlmo_maxpool2_nhwc(_p(x), _p(raw), _p(relu), B, H, W, C, _stream()), 'vlmo_maxpool2_nhwc')


def argmax_reduce(partial, nchunk, ids, M):
    _check(lib().vlmo_argmax_reduce(_p(partial), nchunk, _p(ids), M, _stream()), 'vlmo_argmax_reduce')


def dvae_embed(ids, table, bias, out):
    """out f16 [M, n_init] = fp16(table[ids] + bias); ids int64 [M] already checked to lie in [0, vocab)."""
    vocab, n_init = table.shape
    _check(lib().vlmo_dvae_embed(_p(ids), _p(table), _p(bias), _p(out), ids.numel(), vocab, n_init, _stream()),
           'vlmo_dvae_embed')


def upsample2_nhwc(x, out, B, H, W, C):
    """Nearest-neighbour 2x upsampling of an NHWC map: x [B*H*W, C] -> out [B*2H*2W, C] (f16)."""
    _check(lib().vlmo_upsample2_nhwc(_p(x), _p(out), B, H, W, C, _stream()), 'vlmo_upsample2_nhwc')


def dvae_out_head(x, w, bias, out, B, H, W):
    """out f32 [B, Cout, H, W] = conv1x1(relu(x)) + bias; x f16 [B*H*W, C], w f16 [Cout, C], Cout <= 8."""
    Cout, C = w.shape
    _check(lib().vlmo_dvae_out_head(_p(x), _p(w), _p(bias), _p(out), B, H, W, C, Cout, _stream()), 'vlmo_dvae_out_head')


def conv4s2_nhwc(x, B, H, W, Cin, w, Cout, out, *, bias=None, relu=False):
    """Conv2d(Cin, Cout, 4, stride=2, padding=1): x f16 [B*H*W, Cin], w f16 [Cout, 16*Cin] (tap-major) ->
    out f16 [B*(H/2)*(W/2), Cout], bias and optional ReLU fused."""
    e = _epilogue(out, bias=bias, relu=int(relu))
    rc = lib().vlmo_conv4s2_nhwc(_dt(x), _p(x), B, H, W, Cin, _p(w), Cout, _p(zero_page(x.device)), ctypes.byref(e),
                                 _stream())
    _check(rc, 'vlmo_conv4s2_nhwc')


def convT4s2_nhwc(x, B, H, W, Cin, w, Cout, out, *, bias=None, relu=False):
    """ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1): x f16 [B*H*W, Cin], w f16 [4, Cout, 4*Cin] (one quarter per
    output parity, see include/vlmo_hip.h) -> out f16 [B*2H*2W, Cout], bias and optional ReLU fused."""
    e = _epilogue(out, bias=bias, relu=int(relu))
    rc = lib().vlmo_convt4s2_nhwc(_dt(x), _p(x), B, H, W, Cin, _p(w), Cout, _p(zero_page(x.device)), ctypes.byref(e),
                                  _stream())
    _check(rc, 'vlmo_convt4s2_nhwc')


def dvae_patch4s2(x, out, Kpad):
    """x f32 [B, C, H, W] -> out f16 [B*(H/2)*(W/2), Kpad]: the 4x4 stride-2 patches, column = c*16 + ky*4 + kx."""
    B, C, H, W = x.shape
    _check(lib().vlmo_dvae_patch4s2(_p(x), _p(out), B, C, H, W, Kpad, _stream()), 'vlmo_dvae_patch4s2')


def dvae_out_head_linear(x, w, bias, out, B, H, W):
    """out f32 [B, Cout, H, W] = conv1x1(x) + bias (no ReLU); x f16 [B*H*W, C], w f16 [Cout, C], Cout <= 8."""
    Cout, C = w.shape
    _check(lib().vlmo_dvae_out_head_linear(_p(x), _p(w), _p(bias), _p(out), B, H, W, C, Cout, _stream()),
           'vlmo_dvae_out_head_linear')


def gemm_tn_multi(problems, dtype=BF16):
    """problems: [(A, B, C, M, N1, N2, accumulate[, alpha])] with A [M, >=N1], B [M, >=N2] bf16/f16 and C [N1, >=N2]
    fp32: C (+)= alpha * A^T B, alpha 1 when the tuple leaves it out."""
    n = len(problems)
    arr = (TnProblem * n)()
    for i, (A, B, C, M, N1, N2, acc, *alpha) in enumerate(problems):
        arr[i] = TnProblem(_p(A), _p(B), _p(C), A.stride(0), B.stride(0), C.stride(0), M, N1, N2,
                           float(alpha[0]) if alpha else 1.0, int(acc))
    _check(lib().vlmo_gemm_tn_multi(dtype, arr, n, _stream()), 'vlmo_gemm_tn_multi')


TN_ORDER, TN_NOP = 1024, 0xFFFF      # a launch's placement table: entries, and the code of a workgroup that runs nothing


def gemm_tn_multi_plan(shapes):
    """What vlmo_gemm_tn_multi does with problems of these shapes (a host query: no GPU, no tensors).
    shapes: [(M, N1, N2, accumulate)].  Returns one dict per launch: q0, nq (the problems it takes), problems
    [(tiles, splits, kt_per_split, mode, zero_first)], grid and order (grid codes: (problem - q0) << 12 | workgroup
    inside the problem, or TN_NOP; entry b runs on XCD b % 8)."""
    n = len(shapes)
    arr = (TnProblem * n)()
    for i, (M, N1, N2, acc) in enumerate(shapes):
        arr[i] = TnProblem(None, None, None, N1, N2, N2, M, N1, N2, 1.0, int(acc))
    nl, q0 = _i32(0), (_i32 * (n + 1))()
    pp, grid, order = (TnProblemPlan * n)(), (_i32 * n)(), (ctypes.c_uint16 * (n * TN_ORDER))()
    _check(lib().vlmo_gemm_tn_multi_plan(arr, n, ctypes.byref(nl), q0, pp, grid, order), 'vlmo_gemm_tn_multi_plan')
    return [dict(q0=q0[k], nq=q0[k + 1] - q0[k],
                 problems=[(p.tiles, p.splits, p.kt_per_split, p.mode, p.zero_first) for p in pp[q0[k]:q0[k + 1]]],
                 grid=grid[k], order=list(order[k * TN_ORDER:k * TN_ORDER + grid[k]]))
            for k in range(nl.value)]


def colwork_multi(jobs, dtype=BF16):
    """jobs: [(kind, src, rows, ncols, outs, n0)]; kind 0 = fold fp32 partial rows src [rows, ncols],
    kind 1 = column sums of the bf16/f16 matrix src [rows, ld]."""
    n = len(jobs)
    arr = (ColJob * n)()
    for i, (kind, src, rows, ncols, outs, n0) in enumerate(jobs):
        o = (ctypes.c_void_p * 4)(*[_p(t) for t in (list(outs) + [None] * 4)[:4]])
        arr[i] = ColJob(kind, src.stride(0), _p(src), rows, ncols, o, n0, 0)
    _check(lib().vlmo_colwork_multi(dtype, arr, n, _stream()), 'vlmo_colwork_multi')


def event_create():
    out = ctypes.c_void_p()
    _check(lib().vlmo_event_create(ctypes.byref(out)), 'vlmo_event_create')
    return out.value


def stream_wait_event(stream, ev):
    """stream: torch stream (or raw handle); ev: handle from event_create()."""
    raw = stream.cuda_stream if hasattr(stream, 'cuda_stream') else stream
    _check(lib().vlmo_stream_wait_event(raw, ev), 'vlmo_stream_wait_event')


# ---- gradient exchange (include/vlmo_hip.h: vlmo_comm_*) -------------------------------------------------------------
COMM_ID_BYTES = 128


def comm_available():
    return bool(lib().vlmo_comm_available())


def comm_unique_id():
    """128 opaque bytes; rank 0 creates them, every rank passes the same ones to comm_init."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(lib().vlmo_comm_unique_id(buf), 'vlmo_comm_unique_id')
    return buf.raw


def comm_init(uid, rank, world):
    if len(uid) != COMM_ID_BYTES:
        raise ValueError(f'communicator id must be {COMM_ID_BYTES} bytes')
    out = ctypes.c_void_p()
    _check(lib().vlmo_comm_init(ctypes.byref(out), ctypes.c_char_p(bytes(uid)), rank, world), 'vlmo_comm_init')
    return out.value


def comm_destroy(comm):
    _check(lib().vlmo_comm_destroy(comm), 'vlmo_comm_destroy')


def comm_count(comm):
    """ranks in the communicator, as RCCL reports it."""
    n = ctypes.c_int(0)
    _check(lib().vlmo_comm_count(comm, ctypes.byref(n), None), 'vlmo_comm_count')
    return n.value


def comm_all_reduce(comm, t, stream=None):
    """in-place sum over the ranks, enqueued on `stream` (default: the current stream)."""
    raw = _stream() if stream is None else stream.cuda_stream
    _check(lib().vlmo_comm_all_reduce(comm, _p(t), _p(t), t.numel(), _dt(t), raw), 'vlmo_comm_all_reduce')


def comm_reduce_scatter(comm, out, src, stream=None):
    assert src.numel() % out.numel() == 0 and src.dtype == out.dtype
    raw = _stream() if stream is None else stream.cuda_stream
    _check(lib().vlmo_comm_reduce_scatter(comm, _p(src), _p(out), out.numel(), _dt(out), raw),
           'vlmo_comm_reduce_scatter')


def comm_all_gather(comm, out, src, stream=None):
    assert out.numel() % src.numel() == 0 and src.dtype == out.dtype
    raw = _stream() if stream is None else stream.cuda_stream
    _check(lib().vlmo_comm_all_gather(comm, _p(src), _p(out), src.numel(), _dt(src), raw), 'vlmo_comm_all_gather')


def grad_pack(src, dst, scale, stream=None):
    """dst (bf16) = src (fp32) * scale, one pass."""
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    raw = _stream() if stream is None else stream.cuda_stream
    _check(lib().vlmo_grad_pack(_p(src), _p(dst), src.numel(), float(scale), raw), 'vlmo_grad_pack')


def grad_unpack(src, dst, stream=None):
    assert src.dtype == torch.bfloat16 and dst.dtype == torch.float32 and src.numel() == dst.numel()
    raw = _stream() if stream is None else stream.cuda_stream
    _check(lib().vlmo_grad_unpack(_p(src), _p(dst), src.numel(), raw), 'vlmo_grad_unpack')


def stack_fwd(sdesc):
    _check(lib().vlmo_stack_fwd(ctypes.byref(sdesc), _stream()), 'vlmo_stack_fwd')


def stack_bwd(sdesc):
    _check(lib().vlmo_stack_bwd(ctypes.byref(sdesc), _stream()), 'vlmo_stack_bwd')


def ce_reduce(partial, nchunk, labels, ignore_index, lse, loss, pred, M):
    _check(lib().vlmo_ce_reduce(_p(partial), nchunk, _p(labels), ignore_index, _p(lse), _p(loss), _p(pred), M, _stream()),
           'vlmo_ce_reduce')


def ln_gelu_fwd(x, w, b, h, mean, rstd, M, d, eps=1e-12):
    """h (bf16 [M, >= d], pad columns zeroed) = GELU(LayerNorm(x[:, :d]) * w + b); x fp32."""
    _check(lib().vlmo_ln_gelu_fwd(_p(x), x.stride(0), _p(w), _p(b), _p(h), h.stride(0), _p(mean), _p(rstd), M, d, eps,
                                  _stream()), 'vlmo_ln_gelu_fwd')


def ln_gelu_bwd(dh, x, w, b, mean, rstd, M, d, *, dx=None, dxb=None, dw=None, db=None, dbias=None):
    """Backward of ln_gelu_fwd: dx fp32 and / or dxb bf16 (pad columns zeroed); dw, db, dbias overwritten."""
    ws = workspace(x.device, 3 * d)          # >= min(M, 128) partial rows of 3d floats
    _check(lib().vlmo_ln_gelu_bwd(_p(dh), dh.stride(0), _p(x), x.stride(0), _p(w), _p(b), _p(mean), _p(rstd), _p(dx),
                                  dx.stride(0) if dx is not None else 0, _p(dxb), dxb.stride(0) if dxb is not None else 0,
                                  _p(dw), _p(db), _p(dbias), M, d, _p(ws), ws.numel() * 4, _stream()), 'vlmo_ln_gelu_bwd')


def vqa_bce(z, y, B, V, *, row_loss=None, row_arg=None, row_score=None, dscale=None, alpha=1.0, dadd=None, dz=None):
    """Row kernel of the VQA loss (include/vlmo_hip.h: vlmo_vqa_bce); z, y, dadd fp32, dz bf16 [B, multiple of 64]."""
    _check(lib().vlmo_vqa_bce(_p(z), z.stride(0), _p(y), y.stride(0) if y is not None else 0, B, V, _p(row_loss),
                              _p(row_arg), _p(row_score), _p(dscale), float(alpha), _p(dadd),
                              dadd.stride(0) if dadd is not None else 0, _p(dz), dz.stride(0) if dz is not None else 0,
                              _stream()), 'vlmo_vqa_bce')


def isda_update(u, y, B, V, A, count, mean, cov, k, *, ln_mean=None, ln_rstd=None, ln_w=None, ln_b=None):
    """ISDA estimator update in place (include/vlmo_hip.h: vlmo_isda_update) and k int32 [B] = first arg-max of each
    target row.  With ln_w given the features are GELU(LayerNorm(u)) recomputed from the pre-LayerNorm rows u and
    ln_mean / ln_rstd; without, u are the features."""
    for t, n in ((count, 'count'), (mean, 'mean'), (cov, 'cov')):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f'isda_update: {n} must be contiguous fp32')
    _check(lib().vlmo_isda_update(_p(u), u.stride(0), _p(ln_mean), _p(ln_rstd), _p(ln_w), _p(ln_b), _p(y), y.stride(0),
                                  B, V, A, _p(count), _p(mean), _p(cov), _p(k), _stream()), 'vlmo_isda_update')


def _isda_ws(device, B, V, A):
    return torch.empty((lib().vlmo_isda_ws_bytes(B, V, A) + 3) // 4, dtype=torch.float32, device=device)


def isda_aug_fwd(W, k, ck, B, V, A, scale, z):
    """z[:, :V] += scale * sum_a (W[j] - W[k_n])^2 ck[n] (vlmo_isda_aug_fwd); W, ck, z fp32, k int32."""
    ws = _isda_ws(z.device, B, V, A)
    _check(lib().vlmo_isda_aug_fwd(_p(W), W.stride(0), _p(k), _p(ck), ck.stride(0), B, V, A, float(scale), _p(z),
                                   z.stride(0), _p(ws), ws.numel() * 4, _stream()), 'vlmo_isda_aug_fwd')


def isda_aug_bwd(G, W, k, ck, B, V, A, r, dw):
    """dw[:V] += the augmentation's weight gradient for G = d loss / d z_aug bf16 (vlmo_isda_aug_bwd)."""
    if G.dtype != torch.bfloat16:
        raise ValueError('isda_aug_bwd: G must be bf16')
    ws = _isda_ws(dw.device, B, V, A)
    _check(lib().vlmo_isda_aug_bwd(_p(G), G.stride(0), _p(W), W.stride(0), _p(k), _p(ck), ck.stride(0), B, V, A,
                                   float(r), _p(dw), dw.stride(0), _p(ws), ws.numel() * 4, _stream()), 'vlmo_isda_aug_bwd')


def sim_topk(q, g, k, scale=1.0, splits=0):
    """vlmo_sim_topk: the k best rows of g fp32 [Ng, D] for every row of q fp32 [Nq, D] under scale * <q, g> -> (values
    fp32 [Nq, k], indices int32 [Nq, k]), best first, equal scores by ascending index, -inf / -1 past Ng.  Rows may be
    strided (stride(1) == 1).  The per-slice lists of a split gallery live in a workspace allocated for this call."""
    for t, n in ((q, 'q'), (g, 'g')):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f'sim_topk: {n} must be a 2-D fp32 tensor with unit column stride')
    if q.shape[1] != g.shape[1] or q.device != g.device:
        raise ValueError('sim_topk: q and g must have the same width and device')
    Nq, D = q.shape
    Ng = g.shape[0]
    val = torch.empty(Nq, k, dtype=torch.float32, device=q.device)
    idx = torch.empty(Nq, k, dtype=torch.int32, device=q.device)
    nbytes = lib().vlmo_sim_topk_ws_bytes(Nq, Ng, k, splits)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device) if nbytes > 0 else None
    _check(lib().vlmo_sim_topk(_p(q), q.stride(0), _p(g), g.stride(0), Nq, Ng, D, k, float(scale), splits, _p(ws), nbytes,
                               _p(val), _p(idx), _stream()), 'vlmo_sim_topk')
    return val, idx


def relevance_step(A, x_in, x_out, c0, alpha, beta):
    """vlmo_relevance_step: x_out[s, r, c0 + j] = alpha x_in[s, r, c0 + j] + beta sum_k x_in[s, r, c0 + k] A[s, k, j] for
    A fp32 [S, n, n], x_in and x_out fp32 [S, nq, width], all contiguous on one device; the other columns of x_out are
    left as they are."""
    for t, name in ((A, 'A'), (x_in, 'x_in'), (x_out, 'x_out')):
        if t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous() or t.device != A.device:
            raise ValueError(f'relevance_step: {name} must be a contiguous 3-D fp32 tensor on the device of A')
    S, n, n2 = A.shape
    if n != n2 or x_in.shape != x_out.shape or x_in.shape[0] != S:
        raise ValueError(f'relevance_step: need A [S, n, n] and x_in, x_out [S, nq, width], got {tuple(A.shape)}, '
                         f'{tuple(x_in.shape)}, {tuple(x_out.shape)}')
    _check(lib().vlmo_relevance_step(_p(A), _p(x_in), _p(x_out), S, x_in.shape[1], x_in.shape[2], int(c0), n, float(alpha),
                                     float(beta), _stream()), 'vlmo_relevance_step')


FILTER_BICUBIC, FILTER_LANCZOS = 0, 1
FINISH_NORMALIZE, FINISH_MAP_PIXELS = 0, 1
CROP_MAX_SIZE, CROP_MAX_SIDE, CROP_MAX_JOBS = 1024, 8192, 65536


# VlmoImage, VlmoCropJob and VlmoAugSlot as numpy dtypes, made from the ctypes mirrors above: the sizes and offsets of
# include/vlmo_hip.h
_IMAGE_DT, _JOB_DT, _SLOT_DT = np.dtype(Image), np.dtype(CropJob), np.dtype(AugSlot)


def image_records(images):
    """[(offset, H, W)] -> VlmoImage records (numpy, on the host)."""
    return np.array([tuple(im) for im in images], dtype=_IMAGE_DT).reshape(-1)


def crop_job_records(jobs):
    """[(image, top, left, h, w, flip, S, filter, finish, out)] -> (VlmoCropJob records, floats of the intermediate): a
    job's tmp_off is the running sum of the h * S * 3 floats of the jobs in front of it."""
    rec = np.array([(im, top, left, h, w, int(flip), S, filt, fin, 0, 0, out.data_ptr())
                    for im, top, left, h, w, flip, S, filt, fin, out in jobs], dtype=_JOB_DT).reshape(-1)
    run = np.cumsum(rec['h'].astype(np.int64) * rec['S'] * 3)
    rec['tmp_off'][1:] = run[:-1]
    return rec, int(run[-1]) if len(run) else 0


def aug_slot_records(ops, a, b):
    """ops int, a and b float64 arrays [N, n] -> the N * n VlmoAugSlot records, image by image."""
    rec = np.zeros(ops.size, dtype=_SLOT_DT)
    rec['op'], rec['a'], rec['b'] = ops.reshape(-1), a.reshape(-1), b.reshape(-1)
    return rec


def _stage_tables(device, itab, second):
    """The image records and a call's second table in ONE pinned staging buffer, which one asynchronous copy on the current
    stream uploads.  The image table comes first: its records are 16 bytes, so the table behind it stays 8-byte aligned.
    -> ((images, images_dev, second, second_dev): the addresses an entry point takes, to check the host copy and hand the
    device copy to its kernels; the two buffers, for the caller to hold until the entry point has returned)."""
    ibytes, sbytes = itab.nbytes, second.nbytes
    host = torch.empty(max(1, ibytes + sbytes), dtype=torch.uint8, pin_memory=True)
    raw = host.numpy()
    raw[:ibytes], raw[ibytes:ibytes + sbytes] = itab.view('u1'), second.view('u1')
    dev = host.to(device, non_blocking=True)
    return (host.data_ptr(), dev.data_ptr(), host.data_ptr() + ibytes, dev.data_ptr() + ibytes), (host, dev)


def crop_resample(pixels, images, jobs, mean, std, pixel_eps):
    """vlmo_crop_resample: pixels = device uint8 buffer of packed HWC images (4-byte aligned, length a multiple of 4);
    images = [(offset, H, W)]; jobs = [(image, top, left, h, w, flip, S, filter, finish, out)] with out an fp32 [3, S, S]
    contiguous device tensor that the job fills.  Two launches for the whole list; the fp32 intermediates live in a cached
    scratch buffer.  The tables travel as _stage_tables describes."""
    for q, job in enumerate(jobs):
        out, S = job[9], job[6]
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != 3 * S * S or out.device != pixels.device:
            raise ValueError(f'crop_resample: job {q}: out must be a contiguous fp32 [3, {S}, {S}] tensor on the pixels\' device')
    itab, (jtab, total) = image_records(images), crop_job_records(jobs)
    ws = _scratch('crop', pixels.device, total * 4, 1 << 24)
    (ih, idev, jh, jdev), keep = _stage_tables(pixels.device, itab, jtab)
    m3, s3 = (_f32 * 3)(*mean), (_f32 * 3)(*std)
    _check(lib().vlmo_crop_resample(_p(pixels), pixels.numel(), ih, idev, len(itab), jh, jdev, len(jtab), m3, s3,
                                    float(pixel_eps), _p(ws), ws.numel() * 4, _stream()), 'vlmo_crop_resample')


(AUG_SKIP, AUG_IDENTITY, AUG_AUTOCONTRAST, AUG_EQUALIZE, AUG_BRIGHTNESS, AUG_SHARPNESS, AUG_SHEAR_X, AUG_SHEAR_Y,
 AUG_TRANSLATE_X, AUG_TRANSLATE_Y, AUG_ROTATE, AUG_SOLARIZE, AUG_POSTERIZE, AUG_CONTRAST) = range(-1, 13)
AUG_MAX_SLOTS, AUG_MAX_IMAGES, AUG_MAX_SHIFT = 4, 65536, 1000000


def randaug(pixels, images, ops, a, b, fill=128, out=None, scratch=None, ws=None):
    """vlmo_randaug: pixels = device uint8 buffer of packed HWC images (4-byte aligned, length a multiple of 4); images =
    [(offset, H, W)]; ops int [N, n], a and b float64 [N, n] (array-likes on the host): operation AUG_* and its arguments
    for slot s of image i.  Returns a new buffer of the same length with every image's slots applied in order; bytes
    outside the images are not written.  out, scratch (for n > 1) and ws default to fresh / cached buffers.  The tables
    travel as _stage_tables describes; nothing is read back."""
    ops = np.asarray(ops, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ni = len(images)
    if ops.ndim != 2 or ops.shape[0] != ni or a.shape != ops.shape or b.shape != ops.shape:
        raise ValueError(f'randaug: ops, a and b must be [{ni}, n] (got {ops.shape}, {a.shape}, {b.shape})')
    n = ops.shape[1]
    if out is None:
        out = torch.empty_like(pixels)
    if scratch is None and n > 1:
        scratch = torch.empty_like(pixels)
    for t, name in ((pixels, 'pixels'), (out, 'out'), (scratch, 'scratch')):
        if t is not None and (t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or t.device != pixels.device
                              or t.numel() != pixels.numel()):
            raise ValueError(f'randaug: {name} must be a contiguous 1-D uint8 buffer of pixels\' length and device')
    if ws is None:
        ws = _scratch('randaug', pixels.device, lib().vlmo_randaug_ws_bytes(ni), 1 << 20)
    (ih, idev, sh, sdev), keep = _stage_tables(pixels.device, image_records(images), aug_slot_records(ops, a, b))
    _check(lib().vlmo_randaug(_p(pixels), _p(out), _p(scratch), pixels.numel(), ih, idev, ni, sh, sdev, n, int(fill), _p(ws),
                              ws.numel() * ws.element_size(), _stream()), 'vlmo_randaug')
    return out


PROFILE_TAGS = 96


class TensorList(ctypes.Structure):
    """VlmoTensorList (include/vlmo_hip.h): device tables of one multi-tensor optimizer launch."""
    _fields_ = [('p', _vp), ('g', _vp), ('m', _vp), ('v', _vp), ('numel', _vp), ('lr', _vp), ('wd', _vp),
                ('chunk_tensor', _vp), ('chunk_start', _vp), ('n_chunks', _i32), ('chunk', _i32)]


class AdamArgs(ctypes.Structure):
    _fields_ = [('beta1', _f32), ('beta2', _f32), ('eps', _f32), ('inv_bc1', _f32), ('inv_bc2', _f32),
                ('adam_w_mode', _i32)]


def mt_grad_norm(tl, inv_scale, max_norm, partial, out):
    """out[0] = grad norm, out[1] = factor for the raw gradients, out[2] = non-finite flag (device floats)."""
    _check(lib().vlmo_mt_grad_norm(ctypes.byref(tl), float(inv_scale), float(max_norm), _p(partial), _p(out), _stream()),
           'vlmo_mt_grad_norm')


def mt_adam(tl, args, ctl=None):
    _check(lib().vlmo_mt_adam(ctypes.byref(tl), ctypes.byref(args), _p(ctl), _stream()), 'vlmo_mt_adam')


def mt_ema(tl, w):
    """Weight average in place: tensor tl.p[t] <- tl.p[t] + w * (tl.g[t] - tl.p[t]) for every tensor of the list."""
    _check(lib().vlmo_mt_ema(ctypes.byref(tl), float(w), _stream()), 'vlmo_mt_ema')


def mt_adam_ema(tl, args, ctl, ema, w):
    """mt_adam, then the average of the new parameter values in the same pass; ema = device int64 table parallel to
    tl.p holding the address of each tensor's average (0: none)."""
    _check(lib().vlmo_mt_adam_ema(ctypes.byref(tl), ctypes.byref(args), _p(ctl), _p(ema), float(w), _stream()),
           'vlmo_mt_adam_ema')


def side_stream_create(low_priority=True, cu_mask=None):
    """Native stream for the weight-gradient work (include/vlmo_hip.h: vlmo_side_stream_create) -> raw
    hipStream_t value.  Create it with the target device current."""
    out = ctypes.c_void_p()
    if cu_mask:
        words = (ctypes.c_uint32 * len(cu_mask))(*cu_mask)
        rc = lib().vlmo_side_stream_create(0, words, len(cu_mask), ctypes.byref(out))
    else:
        rc = lib().vlmo_side_stream_create(1 if low_priority else 0, None, 0, ctypes.byref(out))
    _check(rc, 'vlmo_side_stream_create')
    return out.value


def profile_start(max_records=1 << 15):
    _check(lib().vlmo_profile_start(max_records), 'vlmo_profile_start')


def profile_stop():
    """-> {tag: (seconds, flops, launches)} for the launches recorded since profile_start()."""
    n = PROFILE_TAGS
    ms, fl, ln = (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_int64 * n)()
    lib().vlmo_profile_stop(n, ms, fl, ln)
    names = {0: 'bias', 1: 'bias_gelu', 2: 'resid', 3: 'dgelu', 4: 'f32', 5: 'dual', 6: 'argmax', 7: 'ce', 8: 'ce_bwd'}
    out = {}
    for t in range(n):
        if ln[t]:
            if t in (64, 72):
                name = 'gemm_tn_kernel<%s>' % ('256x256' if t == 72 else '128x128')
            elif t == 73:
                name = 'gemm_tn_multi_kernel<256x256>'
            elif 80 <= t < 96:
                name = f'gemm_nt16_kernel<{names.get(t - 80, t - 80)},Hx256>'
            elif 48 <= t < 64:
                name = f'gemm_nt_kernel<{names.get(t - 48, t - 48)},256x128>'
            elif t >= 32:
                name = f'conv_nt_kernel<{names.get(t - 32, t - 32)}>'
            else:
                name = f'gemm_nt_kernel<{names.get(t & 15, t & 15)},{"256x256" if t & 16 else "128x128"}>'
            out[name] = (ms[t] * 1e-3, fl[t], ln[t])
    return out
