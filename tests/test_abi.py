"""The C-ABI library builds, loads and exports every symbol include/vlmo_hip.h
declares, at the ABI version the header states (no compute: runs without a GPU)."""
import ctypes
import os
import re

from exploremultimodal_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'vlmo_hip.h')).read()


def _declared():
    return sorted(set(re.findall(r'\b(vlmo_[a-z0-9_]+)\s*\(', _header())))


def _header_abi_version():
    m = re.search(r'^#define\s+VLMO_ABI_VERSION\s+(\d+)\s*$', _header(), re.M)
    assert m, 'vlmo_hip.h does not define VLMO_ABI_VERSION'
    return int(m.group(1))


def test_library_exports_header_symbols_at_header_abi_version():
    import __graft_entry__ as ge
    if not os.path.exists(hip.LIB_PATH):
        ge.build()
    L = ctypes.CDLL(hip.LIB_PATH)
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), f'{n} declared in vlmo_hip.h but not exported'
    assert sorted(hip.exported_symbols()) == names, 'hip.py binding list and header disagree'
    L.vlmo_abi_version.restype = ctypes.c_int
    assert L.vlmo_abi_version() == hip.ABI_VERSION == _header_abi_version()


def test_missing_library_fails_loudly(monkeypatch):
    import pytest
    monkeypatch.setattr(hip, 'LIB_PATH', '/nonexistent/libvlmo_hip.so')
    monkeypatch.setattr(hip, '_lib', None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.lib()


def test_stack_bwd_workspace_layout():
    """vlmo_stack_bwd_ws_bytes, the one definition of a block's column workspace (no GPU: a host function): monotone in
    every argument; no larger than the formula the engine carried before it, at the Base (B = 64) and Large (B = 32)
    training shapes with 2 B sequences; and room for the six fold slots of the partial rows at the smallest stack
    shape of the suite (mini, one 5-token text + one image: M = 22)."""
    L = hip.lib()
    ws = L.vlmo_stack_bwd_ws_bytes
    base = (16704, 768, 3072, 128)
    for k, steps in enumerate([(1, 15, 16, 17), (4, 64), (8, 1024), (1, 2, 64)]):
        prev = ws(*base)
        for s_ in steps:
            a = list(base)
            a[k] += s_
            assert ws(*a) >= prev, (k, s_)
            prev = ws(*a)
        assert prev > ws(*base), k

    def old_bytes(M, d, hid, B):
        return 4 * (6 * L.vlmo_reduce_ws_bytes(2 * d) // 4 + (M // 16 + 4) * hid + 4 * B * d)
    for M, d, hid, seqs in [base, (8352, 1024, 4096, 64)]:
        assert 0 < ws(M, d, hid, seqs) <= old_bytes(M, d, hid, seqs // 2), (M, d, hid, seqs)
    assert ws(22, 128, 512, 2) >= 6 * L.vlmo_reduce_ws_bytes(2 * 128)
