"""The C-ABI library (libnfx.so) loads without a GPU and exports every symbol include/nfx.h
declares; host-only entry points (sizes, version, argument validation) behave."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import nfs_amd
from nfs_amd import _lib

HEADER = os.path.join(ROOT, "include", "nfx.h")


def declared_symbols():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"\b(nfx_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 14
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(_lib.EXPORTED_SYMBOLS) == syms


def test_abi_version_and_sizes():
    L = _lib.lib()
    assert L.nfx_abi_version() == 3
    assert L.nfx_affine_packed_floats(2, 64) > 0
    assert L.nfx_affine_packed_floats(2, 64) % 4 == 0
    assert L.nfx_spline_packed_floats(2, 64, 8) % 4 == 0
    assert L.nfx_made_packed_floats(63, 64) % 4 == 0
    assert L.nfx_affine_packed_floats(0, 64) == 0
    assert L.nfx_gauss_workspace_bytes(1 << 20) >= 8


def test_invalid_arguments_fail_before_any_launch():
    """Argument validation happens on the host: no device pointer is touched."""
    L = _lib.lib()
    rc = L.nfx_affine_coupling(None, None, None, None, 16, 2, 64, 0, 0, None)
    assert rc == -1 and b"direction" in L.nfx_last_error()
    rc = L.nfx_affine_coupling(None, None, None, None, 16, 9, 64, 1, 0, None)
    assert rc in (-1, -2)
    rc = L.nfx_spline_coupling(None, None, None, None, 16, 2, 64, 12, 5.0, 1e-3, 1e-3, 1e-3, 0, 0.0, 0.0, 1, 0, None)
    assert rc == -2 and b"K=12" in L.nfx_last_error()
    rc = L.nfx_made_affine(None, None, None, None, 16, 63, 64, 7, 0, None)
    assert rc == -1
    rc = L.nfx_rqs_unit(None, None, None, None, None, None, 16, 40, 1e-3, 1e-3, 1e-3, 0, None)
    assert rc == -2
    # B == 0 is a valid no-op
    assert L.nfx_affine_coupling(None, None, None, None, 0, 2, 64, 1, 0, None) == 0
    # between-layer BatchNorm
    rc = L.nfx_flowbn_apply(None, None, None, 1, 1, 1, 1, 1e-5, 16, 2, 0, None)
    assert rc == -1 and b"direction" in L.nfx_last_error()
    rc = L.nfx_flowbn_apply(None, None, None, 1, 1, 1, 1, 1e-5, 16, 2000, 1, None)
    assert rc == -2
    assert L.nfx_flowbn_apply(None, None, None, 1, 1, 1, 1, 1e-5, 0, 2, 1, None) == 0
    assert L.nfx_flowbn_workspace_bytes(1 << 20, 63) >= 8 * 63 * 2


def test_product_raises_without_library(monkeypatch, tmp_path):
    """No silent eager fallback: a missing libnfx.so is a loud error."""
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.NfxLibraryError):
        _lib.load(str(tmp_path / "missing.so"))


def test_affine_kernel_policy_roundtrip():
    """Host-only entry point: set/read the affine kernel policy (no GPU call)."""
    f = _lib.load().nfx_affine_kernel_policy
    prev = f(-1)
    assert prev in (_lib.NFX_AFFINE_AUTO, _lib.NFX_AFFINE_STREAMING, _lib.NFX_AFFINE_SMALL)
    assert f(_lib.NFX_AFFINE_SMALL) == prev
    assert f(-1) == _lib.NFX_AFFINE_SMALL
    assert f(7) == _lib.NFX_EINVAL
    assert f(prev) == _lib.NFX_AFFINE_SMALL
    assert f(-1) == prev


def test_any_shape_entry_points_validate_on_the_host():
    """The any-shape path (csrc/nfx_generic.hip): shape / variant / mode checks and the B == 0
    no-ops return before any device call; workspace sizes are host arithmetic."""
    L = _lib.lib()
    EINVAL, EUNSUP = _lib.NFX_EINVAL, _lib.NFX_EUNSUPPORTED
    assert L.nfx_linear_forward(None, None, None, None, None, None, None, None, -1, 4, 4, 0, None) == EINVAL
    assert L.nfx_linear_forward(None, None, None, None, None, None, None, None, 0, 4, 4, 0, None) == 0
    assert L.nfx_linear_forward(None, None, None, None, None, None, None, None, 8, 4, 4, 0, None) == EINVAL
    ps = ctypes.c_void_p(1)
    assert L.nfx_linear_forward(ps, ps, None, None, None, ps, None, ps, 8, 4, 4, 0, None) == EINVAL
    assert b"post_scale" in L.nfx_last_error()
    assert L.nfx_linear_backward_data(None, None, None, None, None, None, 8, 0, 4, 0, None) == EINVAL
    assert L.nfx_linear_backward_weight(None, None, None, None, None, None, 8, 4, 4, None, None) == EINVAL
    assert L.nfx_linear_workspace_bytes(1 << 20, 128, 128) >= 128 * 128 * 4
    assert L.nfx_linear_workspace_bytes(0, 128, 128) == 0
    assert L.nfx_spline_elem_forward(None, None, None, None, None, 8, 2, 12, 5.0, 1e-3, 1e-3, 1e-3, 1, 0,
                                     None) == EUNSUP
    assert L.nfx_spline_elem_backward(None, None, None, None, None, None, None, 8, 2, 8, 5.0, 1e-3, 1e-3, 1e-3, 0,
                                      None) == EINVAL
    # the MADE element map: parallel variants only; a sequential step needs a sequential variant
    assert L.nfx_made_elem_forward(None, None, None, None, 8, 4, _lib.NFX_MAF_FORWARD, 0, None) == EINVAL
    assert L.nfx_made_elem_step(None, None, None, None, 8, 4, 0, _lib.NFX_MAF_INVERSE, None) == EINVAL
    assert L.nfx_made_elem_step(None, None, None, None, 8, 4, 4, _lib.NFX_MAF_FORWARD, None) == EINVAL
    assert L.nfx_made_elem_seq_backward(None, None, None, None, None, None, None, 8, 4, _lib.NFX_IAF_INVERSE, 3,
                                        None) == EINVAL
    assert L.nfx_made_elem_backward(None, None, None, None, None, None, 0, 4, _lib.NFX_IAF_FORWARD, None) == 0
    assert L.nfx_affine_elem_forward(None, None, None, None, None, None, 8, 4, 0, 0, None) == EINVAL
    assert L.nfx_arqs_step(None, None, None, None, None, None, None, None, 8, 4, 1, 0, 1, 0, 1e-3, 1e-3, 1e-3,
                           None) == EUNSUP
    assert L.nfx_arqs_step(None, None, None, None, None, None, None, None, 8, 4, 8, 0, 1, 5, 1e-3, 1e-3, 1e-3,
                           None) == EINVAL
    assert L.nfx_bn_prepare(None, None, None, None, None, 1e-5, 0.1, 0, 0, None, None, None, None, None) == EINVAL
    assert L.nfx_bn_workspace_bytes(1 << 20, 64) >= 2 * 64 * 8


# ---- the signature table against the header, and the checked handle --------------------------
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "const char*": ctypes.c_char_p, "const NfxMlpRaw*": ctypes.POINTER(_lib.NfxMlpRaw)}


def ctype_of(c_type):
    """The ctypes type a C type of include/nfx.h binds to."""
    c_type = " ".join(c_type.replace("*", "* ").split()).replace(" *", "*")
    if c_type in _SCALARS:
        return _SCALARS[c_type]
    if c_type.endswith("* const*"):
        return ctypes.POINTER(ctypes.c_void_p)
    assert c_type.endswith("*"), c_type
    return ctypes.c_void_p


def declarations():
    """[(return type, name, [parameter types])] of every `<ret> nfx_name(<params>);` in the header."""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\s*\b(nfx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        params = [" ".join(p.split()) for p in params.split(",")]
        params = [re.match(r"^(.*?)\w+$", p).group(1).strip() for p in params if p not in ("", "void")]
        out.append((ret.strip(), name, params))
    return out


def test_signature_table_matches_the_header():
    """Arity, return type and every parameter's type class of _SIGNATURES equal the header's: an
    `int` bound where the header says `int64_t` would corrupt arguments silently."""
    decls = declarations()
    assert sorted(n for _, n, _ in decls) == declared_symbols() and len(decls) >= 104
    assert _lib.EXPORTED_SYMBOLS == tuple(_lib._SIGNATURES)
    bad = []
    for ret, name, params in decls:
        res, args = _lib._SIGNATURES[name]
        if res is not ctype_of(ret):
            bad.append(f"{name}: returns {ret}, bound as {res.__name__}")
        if len(args) != len(params):
            bad.append(f"{name}: {len(params)} parameters, {len(args)} bound")
            continue
        bad += [f"{name}: parameter {i} is {p}, bound as {a.__name__}"
                for i, (p, a) in enumerate(zip(params, args)) if a is not ctype_of(p)]
    assert not bad, bad


def test_value_returning_symbols_are_the_documented_ones():
    ints = {n for n, (res, _) in _lib._SIGNATURES.items() if res is ctypes.c_int}
    assert _lib._VALUE_RETURNING <= ints
    assert _lib._VALUE_RETURNING == {n for n in ints if n == "nfx_abi_version" or n.endswith(("_policy", "_supported"))}
    N = _lib.checked()
    for name in _lib.EXPORTED_SYMBOLS:
        want = _lib._raise_on_status if name in ints - _lib._VALUE_RETURNING else None
        assert getattr(N, name).errcheck is want, name


def test_checked_handle_raises_and_raw_handle_does_not():
    N, L = _lib.checked(), _lib.lib()
    assert N.nfx_affine_coupling is not L.nfx_affine_coupling
    with pytest.raises(_lib.NfxError) as e:
        N.nfx_affine_coupling(None, None, None, None, 16, 2, 64, 0, 0, None)
    assert all(s in str(e.value) for s in ("nfx_affine_coupling", "rc=-1", "direction"))
    assert N.nfx_affine_coupling(None, None, None, None, 0, 2, 64, 1, 0, None) == _lib.NFX_OK
    assert L.nfx_affine_coupling(None, None, None, None, 16, 2, 64, 0, 0, None) == -1
    assert L.nfx_affine_coupling.errcheck is None


def test_checked_errors_carry_the_true_symbol_name():
    """The three entry points whose hand-written labels named another function: each host-side
    rejection (layer 0; stage 0; null statistics) is reported under the symbol that was called."""
    N = _lib.checked()
    with pytest.raises(_lib.NfxError, match=r"^nfx_affine_train_stats_keep failed \(rc=-1\): .*layer"):
        N.nfx_affine_train_stats_keep(None, None, 16, 2, 64, 0, None, None, None, None)
    with pytest.raises(_lib.NfxError, match=r"^nfx_affine_train_backward_keep failed \(rc=-1\): .*stage"):
        N.nfx_affine_train_backward_keep(None, None, None, None, None, 16, 2, 64, 1, 0, None, None, None, None, None)
    with pytest.raises(_lib.NfxError, match=r"^nfx_affine_train_update_running_counted failed \(rc=-1\): "):
        N.nfx_affine_train_update_running_counted(None, None, None, None, None, 64, 0.1, None)


def test_device_pointer_arguments_take_tensors():
    """DevicePtr: None is null, a tensor its data_ptr(), an int itself; end to end with CPU tensors
    through validation that returns before any device call."""
    import torch
    x, w, ps, y = torch.zeros(8, 4), torch.zeros(4, 4), torch.zeros(4), torch.zeros(8, 4)
    as_c_void_p = ctypes.c_void_p.from_param
    assert _lib.DevicePtr.from_param(None) is None
    assert repr(_lib.DevicePtr.from_param(x)) == repr(as_c_void_p(x.data_ptr()))
    assert repr(_lib.DevicePtr.from_param(7)) == repr(as_c_void_p(7)) and "0x7" in repr(as_c_void_p(7))
    big = (1 << 47) + 8  # an address beyond 32 bits arrives whole
    assert repr(_lib.DevicePtr.from_param(big)) == repr(as_c_void_p(big)) and hex(big) in repr(as_c_void_p(big))
    N = _lib.checked()
    with pytest.raises(_lib.NfxError, match="post_scale"):
        N.nfx_linear_forward(x, w, None, None, None, ps, None, y, 8, 4, 4, 0, None)
    assert N.nfx_linear_forward(x, w, None, None, None, None, None, y, 0, 4, 4, 0, None) == _lib.NFX_OK


def test_checked_value_returning_symbols_do_not_raise():
    N = _lib.checked()
    assert N.nfx_affine_kernel_policy(7) == _lib.NFX_EINVAL
    assert N.nfx_cnf_supported(16, 9, 64) == 0
    assert N.nfx_abi_version() == 3 and N.nfx_gauss_workspace_bytes(1 << 20) >= 8
    assert isinstance(N.nfx_last_error(), bytes)
